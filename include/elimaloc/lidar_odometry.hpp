// lidar_odometry.hpp -- LiDAR odometry on a rolling local map kept on the device (include/elimaloc_hip.h, "LiDAR odometry on a rolling
// local map"): the C++ face of elm_odometry in the shim's types.  Every scan is registered against the local map and, when it is a
// keyframe, inserted by one device build that also forgets what lies farther than max_range_m from the new pose; after the scan's own
// upload no point crosses the bus.  The rules (first scan, keyframe test, insert, prediction, failed steps) are those of the C header.
#pragma once
#include <vector>

#include "registration.hpp"

struct OdometryConfig {
    double voxel_size = 1.0;
    int max_points_per_voxel = 30;
    double max_range_m = 100.0;     // stored points farther than this from the new pose's translation are forgotten at an insert
    double key_min_trans_m = 0.0;   // insert only when the pose moved this far from the last inserted one (0, 0: every scan)
    double key_min_rot_rad = 0.0;
    RegistrationConfig reg;         // method, gates, search distances: all four methods are legal
    elm_odometry_config c_struct() const {
        elm_odometry_config c;
        elm_odometry_config_default(&c);
        c.voxel_size = voxel_size;
        c.max_points_per_voxel = max_points_per_voxel;
        c.max_range_m = max_range_m;
        c.key_min_trans_m = key_min_trans_m;
        c.key_min_rot_rad = key_min_rot_rad;
        c.reg = reg.c_struct();
        return c;
    }
};

struct OdometryStep {
    elimaloc::Matrix4d pose;    // map <- scan frame
    bool registered = false;    // false for the first scan
    bool is_success = false;
    bool inserted = false;
    elm_reg_result reg;         // the registration's result (registered only)
    elm_build_sources_stats build; // the insert's counts (inserted only)
};

class LidarOdometry {
public:
    using RadarPointVector = VoxelHashMap::RadarPointVector;
    explicit LidarOdometry(const OdometryConfig& config = OdometryConfig()) {
        const elm_odometry_config c = config.c_struct();
        elimaloc::check(elm_odometry_create(VoxelHashMap::ctx(), &c, &odom_), VoxelHashMap::ctx(), "elm_odometry_create");
    }
    LidarOdometry(const LidarOdometry&) = delete; // owns device memory
    LidarOdometry& operator=(const LidarOdometry&) = delete;
    ~LidarOdometry() { elm_odometry_destroy(odom_); }

    // One scan (sensor frame, PointStruct::pose), uploaded for the call, from `guess` (nullptr: Predict()).
    inline OdometryStep Step(const RadarPointVector& scan, const elimaloc::Matrix4d* guess = nullptr) {
        std::vector<float> xyz(3 * scan.size());
        for (size_t i = 0; i < scan.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scan[i].pose(k);
        elm_scan* s = nullptr;
        elimaloc::check(elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scan.size(), scan.size(), &s), VoxelHashMap::ctx(), "elm_scan_upload");
        elm_odometry_step st;
        const int rc = elm_odometry_step_scan(odom_, s, guess ? guess->data() : nullptr, &st); // column-major on both sides
        elm_scan_destroy(s);
        elimaloc::check(rc, VoxelHashMap::ctx(), "elm_odometry_step_scan");
        OdometryStep out;
        for (int k = 0; k < 16; ++k) out.pose.data()[k] = st.T[k];
        out.registered = st.registered != 0;
        out.is_success = st.is_success != 0;
        out.inserted = st.inserted != 0;
        out.reg = st.reg;
        out.build = st.build;
        return out;
    }
    // the constant-velocity guess of the next pose: T_{k-1} (T_{k-2}^-1 T_{k-1}); the last pose with one, identity with none
    inline elimaloc::Matrix4d Predict() const {
        elimaloc::Matrix4d T;
        elimaloc::check(elm_odometry_predict(odom_, T.data()), VoxelHashMap::ctx(), "elm_odometry_predict");
        return T;
    }
    // the local map: owned by this object, valid until the next inserting Step / Reset / destruction; nullptr before the first scan
    inline const elm_map* Map() const { return elm_odometry_map(odom_); }
    inline void Reset() { elimaloc::check(elm_odometry_reset(odom_), VoxelHashMap::ctx(), "elm_odometry_reset"); }

private:
    elm_odometry* odom_ = nullptr;
};
