// Call lines of the local-map part of the C++ shim (include/elimaloc/voxel_hash_map.hpp: VoxelHashMap::UpdatedFromScans;
// include/elimaloc/lidar_odometry.hpp: OdometryConfig, LidarOdometry), compiled by tests/test_local_map_abi.py as
// tests/shim_harness/build_calls.cpp is: the Eigen-typed form against tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run
// without an argument it touches no device.
#include "lidar_odometry.hpp"

// a map built from two scans at their poses, then rolled forward by one more scan with what is far behind forgotten; an odometry object
// fed the same scans: the points the maps hold and the steps that inserted
size_t points_after_scans(const std::vector<PointStruct>& scan, const Eigen::Matrix4d& pose) {
    VoxelHashMap empty(1.0, 30), log_map, rolled;
    elm_build_sources_stats stats;
    empty.UpdatedFromScans(std::vector<VoxelHashMap::RadarPointVector>(2, scan), std::vector<Eigen::Matrix4d>(2, pose), log_map);
    const Eigen::Vector3d centre(pose(0, 3), pose(1, 3), pose(2, 3));
    log_map.UpdatedFromScans(std::vector<VoxelHashMap::RadarPointVector>(1, scan), std::vector<Eigen::Matrix4d>(1, pose), rolled, &centre, 25.0,
                             &stats);
    OdometryConfig config;
    config.max_range_m = 25.0;
    config.key_min_trans_m = 0.5;
    config.key_min_rot_rad = 0.05;
    config.reg.icp_method = IcpMethod::P2P;
    LidarOdometry odometry(config);
    const OdometryStep first = odometry.Step(scan, &pose);
    const Eigen::Matrix4d guess = odometry.Predict();
    const OdometryStep second = odometry.Step(scan);
    size_t n = log_map.Pointcloud().size() + rolled.Pointcloud().size() + (size_t)stats.n_points + (size_t)first.inserted + (size_t)second.inserted;
    if (odometry.Map() != nullptr && guess(3, 3) == 1.0) ++n;
    odometry.Reset();
    return n;
}

int main(int argc, char**) {
    if (argc > 1) return (int)points_after_scans(std::vector<PointStruct>(1), Eigen::Matrix4d::Identity());
    return 0;
}
