// voxel_hash_map.hpp -- drop-in shim with the reference's class name, member names and signatures
// (pcm_matching/include/voxel_hash_map.hpp:41-335) over the C ABI in elimaloc_hip.h.
// pcm_matching.cpp / pcm_matching.hpp compile against this header instead of the reference's: with <Eigen/Core> present
// every Eigen-typed member of the reference (PointStruct::pose/local, CovStruct::cov/mean, Voxel) has its Eigen type
// (linalg_types.hpp); without Eigen (this repository's build image) the same members are minimal fixed-size stand-ins.
// tests/test_shim_compile.py compiles the reference's literal call lines against this header with a test-only Eigen stub.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "../elimaloc_hip.h"
#include "linalg_types.hpp"

namespace elimaloc {
// The process-wide context of the shims.  ELM_DEVICES="0,1,2,3" (e.g. exported by the launch file): a device GROUP -- the map is replicated
// on those GPUs, every RunRegister shards its scan over them and all-reduces the 6x6 normal equations per ICP iteration (RCCL over xGMI);
// pcm_matching.cpp's call sites (pcm.cpp:82-105, 280-282, 412-414) do not change.  Unset: device 0.
inline elm_ctx* default_context() {
    static elm_ctx* ctx = [] {
        std::vector<int> ids;
        if (const char* e = std::getenv("ELM_DEVICES")) {
            for (const char* p = e; *p;) {
                char* end = nullptr;
                const long v = std::strtol(p, &end, 10);
                if (end == p) break;
                ids.push_back((int)v);
                p = end;
                while (*p == ',' || *p == ' ') ++p;
            }
        }
        if (ids.empty()) ids.push_back(0);
        elm_ctx* c = nullptr;
        int rc = elm_ctx_create_multi(ids.data(), (int)ids.size(), &c);
        if (rc != ELM_OK) throw std::runtime_error(std::string("elm_ctx_create_multi: ") + elm_strerror(rc));
        return c;
    }();
    return ctx;
}
inline void check(int rc, elm_ctx* ctx, const char* what) {
    if (rc != ELM_OK) throw std::runtime_error(std::string(what) + ": " + elm_strerror(rc) + " " + elm_last_error(ctx));
}
} // namespace elimaloc

// vhm.hpp:41-53
struct CovStruct {
    elimaloc::Matrix3d cov;  // 3x3 covariance matrix
    elimaloc::Vector3d mean; // 3D mean vector
    CovStruct() : cov(elimaloc::Matrix3d::Identity()), mean(elimaloc::Vector3d::Zero()) {}
    CovStruct(const elimaloc::Matrix3d& c, const elimaloc::Vector3d& m) : cov(c), mean(m) {}
    void reset() {
        cov = elimaloc::Matrix3d::Identity();
        mean = elimaloc::Vector3d::Zero();
    }
};

// vhm.hpp:55-87; pose/local are float32-exact in the reference (filled from float32 PCL points, pcm.hpp:205-215)
struct PointStruct {
    elimaloc::Vector3d pose;
    elimaloc::Vector3d local;
    CovStruct covariance;
    float vel;       // mps
    float azi_angle; // deg
    float ele_angle; // deg
    double intensity;
    PointStruct()
        : pose(elimaloc::Vector3d::Zero()), local(elimaloc::Vector3d::Zero()), covariance(CovStruct()), vel(0.0), azi_angle(0.0),
          ele_angle(0.0), intensity(0.0) {}
    void reset() {
        pose.setZero();
        local.setZero();
        covariance.reset();
        vel = 0.0;
        azi_angle = 0.0;
        ele_angle = 0.0;
        intensity = 0.0;
    }
};

// the reference's layout (vhm.hpp:55-87: 24 + 24 + 96 + 3 floats + pad + 8; Vector3d / Matrix3d of doubles are not "fixed-size
// vectorizable" in Eigen, so neither struct carries an alignment requirement beyond 8 bytes or needs EIGEN_MAKE_ALIGNED_OPERATOR_NEW, and
// std::vector<PointStruct> uses the default allocator there as here)
static_assert(sizeof(CovStruct) == 96 && sizeof(PointStruct) == 168 && alignof(PointStruct) == 8, "PointStruct must keep the reference's layout");

// elm_freespace_config with its defaults (include/elimaloc_hip.h, free-space check): the ray sampling of VoxelHashMap::CheckFreeSpace
struct FreeSpaceConfig : elm_freespace_config {
    FreeSpaceConfig() { elm_freespace_config_default(this); }
};

// elm_raycast_config with its defaults (include/elimaloc_hip.h, ray casting): the traversal and comparison of VoxelHashMap::RayCast
struct RayCastConfig : elm_raycast_config {
    RayCastConfig() { elm_raycast_config_default(this); }
};

// elm_evidence_config with its defaults (include/elimaloc_hip.h, map evidence): the walk of MapEvidence::Accumulate
struct EvidenceConfig : elm_evidence_config {
    EvidenceConfig() { elm_evidence_config_default(this); }
};

// elm_evidence_rule with its defaults: when a cell's counters make it stale (a starting point, not a measured optimum)
struct EvidenceRule : elm_evidence_rule {
    EvidenceRule() { elm_evidence_rule_default(this); }
};

// elm_growth_config with its defaults (include/elimaloc_hip.h, map growth): the evidence walk plus the clearance of MapGrowth::Accumulate
struct GrowthConfig : elm_growth_config {
    GrowthConfig() { elm_growth_config_default(this); }
};

// elm_growth_rule with its defaults: when a candidate cell's counters make it appeared (a starting point, not a measured optimum)
struct GrowthRule : elm_growth_rule {
    GrowthRule() { elm_growth_rule_default(this); }
};

// elm_growth_object_rule with its defaults: the member rule, the connectivity (6, 18 or 26) and the smallest object (starting points, not
// measured optima)
struct GrowthObjectRule : elm_growth_object_rule {
    GrowthObjectRule() { elm_growth_object_rule_default(this); }
};

class MapEvidence;
class MapGrowth;

struct VoxelHashMap {
    using RadarPointVector = std::vector<PointStruct>;
    using RadarPointVectorTuple = std::tuple<RadarPointVector, RadarPointVector>;
    using Voxel = elimaloc::Vector3i;

    VoxelHashMap() {}
    VoxelHashMap(double voxel_size, int max_points_per_voxel) { Init(voxel_size, max_points_per_voxel); }
    VoxelHashMap(const VoxelHashMap&) = delete; // owns device memory (the reference's node never copies its map either)
    VoxelHashMap& operator=(const VoxelHashMap&) = delete;
    ~VoxelHashMap() { Release(); }

    void Init(double voxel_size, int max_points_per_voxel) { // vhm.cpp:26-29
        voxel_size_ = voxel_size;
        max_points_per_voxel_ = max_points_per_voxel;
    }
    // vhm.cpp:270-285.  Repeated calls append (the device map is rebuilt from the concatenation, which is what
    // sequential AddPoints calls produce in the reference).
    // true: the map is built by elm_map_build_device (the same map, byte for byte) instead of the host build
    void BuildOnDevice(bool on) { device_build_ = on; }
    // true: the map's P2P / GICP cell grid is laid out on the device (elm_map_set_index_build: the same grid, byte for byte) instead of
    // on the host; holds for the index this map builds from now on and for the maps derived from it.  An index already built stays.
    void BuildIndexOnDevice(bool on) {
        device_index_ = on;
        if (map_) elimaloc::check(elm_map_set_index_build(map_, on ? ELM_INDEX_BUILD_DEVICE : ELM_INDEX_BUILD_HOST), ctx(), "elm_map_set_index_build");
    }
    void AddPoints(const RadarPointVector& points) {
        Materialize();
        xyz_.reserve(xyz_.size() + 3 * points.size());
        for (const auto& p : points) {
            xyz_.push_back((float)p.pose(0));
            xyz_.push_back((float)p.pose(1));
            xyz_.push_back((float)p.pose(2));
        }
        Release();
    }
    void AddPoints(const float* xyz, size_t n) { // float32 fast path for callers that hold the PCD's own arrays
        Materialize();
        xyz_.insert(xyz_.end(), xyz, xyz + 3 * n);
        Release();
    }
    void Update(const RadarPointVector& points, const elimaloc::Vector3d&) { AddPoints(points); } // vhm.cpp:268
    // `out` becomes this map after AddPoints(points), built on the device (elm_map_build_device): this map stays as it is and resident,
    // and only `points` cross the bus.  (Filled in place: a map owns device memory and is not copied.)
    void Updated(const RadarPointVector& points, VoxelHashMap& out) const {
        std::vector<float> xyz(3 * points.size());
        for (size_t i = 0; i < points.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)points[i].pose(k);
        Derive(nullptr, xyz.data(), points.size(), out);
    }
    // `out` becomes the device build (elm_map_build_device_from) of this map's stored points -- all of them, or with keep_center those
    // within keep_radius of it (a closed sphere) -- followed by the scans (sensor frame, PointStruct::pose) at their poses, map <- scan
    // frame: each scan is uploaded once and transformed on the device, point = float32(R p + t); the stored points never leave HBM and
    // no drop flags exist.  stats, when given: the counts of the build.
    void UpdatedFromScans(const std::vector<RadarPointVector>& scans, const std::vector<elimaloc::Matrix4d>& poses, VoxelHashMap& out,
                          const elimaloc::Vector3d* keep_center = nullptr, double keep_radius = 0.0,
                          elm_build_sources_stats* stats = nullptr) const {
        if (scans.size() != poses.size()) elimaloc::check(ELM_ERR_INVALID, ctx(), "VoxelHashMap::UpdatedFromScans");
        std::vector<double> T(16 * poses.size());
        for (size_t h = 0; h < poses.size(); ++h)
            for (int k = 0; k < 16; ++k) T[16 * h + k] = poses[h].data()[k]; // column-major on both sides
        std::vector<elm_scan*> res(scans.size(), nullptr);
        int rc = ELM_OK;
        for (size_t j = 0; j < scans.size() && rc == ELM_OK; ++j) {
            std::vector<float> xyz(3 * scans[j].size());
            for (size_t i = 0; i < scans[j].size(); ++i)
                for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scans[j][i].pose(k);
            rc = elm_scan_upload(ctx(), xyz.data(), scans[j].size(), scans[j].size(), &res[j]);
        }
        elm_map* m = nullptr;
        if (rc == ELM_OK) {
            elm_build_sources src;
            src.base = handle();
            src.keep_within = keep_center ? 1 : 0;
            for (int k = 0; k < 3; ++k) src.keep_center[k] = keep_center ? (*keep_center)(k) : 0.0;
            src.keep_radius_m = keep_center ? keep_radius : 0.0;
            src.scans = res.data();
            src.poses16 = T.data();
            src.n_jobs = (int32_t)scans.size();
            rc = elm_map_build_device_from(ctx(), &src, voxel_size_, max_points_per_voxel_, &m, stats);
        }
        for (elm_scan* s : res)
            if (s) elm_scan_destroy(s);
        elimaloc::check(rc, ctx(), "elm_map_build_device_from");
        out.Adopt(*this, m);
    }
    void CalVoxelCovAll() { // vhm.hpp:183-193
        want_voxel_cov_ = true;
        elimaloc::check(elm_map_cal_voxel_cov_all(handle()), ctx(), "CalVoxelCovAll");
    }
    void CalPointCovAll(double d_search_dist) { // vhm.hpp:252-257
        want_point_cov_ = d_search_dist;
        elimaloc::check(elm_map_cal_point_cov_all(handle(), d_search_dist), ctx(), "CalPointCovAll");
    }
    inline Voxel PointToVoxel(const elimaloc::Vector3d& point, const double voxel_size) const { // vhm.hpp:176-180
        return Voxel(static_cast<int>(std::floor(point.x() / voxel_size)), static_cast<int>(std::floor(point.y() / voxel_size)),
                     static_cast<int>(std::floor(point.z() / voxel_size)));
    }
    // vhm.hpp:260-283: the first point of every floor-keyed voxel.  The reference emits unordered_map iteration order (only
    // the set is contractual); here the kept points come back in input order.
    inline std::vector<PointStruct> VoxelDownsample(const std::vector<PointStruct>& points, const double voxel_size) const {
        std::vector<float> xyz(3 * points.size());
        for (size_t i = 0; i < points.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)points[i].pose(k);
        std::vector<int64_t> keep(points.size());
        size_t n_keep = 0;
        elimaloc::check(elm_voxel_downsample(xyz.data(), points.size(), voxel_size, keep.data(), &n_keep), ctx(), "VoxelDownsample");
        std::vector<PointStruct> points_downsampled;
        points_downsampled.reserve(n_keep);
        for (size_t k = 0; k < n_keep; ++k) points_downsampled.emplace_back(points[(size_t)keep[k]]);
        return points_downsampled;
    }
    inline bool Empty() const { return elm_map_empty(handle()) != 0; } // vhm.hpp:325
    inline void Clear() { // vhm.hpp:324
        Release();
        xyz_.clear();
        derived_ = false;
    }
    std::vector<PointStruct> Pointcloud() const { // vhm.cpp:245-255
        elm_map_info mi;
        elimaloc::check(elm_map_get_info(handle(), &mi), ctx(), "elm_map_get_info");
        std::vector<double> xyz(3 * mi.n_points), cov(9 * mi.n_points), mean(3 * mi.n_points);
        elimaloc::check(elm_map_download_points(handle(), xyz.data(), cov.data(), mean.data(), mi.n_points), ctx(), "Pointcloud");
        std::vector<PointStruct> out(mi.n_points);
        for (size_t i = 0; i < out.size(); ++i) {
            for (int k = 0; k < 3; ++k) {
                out[i].pose(k) = out[i].local(k) = xyz[3 * i + k];
                out[i].covariance.mean(k) = mean[3 * i + k];
            }
            for (int k = 0; k < 9; ++k) out[i].covariance.cov.data()[k] = cov[9 * i + k]; // both column-major
        }
        return out;
    }
    std::vector<CovStruct> Covariances() const { // vhm.cpp:257-265: voxels holding more than 2 points
        elm_map_info mi;
        elimaloc::check(elm_map_get_info(handle(), &mi), ctx(), "elm_map_get_info");
        std::vector<int32_t> npts(mi.n_voxels);
        std::vector<double> cov(9 * mi.n_voxels), mean(3 * mi.n_voxels);
        elimaloc::check(elm_map_download_voxels(handle(), nullptr, npts.data(), cov.data(), mean.data(), mi.n_voxels), ctx(), "Covariances");
        std::vector<CovStruct> out;
        for (size_t v = 0; v < mi.n_voxels; ++v)
            if (npts[v] > 2) {
                CovStruct c;
                for (int k = 0; k < 9; ++k) c.cov.data()[k] = cov[9 * v + k];
                for (int k = 0; k < 3; ++k) c.mean(k) = mean[3 * v + k];
                out.push_back(c);
            }
        return out;
    }
    // vhm.cpp:31-88 / 90-151 / 153-206: the correspondence calls of the reference's public interface.  RunRegister never needs them
    // here (its iterations search and accumulate in one kernel); a caller that wants the pairs themselves gets them from the same
    // search (elm_map_get_correspondences), in input order like the reference's vectors.  Source points are copied whole (every
    // PointStruct member), targets carry pose / local / covariance of the matched map point (or voxel); a point without any
    // neighbour bucket pairs with the default-constructed target when the origin is within range (vhm.cpp:37 / :105).
    std::tuple<std::vector<PointStruct>, std::vector<PointStruct>> GetCorrespondencePoints(const RadarPointVector& vec_points,
                                                                                           double d_max_correspondence_dist) const {
        std::vector<uint32_t> src;
        std::vector<int32_t> tgt;
        Pairs(0, vec_points, d_max_correspondence_dist, src, tgt);
        const std::vector<PointStruct> cloud = tgt.empty() ? std::vector<PointStruct>() : Pointcloud();
        std::vector<PointStruct> vec_source, vec_target;
        vec_source.reserve(src.size());
        vec_target.reserve(src.size());
        for (size_t k = 0; k < src.size(); ++k) {
            vec_source.emplace_back(vec_points[src[k]]);
            vec_target.emplace_back(tgt[k] >= 0 ? cloud[(size_t)tgt[k]] : PointStruct());
        }
        return std::make_tuple(std::move(vec_source), std::move(vec_target));
    }
    std::tuple<std::vector<PointStruct>, std::vector<CovStruct>> GetCorrespondencesCov(const RadarPointVector& vec_points,
                                                                                      double d_max_correspondence_dist) const {
        return CovPairs(1, vec_points, d_max_correspondence_dist);
    }
    std::tuple<std::vector<PointStruct>, std::vector<CovStruct>> GetCorrespondencesAllCov(const RadarPointVector& vec_points,
                                                                                         double d_max_correspondence_dist) const {
        return CovPairs(2, vec_points, d_max_correspondence_dist);
    }
    // vhm.cpp:208-243: key arithmetic only (whether or not such voxels exist): range 0 the voxel itself, 1 the seven
    // (0, +x, -x, +y, -y, +z, -z), anything else the 27 of the 3 x 3 x 3 block, x slowest
    std::vector<Voxel> GetAdjacentVoxels(const PointStruct& point, int range) const {
        const Voxel voxel = PointToVoxel(point.pose, voxel_size_);
        const int vx = voxel(0), vy = voxel(1), vz = voxel(2);
        if (range == 0) return std::vector<Voxel>{voxel};
        if (range == 1)
            return std::vector<Voxel>{Voxel(vx, vy, vz), Voxel(vx + 1, vy, vz), Voxel(vx - 1, vy, vz), Voxel(vx, vy + 1, vz),
                                      Voxel(vx, vy - 1, vz), Voxel(vx, vy, vz + 1), Voxel(vx, vy, vz - 1)};
        std::vector<Voxel> voxels;
        voxels.reserve(27);
        for (int i = vx - 1; i < vx + 2; ++i)
            for (int j = vy - 1; j < vy + 2; ++j)
                for (int k = vz - 1; k < vz + 2; ++k) voxels.emplace_back(i, j, k);
        return voxels;
    }
    // `out` becomes a map of this map's voxel size and cap, built by the usual build from this map's stored points followed by the points
    // of the cells that `growth` (a MapGrowth of this map) calls appeared, in cell order: the spacing rule and the voxel cap apply to them.
    // (Filled in place: a map owns device memory and is not copied.)  device: the same map by the device build; only the appeared points
    // cross the bus.
    inline void WithAppeared(const MapGrowth& growth, VoxelHashMap& out, const GrowthRule& rule = GrowthRule(), bool device = false) const;
    // `out` becomes a map of this map's voxel size and cap, built by the usual build from the stored points that `evidence` (a MapEvidence
    // of this map) does not call stale.  device: the same map by the device build; only the flags cross the bus.
    inline void WithoutStale(const MapEvidence& evidence, VoxelHashMap& out, const EvidenceRule& rule = EvidenceRule(), bool device = false) const;

    inline bool FindGroundHeight(const elimaloc::Vector2d& position, double& ground_z) const { // vhm.hpp:285-322
        int found = 0;
        elimaloc::check(elm_map_find_ground_height(handle(), position(0), position(1), &ground_z, &found), ctx(), "FindGroundHeight");
        return found != 0;
    }

    // FindGroundHeight of many xy positions in one device call (elm_map_ground_heights; bit for bit the single query): z = 0 where not found
    inline void FindGroundHeights(const std::vector<double>& xy, std::vector<double>& ground_z, std::vector<int32_t>& found) const {
        const size_t n = xy.size() / 2;
        ground_z.assign(n, 0.0);
        found.assign(n, 0);
        elimaloc::check(elm_map_ground_heights(ctx(), handle(), xy.data(), n, ground_z.data(), found.data()), ctx(), "FindGroundHeights");
    }

    // Free-space check of a scan (sensor frame, PointStruct::pose) at poses (elm_map_check_free_space): per pose the counted rays, those
    // that pass through occupied fine cells of the map before their end point, the end points in / next to an occupied cell.  A pose whose
    // rays pierce the map is a wrong pose -- or, at a trusted pose, a changed map.  hits (optional): the occupied samples of every ray,
    // [pose][point] in the resident scan's order.
    inline std::vector<elm_freespace_stats> CheckFreeSpace(const RadarPointVector& scan, const std::vector<elimaloc::Matrix4d>& poses,
                                                           const FreeSpaceConfig& config = FreeSpaceConfig(),
                                                           std::vector<uint16_t>* hits = nullptr) const {
        std::vector<float> xyz(3 * scan.size());
        for (size_t i = 0; i < scan.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scan[i].pose(k);
        std::vector<double> T(16 * poses.size());
        for (size_t h = 0; h < poses.size(); ++h)
            for (int k = 0; k < 16; ++k) T[16 * h + k] = poses[h].data()[k]; // column-major on both sides
        std::vector<elm_freespace_stats> stats(poses.size());
        if (hits) hits->assign(poses.size() * scan.size(), 0);
        elm_scan* s = nullptr;
        elimaloc::check(elm_scan_upload(ctx(), xyz.data(), scan.size(), scan.size(), &s), ctx(), "elm_scan_upload");
        const int rc = elm_map_check_free_space(ctx(), handle(), s, T.data(), (int)poses.size(), &config, stats.data(),
                                                hits && !hits->empty() ? hits->data() : nullptr);
        elm_scan_destroy(s);
        elimaloc::check(rc, ctx(), "CheckFreeSpace");
        return stats;
    }

    // The per-beam outputs of RayCast, each [pose][beam] in the resident scan's order (see elm_map_raycast)
    struct RayCastArrays {
        std::vector<double> range_in, range_out; // -1 for a beam that did not hit
        std::vector<int32_t> cell;               // x, y, z of the hit fine cell
        std::vector<uint8_t> flag;               // 0 not cast, 1 hit, 2 miss, 3 truncated
    };

    // Ray cast of the beams of a scan (sensor frame, PointStruct::pose; beam i runs from config.origin through point i) at poses
    // (elm_map_raycast): per pose the beams that hit / miss the map and, for a real scan, how its measured ranges lie to the expected
    // ones (match / through / front).  arrays (optional): the expected range interval, hit cell and flag of every beam.
    inline std::vector<elm_raycast_stats> RayCast(const RadarPointVector& scan, const std::vector<elimaloc::Matrix4d>& poses,
                                                  const RayCastConfig& config = RayCastConfig(), RayCastArrays* arrays = nullptr) const {
        std::vector<float> xyz(3 * scan.size());
        for (size_t i = 0; i < scan.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scan[i].pose(k);
        std::vector<double> T(16 * poses.size());
        for (size_t h = 0; h < poses.size(); ++h)
            for (int k = 0; k < 16; ++k) T[16 * h + k] = poses[h].data()[k]; // column-major on both sides
        std::vector<elm_raycast_stats> stats(poses.size());
        const size_t beams = poses.size() * scan.size();
        if (arrays) {
            arrays->range_in.assign(beams, -1.0);
            arrays->range_out.assign(beams, -1.0);
            arrays->cell.assign(3 * beams, 0);
            arrays->flag.assign(beams, 0);
        }
        const bool want = arrays && beams;
        elm_scan* s = nullptr;
        elimaloc::check(elm_scan_upload(ctx(), xyz.data(), scan.size(), scan.size(), &s), ctx(), "elm_scan_upload");
        const int rc = elm_map_raycast(ctx(), handle(), s, T.data(), (int)poses.size(), &config, stats.data(), want ? arrays->range_in.data() : nullptr,
                                       want ? arrays->range_out.data() : nullptr, want ? arrays->cell.data() : nullptr,
                                       want ? arrays->flag.data() : nullptr);
        elm_scan_destroy(s);
        elimaloc::check(rc, ctx(), "RayCast");
        return stats;
    }

    void Pairs(int what, const RadarPointVector& vec_points, double max_dist, std::vector<uint32_t>& src, std::vector<int32_t>& tgt) const {
        std::vector<double> xyz(3 * vec_points.size());
        for (size_t i = 0; i < vec_points.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = vec_points[i].pose(k);
        const size_t cap = vec_points.size() * (what == 2 ? 7 : 1);
        src.resize(cap);
        tgt.resize(cap);
        size_t n_pairs = 0;
        elimaloc::check(elm_map_get_correspondences(ctx(), handle(), what, xyz.data(), vec_points.size(), max_dist, src.data(), tgt.data(), cap, &n_pairs),
                        ctx(), "elm_map_get_correspondences");
        src.resize(n_pairs);
        tgt.resize(n_pairs);
    }
    std::tuple<std::vector<PointStruct>, std::vector<CovStruct>> CovPairs(int what, const RadarPointVector& vec_points, double max_dist) const {
        std::vector<uint32_t> src;
        std::vector<int32_t> tgt;
        Pairs(what, vec_points, max_dist, src, tgt);
        elm_map_info mi;
        elimaloc::check(elm_map_get_info(handle(), &mi), ctx(), "elm_map_get_info");
        std::vector<double> cov(9 * mi.n_voxels), mean(3 * mi.n_voxels);
        if (!tgt.empty()) elimaloc::check(elm_map_download_voxels(handle(), nullptr, nullptr, cov.data(), mean.data(), mi.n_voxels), ctx(), "elm_map_download_voxels");
        std::vector<PointStruct> vec_source;
        std::vector<CovStruct> vec_target;
        vec_source.reserve(src.size());
        vec_target.reserve(src.size());
        for (size_t k = 0; k < src.size(); ++k) {
            vec_source.emplace_back(vec_points[src[k]]);
            CovStruct c; // (the default: identity covariance at the origin)
            if (tgt[k] >= 0) {
                for (int q = 0; q < 9; ++q) c.cov.data()[q] = cov[9 * (size_t)tgt[k] + q]; // both column-major
                for (int q = 0; q < 3; ++q) c.mean(q) = mean[3 * (size_t)tgt[k] + q];
            }
            vec_target.push_back(c);
        }
        return std::make_tuple(std::move(vec_source), std::move(vec_target));
    }
    // the device-resident map (built lazily from the accumulated points on first use; const like the reference's read paths)
    elm_map* handle() const {
        if (!map_) {
            if (device_build_)
                elimaloc::check(elm_map_build_device(ctx(), nullptr, nullptr, xyz_.data(), xyz_.size() / 3, voxel_size_, max_points_per_voxel_, &map_), ctx(),
                                "elm_map_build_device");
            else
                elimaloc::check(elm_map_build(ctx(), xyz_.data(), xyz_.size() / 3, voxel_size_, max_points_per_voxel_, &map_), ctx(), "elm_map_build");
            if (device_index_) elimaloc::check(elm_map_set_index_build(map_, ELM_INDEX_BUILD_DEVICE), ctx(), "elm_map_set_index_build");
            if (want_voxel_cov_) elimaloc::check(elm_map_cal_voxel_cov_all(map_), ctx(), "CalVoxelCovAll");
            if (want_point_cov_ > 0) elimaloc::check(elm_map_cal_point_cov_all(map_, want_point_cov_), ctx(), "CalPointCovAll");
        }
        return map_;
    }
    static elm_ctx* ctx() { return elimaloc::default_context(); }

    double voxel_size_ = 1.0;
    int max_points_per_voxel_ = 30;

private:
    void Release() {
        if (map_) elm_map_destroy(map_);
        map_ = nullptr;
    }
    // `out` becomes the device build of this map's stored points without those that drop (one byte per stored point, nullptr: none)
    // marks, followed by the n points of xyz
    void Derive(const uint8_t* drop, const float* xyz, size_t n, VoxelHashMap& out) const {
        elm_map* m = nullptr;
        elimaloc::check(elm_map_build_device(ctx(), handle(), drop, xyz, n, voxel_size_, max_points_per_voxel_, &m), ctx(), "elm_map_build_device");
        out.Adopt(*this, m);
    }
    // this map becomes m, a device build made from `from`: its sizes and build preferences
    void Adopt(const VoxelHashMap& from, elm_map* m) {
        const double vs = from.voxel_size_;
        const int cap = from.max_points_per_voxel_;
        const bool db = from.device_build_, di = from.device_index_;
        Clear();
        Init(vs, cap);
        device_build_ = db;
        device_index_ = di;
        map_ = m;
        derived_ = true;
        if (device_index_) elimaloc::check(elm_map_set_index_build(m, ELM_INDEX_BUILD_DEVICE), ctx(), "elm_map_set_index_build");
    }
    // a map made by Derive holds no input points: before it takes more, its stored points (which replay to themselves) become its input
    void Materialize() {
        if (!derived_) return;
        elm_map_info mi;
        elimaloc::check(elm_map_get_info(map_, &mi), ctx(), "elm_map_get_info");
        std::vector<double> xyz(3 * mi.n_points);
        if (mi.n_points) elimaloc::check(elm_map_download_points(map_, xyz.data(), nullptr, nullptr, mi.n_points), ctx(), "elm_map_download_points");
        xyz_.assign(xyz.begin(), xyz.end()); // stored coordinates are float32 values: the conversion is exact
        derived_ = false;
    }
    std::vector<float> xyz_;
    mutable elm_map* map_ = nullptr;
    bool device_build_ = false;
    bool device_index_ = false;
    bool derived_ = false;
    bool want_voxel_cov_ = false;
    double want_point_cov_ = -1.0;
};

// Map change evidence (include/elimaloc_hip.h, map evidence): per occupied fine cell of a map the beams seen through it and the beams that
// ended in it, kept on the device and fed with scans at trusted poses.  It is bound to the map as built when it is made: destroy it
// before the map, and do not use it after the map has taken more points.
class MapEvidence {
public:
    using RadarPointVector = VoxelHashMap::RadarPointVector;
    explicit MapEvidence(const VoxelHashMap& map, int sub = 4) : sub_(sub) {
        elimaloc::check(elm_evidence_create(VoxelHashMap::ctx(), map.handle(), sub, &ev_), VoxelHashMap::ctx(), "elm_evidence_create");
    }
    MapEvidence(const MapEvidence&) = delete; // owns device memory
    MapEvidence& operator=(const MapEvidence&) = delete;
    ~MapEvidence() { elm_evidence_destroy(ev_); }

    // One observation per scan (sensor frame, PointStruct::pose) at its pose, all in one launch (elm_evidence_accumulate_batch): the
    // statistics of every observation.  config.sub is set to this object's.
    inline std::vector<elm_evidence_stats> Accumulate(const std::vector<RadarPointVector>& scans, const std::vector<elimaloc::Matrix4d>& poses,
                                                      EvidenceConfig config = EvidenceConfig()) {
        config.sub = sub_;
        std::vector<elm_evidence_stats> stats(scans.size());
        if (scans.empty() || scans.size() != poses.size()) {
            elimaloc::check(scans.empty() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "MapEvidence::Accumulate");
            return stats;
        }
        std::vector<double> T(16 * poses.size());
        for (size_t h = 0; h < poses.size(); ++h)
            for (int k = 0; k < 16; ++k) T[16 * h + k] = poses[h].data()[k]; // column-major on both sides
        std::vector<elm_scan*> res(scans.size(), nullptr);
        int rc = ELM_OK;
        for (size_t j = 0; j < scans.size() && rc == ELM_OK; ++j) {
            std::vector<float> xyz(3 * scans[j].size());
            for (size_t i = 0; i < scans[j].size(); ++i)
                for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scans[j][i].pose(k);
            rc = elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scans[j].size(), scans[j].size(), &res[j]);
        }
        if (rc == ELM_OK) rc = elm_evidence_accumulate_batch(VoxelHashMap::ctx(), ev_, res.data(), T.data(), (int)scans.size(), &config, stats.data());
        for (elm_scan* s : res)
            if (s) elm_scan_destroy(s);
        elimaloc::check(rc, VoxelHashMap::ctx(), "MapEvidence::Accumulate");
        return stats;
    }
    inline elm_evidence_stats Accumulate(const RadarPointVector& scan, const elimaloc::Matrix4d& pose, const EvidenceConfig& config = EvidenceConfig()) {
        return Accumulate(std::vector<RadarPointVector>(1, scan), std::vector<elimaloc::Matrix4d>(1, pose), config)[0];
    }

    // The counters, entry for entry with elm_map_fine_cells(map, sub)
    inline void Counts(std::vector<uint32_t>& through, std::vector<uint32_t>& hit) const {
        size_t n = 0;
        elimaloc::check(elm_evidence_counts(VoxelHashMap::ctx(), ev_, nullptr, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_evidence_counts");
        through.assign(n, 0);
        hit.assign(n, 0);
        if (n) elimaloc::check(elm_evidence_counts(VoxelHashMap::ctx(), ev_, through.data(), hit.data(), n, &n), VoxelHashMap::ctx(), "elm_evidence_counts");
    }

    // One flag per stored point (elm_map_download_points order): 1 when its fine cell is stale by the rule
    inline std::vector<uint8_t> StalePoints(const EvidenceRule& rule = EvidenceRule()) const {
        size_t n = 0;
        elimaloc::check(elm_evidence_stale_points(VoxelHashMap::ctx(), ev_, &rule, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_evidence_stale_points");
        std::vector<uint8_t> flags(n, 0);
        if (n) elimaloc::check(elm_evidence_stale_points(VoxelHashMap::ctx(), ev_, &rule, flags.data(), n, &n), VoxelHashMap::ctx(), "elm_evidence_stale_points");
        return flags;
    }

    inline void Reset() { elimaloc::check(elm_evidence_reset(VoxelHashMap::ctx(), ev_), VoxelHashMap::ctx(), "elm_evidence_reset"); }

private:
    elm_evidence* ev_ = nullptr;
    int sub_ = 4;
};

// Map growth (include/elimaloc_hip.h, map growth): per candidate fine cell -- a cell the map does not occupy and in which beams ended --
// the beams that ended in it, the beams that later passed through it and where in it the end points lay, kept on the device and fed with
// scans at trusted poses.  It is bound to the map as built when it is made: destroy it before the map, and do not use it after the map
// has taken more points.  capacity: the most candidate cells it holds; a call needs room for one candidate per beam.
class MapGrowth {
public:
    using RadarPointVector = VoxelHashMap::RadarPointVector;
    MapGrowth(const VoxelHashMap& map, size_t capacity, int sub = 4) : sub_(sub) {
        elimaloc::check(elm_growth_create(VoxelHashMap::ctx(), map.handle(), sub, capacity, &g_), VoxelHashMap::ctx(), "elm_growth_create");
    }
    MapGrowth(const MapGrowth&) = delete; // owns device memory
    MapGrowth& operator=(const MapGrowth&) = delete;
    ~MapGrowth() { elm_growth_destroy(g_); }

    // One observation per scan (sensor frame, PointStruct::pose) at its pose, all in ONE call (elm_growth_accumulate_batch): the end points
    // of all scans are recorded before any beam walks.  The statistics of every observation.  config.sub is set to this object's.
    inline std::vector<elm_growth_stats> Accumulate(const std::vector<RadarPointVector>& scans, const std::vector<elimaloc::Matrix4d>& poses,
                                                    GrowthConfig config = GrowthConfig()) {
        config.sub = sub_;
        std::vector<elm_growth_stats> stats(scans.size());
        if (scans.empty() || scans.size() != poses.size()) {
            elimaloc::check(scans.empty() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "MapGrowth::Accumulate");
            return stats;
        }
        std::vector<double> T(16 * poses.size());
        for (size_t h = 0; h < poses.size(); ++h)
            for (int k = 0; k < 16; ++k) T[16 * h + k] = poses[h].data()[k]; // column-major on both sides
        std::vector<elm_scan*> res(scans.size(), nullptr);
        int rc = ELM_OK;
        for (size_t j = 0; j < scans.size() && rc == ELM_OK; ++j) {
            std::vector<float> xyz(3 * scans[j].size());
            for (size_t i = 0; i < scans[j].size(); ++i)
                for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scans[j][i].pose(k);
            rc = elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scans[j].size(), scans[j].size(), &res[j]);
        }
        if (rc == ELM_OK) rc = elm_growth_accumulate_batch(VoxelHashMap::ctx(), g_, res.data(), T.data(), (int)scans.size(), &config, stats.data());
        for (elm_scan* s : res)
            if (s) elm_scan_destroy(s);
        elimaloc::check(rc, VoxelHashMap::ctx(), "MapGrowth::Accumulate");
        return stats;
    }
    inline elm_growth_stats Accumulate(const RadarPointVector& scan, const elimaloc::Matrix4d& pose, const GrowthConfig& config = GrowthConfig()) {
        return Accumulate(std::vector<RadarPointVector>(1, scan), std::vector<elimaloc::Matrix4d>(1, pose), config)[0];
    }

    // The candidate cells in ascending (x, y, z) order: cells3 [n][3], hit [n], through [n], sums3 [n][3]
    inline void Cells(std::vector<int32_t>& cells3, std::vector<uint32_t>& hit, std::vector<uint32_t>& through, std::vector<uint64_t>& sums3) const {
        size_t n = 0;
        elimaloc::check(elm_growth_cells(VoxelHashMap::ctx(), g_, nullptr, nullptr, nullptr, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_growth_cells");
        cells3.assign(3 * n, 0);
        hit.assign(n, 0);
        through.assign(n, 0);
        sums3.assign(3 * n, 0);
        if (n)
            elimaloc::check(elm_growth_cells(VoxelHashMap::ctx(), g_, cells3.data(), hit.data(), through.data(), sums3.data(), n, &n),
                            VoxelHashMap::ctx(), "elm_growth_cells");
    }

    // The mean end point (x, y, z, float64) of every cell that the rule calls appeared, in cell order
    inline std::vector<double> AppearedPoints(const GrowthRule& rule = GrowthRule()) const {
        size_t n = 0;
        elimaloc::check(elm_growth_appeared_points(VoxelHashMap::ctx(), g_, &rule, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_growth_appeared_points");
        std::vector<double> xyz(3 * n, 0.0);
        if (n) elimaloc::check(elm_growth_appeared_points(VoxelHashMap::ctx(), g_, &rule, xyz.data(), n, &n), VoxelHashMap::ctx(), "elm_growth_appeared_points");
        return xyz;
    }

    inline void Reset() { elimaloc::check(elm_growth_reset(VoxelHashMap::ctx(), g_), VoxelHashMap::ctx(), "elm_growth_reset"); }

    // The appeared cells grouped into objects on the device (include/elimaloc_hip.h, map growth: objects).  The result is held until the
    // next Accumulate, Reset or FindObjects; Objects, CellObjects and BeamObjects read it.
    inline elm_growth_object_stats FindObjects(const GrowthObjectRule& rule = GrowthObjectRule()) {
        elm_growth_object_stats st;
        elimaloc::check(elm_growth_find_objects(VoxelHashMap::ctx(), g_, &rule, &st), VoxelHashMap::ctx(), "elm_growth_find_objects");
        return st;
    }
    // The objects in ascending label order
    inline std::vector<elm_growth_object> Objects() const {
        size_t n = 0;
        elimaloc::check(elm_growth_objects(VoxelHashMap::ctx(), g_, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_growth_objects");
        std::vector<elm_growth_object> objs(n);
        if (n) elimaloc::check(elm_growth_objects(VoxelHashMap::ctx(), g_, objs.data(), n, &n), VoxelHashMap::ctx(), "elm_growth_objects");
        return objs;
    }
    // One value per candidate cell in Cells' order: the object's index, -2 in a small component, -1 for a cell that is not a member
    inline std::vector<int32_t> CellObjects() const {
        size_t n = 0;
        elimaloc::check(elm_growth_cell_objects(VoxelHashMap::ctx(), g_, nullptr, 0, &n), VoxelHashMap::ctx(), "elm_growth_cell_objects");
        std::vector<int32_t> obj(n, -1);
        if (n) elimaloc::check(elm_growth_cell_objects(VoxelHashMap::ctx(), g_, obj.data(), n, &n), VoxelHashMap::ctx(), "elm_growth_cell_objects");
        return obj;
    }
    // One value per beam of the scan (sensor frame, PointStruct::pose) at its pose, in the resident scan's order (the upload orders the
    // points; resident_xyz, optional, receives them in that order, packed x, y, z): the index of the object the beam ends on, -2 for a
    // small component, -1 for anything else.  config.sub is set to this object's.
    inline std::vector<int32_t> BeamObjects(const RadarPointVector& scan, const elimaloc::Matrix4d& pose, GrowthConfig config = GrowthConfig(),
                                            std::vector<float>* resident_xyz = nullptr) const {
        config.sub = sub_;
        std::vector<int32_t> obj(scan.size(), -1);
        if (resident_xyz) resident_xyz->assign(3 * scan.size(), 0.0f);
        if (scan.empty()) return obj;
        std::vector<float> xyz(3 * scan.size());
        for (size_t i = 0; i < scan.size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = (float)scan[i].pose(k);
        elm_scan* res = nullptr;
        int rc = elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scan.size(), scan.size(), &res);
        if (rc == ELM_OK) rc = elm_growth_beam_objects(VoxelHashMap::ctx(), g_, res, pose.data(), &config, obj.data());
        if (rc == ELM_OK && resident_xyz) rc = elm_scan_download(res, resident_xyz->data(), scan.size());
        if (res) elm_scan_destroy(res);
        elimaloc::check(rc, VoxelHashMap::ctx(), "MapGrowth::BeamObjects");
        return obj;
    }

private:
    elm_growth* g_ = nullptr;
    int sub_ = 4;
};

inline void VoxelHashMap::WithoutStale(const MapEvidence& evidence, VoxelHashMap& out, const EvidenceRule& rule, bool device) const {
    const std::vector<uint8_t> flags = evidence.StalePoints(rule);
    if (device) {
        Derive(flags.data(), nullptr, 0, out);
        return;
    }
    std::vector<double> xyz(3 * flags.size());
    if (!flags.empty()) elimaloc::check(elm_map_download_points(handle(), xyz.data(), nullptr, nullptr, flags.size()), ctx(), "WithoutStale");
    std::vector<float> f;
    for (size_t i = 0; i < flags.size(); ++i)
        if (!flags[i])
            for (int k = 0; k < 3; ++k) f.push_back((float)xyz[3 * i + k]); // stored coordinates are float32 values: their conversion is exact
    out.Clear();
    out.Init(voxel_size_, max_points_per_voxel_);
    out.AddPoints(f.data(), f.size() / 3);
}

inline void VoxelHashMap::WithAppeared(const MapGrowth& growth, VoxelHashMap& out, const GrowthRule& rule, bool device) const {
    const std::vector<double> fresh = growth.AppearedPoints(rule);
    if (device) {
        const std::vector<float> f(fresh.begin(), fresh.end());
        Derive(nullptr, f.data(), f.size() / 3, out);
        return;
    }
    elm_map_info mi;
    elimaloc::check(elm_map_get_info(handle(), &mi), ctx(), "elm_map_get_info");
    std::vector<double> xyz(3 * mi.n_points), cov(9 * mi.n_points), mean(3 * mi.n_points);
    if (mi.n_points) elimaloc::check(elm_map_download_points(handle(), xyz.data(), cov.data(), mean.data(), mi.n_points), ctx(), "WithAppeared");
    xyz.insert(xyz.end(), fresh.begin(), fresh.end());
    std::vector<float> f(xyz.size());
    for (size_t i = 0; i < xyz.size(); ++i) f[i] = (float)xyz[i]; // stored coordinates are float32 values: their conversion is exact
    out.Clear();
    out.Init(voxel_size_, max_points_per_voxel_);
    out.AddPoints(f.data(), f.size() / 3);
}
