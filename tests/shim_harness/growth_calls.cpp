// Call lines of the map-growth part of the C++ shim (include/elimaloc/voxel_hash_map.hpp: GrowthConfig, GrowthRule, MapGrowth,
// VoxelHashMap::WithAppeared), compiled by tests/test_growth_abi.py as tests/shim_harness/pcm_calls.cpp is: the Eigen-typed form against
// tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device.
#include "registration.hpp"

// a replayed trajectory accumulated on the map in one call, then the map grown by what the default rule calls appeared: the number of
// stored points the new map gained
size_t grown_by(const std::vector<std::vector<PointStruct>>& scans, const std::vector<Eigen::Matrix4d>& poses, const VoxelHashMap& map,
                VoxelHashMap& grown) {
    MapGrowth growth(map, 1u << 20, 4);
    GrowthConfig cfg;
    cfg.clearance_cells = 2;
    cfg.end_margin_frac = 0.25;
    cfg.origin[2] = 0.1;
    const std::vector<elm_growth_stats> st = growth.Accumulate(scans, poses, cfg);
    const elm_growth_stats one = growth.Accumulate(scans[0], poses[0]);
    std::vector<int32_t> cells3;
    std::vector<uint32_t> hit, through;
    std::vector<uint64_t> sums3;
    growth.Cells(cells3, hit, through, sums3);
    GrowthRule rule;
    rule.min_hit = 5;
    const std::vector<double> strict = growth.AppearedPoints(rule);
    const std::vector<double> dflt = growth.AppearedPoints();
    map.WithAppeared(growth, grown, rule);
    map.WithAppeared(growth, grown);
    growth.Reset();
    const size_t before = map.Pointcloud().size(), after = grown.Pointcloud().size();
    return after - before + 0 * (st.size() + one.n_end_new + one.n_dropped + cells3.size() + hit.size() + through.size() + sums3.size() +
                                 strict.size() + dflt.size());
}

int main(int argc, char**) {
    if (argc > 1) {
        std::vector<std::vector<PointStruct>> s(1);
        VoxelHashMap m, grown;
        return (int)grown_by(s, std::vector<Eigen::Matrix4d>(1, Eigen::Matrix4d::Identity()), m, grown);
    }
    return 0;
}
