// Call lines of the growth-objects part of the C++ shim (include/elimaloc/voxel_hash_map.hpp: GrowthObjectRule, MapGrowth::FindObjects,
// Objects, CellObjects, BeamObjects), compiled by tests/test_growth_objects_abi.py as tests/shim_harness/growth_calls.cpp is: the
// Eigen-typed form against tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device.
#include "registration.hpp"

// a replayed trajectory accumulated on the map in one call, the appeared cells grouped into objects of at least five cells, and the beams
// of the first scan that end on the largest of them
size_t beams_on_largest(const std::vector<std::vector<PointStruct>>& scans, const std::vector<Eigen::Matrix4d>& poses, const VoxelHashMap& map) {
    MapGrowth growth(map, 1u << 20, 4);
    GrowthConfig cfg;
    growth.Accumulate(scans, poses, cfg);
    GrowthObjectRule rule;
    rule.connectivity = 18;
    rule.min_cells = 5;
    const elm_growth_object_stats st = growth.FindObjects(rule);
    const elm_growth_object_stats dflt = growth.FindObjects();
    const std::vector<elm_growth_object> objs = growth.Objects();
    const std::vector<int32_t> of_cell = growth.CellObjects();
    std::vector<float> resident;
    const std::vector<int32_t> of_beam = growth.BeamObjects(scans[0], poses[0], cfg, &resident);
    const std::vector<int32_t> again = growth.BeamObjects(scans[0], poses[0]);
    int32_t largest = -1;
    for (size_t k = 0; k < objs.size(); ++k)
        if (largest < 0 || objs[k].n_cells > objs[(size_t)largest].n_cells) largest = (int32_t)k;
    size_t n = 0;
    for (int32_t v : of_beam) n += largest >= 0 && v == largest;
    return n + 0 * (st.n_members + st.n_small + st.n_small_cells + dflt.n_objects + dflt.max_cells + of_cell.size() + resident.size() + again.size() +
                    (objs.empty() ? 0 : (size_t)(objs[0].label[0] + objs[0].lo[1] + objs[0].hi[2]) + objs[0].hit + objs[0].through + objs[0].cell_sum[0]));
}

int main(int argc, char**) {
    if (argc > 1) {
        std::vector<std::vector<PointStruct>> s(1);
        VoxelHashMap m;
        return (int)beams_on_largest(s, std::vector<Eigen::Matrix4d>(1, Eigen::Matrix4d::Identity()), m);
    }
    return 0;
}
