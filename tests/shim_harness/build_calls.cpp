// Call lines of the device-map-build part of the C++ shim (include/elimaloc/voxel_hash_map.hpp: VoxelHashMap::BuildOnDevice, Updated,
// WithoutStale and WithAppeared with their trailing `device`), compiled by tests/test_map_build_device_abi.py as
// tests/shim_harness/objects_calls.cpp is: the Eigen-typed form against tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run
// without an argument it touches no device.
#include "registration.hpp"

// a map built on the device, updated with a scan's points, pruned by the evidence and grown by the growth of one replayed scan: the
// points the four maps hold
size_t points_after_edits(const std::vector<PointStruct>& cloud, const std::vector<PointStruct>& scan, const Eigen::Matrix4d& pose) {
    VoxelHashMap map(1.0, 30);
    map.BuildOnDevice(true);
    map.AddPoints(cloud);
    VoxelHashMap updated, pruned, pruned_host, grown, grown_host;
    map.Updated(scan, updated);
    MapEvidence evidence(map, 4);
    evidence.Accumulate(scan, pose);
    map.WithoutStale(evidence, pruned, EvidenceRule(), true);
    map.WithoutStale(evidence, pruned_host);
    MapGrowth growth(map, 1u << 16, 4);
    growth.Accumulate(scan, pose);
    map.WithAppeared(growth, grown, GrowthRule(), true);
    map.WithAppeared(growth, grown_host);
    updated.AddPoints(scan); // a map made on the device path takes more points like any other
    return updated.Pointcloud().size() + pruned.Pointcloud().size() + pruned_host.Pointcloud().size() + grown.Pointcloud().size() +
           grown_host.Pointcloud().size();
}

int main(int argc, char**) {
    if (argc > 1) return (int)points_after_edits(std::vector<PointStruct>(1), std::vector<PointStruct>(1), Eigen::Matrix4d::Identity());
    return 0;
}
