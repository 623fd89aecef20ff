// Call lines of the device-index-build part of the C++ shim (include/elimaloc/voxel_hash_map.hpp: VoxelHashMap::BuildIndexOnDevice, alone,
// with BuildOnDevice, and on a map made by Updated), compiled by tests/test_index_build_device_abi.py as tests/shim_harness/build_calls.cpp
// is: the Eigen-typed form against tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device.
#include "registration.hpp"

// a map whose cell grid is built on the device, before and after its handle exists, and a map derived from it: the points they hold
size_t points_with_device_index(const std::vector<PointStruct>& cloud, const std::vector<PointStruct>& scan) {
    VoxelHashMap map(1.0, 30);
    map.BuildIndexOnDevice(true);
    map.AddPoints(cloud);
    VoxelHashMap both(1.0, 30);
    both.BuildOnDevice(true);
    both.AddPoints(cloud);
    const size_t built = both.Pointcloud().size(); // the handle exists now
    both.BuildIndexOnDevice(true);
    both.BuildIndexOnDevice(false);
    VoxelHashMap updated;
    map.Updated(scan, updated); // keeps the preference
    return built + map.Pointcloud().size() + updated.Pointcloud().size();
}

int main(int argc, char**) {
    if (argc > 1) return (int)points_with_device_index(std::vector<PointStruct>(1), std::vector<PointStruct>(1));
    return 0;
}
