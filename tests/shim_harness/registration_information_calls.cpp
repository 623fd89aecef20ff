// Call lines of the registration-information part of the C++ shim (include/elimaloc/registration_information.hpp: RegInfoConfig,
// RegisterInformation, InformationMatrix), compiled by tests/test_reginfo_abi.py as tests/shim_harness/growth_calls.cpp is: the Eigen-typed
// form against tests/fake_eigen, C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device.  Run as
// `registration_information_calls DIR N` (tests/test_reginfo.py) it reads DIR/map.f32 (the map's points), DIR/scan<k>.f32 and
// DIR/pose<k>.f64 (column-major) for k < N, registers the information of the N jobs in one call -- GICP on point covariances of 0.4 m, the
// plane metric, min_eigen_ratio 1e-6 -- and writes the N results as they are to DIR/results.bin.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "registration_information.hpp"

template <class T>
static std::vector<T> read_all(const std::string& path) {
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

static std::vector<elm_reginfo_result> information_of(const std::vector<VoxelHashMap::RadarPointVector>& scans, const std::vector<Eigen::Matrix4d>& poses,
                                                      const VoxelHashMap& map) {
    RegistrationConfig reg;
    reg.icp_method = IcpMethod::GICP;
    RegInfoConfig cfg;
    cfg.metric = ELM_REGINFO_METRIC_PLANE;
    cfg.min_eigen_ratio = 1e-6;
    std::vector<elm_reginfo_result> all = RegisterInformation(scans, map, poses, reg, cfg);
    const elm_reginfo_result one = RegisterInformation(scans[0], map, poses[0], reg); // the defaults: the method's metric
    const Eigen::Matrix6d info = InformationMatrix(one);
    if (info(0, 1) != info(1, 0) || one.n_points != all[0].n_points) all.clear();
    return all;
}

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    const std::string dir = argv[1];
    const int n = std::atoi(argv[2]);
    const std::vector<float> world = read_all<float>(dir + "/map.f32");
    if (world.empty() || n < 1) return 2;
    VoxelHashMap map(1.0, 30);
    map.AddPoints(world.data(), world.size() / 3);
    map.CalPointCovAll(0.4);
    std::vector<VoxelHashMap::RadarPointVector> scans((size_t)n);
    std::vector<Eigen::Matrix4d> poses((size_t)n, Eigen::Matrix4d::Identity());
    for (int k = 0; k < n; ++k) {
        const std::vector<float> xyz = read_all<float>(dir + "/scan" + std::to_string(k) + ".f32");
        const std::vector<double> T = read_all<double>(dir + "/pose" + std::to_string(k) + ".f64");
        if (xyz.empty() || T.size() != 16) return 3;
        scans[(size_t)k].resize(xyz.size() / 3);
        for (size_t i = 0; i < xyz.size() / 3; ++i)
            for (int c = 0; c < 3; ++c) scans[(size_t)k][i].pose.data()[c] = (double)xyz[3 * i + (size_t)c];
        for (int q = 0; q < 16; ++q) poses[(size_t)k].data()[q] = T[(size_t)q];
    }
    const std::vector<elm_reginfo_result> res = information_of(scans, poses, map);
    if (res.size() != (size_t)n) return 4;
    FILE* f = std::fopen((dir + "/results.bin").c_str(), "wb");
    if (!f) return 5;
    const bool ok = std::fwrite(res.data(), sizeof(elm_reginfo_result), res.size(), f) == res.size();
    std::fclose(f);
    return ok ? 0 : 6;
}
