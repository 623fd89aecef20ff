// loop_consistency.hpp -- loop closing: the largest set of mutually consistent loop measurements (include/elimaloc_hip_loops.h), the C++
// face of elm_loops_consistency in the shim's types.  It runs before a PoseGraph sees the loops: keep the members, add only them.
#pragma once
#include <vector>

#include "registration.hpp"

struct LoopMeasurement {
    int a = 0, b = 1;
    elimaloc::Matrix4d Z = elimaloc::Matrix4d::Identity(); // ~ T_a^-1 T_b
    double var_t = 1.0, var_r = 1.0;                       // m^2, rad^2
};

struct LoopConsistencyResult {
    elm_loops_result result;
    std::vector<uint8_t> member; // [loops]: 1 for a member of the clique
    std::vector<int32_t> degree; // [loops]: the loop's consistent partners
    std::vector<int> members() const {
        std::vector<int> out;
        for (size_t k = 0; k < member.size(); ++k)
            if (member[k]) out.push_back((int)k);
        return out;
    }
};

// poses: the odometry chain in index order.  config: NULL for the defaults (gamma 16.81, q_t = q_r = 0).
inline LoopConsistencyResult LoopConsistency(const std::vector<elimaloc::Matrix4d>& poses, const std::vector<LoopMeasurement>& loops,
                                             const elm_loops_config* config = nullptr) {
    elm_loops_config c;
    elm_loops_config_default(&c);
    if (config) c = *config;
    const size_t n = poses.size(), L = loops.size();
    std::vector<double> P(16 * n + 1), Z(16 * L + 1), vt(L + 1), vr(L + 1);
    std::vector<int32_t> a(L + 1), b(L + 1);
    for (size_t v = 0; v < n; ++v)
        for (int q = 0; q < 16; ++q) P[16 * v + (size_t)q] = poses[v].data()[q];
    for (size_t k = 0; k < L; ++k) {
        a[k] = loops[k].a;
        b[k] = loops[k].b;
        vt[k] = loops[k].var_t;
        vr[k] = loops[k].var_r;
        for (int q = 0; q < 16; ++q) Z[16 * k + (size_t)q] = loops[k].Z.data()[q];
    }
    LoopConsistencyResult out;
    out.member.assign(L + 1, 0);
    out.degree.assign(L + 1, 0);
    elimaloc::check(elm_loops_consistency(VoxelHashMap::ctx(), P.data(), n, a.data(), b.data(), Z.data(), vt.data(), vr.data(), L, &c, &out.result,
                                          out.member.data(), out.degree.data(), nullptr, nullptr),
                    VoxelHashMap::ctx(), "elm_loops_consistency");
    out.member.pop_back();
    out.degree.pop_back();
    return out;
}

// host only: e[6] of one pair, loop k = (Ta, Tb, Zk) predicted from loop l = (Tc, Td, Zl)
inline void LoopPairTerms(const elimaloc::Matrix4d& Ta, const elimaloc::Matrix4d& Tb, const elimaloc::Matrix4d& Zk, const elimaloc::Matrix4d& Tc,
                          const elimaloc::Matrix4d& Td, const elimaloc::Matrix4d& Zl, double* e) {
    elimaloc::check(elm_loops_pair_terms(Ta.data(), Tb.data(), Zk.data(), Tc.data(), Td.data(), Zl.data(), e), nullptr, "elm_loops_pair_terms");
}
