// loop_covariance.hpp -- loop closing under a propagated covariance (include/elimaloc_hip_loopcov.h): the C++ face of elm_loopcov_chain and
// elm_loopcov_consistency in the shim's types.  Covariances are 6 x 6 in the order [translation; rotation]; they are symmetric, so their
// storage order does not matter.
#pragma once
#include <vector>

#include "loop_consistency.hpp"

struct LoopMeasurementCov {
    int a = 0, b = 1;
    elimaloc::Matrix4d Z = elimaloc::Matrix4d::Identity();     // ~ T_a^-1 T_b
    elimaloc::Matrix6d cov = elimaloc::Matrix6d::Identity();   // of xi in Z = X_true (+) xi
};

struct LoopConsistencyCovResult {
    elm_loopcov_result result;
    std::vector<uint8_t> member; // [loops]: 1 for a member of the clique
    std::vector<int32_t> degree; // [loops]: the loop's consistent partners
    std::vector<int> members() const {
        std::vector<int> out;
        for (size_t k = 0; k < member.size(); ++k)
            if (member[k]) out.push_back((int)k);
        return out;
    }
};

namespace loop_covariance_detail {
inline std::vector<double> flat(const std::vector<elimaloc::Matrix4d>& poses) {
    std::vector<double> P(16 * poses.size() + 1);
    for (size_t v = 0; v < poses.size(); ++v)
        for (int q = 0; q < 16; ++q) P[16 * v + (size_t)q] = poses[v].data()[q];
    return P;
}
inline std::vector<double> flat(const std::vector<elimaloc::Matrix6d>& mats) {
    std::vector<double> M(36 * mats.size() + 1);
    for (size_t v = 0; v < mats.size(); ++v)
        for (int q = 0; q < 36; ++q) M[36 * v + (size_t)q] = mats[v].data()[q];
    return M;
}
} // namespace loop_covariance_detail

// W[v]: the covariance of the odometry from pose 0 to pose v in the frame of pose 0.  Q: one covariance for every step, or one per step
// (poses.size() - 1 of them).  local (when not NULL) takes S[v], the same in v's own tangent.
inline std::vector<elimaloc::Matrix6d> ChainCovariance(const std::vector<elimaloc::Matrix4d>& poses, const std::vector<elimaloc::Matrix6d>& Q,
                                                       std::vector<elimaloc::Matrix6d>* local = nullptr) {
    const size_t n = poses.size();
    const std::vector<double> P = loop_covariance_detail::flat(poses), Qf = loop_covariance_detail::flat(Q);
    std::vector<double> W(36 * n + 1), S(local ? 36 * n + 1 : 0);
    elimaloc::check(elm_loopcov_chain(VoxelHashMap::ctx(), P.data(), n, Qf.data(), Q.size(), W.data(), local ? S.data() : nullptr), VoxelHashMap::ctx(),
                    "elm_loopcov_chain");
    std::vector<elimaloc::Matrix6d> out(n);
    if (local) local->resize(n);
    for (size_t v = 0; v < n; ++v)
        for (int q = 0; q < 36; ++q) {
            out[v].data()[q] = W[36 * v + (size_t)q];
            if (local) (*local)[v].data()[q] = S[36 * v + (size_t)q];
        }
    return out;
}

// poses: the odometry chain in index order.  config: NULL for the defaults (gamma 16.81); its q_t and q_r stay 0.
inline LoopConsistencyCovResult LoopConsistencyCov(const std::vector<elimaloc::Matrix4d>& poses, const std::vector<LoopMeasurementCov>& loops,
                                                   const std::vector<elimaloc::Matrix6d>& Q, const elm_loops_config* config = nullptr) {
    elm_loops_config c;
    elm_loops_config_default(&c);
    if (config) c = *config;
    const size_t n = poses.size(), L = loops.size();
    const std::vector<double> P = loop_covariance_detail::flat(poses), Qf = loop_covariance_detail::flat(Q);
    std::vector<double> Z(16 * L + 1), Sg(36 * L + 1);
    std::vector<int32_t> a(L + 1), b(L + 1);
    for (size_t k = 0; k < L; ++k) {
        a[k] = loops[k].a;
        b[k] = loops[k].b;
        for (int q = 0; q < 16; ++q) Z[16 * k + (size_t)q] = loops[k].Z.data()[q];
        for (int q = 0; q < 36; ++q) Sg[36 * k + (size_t)q] = loops[k].cov.data()[q];
    }
    LoopConsistencyCovResult out;
    out.member.assign(L + 1, 0);
    out.degree.assign(L + 1, 0);
    elimaloc::check(elm_loopcov_consistency(VoxelHashMap::ctx(), P.data(), n, a.data(), b.data(), Z.data(), Sg.data(), L, Qf.data(), Q.size(), &c,
                                            &out.result, out.member.data(), out.degree.data(), nullptr, nullptr),
                    VoxelHashMap::ctx(), "elm_loopcov_consistency");
    out.member.pop_back();
    out.degree.pop_back();
    return out;
}
