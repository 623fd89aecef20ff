// elm_dev_loops.hpp -- the pair term of the loop consistency check (include/elimaloc_hip_loops.h): loop k predicted
// from loop l through the odometry, the pose graph's own residual of that prediction against Z_k, and the scalar s.  Host and device run
// this same code (elm_loops_pair_terms is the host's call of it).  Float64, pose rows as pose_rows12, no contraction; every sum of three
// products is the first two, then the third.
#pragma once
#include "elm_dev_pgraph.hpp"

namespace elm {

// X_uv = T_u^-1 T_v = [R_u^T R_v | R_u^T (t_v - t_u)]
ELM_HD void lc_between(const double Pu[12], const double Pv[12], double R[9], double t[3]) {
    double Ru[9], tu[3], Rv[9], tv[3];
    pg_split(Pu, Ru, tu);
    pg_split(Pv, Rv, tv);
    const double dt[3] = {tv[0] - tu[0], tv[1] - tu[1], tv[2] - tu[2]};
    pg_mul3_at(Ru, Rv, R);
    pg_mul3_atv(Ru, dt, t);
}

// [R | t] <- [R | t] [Rb | tb] = [R Rb | R tb + t]
ELM_HD void lc_compose(double R[9], double t[3], const double Rb[9], const double tb[3]) {
    double Rn[9];
    mul3(R, Rb, Rn);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = ((R[r * 3] * tb[0] + R[r * 3 + 1] * tb[1]) + R[r * 3 + 2] * tb[2]) + t[r];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = Rn[q];
}

// e of the pair (k, l): Zhat = (X_{a_k a_l} Z_l) X_{b_l b_k}, e = pg_residual(I, Zhat, Z_k)
ELM_HD void lc_pair_e(const double Pak[12], const double Pbk[12], const double PZk[12], const double Pal[12], const double Pbl[12],
                      const double PZl[12], double e[6]) {
    double R[9], t[3], Rb[9], tb[3];
    lc_between(Pak, Pal, R, t);
    pg_split(PZl, Rb, tb);
    lc_compose(R, t, Rb, tb);
    lc_between(Pbl, Pbk, Rb, tb);
    lc_compose(R, t, Rb, tb);
    const double I[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    const double Zh[12] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]};
    pg_residual(I, Zh, PZk, e);
}

// s of the pair from e, the two loops' variances and the odometry steps m of the cycle
ELM_HD double lc_pair_s(const double e[6], double vt_k, double vt_l, double vr_k, double vr_l, double m, double q_t, double q_r) {
    const double et = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], er = (e[3] * e[3] + e[4] * e[4]) + e[5] * e[5];
    return et / ((vt_k + vt_l) + q_t * m) + er / ((vr_k + vr_l) + q_r * m);
}

} // namespace elm
