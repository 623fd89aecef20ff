// elm_dev_loopcov.hpp -- the 6 x 6 arithmetic of the loop consistency check with a propagated covariance (include/elimaloc_hip_loopcov.h;
// DESIGN.md section 25): the Ad sandwich on symmetric 21-entry storage by Ad's block structure, the L D L^T quadratic form, the term of one
// chain step and the pair term.  Host and device run this same code (elm_loopcov_pair_terms is the host's call of it).  Float64, no
// contraction; every loop has constant bounds and is unrolled, so no array here is indexed by a value known only at run time.
#pragma once
#include "elm_dev_loops.hpp"

namespace elm {

constexpr int kLcvSym = 21; // the upper triangle of a symmetric 6 x 6, row by row
// the slot of entry (i, j), i <= j
ELM_HD constexpr int lcv_ix(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }
ELM_HD constexpr int lcv_sx(int i, int j) { return i <= j ? lcv_ix(i, j) : lcv_ix(j, i); }

ELM_HD void lcv_from36(const double M[36], double S[kLcvSym]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) S[lcv_ix(i, j)] = M[i * 6 + j];
}
ELM_HD void lcv_to36(const double S[kLcvSym], double M[36]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) M[i * 6 + j] = S[lcv_sx(i, j)];
}

// [R | t]^-1 = [R^T | -R^T t]
ELM_HD void lcv_inverse(const double R[9], const double t[3], double Ri[9], double ti[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Ri[i * 3 + j] = R[j * 3 + i];
    double u[3];
    pg_mul3_atv(R, t, u);
    ti[0] = -u[0];
    ti[1] = -u[1];
    ti[2] = -u[2];
}

// X K^T for K = [t]x: row i of the result is (row i of X) x (-t) ... written out: (X K^T)_ij = sum_m X_im K_jm
ELM_HD void lcv_mul_kt(const double X[9], const double t[3], double out[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i * 3] = X[i * 3 + 2] * t[1] - X[i * 3 + 1] * t[2];
        out[i * 3 + 1] = X[i * 3] * t[2] - X[i * 3 + 2] * t[0];
        out[i * 3 + 2] = X[i * 3 + 1] * t[0] - X[i * 3] * t[1];
    }
}

// R M R^T for a general 3 x 3 M
ELM_HD void lcv_rot3(const double R[9], const double M[9], double out[9]) {
    double T[9];
    mul3(R, M, T);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = (T[i * 3] * R[j * 3] + T[i * 3 + 1] * R[j * 3 + 1]) + T[i * 3 + 2] * R[j * 3 + 2];
}

// out = Ad(X) S Ad(X)^T for X = [R | t].  With S = [[A, B], [B^T, D]], A' = R A R^T and so on, K = [t]x:
//   rotation block D', cross block M = B' + K D', translation block A' + (B' K^T)^T + M K^T.
// The two symmetric blocks are computed on and above their diagonal only, so the result is exactly symmetric.
ELM_HD void lcv_sandwich(const double R[9], const double t[3], const double S[kLcvSym], double out[kLcvSym]) {
    double A[9], B[9], D[9], Ar[9], Br[9], Dr[9], DK[9], BK[9], M[9], MK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[i * 3 + j] = S[lcv_sx(i, j)];
            B[i * 3 + j] = S[lcv_ix(i, 3 + j)];
            D[i * 3 + j] = S[lcv_sx(3 + i, 3 + j)];
        }
    lcv_rot3(R, A, Ar);
    lcv_rot3(R, B, Br);
    lcv_rot3(R, D, Dr);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) Dr[i * 3 + j] = Dr[j * 3 + i]; // the upper triangle stands for both
    lcv_mul_kt(Dr, t, DK); // D' K^T, whose transpose is K D'
    lcv_mul_kt(Br, t, BK);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = Br[i * 3 + j] + DK[j * 3 + i];
    lcv_mul_kt(M, t, MK);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j >= i) {
                out[lcv_ix(i, j)] = (Ar[i * 3 + j] + BK[j * 3 + i]) + MK[i * 3 + j];
                out[lcv_ix(3 + i, 3 + j)] = Dr[i * 3 + j];
            }
            out[lcv_ix(i, 3 + j)] = M[i * 3 + j];
        }
}

// e^T A^-1 e by an L D L^T of A without pivoting in index order: s = sum_j y_j^2 / d_j with L y = e.  A pivot that is not finite or
// not > 0: NaN.  Every inner sum runs over p = 0 .. j - 1 in that order.
ELM_HD double lcv_ldl_form(const double A[kLcvSym], const double e[6]) {
    double Lm[36], d[6], y[6];
    bool ok = true;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[lcv_ix(j, j)];
#pragma unroll
        for (int p = 0; p < j; ++p) dj -= (Lm[j * 6 + p] * Lm[j * 6 + p]) * d[p];
        ok = ok && (dj > 0.0) && (dj <= 1.7976931348623157e308);
        d[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[lcv_ix(j, i)];
#pragma unroll
            for (int p = 0; p < j; ++p) v -= (Lm[i * 6 + p] * Lm[j * 6 + p]) * d[p];
            Lm[i * 6 + j] = v / dj;
        }
        double yj = e[j];
#pragma unroll
        for (int p = 0; p < j; ++p) yj -= Lm[j * 6 + p] * y[p];
        y[j] = yj;
        s += (yj * yj) / dj;
    }
    return ok ? s : (double)NAN;
}
// every pivot of A's L D L^T is finite and > 0
ELM_HD bool lcv_ldl_ok(const double A[kLcvSym]) {
    const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    return lcv_ldl_form(A, zero) == 0.0;
}

// P_v = Ad(Y_{v+1}) Q_v Ad(Y_{v+1})^T from pose 0's rows and pose v + 1's
ELM_HD void lcv_step_term(const double P0[12], const double Pn[12], const double Q[kLcvSym], double out[kLcvSym]) {
    double R[9], t[3];
    lc_between(P0, Pn, R, t);
    lcv_sandwich(R, t, Q, out);
}

// S_v = Ad(Y_v^-1) W_v Ad(Y_v^-1)^T
ELM_HD void lcv_local(const double P0[12], const double Pv[12], const double W[kLcvSym], double out[kLcvSym]) {
    double R[9], t[3], Ri[9], ti[3];
    lc_between(P0, Pv, R, t);
    lcv_inverse(R, t, Ri, ti);
    lcv_sandwich(Ri, ti, W, out);
}

// The pair term on re-based pose rows Y, in the stages the kernel runs between its loads.  Frames: e and the three transforms whose Ad
// are G_A = Ad((Y_{a_l} Z_l B)^-1), G_l = Ad(B^-1), G_B = Ad(Y_{b_k}^-1), B = X_{b_l b_k}.
struct LcvFrames {
    double RA[9], tA[3], Rl[9], tl[3], RB[9], tB[3];
};
ELM_HD void lcv_pair_frames(const double Yak[12], const double Ybk[12], const double PZk[12], const double Yal[12], const double Ybl[12],
                            const double PZl[12], double e[6], LcvFrames& F) {
    lc_pair_e(Yak, Ybk, PZk, Yal, Ybl, PZl, e);
    double RX[9], tX[3], R[9], t[3], Rz[9], tz[3];
    lc_between(Ybl, Ybk, RX, tX);
    pg_split(Yal, R, t);
    pg_split(PZl, Rz, tz);
    lc_compose(R, t, Rz, tz);
    lc_compose(R, t, RX, tX);
    lcv_inverse(R, t, F.RA, F.tA);
    lcv_inverse(RX, tX, F.Rl, F.tl);
    pg_split(Ybk, R, t);
    lcv_inverse(R, t, F.RB, F.tB);
}
// cov <- cov + Ad(X) S Ad(X)^T
ELM_HD void lcv_pair_add(const double R[9], const double t[3], const double S[kLcvSym], double cov[kLcvSym]) {
    double term[kLcvSym];
    lcv_sandwich(R, t, S, term);
#pragma unroll
    for (int c = 0; c < kLcvSym; ++c) cov[c] = cov[c] + term[c];
}
// Sigma_e = Sigma_k + Sigma_Zhat, and s
ELM_HD double lcv_pair_finish(const double Sk[kLcvSym], const double e[6], double cov[kLcvSym]) {
#pragma unroll
    for (int c = 0; c < kLcvSym; ++c) cov[c] = Sk[c] + cov[c];
    return lcv_ldl_form(cov, e);
}
// the whole pair: e, Sigma_e (21 entries) and s.  Ca = C(a_k, a_l), Cb = C(b_k, b_l).
ELM_HD double lcv_pair(const double Yak[12], const double Ybk[12], const double PZk[12], const double Sk[kLcvSym], const double Yal[12],
                       const double Ybl[12], const double PZl[12], const double Sl[kLcvSym], const double Ca[kLcvSym], const double Cb[kLcvSym],
                       double e[6], double cov[kLcvSym]) {
    LcvFrames F;
    lcv_pair_frames(Yak, Ybk, PZk, Yal, Ybl, PZl, e, F);
    lcv_sandwich(F.RA, F.tA, Ca, cov);
    lcv_pair_add(F.Rl, F.tl, Sl, cov);
    lcv_pair_add(F.RB, F.tB, Cb, cov);
    return lcv_pair_finish(Sk, e, cov);
}

} // namespace elm
