// elm_k_pginit.hip -- the pose graph's linear initialization (elm_posegraph_initialize; the contract is in
// include/elimaloc_hip_posegraph_init.h): the edge terms of the rotation problem and of the translation problem,
// written into the contribution arrays that k_pg_linearize writes (component-major, H_ij with its rows at i and its columns at j), so
// that k_pg_nodes, the chain factor and the conjugate gradients run on them as they are; and the two kernels that apply a solution to
// the trial poses.  Float64, no contraction.  No atomics, no inline assembly, no scratch; plain launches on the context's stream.
//   K13a k_pgi_rot_terms    a lane group of 8 per edge, the lane is the column: H_ii = H_jj = w_r I, H_ij = -w_r blockdiag(R_Z, R_Z), g_i, g_j
//   K13b k_pgi_trans_terms  the same layout: H_ii = H_jj = w_t I, H_ij = -w_t R_i^T R_j in the top-left block, g_i, g_j
//   K13c k_pgi_rot_apply    one lane per node: rows + Delta, the closed-form projection, the trial pose; the workgroup's degenerate count
//                           (pg_block_sum of elm_dev_pgraph.hpp)
//   K13d k_pgi_trans_apply  one lane per node: t <- t + R v in the trial poses
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

// one of three values by an index that varies by lane (an indexed register array would go to scratch)
__device__ __forceinline__ double pgi_sel3(uint32_t k, double a, double b, double c) { return k == 0u ? a : (k == 1u ? b : c); }

__device__ __forceinline__ double pgi_norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

} // namespace

// K13a.  Lane c = 3 k + m (c < 6) of an edge's group owns column c of the edge's 6 x 6 blocks and entry c of its gradients: row k of the
// two rotations, component m.  It reads only its own row rho^k of R_i and R_j.  e^k = R_Z^T rho^k_i - rho^k_j;
// g_i[c] = w (R_Z e^k)[m], g_j[c] = -w e^k[m]; H_ij[a][c] = -w R_Z[a - 3 k][m] inside the lane's diagonal block, 0 outside.
__global__ __launch_bounds__(256) void k_pgi_rot_terms(const PgDev d, const double* __restrict__ poses) {
    const uint32_t e = blockIdx.x * (256u / kPgLanesPerEdge) + threadIdx.x / kPgLanesPerEdge, c = threadIdx.x % kPgLanesPerEdge;
    if (e >= d.E || c >= 6u) return;
    const uint32_t k = c < 3u ? 0u : 1u, m = c - 3u * k;
    const double* __restrict__ pz = d.Z + 12 * (size_t)e;
    const double* __restrict__ om = d.info + 36 * (size_t)e;
    const double* __restrict__ pi = poses + 12 * (size_t)d.ei[e] + 4u * k;
    const double* __restrict__ pj = poses + 12 * (size_t)d.ej[e] + 4u * k;
    double RZ[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) RZ[a * 3 + b] = pz[a * 4 + b];
    const double w = ((om[21] + om[28]) + om[35]) / 3.0;
    const double ri[3] = {pi[0], pi[1], pi[2]};
    double eb[3];
    pg_mul3_atv(RZ, ri, eb);
#pragma unroll
    for (int a = 0; a < 3; ++a) eb[a] = eb[a] - pj[a];
    // row m and column m of R_Z
    const double r0 = pgi_sel3(m, RZ[0], RZ[3], RZ[6]), r1 = pgi_sel3(m, RZ[1], RZ[4], RZ[7]), r2 = pgi_sel3(m, RZ[2], RZ[5], RZ[8]);
    const double c0 = pgi_sel3(m, RZ[0], RZ[1], RZ[2]), c1 = pgi_sel3(m, RZ[3], RZ[4], RZ[5]), c2 = pgi_sel3(m, RZ[6], RZ[7], RZ[8]);
    const size_t S = d.e_stride;
    d.gi[c * S + e] = w * ((r0 * eb[0] + r1 * eb[1]) + r2 * eb[2]);
    d.gj[c * S + e] = -(w * pgi_sel3(m, eb[0], eb[1], eb[2]));
    const double col[3] = {c0, c1, c2};
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        const double dg = a == c ? w : 0.0;
        d.Hii[(a * 6u + c) * S + e] = dg;
        d.Hjj[(a * 6u + c) * S + e] = dg;
        d.Hij[(a * 6u + c) * S + e] = (a / 3u == k) ? -(w * col[a % 3u]) : 0.0;
    }
}

// K13b.  Lanes 0 .. 2 own the columns of the translation block, lanes 3 .. 5 the padding (the diagonal w alone).  u = R_i^T (t_j - t_i)
// - t_Z; g_i = -w u, g_j = w R_ij^T u, H_ij = -w R_ij with R_ij = R_i^T R_j: R_Z has dropped out of every product (the contract).
__global__ __launch_bounds__(256) void k_pgi_trans_terms(const PgDev d, const double* __restrict__ poses) {
    const uint32_t e = blockIdx.x * (256u / kPgLanesPerEdge) + threadIdx.x / kPgLanesPerEdge, c = threadIdx.x % kPgLanesPerEdge;
    if (e >= d.E || c >= 6u) return;
    const bool pad = c >= 3u;
    const uint32_t m = pad ? c - 3u : c;
    const double* __restrict__ om = d.info + 36 * (size_t)e;
    double Pi[12], Pj[12], PZ[12], Ri[9], ti[3], Rj[9], tj[3];
    pg_load_edge_poses(d, poses, e, Pi, Pj, PZ); // (of the measurement only t_Z is used)
    pg_split(Pi, Ri, ti);
    pg_split(Pj, Rj, tj);
    const double w = ((om[0] + om[7]) + om[14]) / 3.0;
    const double dt[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    double u[3];
    pg_mul3_atv(Ri, dt, u);
    u[0] = u[0] - PZ[3];
    u[1] = u[1] - PZ[7];
    u[2] = u[2] - PZ[11];
    // column m of R_j, then column m of R_ij
    const double q0 = pgi_sel3(m, Rj[0], Rj[1], Rj[2]), q1 = pgi_sel3(m, Rj[3], Rj[4], Rj[5]), q2 = pgi_sel3(m, Rj[6], Rj[7], Rj[8]);
    double col[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) col[a] = (Ri[a] * q0 + Ri[3 + a] * q1) + Ri[6 + a] * q2;
    const size_t S = d.e_stride;
    d.gi[c * S + e] = pad ? 0.0 : -(w * pgi_sel3(m, u[0], u[1], u[2]));
    d.gj[c * S + e] = pad ? 0.0 : w * ((col[0] * u[0] + col[1] * u[1]) + col[2] * u[2]);
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        const double dg = a == c ? w : 0.0;
        d.Hii[(a * 6u + c) * S + e] = dg;
        d.Hjj[(a * 6u + c) * S + e] = dg;
        d.Hij[(a * 6u + c) * S + e] = (a < 3u && !pad) ? -(w * col[a % 3u]) : 0.0;
    }
}

// K13c.  One lane per node.  rows[v] = the first two rows of R_v, plus the solve's Delta where the node is active.  An active node's
// rows are projected (the contract's closed form) into the trial pose; a degenerate one and every inactive node keep their pose bit for
// bit.  The workgroup's count of degenerate nodes goes to slot blockIdx.x, by the fixed tree of pg_block_sum.
__global__ __launch_bounds__(256) void k_pgi_rot_apply(const PgDev d, const double* __restrict__ poses, double* __restrict__ trial,
                                                       double* __restrict__ rows, double* __restrict__ slots) {
    __shared__ double buf[kPgBlock];
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    double bad = 0.0;
    if (v < d.N) {
        double P[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) P[q] = poses[12 * (size_t)v + q];
        double y[6] = {P[0], P[1], P[2], P[4], P[5], P[6]};
        const bool act = d.active[v] != 0;
        if (act) {
#pragma unroll
            for (int q = 0; q < 6; ++q) y[q] = y[q] + d.x[6 * (size_t)v + q];
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) rows[6 * (size_t)v + q] = y[q];
        if (act) {
            const double n1 = pgi_norm3(y[0], y[1], y[2]), n2 = pgi_norm3(y[3], y[4], y[5]);
            bool ok = !(n1 < kPgInitDegenerate) && !(n2 < kPgInitDegenerate);
            if (ok) {
                const double u[3] = {y[0] / n1, y[1] / n1, y[2] / n1}, w[3] = {y[3] / n2, y[4] / n2, y[5] / n2};
                double s[3] = {u[0] + w[0], u[1] + w[1], u[2] + w[2]}, t[3] = {u[0] - w[0], u[1] - w[1], u[2] - w[2]};
                const double ns = pgi_norm3(s[0], s[1], s[2]), nt = pgi_norm3(t[0], t[1], t[2]);
                ok = !(ns < kPgInitDegenerate) && !(nt < kPgInitDegenerate);
                if (ok) {
                    const double rt2 = sqrt(2.0);
                    double r1[3], r2[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        s[q] = s[q] / ns;
                        t[q] = t[q] / nt;
                        r1[q] = (s[q] + t[q]) / rt2;
                        r2[q] = (s[q] - t[q]) / rt2;
                    }
                    P[0] = r1[0]; P[1] = r1[1]; P[2] = r1[2];
                    P[4] = r2[0]; P[5] = r2[1]; P[6] = r2[2];
                    P[8] = r1[1] * r2[2] - r1[2] * r2[1];
                    P[9] = r1[2] * r2[0] - r1[0] * r2[2];
                    P[10] = r1[0] * r2[1] - r1[1] * r2[0];
                }
            }
            bad = ok ? 0.0 : 1.0;
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) trial[12 * (size_t)v + q] = P[q];
    }
    const double n = pg_block_sum(bad, buf); // whole numbers of at most 256: exact
    if (threadIdx.x == 0) slots[blockIdx.x] = n;
}

// K13d.  One lane per node, in place on the trial poses: t <- t + R v for an active node (the arithmetic of pg_retract's translation;
// the rotation is not touched, so not even a zero's sign changes).
__global__ __launch_bounds__(256) void k_pgi_trans_apply(const PgDev d, double* __restrict__ trial) {
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    if (v >= d.N || !d.active[v]) return;
    double* __restrict__ P = trial + 12 * (size_t)v;
    const double x0 = d.x[6 * (size_t)v], x1 = d.x[6 * (size_t)v + 1], x2 = d.x[6 * (size_t)v + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r * 4 + 3] = P[r * 4 + 3] + ((P[r * 4] * x0 + P[r * 4 + 1] * x1) + P[r * 4 + 2] * x2);
}

void launch_pgi_rot_terms(hipStream_t s, const PgDev& d, const double* poses) {
    if (!d.E) return;
    hipLaunchKernelGGL(k_pgi_rot_terms, dim3(pg_edge_group_blocks(d.E)), dim3(256), 0, s, d, poses);
}

void launch_pgi_trans_terms(hipStream_t s, const PgDev& d, const double* poses) {
    if (!d.E) return;
    hipLaunchKernelGGL(k_pgi_trans_terms, dim3(pg_edge_group_blocks(d.E)), dim3(256), 0, s, d, poses);
}

void launch_pgi_rot_apply(hipStream_t s, const PgDev& d, const double* poses, double* trial, double* rows, double* slots) {
    if (!d.N) return;
    hipLaunchKernelGGL(k_pgi_rot_apply, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, poses, trial, rows, slots);
}

void launch_pgi_trans_apply(hipStream_t s, const PgDev& d, double* trial) {
    if (!d.N) return;
    hipLaunchKernelGGL(k_pgi_trans_apply, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, trial);
}

} // namespace elm
