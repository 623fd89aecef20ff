// elm_k_pginitp.hip -- the pose graph's linear initialization with the priors in it (elm_posegraph_initialize_priors; the contract is in
// include/elimaloc_hip_posegraph_init_prior.h): the priors' terms of the rotation problem and of the translation
// problem, written into the prior arrays that k_pgp_linearize writes (component-major with the prior capacity as stride), so that
// k_pgp_nodes adds them onto the node sums of elm_k_pginit.hip's edge terms in the contract's order; and the rigid alignment of the
// components that only position priors hold.  Float64, no contraction.  No atomics, no inline assembly, no scratch; plain launches on the
// context's stream; every sum has a fixed order.
//   K18a k_pgip_terms        one lane per prior: g_q and H_q = w I_6 of the stage, w the stage's weight of the prior (0: masked)
//   K18b k_pgip_align_sums   one workgroup per aligned component: W, sum w a, sum w b, the centroids, then S about them
//   K18c k_pgip_align_apply  one lane per node: R <- G R, t <- c_b + G (t - c_a) for the nodes of aligned components
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"

namespace elm {

// K18a.  stage 0, rotations: e = y_v - [rho1_Z; rho2_Z], g = w e.  stage 1, translations: u = (t_v - t_Z) + R_v l, g = [w R_v^T u; 0].
// H = w I_6 in both.  A weight that is not positive stores zeros: the prior is not in the stage.
__global__ __launch_bounds__(256) void k_pgip_terms(const PgPriorDev p, const double* __restrict__ poses, const double* __restrict__ weight,
                                                    int stage) {
    const uint32_t q = blockIdx.x * kPgBlock + threadIdx.x;
    if (q >= p.P) return;
    const double wq = weight[q];
    const bool in = wq > 0.0;
    const double w = in ? wq : 0.0;
    const double* __restrict__ pv = poses + 12 * (size_t)p.node[q];
    const double* __restrict__ pz = p.Z + 12 * (size_t)q;
    double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (in) {
        if (stage == 0) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) g[3 * k + m] = w * (pv[4 * k + m] - pz[4 * k + m]);
        } else {
            double Pv[12], R[9], t[3], u[3], Rtu[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) Pv[k] = pv[k];
            pg_split(Pv, R, t);
            const double l0 = p.lever[3 * (size_t)q], l1 = p.lever[3 * (size_t)q + 1], l2 = p.lever[3 * (size_t)q + 2];
#pragma unroll
            for (int a = 0; a < 3; ++a) u[a] = (t[a] - pz[4 * a + 3]) + ((R[a * 3] * l0 + R[a * 3 + 1] * l1) + R[a * 3 + 2] * l2);
            pg_mul3_atv(R, u, Rtu);
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = w * Rtu[a];
        }
    }
    const size_t S = p.p_stride;
#pragma unroll
    for (int c = 0; c < 6; ++c) p.g[c * S + q] = g[c];
#pragma unroll
    for (int k = 0; k < 36; ++k) p.H[k * S + q] = (k % 7 == 0) ? w : 0.0;
}

// the point a_q = t_v + R_v l_q of prior q at `poses`
__device__ __forceinline__ void pgip_point(const PgPriorDev& p, const double* __restrict__ poses, uint32_t q, double a[3]) {
    const double* __restrict__ pv = poses + 12 * (size_t)p.node[q];
    const double l0 = p.lever[3 * (size_t)q], l1 = p.lever[3 * (size_t)q + 1], l2 = p.lever[3 * (size_t)q + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) a[r] = pv[4 * r + 3] + ((pv[4 * r] * l0 + pv[4 * r + 1] * l1) + pv[4 * r + 2] * l2);
}

// K18b.  Workgroup c takes the priors list[first[c] .. first[c + 1]) of aligned component c, ascending: lane t adds entries t, t + 256,
// ... in that order, then the fixed tree of pg_block_sum.  Pass 1: W, sum w a, sum w b; every lane gets the sums back through LDS and
// forms the same centroids.  Pass 2: the nine entries of S = sum w (b - c_b)(a - c_a)^T.  Row c of out [16]: c_a, c_b, S row-major, W.
__global__ __launch_bounds__(256) void k_pgip_align_sums(const PgPriorDev p, const double* __restrict__ poses, const double* __restrict__ weight,
                                                         const uint32_t* __restrict__ first, const uint32_t* __restrict__ list,
                                                         double* __restrict__ out) {
    __shared__ double buf[kPgBlock];
    const uint32_t k0 = first[blockIdx.x], k1 = first[blockIdx.x + 1];
    double W = 0.0, sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += kPgBlock) {
        const uint32_t q = list[k];
        const double w = weight[q];
        double a[3];
        pgip_point(p, poses, q, a);
        W += w;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            sa[r] += w * a[r];
            sb[r] += w * p.Z[12 * (size_t)q + 4 * r + 3];
        }
    }
    W = pg_block_sum(W, buf);
    double ca[3], cb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        ca[r] = pg_block_sum(sa[r], buf) / W;
        cb[r] = pg_block_sum(sb[r], buf) / W;
    }
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = k0 + threadIdx.x; k < k1; k += kPgBlock) {
        const uint32_t q = list[k];
        const double w = weight[q];
        double a[3];
        pgip_point(p, poses, q, a);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double wb = w * (p.Z[12 * (size_t)q + 4 * r + 3] - cb[r]);
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r * 3 + c] += wb * (a[c] - ca[c]);
        }
    }
    double* __restrict__ row = out + 16 * (size_t)blockIdx.x;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double s = pg_block_sum(S[k], buf);
        if (threadIdx.x == 0) row[6 + k] = s;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            row[r] = ca[r];
            row[3 + r] = cb[r];
        }
        row[15] = W;
    }
}

// K18c.  In place on the trial poses.  comp[v] is the node's aligned component or -1; xf row [21]: G row-major, c_a, c_b.  A node outside
// every aligned component is not touched: its pose keeps its bits.
__global__ __launch_bounds__(256) void k_pgip_align_apply(uint32_t N, const int32_t* __restrict__ comp, const double* __restrict__ xf,
                                                          double* __restrict__ trial) {
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    if (v >= N) return;
    const int32_t c = comp[v];
    if (c < 0) return;
    const double* __restrict__ x = xf + 21 * (size_t)c;
    double G[9], P[12], R[9], t[3], Rn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) G[k] = x[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = trial[12 * (size_t)v + k];
    pg_split(P, R, t);
    mul3(G, R, Rn);
    const double d[3] = {t[0] - x[9], t[1] - x[10], t[2] - x[11]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P[r * 4] = Rn[r * 3];
        P[r * 4 + 1] = Rn[r * 3 + 1];
        P[r * 4 + 2] = Rn[r * 3 + 2];
        P[r * 4 + 3] = x[12 + r] + ((G[r * 3] * d[0] + G[r * 3 + 1] * d[1]) + G[r * 3 + 2] * d[2]);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) trial[12 * (size_t)v + k] = P[k];
}

void launch_pgip_terms(hipStream_t s, const PgPriorDev& p, const double* poses, const double* weight, int stage) {
    hipLaunchKernelGGL(k_pgip_terms, dim3(pg_blocks(p.P)), dim3(256), 0, s, p, poses, weight, stage);
}

void launch_pgip_align_sums(hipStream_t s, const PgPriorDev& p, const double* poses, const double* weight, const uint32_t* first,
                            const uint32_t* list, uint32_t n_comps, double* out) {
    hipLaunchKernelGGL(k_pgip_align_sums, dim3(n_comps), dim3(256), 0, s, p, poses, weight, first, list, out);
}

void launch_pgip_align_apply(hipStream_t s, uint32_t N, const int32_t* comp, const double* xf, double* trial) {
    hipLaunchKernelGGL(k_pgip_align_apply, dim3(pg_blocks(N)), dim3(256), 0, s, N, comp, xf, trial);
}

} // namespace elm
