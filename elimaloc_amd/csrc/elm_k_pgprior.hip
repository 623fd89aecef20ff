// elm_k_pgprior.hip -- the pose graph's priors (elm_posegraph_*prior*; the contract is in include/elimaloc_hip_posegraph_prior.h;
// DESIGN.md section 27): the linearization of the absolute pose / position factors, their addition onto the node sums of the edges, and
// their part of the robust cost.  A prior touches H_vv, g_v and the cost only, so the product, both preconditioners, the conjugate
// gradients, the retraction and the covariances of elm_k_pgraph.hip, elm_k_pgchain.hip and elm_k_pgcov.hip serve it as they are.
// Float64, no atomics, plain launches on the context's stream; every sum has a fixed order.
//   K17a k_pgp_linearize  a lane group of 8 per prior, the lane is the column: r, J, s, w and the prior's g_q and H_q
//   K17b k_pgp_nodes      one wavefront per node that has priors, the lane is the component: H_vv and g_v completed
//   K17c k_pgp_cost / k_pgp_finish   rho_q at given poses, fixed-order reduction, the three totals added onto the edges' record
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"

namespace elm {

// the pose rows of prior q's node at `poses`, of its measurement, and its lever arm
__device__ __forceinline__ void pgp_load(const PgPriorDev& p, const double* __restrict__ poses, uint32_t q, double Pv[12], double PZ[12], double l[3]) {
    const double* __restrict__ pv = poses + 12 * (size_t)p.node[q];
    const double* __restrict__ pz = p.Z + 12 * (size_t)q;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        Pv[k] = pv[k];
        PZ[k] = pz[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) l[k] = p.lever[3 * (size_t)q + k];
}

// K17a.  As k_pg_linearize: lanes 0 .. 5 of a group of 8 are the columns c of the prior's 6 x 6 results (lanes 6 and 7 compute column 5
// again and store nothing).  Every lane evaluates r and the three non-zero blocks of J in registers (pg_prior_blocks); lane 0 lays J and
// r out in LDS, from where each lane takes its column J_c and r_c.  Omega is read a row at a time: (Omega J)_c and Omega r come from
// each row.  Then g_q[c] = w J_c . (Omega r) and H_q[a][c] = w J_a . (Omega J)_c, the rows of J^T from the blocks.  Stores are
// component-major with the prior capacity as stride.
__global__ __launch_bounds__(256) void k_pgp_linearize(const PgPriorDev p, const double* __restrict__ poses, double huber_k) {
    __shared__ double s_J[256 / kPgLanesPerPrior][36], s_r[256 / kPgLanesPerPrior][6];
    const uint32_t grp = threadIdx.x / kPgLanesPerPrior, lane = threadIdx.x % kPgLanesPerPrior;
    const uint32_t q_raw = blockIdx.x * (256u / kPgLanesPerPrior) + grp;
    const bool valid = q_raw < p.P;
    const uint32_t q = valid ? q_raw : p.P - 1u; // (the launch has P >= 1)
    const uint32_t c = lane < 6u ? lane : 5u;
    double Pv[12], PZ[12], l[3];
    pgp_load(p, poses, q, Pv, PZ, l);
    double r[6];
    PgPriorBlocks K;
    pg_prior_blocks(Pv, PZ, l, r, K);
    if (lane == 0u) {
        pg_prior_full(K, s_J[grp]);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_r[grp][k] = r[k];
    }
    __syncthreads();
    double Jc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Jc[k] = s_J[grp][k * 6 + c];
    const double rc = s_r[grp][c];
    if (!valid) return;
    double OJ[6], Or[6];
    const double* __restrict__ om = p.info + 36 * (size_t)q;
#pragma unroll
    for (int row = 0; row < 6; ++row) {
        double o[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = om[row * 6 + k];
        double a = o[0] * Jc[0], b = o[0] * r[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            a += o[k] * Jc[k];
            b += o[k] * r[k];
        }
        OJ[row] = a;
        Or[row] = b;
    }
    double s = r[0] * Or[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s += r[k] * Or[k];
    const double w = pg_huber_weight(s, huber_k);
    if (lane >= 6u) return;
    const size_t S = p.p_stride;
    if (lane == 0u) {
        p.s[q] = s;
        p.w[q] = w;
    }
    p.r[c * S + q] = rc;
    double g = Jc[0] * Or[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) g += Jc[k] * Or[k];
    p.g[c * S + q] = w * g;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        p.J[(a * 6 + c) * S + q] = Jc[a];
        // row a of J^T against the column (Omega J)_c: only the non-zero blocks
        double h;
        if (a < 3) {
            h = (K.Jtt[a] * OJ[0] + K.Jtt[3 + a] * OJ[1]) + K.Jtt[6 + a] * OJ[2];
        } else {
            const int b = a - 3;
            h = ((K.Jtr[b] * OJ[0] + K.Jtr[3 + b] * OJ[1]) + K.Jtr[6 + b] * OJ[2]) + ((K.Jrr[b] * OJ[3] + K.Jrr[3 + b] * OJ[4]) + K.Jrr[6 + b] * OJ[5]);
        }
        p.H[(a * 6 + c) * S + q] = w * h;
    }
}

// K17b.  One wavefront per node that has priors, four per workgroup; lanes 0 .. 35 are the entries of H_vv, lanes 36 .. 41 those of
// g_v.  Each lane reads what k_pg_nodes(sum = 1) stored -- the node's edges in ascending edge index -- adds the node's priors in
// ascending prior index, one addition per prior, and stores back.  No barrier: a wavefront without a row leaves.
__global__ __launch_bounds__(256) void k_pgp_nodes(const PgDev d, const PgPriorDev p) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * 4u + wave;
    if (row >= p.n_rows || lane >= 42u) return;
    const uint32_t v = p.row_node[row];
    const size_t S = p.p_stride;
    const double* __restrict__ from = lane < 36u ? p.H + lane * S : p.g + (lane - 36u) * S;
    double* const to = lane < 36u ? d.Hd + 36 * (size_t)v + lane : d.g + 6 * (size_t)v + (lane - 36u);
    double acc = *to;
    const uint32_t k1 = p.row_first[row + 1];
    for (uint32_t k = p.row_first[row]; k < k1; ++k) acc += from[p.order[k]];
    *to = acc;
}

// K17c.  One lane per prior: s_q and rho_q at the given poses; the workgroup's sums of s, rho and the outlier count to its three slots.
__global__ __launch_bounds__(256) void k_pgp_cost(const PgPriorDev p, const double* __restrict__ poses, double huber_k) {
    __shared__ double buf[kPgBlock];
    const uint32_t q = blockIdx.x * kPgBlock + threadIdx.x;
    double s = 0.0, rho = 0.0, out = 0.0;
    if (q < p.P) {
        double Pv[12], PZ[12], l[3], r[6];
        pgp_load(p, poses, q, Pv, PZ, l);
        pg_prior_residual(Pv, PZ, l, r);
        const double* __restrict__ om = p.info + 36 * (size_t)q;
        double Or[6];
        pg_mv6(om, r, Or);
        s = pg_dot6(r, Or);
        rho = pg_huber_cost(s, huber_k);
        out = pg_huber_weight(s, huber_k) < 1.0 ? 1.0 : 0.0;
    }
    const uint32_t nb = gridDim.x;
    const double ts = pg_block_sum(s, buf);
    const double tr = pg_block_sum(rho, buf);
    const double to = pg_block_sum(out, buf);
    if (threadIdx.x == 0) {
        p.part_cost[blockIdx.x] = ts;
        p.part_cost[nb + blockIdx.x] = tr;
        p.part_cost[2 * nb + blockIdx.x] = to;
    }
}
// one workgroup, after k_pg_finish: the priors' three totals, each added once onto the edges'
__global__ __launch_bounds__(256) void k_pgp_finish(const PgDev d, const PgPriorDev p, uint32_t n_slots) {
    __shared__ double buf[kPgBlock];
    const double chi2 = pg_sum_slots(p.part_cost, n_slots, buf);
    const double cost = pg_sum_slots(p.part_cost + n_slots, n_slots, buf);
    const double nout = pg_sum_slots(p.part_cost + 2 * (size_t)n_slots, n_slots, buf);
    if (threadIdx.x == 0) {
        d.out->chi2 = d.out->chi2 + chi2;
        d.out->cost = d.out->cost + cost;
        d.out->n_outliers = d.out->n_outliers + nout;
    }
}

void launch_pgp_linearize(hipStream_t s, const PgPriorDev& p, const double* poses, double huber_k) {
    const uint32_t nb = (uint32_t)(((size_t)p.P * kPgLanesPerPrior + 255) / 256);
    hipLaunchKernelGGL(k_pgp_linearize, dim3(nb), dim3(256), 0, s, p, poses, huber_k);
}

void launch_pgp_nodes(hipStream_t s, const PgDev& d, const PgPriorDev& p) {
    hipLaunchKernelGGL(k_pgp_nodes, dim3((p.n_rows + 3) / 4), dim3(256), 0, s, d, p);
}

void launch_pgp_cost(hipStream_t s, const PgDev& d, const PgPriorDev& p, const double* poses, double huber_k) {
    const uint32_t nb = pg_blocks(p.P);
    hipLaunchKernelGGL(k_pgp_cost, dim3(nb), dim3(256), 0, s, p, poses, huber_k);
    hipLaunchKernelGGL(k_pgp_finish, dim3(1), dim3(256), 0, s, d, p, nb);
}

} // namespace elm
