// elm_k_pgraph.hip -- the pose graph (elm_posegraph_*; the contract is in include/elimaloc_hip.h, "pose graph"): the
// SE(3) linearization of relative-pose edges, the per-node assembly with the damped block-Jacobi inverses, the preconditioned conjugate
// gradients on the block-sparse normal equations, the retraction and the robust cost.  Float64.  No float atomics: every sum has a fixed
// order -- a node's sums run over its incidence list in ascending edge index, an inner product is a fixed tree per workgroup into a
// fixed slot and a fixed reduction of the slots.  Kernel boundaries are the only barriers between workgroups; the launches are plain
// launches on the context's stream.
//   K12a k_pg_linearize  a lane group of 8 per edge, the lane is the column: r, A, B, s, w and the edge's five contributions
//   K12b k_pg_nodes      one wavefront per node, the lane is the component: H_vv, g_v, the active rule, the damping, the 6 x 6 inverse
//   K12c k_pg_pcg_init<jacobi> / k_pg_pcg_begin   x = 0, r = -g, (z = M^-1 r, p = z;) r0^T z0
//   K12d k_pg_spmv (+ k_pg_spmv_hub)      q = (H + lambda diag H) p, partials of p^T q
//   K12e k_pg_update<jacobi>   alpha from the partials; x, r, (z; partials of r^T z)
//   K12f k_pg_direction  beta, the stop test and the iteration count from the partials; p
//   K12g k_pg_retract    trial poses, partials of max |x|
//   K12h k_pg_cost / k_pg_finish          rho_e at given poses, fixed-order reduction to one record
// The conjugate gradients are composed once, in launch_pg_pcg_begin and launch_pg_pcg_iteration, with a preconditioner seam: the
// <true> instantiations of K12c and K12e apply the block-Jacobi Minv themselves; with a chain (elm_k_pgchain.hip) the <false> ones leave
// z, the first p and the r^T z slots to launch_pgc_apply, whose level-0 launch writes them.  The fixed-order reductions and the 6 x 6
// block helpers are in elm_dev_pgraph.hpp.
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"

namespace elm {

// K12a.  Lanes 0 .. 5 of a group of 8 are the columns c of the edge's 6 x 6 results (lanes 6 and 7 compute column 5 again and store
// nothing).  Every lane of the group evaluates r and the five non-zero 3 x 3 blocks of A and B in registers (pg_edge_blocks); lane 0
// lays A, B and r out in LDS, from where each lane takes its columns A_c, B_c and r_c (an index that varies by lane would put a
// register array into scratch).  Omega is read a row at a time and never held whole: (Omega A)_c, (Omega B)_c and Omega r come from
// each row.  Then g_i[c] = w A_c . (Omega r), H_ii[a][c] = w A_a . (Omega A)_c, H_ij[a][c] = w A_a . (Omega B)_c,
// H_jj[a][c] = w B_a . (Omega B)_c, the rows A_a, B_a from the blocks.  Stores are component-major: for a fixed component the 8 edges
// of a wavefront are consecutive.
__global__ __launch_bounds__(256) void k_pg_linearize(const PgDev d, const double* __restrict__ poses, double huber_k) {
    __shared__ double s_A[256 / kPgLanesPerEdge][36], s_B[256 / kPgLanesPerEdge][36], s_r[256 / kPgLanesPerEdge][6];
    const uint32_t grp = threadIdx.x / kPgLanesPerEdge, lane = threadIdx.x % kPgLanesPerEdge;
    const uint32_t e_raw = blockIdx.x * (256u / kPgLanesPerEdge) + grp;
    const bool valid = e_raw < d.E;
    const uint32_t e = valid ? e_raw : d.E - 1u; // (the launch has E >= 1)
    const uint32_t c = lane < 6u ? lane : 5u;
    double Pi[12], Pj[12], PZ[12];
    pg_load_edge_poses(d, poses, e, Pi, Pj, PZ);
    double r[6];
    PgBlocks K;
    pg_edge_blocks(Pi, Pj, PZ, r, K);
    if (lane == 0u) {
        pg_blocks_full(K, s_A[grp], s_B[grp]);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_r[grp][k] = r[k];
    }
    __syncthreads();
    double Ac[6], Bc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        Ac[k] = s_A[grp][k * 6 + c];
        Bc[k] = s_B[grp][k * 6 + c];
    }
    const double rc = s_r[grp][c];
    if (!valid) return;
    double OA[6], OB[6], Or[6];
    const double* __restrict__ om = d.info + 36 * (size_t)e;
#pragma unroll
    for (int row = 0; row < 6; ++row) {
        double o[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = om[row * 6 + k];
        double a = o[0] * Ac[0], b = o[0] * Bc[0], q = o[0] * r[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            a += o[k] * Ac[k];
            b += o[k] * Bc[k];
            q += o[k] * r[k];
        }
        OA[row] = a;
        OB[row] = b;
        Or[row] = q;
    }
    double s = r[0] * Or[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) s += r[k] * Or[k];
    const double w = pg_huber_weight(s, huber_k);
    if (lane >= 6u) return;
    const size_t S = d.e_stride;
    if (lane == 0u) {
        d.s[e] = s;
        d.w[e] = w;
    }
    d.r[c * S + e] = rc;
    double gi = Ac[0] * Or[0], gj = Bc[0] * Or[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        gi += Ac[k] * Or[k];
        gj += Bc[k] * Or[k];
    }
    d.gi[c * S + e] = w * gi;
    d.gj[c * S + e] = w * gj;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        d.A[(a * 6 + c) * S + e] = Ac[a];
        d.B[(a * 6 + c) * S + e] = Bc[a];
        // row a of A^T and B^T against the columns (Omega A)_c, (Omega B)_c: only the non-zero blocks
        double hii, hij, hjj;
        if (a < 3) {
            hii = (K.Att[a] * OA[0] + K.Att[3 + a] * OA[1]) + K.Att[6 + a] * OA[2];
            hij = (K.Att[a] * OB[0] + K.Att[3 + a] * OB[1]) + K.Att[6 + a] * OB[2];
            hjj = (K.Btt[a] * OB[0] + K.Btt[3 + a] * OB[1]) + K.Btt[6 + a] * OB[2];
        } else {
            const int b = a - 3;
            hii = ((K.Atr[b] * OA[0] + K.Atr[3 + b] * OA[1]) + K.Atr[6 + b] * OA[2]) +
                  ((K.Arr[b] * OA[3] + K.Arr[3 + b] * OA[4]) + K.Arr[6 + b] * OA[5]);
            hij = ((K.Atr[b] * OB[0] + K.Atr[3 + b] * OB[1]) + K.Atr[6 + b] * OB[2]) +
                  ((K.Arr[b] * OB[3] + K.Arr[3 + b] * OB[4]) + K.Arr[6 + b] * OB[5]);
            hjj = (K.Brr[b] * OB[3] + K.Brr[3 + b] * OB[4]) + K.Brr[6 + b] * OB[5];
        }
        d.Hii[(a * 6 + c) * S + e] = w * hii;
        d.Hij[(a * 6 + c) * S + e] = w * hij;
        d.Hjj[(a * 6 + c) * S + e] = w * hjj;
    }
}

// K12b.  One wavefront per node, four per workgroup; lanes 0 .. 35 are the entries of H_vv, lanes 36 .. 41 those of g_v.  With `sum`
// each lane walks the node's incidence list in ascending edge index, one addition per edge (a hub of any degree keeps all its lanes
// busy and the order of the contract); without it the stored H_vv is read back.  A fixed node and a free node whose block is all zero
// are not active.  Lane 0 inverts the damped block H_vv + lambda diag(H_vv) in LDS (inv6_ws).
__global__ __launch_bounds__(256) void k_pg_nodes(const PgDev d, double lambda, int sum) {
    __shared__ double s_h[4][36], s_inv[4][36], s_ws[4][36];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t v = blockIdx.x * 4u + wave;
    const bool valid = v < d.N;
    double acc = 0.0;
    if (valid && lane < 42u) {
        if (sum) {
            const size_t S = d.e_stride;
            const double* __restrict__ from_i = lane < 36u ? d.Hii + lane * S : d.gi + (lane - 36u) * S;
            const double* __restrict__ from_j = lane < 36u ? d.Hjj + lane * S : d.gj + (lane - 36u) * S;
            const uint32_t k1 = d.inc_start[v + 1];
            for (uint32_t k = d.inc_start[v]; k < k1; ++k) {
                const uint32_t ent = d.inc[k];
                acc += (ent & 1u) ? from_j[ent >> 1] : from_i[ent >> 1];
            }
            if (lane < 36u) d.Hd[36 * (size_t)v + lane] = acc;
            else d.g[6 * (size_t)v + (lane - 36u)] = acc;
        } else if (lane < 36u) {
            acc = d.Hd[36 * (size_t)v + lane];
        }
    }
    const bool nonzero = __ballot(valid && lane < 36u && acc != 0.0) != 0ull;
    const bool active = valid && nonzero && d.fixed[v] == 0;
    if (lane < 36u) s_h[wave][lane] = (lane % 7u == 0u) ? acc + lambda * acc : acc;
    __syncthreads();
    if (lane == 0u && active) inv6_ws(s_h[wave], s_inv[wave], s_ws[wave]);
    __syncthreads();
    if (valid && lane < 36u) d.Minv[36 * (size_t)v + lane] = active ? s_inv[wave][lane] : 0.0;
    if (valid && lane == 0u) d.active[v] = active ? 1 : 0;
}

// K12c.  One lane per node.  kJacobi: z = Minv r, p = z and the workgroup's partial of r0^T z0 too; without it they are left to the
// preconditioner's apply that follows, and the kernel has no barrier.
template <bool kJacobi>
__global__ __launch_bounds__(256) void k_pg_pcg_init(const PgDev d) {
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    double rz = 0.0;
    if (v < d.N) {
        const bool act = d.active[v] != 0;
        double r[6], z[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = act ? -d.g[6 * (size_t)v + k] : 0.0;
        if constexpr (kJacobi) pg_mv6(d.Minv + 36 * (size_t)v, r, z);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            d.x[6 * (size_t)v + k] = 0.0;
            d.rr[6 * (size_t)v + k] = r[k];
            if constexpr (kJacobi) {
                d.z[6 * (size_t)v + k] = z[k];
                d.p[6 * (size_t)v + k] = z[k];
            }
            d.q[6 * (size_t)v + k] = 0.0;
            if constexpr (kJacobi) rz += r[k] * z[k];
        }
    }
    if constexpr (kJacobi) {
        __shared__ double buf[kPgBlock];
        const double t = pg_block_sum(rz, buf);
        if (threadIdx.x == 0) d.part_rz[blockIdx.x] = t;
    }
}
// one workgroup: r0^T z0 from the slots; a zero right-hand side ends a solve with a tolerance before its first iteration
__global__ __launch_bounds__(256) void k_pg_pcg_begin(const PgDev d, double tol) {
    __shared__ double buf[kPgBlock];
    const double rz0 = pg_sum_slots(d.part_rz, pg_blocks(d.N), buf);
    if (threadIdx.x == 0) {
        const bool over = tol > 0.0 && !(rz0 > 0.0);
        d.state->rz[0] = rz0;
        d.state->rz[1] = 0.0;
        d.state->rz0 = rz0;
        d.state->stop[0] = over ? 1u : 0u;
        d.state->stop[1] = 0u;
        d.state->iters = 0u;
        d.state->converged = over ? 1u : 0u;
    }
}

// One row of q_v = (H_vv + lambda diag H_vv) p_v + sum over the incidence entries k0, k0 + step, ... of the off-diagonal block times the
// neighbour's p: H_ij p_j where v is i, H_ij^T p_i where v is j.
__device__ __forceinline__ double pg_spmv_row(const PgDev& d, uint32_t v, uint32_t c, double lambda, bool with_diag, uint32_t k0, uint32_t k1,
                                              uint32_t step) {
    double qv = 0.0;
    if (with_diag) {
        const double* __restrict__ H = d.Hd + 36 * (size_t)v + 6 * c;
        const double* __restrict__ pv = d.p + 6 * (size_t)v;
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) {
            double h = H[b];
            if (b == c) h = h + lambda * h;
            qv += h * pv[b];
        }
    }
    const size_t S = d.e_stride;
    for (uint32_t k = k0; k < k1; k += step) {
        const uint32_t ent = d.inc[k], e = ent >> 1;
        if (ent & 1u) {
            const double* __restrict__ pn = d.p + 6 * (size_t)d.ei[e];
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) qv += d.Hij[(b * 6u + c) * S + e] * pn[b];
        } else {
            const double* __restrict__ pn = d.p + 6 * (size_t)d.ej[e];
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) qv += d.Hij[(c * 6u + b) * S + e] * pn[b];
        }
    }
    return qv;
}

// K12d.  A lane group of 8 per node, 32 nodes per workgroup; lanes 0 .. 5 of a group are the rows of q_v.  A node of degree above
// kPgHubDegree is left to k_pg_spmv_hub.  The workgroup's partial of p^T q goes to slot blockIdx.x.
__global__ __launch_bounds__(256) void k_pg_spmv(const PgDev d, double lambda, uint32_t it) {
    __shared__ double buf[kPgBlock];
    if (d.state->stop[it & 1u]) return;
    const uint32_t v = blockIdx.x * kPgNodesPerBlock + (threadIdx.x >> 3), c = threadIdx.x & 7u;
    double pq = 0.0;
    if (v < d.N && c < 6u) {
        const uint32_t k0 = d.inc_start[v], k1 = d.inc_start[v + 1];
        if (k1 - k0 <= kPgHubDegree) {
            double qv = 0.0;
            if (d.active[v]) qv = pg_spmv_row(d, v, c, lambda, true, k0, k1, 1u);
            d.q[6 * (size_t)v + c] = qv;
            pq = d.p[6 * (size_t)v + c] * qv;
        }
    }
    const double t = pg_block_sum(pq, buf);
    if (threadIdx.x == 0) d.part_pq[blockIdx.x] = t;
}
// One wavefront per hub.  Group g of its 8 lane groups sums the incidence entries g, g + 8, ... in ascending order (group 0 adds the
// diagonal block first); the 8 sums of a row are added in group order.  The hub's p^T q goes to the slot after the workgroups' slots.
__global__ __launch_bounds__(64) void k_pg_spmv_hub(const PgDev d, double lambda, uint32_t it) {
    __shared__ double s_q[8][8];
    if (d.state->stop[it & 1u]) return;
    const uint32_t v = d.hubs[blockIdx.x], g = threadIdx.x >> 3, c = threadIdx.x & 7u;
    const bool act = d.active[v] != 0;
    const uint32_t k0 = d.inc_start[v], k1 = d.inc_start[v + 1];
    double qv = 0.0;
    if (act && c < 6u) qv = pg_spmv_row(d, v, c, lambda, g == 0u, k0 + g, k1, 8u);
    s_q[g][c] = qv;
    __syncthreads();
    if (g == 0u && c < 6u) {
        double t = s_q[0][c];
#pragma unroll
        for (int h = 1; h < 8; ++h) t += s_q[h][c];
        d.q[6 * (size_t)v + c] = t;
        s_q[0][c] = d.p[6 * (size_t)v + c] * t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_q[0][0];
#pragma unroll
        for (int k = 1; k < 6; ++k) t += s_q[0][k];
        d.part_pq[(d.N + kPgNodesPerBlock - 1) / kPgNodesPerBlock + blockIdx.x] = t;
    }
}

// K12e.  One lane per node.  Every workgroup reduces the partials of p^T q in slot order to the same alpha.  kJacobi: z = Minv r and the
// workgroup's partial of r^T z too; without it the preconditioner's apply that follows writes both.  Every lane reaches every barrier:
// the stop word is the same for the whole launch, and no barrier follows the test of v.
template <bool kJacobi>
__global__ __launch_bounds__(256) void k_pg_update(const PgDev d, uint32_t it) {
    __shared__ double buf[kPgBlock];
    if (d.state->stop[it & 1u]) return;
    const double pq = pg_sum_slots(d.part_pq, pg_pq_slots(d.N, d.n_hubs), buf);
    const double rz_old = d.state->rz[it & 1u];
    const double alpha = pq != 0.0 ? rz_old / pq : 0.0;
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    double rz = 0.0;
    if (v < d.N) {
        double r[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const size_t o = 6 * (size_t)v + k;
            d.x[o] = d.x[o] + alpha * d.p[o];
            r[k] = d.rr[o] - alpha * d.q[o];
            d.rr[o] = r[k];
        }
        if constexpr (kJacobi) {
            const double* __restrict__ M = d.Minv + 36 * (size_t)v;
#pragma unroll
            for (int a = 0; a < 6; ++a) { // a row at a time: the whole block is never held
                const double t = pg_dot6(M + a * 6, r);
                d.z[6 * (size_t)v + a] = t;
                rz += r[a] * t;
            }
        }
    }
    if constexpr (kJacobi) {
        const double t = pg_block_sum(rz, buf);
        if (threadIdx.x == 0) d.part_rz[blockIdx.x] = t;
    }
}

// K12f.  One lane per node.  beta and the stop test from the partials of r^T z; the first workgroup writes the next iteration's state
// (the words of the other parity: nothing this launch reads is written in it).
__global__ __launch_bounds__(256) void k_pg_direction(const PgDev d, double tol, uint32_t it) {
    __shared__ double buf[kPgBlock];
    const uint32_t cur = it & 1u, nxt = cur ^ 1u;
    if (d.state->stop[cur]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) d.state->stop[nxt] = 1u;
        return;
    }
    const double rz_new = pg_sum_slots(d.part_rz, pg_blocks(d.N), buf);
    const double rz_old = d.state->rz[cur];
    const double beta = rz_old != 0.0 ? rz_new / rz_old : 0.0;
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    if (v < d.N) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const size_t o = 6 * (size_t)v + k;
            d.p[o] = d.z[o] + beta * d.p[o];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool over = tol > 0.0 && sqrt(rz_new) <= tol * sqrt(d.state->rz0);
        d.state->rz[nxt] = rz_new;
        d.state->stop[nxt] = over ? 1u : 0u;
        d.state->iters = it + 1u;
        if (over) d.state->converged = 1u;
    }
}

// K12g.  One lane per node: the trial pose of an active node, a copy of the others; the workgroup's largest |x| to its slot.
__global__ __launch_bounds__(256) void k_pg_retract(const PgDev d, const double* __restrict__ poses, double* __restrict__ trial) {
    __shared__ double buf[kPgBlock];
    const uint32_t v = blockIdx.x * kPgBlock + threadIdx.x;
    double m = 0.0;
    if (v < d.N) {
        double P[12], x[6], out[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = poses[12 * (size_t)v + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            x[k] = d.x[6 * (size_t)v + k];
            m = fmax(m, fabs(x[k]));
        }
        if (d.active[v]) {
            pg_retract(P, x, out);
#pragma unroll
            for (int k = 0; k < 12; ++k) trial[12 * (size_t)v + k] = out[k];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) trial[12 * (size_t)v + k] = P[k];
        }
    }
    const double t = pg_block_max(m, buf);
    if (threadIdx.x == 0) d.part_max[blockIdx.x] = t;
}

// K12h.  One lane per edge: s_e and rho_e at the given poses; the workgroup's sums of s, rho and the outlier count to its three slots.
__global__ __launch_bounds__(256) void k_pg_cost(const PgDev d, const double* __restrict__ poses, double huber_k) {
    __shared__ double buf[kPgBlock];
    const uint32_t e = blockIdx.x * kPgBlock + threadIdx.x;
    double s = 0.0, rho = 0.0, out = 0.0;
    if (e < d.E) {
        double Pi[12], Pj[12], PZ[12], r[6];
        pg_load_edge_poses(d, poses, e, Pi, Pj, PZ);
        pg_residual(Pi, Pj, PZ, r);
        const double* __restrict__ om = d.info + 36 * (size_t)e;
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
        d.part_cost[blockIdx.x] = ts;
        d.part_cost[nb + blockIdx.x] = tr;
        d.part_cost[2 * nb + blockIdx.x] = to;
    }
}
// one workgroup: the record of a cost evaluation
__global__ __launch_bounds__(256) void k_pg_finish(const PgDev d, uint32_t n_cost_slots, int want_grad) {
    __shared__ double buf[kPgBlock];
    const double chi2 = pg_sum_slots(d.part_cost, n_cost_slots, buf);
    const double cost = pg_sum_slots(d.part_cost + n_cost_slots, n_cost_slots, buf);
    const double nout = pg_sum_slots(d.part_cost + 2 * (size_t)n_cost_slots, n_cost_slots, buf);
    double m = 0.0;
    for (uint32_t k = threadIdx.x; k < pg_blocks(d.N); k += kPgBlock) m = fmax(m, d.part_max[k]);
    const double dmax = pg_block_max(m, buf);
    double gm = 0.0;
    if (want_grad)
        for (uint32_t v = threadIdx.x; v < d.N; v += kPgBlock)
            if (d.active[v])
                for (int k = 0; k < 6; ++k) gm = fmax(gm, fabs(d.g[6 * (size_t)v + k]));
    const double ginf = pg_block_max(gm, buf);
    if (threadIdx.x == 0) {
        d.out->chi2 = chi2;
        d.out->cost = cost;
        d.out->n_outliers = nout;
        d.out->dmax = dmax;
        d.out->grad_inf = ginf;
    }
}

void launch_pg_linearize(hipStream_t s, const PgDev& d, const double* poses, double huber_k) {
    if (!d.E) return;
    hipLaunchKernelGGL(k_pg_linearize, dim3(pg_edge_group_blocks(d.E)), dim3(256), 0, s, d, poses, huber_k);
}

void launch_pg_nodes(hipStream_t s, const PgDev& d, double lambda, int sum) {
    if (!d.N) return;
    hipLaunchKernelGGL(k_pg_nodes, dim3((d.N + 3) / 4), dim3(256), 0, s, d, lambda, sum);
}

// chain: null for block Jacobi.  A preconditioner's apply comes where the <true> kernels form z themselves: after the first residual
// (first: it writes p = z too) and after every update (gated by the stop word, as every launch of an iteration is).
void launch_pg_pcg_begin(hipStream_t s, const PgDev& d, const PgcDev* chain, double tol) {
    if (!d.N) return;
    if (chain) {
        hipLaunchKernelGGL(k_pg_pcg_init<false>, dim3(pg_blocks(d.N)), dim3(256), 0, s, d);
        launch_pgc_apply(s, d, *chain, 0u, 0, 1);
    } else {
        hipLaunchKernelGGL(k_pg_pcg_init<true>, dim3(pg_blocks(d.N)), dim3(256), 0, s, d);
    }
    hipLaunchKernelGGL(k_pg_pcg_begin, dim3(1), dim3(256), 0, s, d, tol);
}

void launch_pg_pcg_iteration(hipStream_t s, const PgDev& d, const PgcDev* chain, double lambda, double tol, uint32_t it) {
    if (!d.N) return;
    hipLaunchKernelGGL(k_pg_spmv, dim3((d.N + kPgNodesPerBlock - 1) / kPgNodesPerBlock), dim3(256), 0, s, d, lambda, it);
    if (d.n_hubs) hipLaunchKernelGGL(k_pg_spmv_hub, dim3(d.n_hubs), dim3(64), 0, s, d, lambda, it);
    if (chain) {
        hipLaunchKernelGGL(k_pg_update<false>, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, it);
        launch_pgc_apply(s, d, *chain, it, 1, 0);
    } else {
        hipLaunchKernelGGL(k_pg_update<true>, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, it);
    }
    hipLaunchKernelGGL(k_pg_direction, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, tol, it);
}

void launch_pg_retract(hipStream_t s, const PgDev& d, const double* poses, double* trial) {
    if (!d.N) return;
    hipLaunchKernelGGL(k_pg_retract, dim3(pg_blocks(d.N)), dim3(256), 0, s, d, poses, trial);
}

void launch_pg_cost(hipStream_t s, const PgDev& d, const PgPriorDev* prior, const double* poses, double huber_k, double prior_huber_k, int want_grad) {
    const uint32_t nb = pg_blocks(d.E);
    if (nb) hipLaunchKernelGGL(k_pg_cost, dim3(nb), dim3(256), 0, s, d, poses, huber_k);
    hipLaunchKernelGGL(k_pg_finish, dim3(1), dim3(256), 0, s, d, nb, want_grad);
    if (prior) launch_pgp_cost(s, d, *prior, poses, prior_huber_k);
}

} // namespace elm
