// elm_k_pgchain.hip -- the pose graph's chain preconditioner (the contract is in include/elimaloc_hip.h, "pose graph", CHAIN
// PRECONDITIONER): z = M^-1 r for the block-tridiagonal M over the index chain v, v + 1, by block cyclic reduction.
// Gaussian elimination in odd-even order: every pivot is a Schur complement of the symmetric positive definite M, so none is searched
// for.  A level of n nodes is cut into segments of kPgcSeg = 256 consecutive nodes, one workgroup each.  In step t = 0 .. 7 the nodes
// p = 2^t - 1 + m 2^(t+1) of a segment are eliminated, each between its neighbours p - 2^t (for the first of them the last node of the
// segment before, the workgroup's slot "-1") and p + 2^t; after the eighth step the segment's last node alone is left, and the last
// nodes of all segments are the next level's chain.  The level of one segment eliminates its last node too.
//   K12i k_pgc_factor   once per (linearization, lambda) and level: G = pivot^-1 (inv6_ws, symmetrized), A = G M[p][left],
//                       B = G M[p][right]; the running blocks live in global memory, kernel-private to the workgroup
//   K12j k_pgc_fwd      per apply and level below the top: the right-hand side reduced in LDS, b_q -= B^T b_left + A^T b_right
//   K12k k_pgc_top      the top level: forward, the last node, back-substitution x_p = G b_p - A x_left - B x_right
//   K12l k_pgc_back     per level below the top, downwards: back-substitution from the level above's solution
// launch_pgc_apply is the preconditioner's side of the seam in launch_pg_pcg_begin and launch_pg_pcg_iteration (elm_k_pgraph.hip): the
// level-0 launch of k_pgc_top or k_pgc_back writes z, (first: p = z) and the workgroup's partial of r^T z to the slot k_pg_update<true>
// would have written.  A chain break is a zero coupling block; an inactive node and the padding of a segment are identity pivots with
// zero couplings and a zero right-hand side, so their z is 0.  Float64, no atomics, every sum in a fixed order; a remaining node
// gathers from its two eliminated neighbours, left first, so no two lanes write one block.
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"
#include "elm_la.hpp"

namespace elm {

namespace {

constexpr uint32_t kPgcInvLanes = 64; // lanes that invert at a time: 64 x (36 + 36) doubles of LDS

// G <- the symmetrized inverse of the block at G (ws_R, ws_m: 36 doubles of LDS each)
__device__ __forceinline__ void pgc_invert(double* G, double* ws_R, double* ws_m) {
    inv6_ws(G, ws_R, ws_m);
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) G[a * 6 + b] = 0.5 * (ws_R[a * 6 + b] + ws_R[b * 6 + a]);
}

// The right-hand side of the segment's nodes into s_b[(p + 1) * 6 ..], slot 0 (the node before the segment) zero.  Level 0: r; above:
// the last node of segment k of the level below, plus what segment k + 1 there added to it.
__device__ __forceinline__ void pgc_load_rhs(const PgDev& d, const PgcDev& c, const PgcLevel& lv, const PgcLevel& lo, int level0, double* s_b) {
    const uint32_t tid = threadIdx.x, k = blockIdx.x * kPgcSeg + tid;
    if (tid < 6u) s_b[tid] = 0.0;
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        double v = 0.0;
        if (level0) {
            if (k < d.N) v = d.rr[6 * (size_t)k + a];
        } else if (k < lv.n) {
            v = c.bl[6 * (size_t)(lo.soff + k) + a];
            if (k + 1u < lo.nseg) v = v + c.be[6 * (size_t)(lo.soff + k + 1u) + a];
        }
        s_b[(tid + 1u) * 6u + a] = v;
    }
}

// The forward steps on s_b; A, B: the blocks of the segment's first node.
__device__ __forceinline__ void pgc_forward(double* s_b, const double* __restrict__ A, const double* __restrict__ B) {
    const uint32_t tid = threadIdx.x;
#pragma unroll // (the eight steps with their strides as constants: what the compiler chose by itself before the sums were helper calls)
    for (uint32_t t = 0; t < kPgcSteps; ++t) {
        const uint32_t h = 1u << t, cnt = kPgcSeg >> (t + 1u);
        __syncthreads();
        if (tid <= cnt) {
            const uint32_t q1 = tid << (t + 1u); // q + 1: the slot of the remaining node q
            double acc[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[a] = s_b[q1 * 6u + a];
            if (tid >= 1u) { // q is the right neighbour of q - h
                const uint32_t pl = q1 - 1u - h;
                const double* __restrict__ Bp = B + 36 * (size_t)pl;
                double bp[6];
#pragma unroll
                for (int b = 0; b < 6; ++b) bp[b] = s_b[(pl + 1u) * 6u + b];
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[a] = acc[a] - pg_dot6_col(Bp + a, bp);
            }
            if (tid < cnt) { // q is the left neighbour of q + h
                const uint32_t pr = q1 - 1u + h;
                const double* __restrict__ Ap = A + 36 * (size_t)pr;
                double bp[6];
#pragma unroll
                for (int b = 0; b < 6; ++b) bp[b] = s_b[(pr + 1u) * 6u + b];
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[a] = acc[a] - pg_dot6_col(Ap + a, bp);
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) s_b[q1 * 6u + a] = acc[a];
        }
    }
}

// The back-substitution on s_b: slot 0 and the last slot hold the solution of the two nodes that the level above solved.
__device__ __forceinline__ void pgc_backward(double* s_b, const double* __restrict__ G, const double* __restrict__ A, const double* __restrict__ B) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = kPgcSteps; t-- > 0u;) {
        const uint32_t h = 1u << t, cnt = kPgcSeg >> (t + 1u);
        __syncthreads();
        if (tid < cnt) {
            const uint32_t p = h - 1u + (tid << (t + 1u));
            const double* __restrict__ Gp = G + 36 * (size_t)p;
            const double* __restrict__ Ap = A + 36 * (size_t)p;
            const double* __restrict__ Bp = B + 36 * (size_t)p;
            double bp[6], xl[6], xr[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                bp[b] = s_b[(p + 1u) * 6u + b];
                xl[b] = s_b[(p + 1u - h) * 6u + b];
                xr[b] = s_b[(p + 1u + h) * 6u + b];
            }
            double x[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) { // the three sums of pg_dot6 side by side: written apart, the loads of a step overlap less
                double g = Gp[a * 6] * bp[0], l = Ap[a * 6] * xl[0], r = Bp[a * 6] * xr[0];
#pragma unroll
                for (int b = 1; b < 6; ++b) {
                    g += Gp[a * 6 + b] * bp[b];
                    l += Ap[a * 6 + b] * xl[b];
                    r += Bp[a * 6 + b] * xr[b];
                }
                x[a] = (g - l) - r;
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) s_b[(p + 1u) * 6u + a] = x[a];
        }
    }
}

// The end of a level's back-substitution.  Level 0: z, with `first` p = z, and the workgroup's partial of r^T z; above: the solution.
__device__ __forceinline__ void pgc_finish(const PgDev& d, const PgcDev& c, const PgcLevel& lv, int level0, int first, const double* s_b, double* buf) {
    const uint32_t tid = threadIdx.x, k = blockIdx.x * kPgcSeg + tid;
    __syncthreads();
    if (!level0) {
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) c.y[6 * ((size_t)lv.off + k) + a] = s_b[(tid + 1u) * 6u + a];
        return;
    }
    double rz = 0.0;
    if (k < d.N) {
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) {
            const size_t o = 6 * (size_t)k + a;
            const double z = s_b[(tid + 1u) * 6u + a];
            d.z[o] = z;
            if (first) d.p[o] = z;
            rz += d.rr[o] * z;
        }
    }
    const double t = pg_block_sum(rz, buf);
    if (tid == 0u) d.part_rz[blockIdx.x] = t;
}

} // namespace

// K12i.  One workgroup per segment of the level.  The running diagonal block of a node is kept where its G will be, the running coupling
// to its left neighbour in Lw; both are this workgroup's alone, read and written between its own barriers.  Per step: the eliminated
// nodes (64 lanes at a time, each inverting in its own LDS workspace) write G, A and B; then every remaining node takes
// D_q -= M[q][left] B_left and D_q -= M[right][q]^T A_right, and its coupling to its new left neighbour -M[q][left] A_left.
__global__ __launch_bounds__(256) void k_pgc_factor(const PgDev d, const PgcDev c, const PgcLevel lv, const PgcLevel lo, int level0, double lambda) {
    __shared__ double s_R[kPgcInvLanes][36], s_m[kPgcInvLanes][36];
    const uint32_t tid = threadIdx.x, seg = blockIdx.x;
    const size_t base = (size_t)lv.off + (size_t)seg * kPgcSeg;
    double* G = c.G + 36 * base;
    double* A = c.A + 36 * base;
    double* B = c.B + 36 * base;
    double* L = c.Lw + 36 * base;
    double* De = c.De + 36 * (size_t)(lv.soff + seg);
    {
        const uint32_t k = seg * kPgcSeg + tid;
        double* Gp = G + 36 * (size_t)tid;
        double* Lp = L + 36 * (size_t)tid;
        if (level0) {
            const bool act = k < d.N && d.active[k] != 0;
            const uint32_t ent = (act && k > 0u && d.active[k - 1u] != 0) ? c.ce[k - 1u] : kPgcNoEdge;
            const bool link = ent != kPgcNoEdge;
            const size_t S = d.e_stride, e = link ? (size_t)(ent >> 1) : 0;
            const bool rev = (ent & 1u) != 0u;
            for (uint32_t a = 0; a < 6u; ++a)
                for (uint32_t b = 0; b < 6u; ++b) {
                    double h = a == b ? 1.0 : 0.0;
                    if (act) {
                        h = d.Hd[36 * (size_t)k + a * 6u + b];
                        if (a == b) h = h + lambda * h;
                    }
                    Gp[a * 6u + b] = h;
                    // M[k][k - 1]: H_ij^T of an edge stored k - 1 -> k, H_ij of one stored k -> k - 1
                    Lp[a * 6u + b] = link ? d.Hij[((rev ? a * 6u + b : b * 6u + a)) * S + e] : 0.0;
                }
        } else {
            const bool in = k < lv.n;
            const size_t src = 36 * ((size_t)lo.off + (size_t)k * kPgcSeg + (kPgcSeg - 1u));
            const bool more = in && k + 1u < lo.nseg;
            for (uint32_t i = 0; i < 36u; ++i) {
                double h = (i % 7u == 0u) ? 1.0 : 0.0, l = 0.0;
                if (in) {
                    h = c.G[src + i];
                    if (more) h = h + c.De[36 * (size_t)(lo.soff + k + 1u) + i];
                    l = c.Lw[src + i];
                }
                Gp[i] = h;
                Lp[i] = l;
            }
        }
        if (tid < 36u) De[tid] = 0.0;
    }
    for (uint32_t t = 0; t < kPgcSteps; ++t) {
        const uint32_t h = 1u << t, cnt = kPgcSeg >> (t + 1u);
        __syncthreads();
        for (uint32_t m0 = 0; m0 < cnt; m0 += kPgcInvLanes) {
            const uint32_t m = m0 + tid;
            if (tid < kPgcInvLanes && m < cnt) {
                const uint32_t p = h - 1u + (m << (t + 1u));
                double* Gp = G + 36 * (size_t)p;
                const double* Lp = L + 36 * (size_t)p;
                const double* Lr = L + 36 * (size_t)(p + h);
                double* Ap = A + 36 * (size_t)p;
                double* Bp = B + 36 * (size_t)p;
                pgc_invert(Gp, s_R[tid], s_m[tid]);
                for (int a = 0; a < 6; ++a)
                    for (int cc = 0; cc < 6; ++cc) {
                        const double sa = pg_mm6(Gp, Lp, a, cc), sb = pg_mmt6(Gp, Lr, a, cc); // G M[p][left], G M[right][p]^T
                        Ap[a * 6 + cc] = sa;
                        Bp[a * 6 + cc] = sb;
                    }
            }
        }
        __syncthreads();
        if (tid <= cnt) {
            const uint32_t q1 = tid << (t + 1u); // q + 1
            double* Dq = tid == 0u ? De : G + 36 * (size_t)(q1 - 1u);
            if (tid >= 1u) {
                const double* Lq = L + 36 * (size_t)(q1 - 1u);
                const double* Bl = B + 36 * (size_t)(q1 - 1u - h);
                for (int a = 0; a < 6; ++a)
                    for (int cc = 0; cc < 6; ++cc) Dq[a * 6 + cc] = Dq[a * 6 + cc] - pg_mm6(Lq, Bl, a, cc);
            }
            if (tid < cnt) {
                const double* Lr = L + 36 * (size_t)(q1 - 1u + h);
                const double* Ar = A + 36 * (size_t)(q1 - 1u + h);
                for (int a = 0; a < 6; ++a)
                    for (int cc = 0; cc < 6; ++cc) Dq[a * 6 + cc] = Dq[a * 6 + cc] - pg_mtm6(Lr, Ar, a, cc);
            }
            if (tid >= 1u) {
                double* Lq = L + 36 * (size_t)(q1 - 1u);
                const double* Al = A + 36 * (size_t)(q1 - 1u - h);
                for (int a = 0; a < 6; ++a) {
                    double row[6];
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) row[cc] = -pg_mm6(Lq, Al, a, cc);
#pragma unroll
                    for (int cc = 0; cc < 6; ++cc) Lq[a * 6 + cc] = row[cc];
                }
            }
        }
    }
    if (lv.nseg == 1u) { // the top: the last node has no neighbour left
        __syncthreads();
        if (tid == 0u) pgc_invert(G + 36 * (size_t)(kPgcSeg - 1u), s_R[0], s_m[0]);
    }
}

// K12j.
__global__ __launch_bounds__(256) void k_pgc_fwd(const PgDev d, const PgcDev c, const PgcLevel lv, const PgcLevel lo, int level0, uint32_t it, int gate) {
    __shared__ double s_b[(kPgcSeg + 1u) * 6u];
    if (gate && d.state->stop[it & 1u]) return;
    const uint32_t tid = threadIdx.x, seg = blockIdx.x;
    const size_t base = (size_t)lv.off + (size_t)seg * kPgcSeg;
    pgc_load_rhs(d, c, lv, lo, level0, s_b);
    pgc_forward(s_b, c.A + 36 * base, c.B + 36 * base);
    __syncthreads();
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) c.y[6 * (base + tid) + a] = s_b[(tid + 1u) * 6u + a];
    if (tid < 6u) {
        c.bl[6 * (size_t)(lv.soff + seg) + tid] = s_b[kPgcSeg * 6u + tid];
        c.be[6 * (size_t)(lv.soff + seg) + tid] = s_b[tid];
    }
}

// K12k.  One workgroup: the level of one segment.
__global__ __launch_bounds__(256) void k_pgc_top(const PgDev d, const PgcDev c, const PgcLevel lv, const PgcLevel lo, int level0, uint32_t it, int gate,
                                                 int first) {
    __shared__ double s_b[(kPgcSeg + 1u) * 6u];
    __shared__ double buf[kPgBlock];
    if (gate && d.state->stop[it & 1u]) return;
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)lv.off;
    pgc_load_rhs(d, c, lv, lo, level0, s_b);
    pgc_forward(s_b, c.A + 36 * base, c.B + 36 * base);
    __syncthreads();
    double x = 0.0;
    if (tid < 6u) {
        const double* __restrict__ Gp = c.G + 36 * (base + kPgcSeg - 1u) + 6u * tid; // the lane's row
        x = pg_dot6(Gp, s_b + kPgcSeg * 6u);
    }
    __syncthreads();
    if (tid < 6u) s_b[kPgcSeg * 6u + tid] = x;
    pgc_backward(s_b, c.G + 36 * base, c.A + 36 * base, c.B + 36 * base);
    pgc_finish(d, c, lv, level0, first, s_b, buf);
}

// K12l.  up: the level above, whose solution is in y.
__global__ __launch_bounds__(256) void k_pgc_back(const PgDev d, const PgcDev c, const PgcLevel lv, const PgcLevel up, int level0, uint32_t it, int gate,
                                                  int first) {
    __shared__ double s_b[(kPgcSeg + 1u) * 6u];
    __shared__ double buf[kPgBlock];
    if (gate && d.state->stop[it & 1u]) return;
    const uint32_t tid = threadIdx.x, seg = blockIdx.x;
    const size_t base = (size_t)lv.off + (size_t)seg * kPgcSeg;
    const double* src = tid == kPgcSeg - 1u ? c.y + 6 * ((size_t)up.off + seg) : c.y + 6 * (base + tid);
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) s_b[(tid + 1u) * 6u + a] = src[a];
    if (tid < 6u) s_b[tid] = seg > 0u ? c.y[6 * ((size_t)up.off + seg - 1u) + tid] : 0.0;
    pgc_backward(s_b, c.G + 36 * base, c.A + 36 * base, c.B + 36 * base);
    pgc_finish(d, c, lv, level0, first, s_b, buf);
}

void launch_pgc_factor(hipStream_t s, const PgDev& d, const PgcDev& c, double lambda) {
    if (!d.N) return;
    PgcLevel lv[kPgcMaxLevels];
    const uint32_t nl = pgc_levels(d.N, lv);
    for (uint32_t l = 0; l < nl; ++l)
        hipLaunchKernelGGL(k_pgc_factor, dim3(lv[l].nseg), dim3(256), 0, s, d, c, lv[l], lv[l ? l - 1 : 0], l == 0 ? 1 : 0, lambda);
}

void launch_pgc_apply(hipStream_t s, const PgDev& d, const PgcDev& c, uint32_t it, int gate, int first) {
    PgcLevel lv[kPgcMaxLevels];
    const uint32_t nl = pgc_levels(d.N, lv), top = nl - 1;
    for (uint32_t l = 0; l < top; ++l)
        hipLaunchKernelGGL(k_pgc_fwd, dim3(lv[l].nseg), dim3(256), 0, s, d, c, lv[l], lv[l ? l - 1 : 0], l == 0 ? 1 : 0, it, gate);
    hipLaunchKernelGGL(k_pgc_top, dim3(1), dim3(256), 0, s, d, c, lv[top], lv[top ? top - 1 : 0], top == 0 ? 1 : 0, it, gate, first);
    for (uint32_t l = top; l-- > 0u;)
        hipLaunchKernelGGL(k_pgc_back, dim3(lv[l].nseg), dim3(256), 0, s, d, c, lv[l], lv[l + 1], l == 0 ? 1 : 0, it, gate, first);
}
} // namespace elm
