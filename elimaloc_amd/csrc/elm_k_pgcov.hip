// elm_k_pgcov.hip -- columns of the inverse of the pose graph's damped normal equations (elm_posegraph_covariance; the contract is in
// include/elimaloc_hip_posegraph_cov.h): the conjugate gradients of elm_k_pgraph.hip for many unit right-hand sides
// at once.  The requested columns are cut into groups of 64 and THE LANE IS THE COLUMN: the vectors x, r, z, p, q of a group are
// [N][6][64], so a wavefront's access to one component of one node is one 512-byte row, a 6 x 6 block of H or of Minv has the same
// address in every lane (the wave index comes through readfirstlane, so the block's loads can be scalar loads) and every inner product
// is a sum inside the lane until the reduction over nodes.  Float64, no float atomics, no contraction.  The orders:
//   a row of q_v        the diagonal block's six products, then the incidence list in ascending edge index, six products per entry
//                       (the order of pg_spmv_row)
//   p^T q, r^T z        per lane over the wavefront's kPgcovNodesPerWave nodes in node order (components 0 .. 5 inside a node), the four
//                       wavefronts of the workgroup added in wave order -> slot [workgroup][group][64]; the slots by the sixteen
//                       wavefronts of k_pgcov_alpha / k_pgcov_beta, wavefront w adding slots w, w + 16, ... in ascending order, the
//                       sixteen sums added in wave order.  Nothing in it depends on anything but N.
// A column whose stop word is set is frozen: none of its lanes writes a vector or a state word again.  A group whose 64 columns have
// all stopped ends the launches of its workgroups at their first instruction; the word all_stop (every group has stopped) is what the
// host reads.  The state words of an iteration are those of its parity, as in PgState.
//   K13a k_pgcov_begin   r = e, z = p = the column of Minv, r0^T z0 = Minv[c][c]; the stop words of a zero right-hand side
//   K13b k_pgcov_spmv    one wavefront per (kPgcovNodesPerWave nodes, group): q = (H + lambda diag H) p, slots of p^T q
//   K13c k_pgcov_alpha   one workgroup per group: alpha per column
//   K13d k_pgcov_update  x, r, z = Minv r (block Jacobi, fused), slots of r^T z
//   K13e k_pgcov_beta    one workgroup per group: beta, r^T z, the stop test, the iteration count per column; the group's stop word
//   K13f k_pgcov_dir     p = z + beta p; the first workgroup folds the groups' stop words into all_stop
//   K13g k_pgcov_gather  the requested 6 x 6 blocks of x into the download buffer
//   K13h .. K13j         the chain preconditioner's apply for column groups, in place of K13d's z (described where they stand)
// A hub has no kernel of its own: its wavefront walks the whole incidence list (DESIGN.md section 26 says what that costs).
#include <hip/hip_runtime.h>

#include "elm_dev_pgraph.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

// the first double of node v's [6][64] tile in group g
__device__ __forceinline__ size_t cv_at(uint32_t N, uint32_t g, uint32_t v) { return ((size_t)g * N + v) * (6u * kPgcovLanes); }

__device__ __forceinline__ uint32_t wave_index() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// The sum of one value per lane over the workgroup's four wavefronts in wave order; wavefront 0 returns it.
__device__ __forceinline__ double cov_wave_sum4(double v, uint32_t wave, uint32_t lane, double (*s)[kPgcovLanes]) {
    s[wave][lane] = v;
    __syncthreads();
    return ((s[0][lane] + s[1][lane]) + s[2][lane]) + s[3][lane];
}

// The sum of the nb slots of (group g, this lane): wavefront w of the sixteen adds slots w, w + 16, ... ascending, then the sixteen in
// wave order.  Every lane of wavefront 0 returns its column's sum.
__device__ __forceinline__ double cov_sum_slots(const double* __restrict__ slots, uint32_t nb, uint32_t G, uint32_t g, uint32_t wave, uint32_t lane,
                                                double (*s)[kPgcovLanes]) {
    double t = 0.0;
    for (uint32_t k = wave; k < nb; k += kPgcovReduceWaves) t += slots[((size_t)k * G + g) * kPgcovLanes + lane];
    s[wave][lane] = t;
    __syncthreads();
    double sum = s[0][lane];
#pragma unroll
    for (uint32_t w = 1; w < kPgcovReduceWaves; ++w) sum += s[w][lane];
    return sum;
}

// q_v of one active node for the lane's column: every pointer but p and q holds the same address in all 64 lanes.
__device__ __forceinline__ void cov_node_row(const double* __restrict__ Hd, const double* __restrict__ Hij, size_t S, const uint32_t* __restrict__ inc,
                                             const int32_t* __restrict__ ei, const int32_t* __restrict__ ej, uint32_t k0, uint32_t k1,
                                             const double* __restrict__ p, size_t group_base, uint32_t lane, double lambda, const double p6[6],
                                             double q6[6]) {
#pragma unroll
    for (uint32_t a = 0; a < 6u; ++a) {
        double qv = 0.0;
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) {
            double h = Hd[a * 6u + b];
            if (b == a) h = h + lambda * h;
            qv += h * p6[b];
        }
        q6[a] = qv;
    }
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t ent = inc[k], e = ent >> 1;
        const uint32_t nb = (uint32_t)((ent & 1u) ? ei[e] : ej[e]);
        const double* __restrict__ pn = p + group_base + (size_t)nb * (6u * kPgcovLanes) + lane;
        double n6[6];
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) n6[b] = pn[b * kPgcovLanes];
        const double* __restrict__ H = Hij + e;
        if (ent & 1u) { // v is j: H_ij^T p_i
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a)
#pragma unroll
                for (uint32_t b = 0; b < 6u; ++b) q6[a] += H[(b * 6u + a) * S] * n6[b];
        } else {
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a)
#pragma unroll
                for (uint32_t b = 0; b < 6u; ++b) q6[a] += H[(a * 6u + b) * S] * n6[b];
        }
    }
}

// The wavefront's nodes v0 .. of K13b: q of the lane's column (written when the column is live) -> the lane's part of p^T q.  One function
// with every array restrict-qualified, the stores to q included, so that the loads of the blocks, the lists and the flags -- whose
// addresses are the same in all 64 lanes -- are known not to be clobbered and can be scalar loads.
__device__ __forceinline__ double cov_spmv_nodes(const double* __restrict__ Hd, const double* __restrict__ Hij, size_t S, const uint32_t* __restrict__ inc_start,
                                                 const uint32_t* __restrict__ inc, const int32_t* __restrict__ ei, const int32_t* __restrict__ ej,
                                                 const uint8_t* __restrict__ active, uint32_t N, const double* __restrict__ p, double* __restrict__ q,
                                                 size_t group_base, uint32_t v0, uint32_t lane, double lambda, bool live) {
    double pq = 0.0;
    for (uint32_t k = 0; k < kPgcovNodesPerWave; ++k) {
        const uint32_t v = v0 + k;
        if (v >= N) break;
        if (!active[v]) continue; // q, p, r, x of an inactive node stay zero
        const size_t o = group_base + (size_t)v * (6u * kPgcovLanes) + lane;
        double p6[6], q6[6];
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) p6[b] = p[o + b * kPgcovLanes];
        cov_node_row(Hd + 36 * (size_t)v, Hij, S, inc, ei, ej, inc_start[v], inc_start[v + 1], p, group_base, lane, lambda, p6, q6);
        if (live) {
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) q[o + a * kPgcovLanes] = q6[a];
        }
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) pq += p6[a] * q6[a];
    }
    return pq;
}

// The wavefront's nodes of K13d for a live column: x, r, z = Minv r a row at a time (as k_pg_update<true> forms it) -> the lane's part of r^T z.
template <bool kJacobi>
__device__ __forceinline__ double cov_update_nodes(const double* __restrict__ Minv, const uint8_t* __restrict__ active, uint32_t N, double* __restrict__ x,
                                                   double* __restrict__ r, double* __restrict__ z, const double* __restrict__ p,
                                                   const double* __restrict__ q, size_t group_base, uint32_t v0, uint32_t lane, double alpha) {
    double rz = 0.0;
    for (uint32_t k = 0; k < kPgcovNodesPerWave; ++k) {
        const uint32_t v = v0 + k;
        if (v >= N) break;
        if (!active[v]) continue;
        const size_t o = group_base + (size_t)v * (6u * kPgcovLanes) + lane;
        const double* __restrict__ M = Minv + 36 * (size_t)v;
        double r6[6];
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) {
            const size_t at = o + a * kPgcovLanes;
            x[at] = x[at] + alpha * p[at];
            r6[a] = r[at] - alpha * q[at];
            r[at] = r6[a];
        }
        if constexpr (kJacobi) {
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) {
                const double t = pg_dot6(M + a * 6u, r6);
                z[o + a * kPgcovLanes] = t;
                rz += r6[a] * t;
            }
        }
    }
    return rz;
}

} // namespace

// K13a.  One wavefront per group.  Column col0 + 64 g + lane is component c of node col_nodes[column / 6]; a column past the request or of
// an inactive node keeps the zero vectors of the memset before it and stops at once (with a tolerance), converged.
template <bool kJacobi>
__global__ __launch_bounds__(64) void k_pgcov_begin(const PgDev d, const PgCovDev c, double tol) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x, col = g * kPgcovLanes + lane;
    const uint32_t j = c.col0 + col;
    double rz0 = 0.0;
    if (j < c.n_cols) {
        const uint32_t v = (uint32_t)c.col_nodes[j / 6u], comp = j % 6u;
        if (d.active[v]) {
            const double* __restrict__ M = d.Minv + 36 * (size_t)v;
            const size_t o = cv_at(d.N, g, v) + lane;
            if constexpr (kJacobi) {
#pragma unroll
                for (uint32_t a = 0; a < 6u; ++a) {
                    const double t = M[a * 6u + comp];
                    c.z[o + a * kPgcovLanes] = t;
                    c.p[o + a * kPgcovLanes] = t;
                }
                rz0 = M[comp * 6u + comp]; // r^T z of r = e
            }
            c.r[o + comp * kPgcovLanes] = 1.0;
        }
    }
    const bool over = kJacobi && tol > 0.0 && !(rz0 > 0.0); // (with a chain k_pgcov_begin_rz says, after the first apply)
    const uint32_t cols = c.G * kPgcovLanes;
    c.rz[col] = rz0;
    c.rz[cols + col] = 0.0;
    c.rz0[col] = rz0;
    c.rzf[col] = rz0;
    c.alpha[col] = 0.0;
    c.beta[col] = 0.0;
    c.stop[col] = over ? 1u : 0u;
    c.stop[cols + col] = 0u;
    c.iters[col] = 0u;
    c.converged[col] = over ? 1u : 0u;
    const bool all = __ballot(over) == ~0ull;
    if (lane == 0u) {
        c.gstop[g] = all ? 1u : 0u;
        c.gstop[c.G + g] = 0u;
    }
}

// K13b.  grid (pgcov_blocks(N), G); wavefront w of a workgroup takes the nodes (4 blockIdx.x + w) kPgcovNodesPerWave ... one after another.
__global__ __launch_bounds__(256) void k_pgcov_spmv(const PgDev d, const PgCovDev c, double lambda, uint32_t it) {
    __shared__ double s_part[4][kPgcovLanes];
    const uint32_t cur = it & 1u, g = blockIdx.y;
    if (c.gstop[cur * c.G + g]) return; // (the same for the whole workgroup: no barrier is left waiting)
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const bool live = c.stop[(cur * c.G + g) * kPgcovLanes + lane] == 0u;
    const uint32_t v0 = (blockIdx.x * 4u + wave) * kPgcovNodesPerWave;
    const double pq = cov_spmv_nodes(d.Hd, d.Hij, d.e_stride, d.inc_start, d.inc, d.ei, d.ej, d.active, d.N, c.p, c.q, cv_at(d.N, g, 0u), v0, lane, lambda, live);
    const double t = cov_wave_sum4(pq, wave, lane, s_part);
    if (threadIdx.x < kPgcovLanes && live) c.slot_pq[((size_t)blockIdx.x * c.G + g) * kPgcovLanes + lane] = t;
}

// K13c.  One workgroup of sixteen wavefronts per group.
__global__ __launch_bounds__(1024) void k_pgcov_alpha(const PgDev d, const PgCovDev c, uint32_t it) {
    __shared__ double s[kPgcovReduceWaves][kPgcovLanes];
    const uint32_t cur = it & 1u, g = blockIdx.x;
    if (c.gstop[cur * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const double pq = cov_sum_slots(c.slot_pq, pgcov_blocks(d.N), c.G, g, wave, lane, s);
    if (threadIdx.x >= kPgcovLanes) return;
    const uint32_t cols = c.G * kPgcovLanes, col = g * kPgcovLanes + lane;
    if (c.stop[cur * cols + col]) return;
    const double rz_old = c.rz[cur * cols + col];
    c.alpha[col] = pq != 0.0 ? rz_old / pq : 0.0;
}

// K13d.  The geometry of K13b.
template <bool kJacobi>
__global__ __launch_bounds__(256) void k_pgcov_update(const PgDev d, const PgCovDev c, uint32_t it) {
    __shared__ double s_part[4][kPgcovLanes];
    const uint32_t cur = it & 1u, g = blockIdx.y;
    if (c.gstop[cur * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const uint32_t col = g * kPgcovLanes + lane;
    const bool live = c.stop[cur * c.G * kPgcovLanes + col] == 0u;
    const double alpha = c.alpha[col];
    const uint32_t v0 = (blockIdx.x * 4u + wave) * kPgcovNodesPerWave;
    double rz = 0.0;
    if (live) rz = cov_update_nodes<kJacobi>(d.Minv, d.active, d.N, c.x, c.r, c.z, c.p, c.q, cv_at(d.N, g, 0u), v0, lane, alpha);
    if constexpr (!kJacobi) return; // z and the slots of r^T z are the chain apply's
    const double t = cov_wave_sum4(rz, wave, lane, s_part);
    if (threadIdx.x < kPgcovLanes && live) c.slot_rz[((size_t)blockIdx.x * c.G + g) * kPgcovLanes + lane] = t;
}

// K13e.  One workgroup of sixteen wavefronts per group: the next iteration's words of every column, and of the group.
__global__ __launch_bounds__(1024) void k_pgcov_beta(const PgDev d, const PgCovDev c, double tol, uint32_t it, uint32_t n_slots) {
    __shared__ double s[kPgcovReduceWaves][kPgcovLanes];
    const uint32_t cur = it & 1u, nxt = cur ^ 1u, g = blockIdx.x;
    const uint32_t cols = c.G * kPgcovLanes, col = g * kPgcovLanes + (threadIdx.x & 63u);
    if (c.gstop[cur * c.G + g]) {
        if (threadIdx.x < kPgcovLanes) c.stop[nxt * cols + col] = 1u;
        if (threadIdx.x == 0u) c.gstop[nxt * c.G + g] = 1u;
        return;
    }
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const double rz_new = cov_sum_slots(c.slot_rz, n_slots, c.G, g, wave, lane, s);
    if (threadIdx.x >= kPgcovLanes) return;
    bool over = true;
    if (!c.stop[cur * cols + col]) {
        const double rz_old = c.rz[cur * cols + col];
        over = tol > 0.0 && sqrt(rz_new) <= tol * sqrt(c.rz0[col]);
        c.beta[col] = rz_old != 0.0 ? rz_new / rz_old : 0.0;
        c.rz[nxt * cols + col] = rz_new;
        c.rzf[col] = rz_new;
        c.iters[col] = it + 1u;
        if (over) c.converged[col] = 1u;
    }
    c.stop[nxt * cols + col] = over ? 1u : 0u;
    const bool all = __ballot(over) == ~0ull;
    if (lane == 0u) c.gstop[nxt * c.G + g] = all ? 1u : 0u;
}

// K13f.  The geometry of K13b.  The first workgroup folds the groups' words of the next parity (written by K13e, the launch before).
__global__ __launch_bounds__(256) void k_pgcov_dir(const PgDev d, const PgCovDev c, uint32_t it) {
    const uint32_t cur = it & 1u, nxt = cur ^ 1u, g = blockIdx.y;
    if (blockIdx.x == 0u && blockIdx.y == 0u) {
        int mine = 1;
        for (uint32_t k = threadIdx.x; k < c.G; k += 256u) mine &= c.gstop[nxt * c.G + k] ? 1 : 0;
        const int all = __syncthreads_and(mine);
        if (threadIdx.x == 0u) c.all_stop[nxt] = all ? 1u : 0u;
    }
    if (c.gstop[cur * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const uint32_t col = g * kPgcovLanes + lane;
    if (c.stop[cur * c.G * kPgcovLanes + col]) return;
    const double beta = c.beta[col];
    const uint32_t v0 = (blockIdx.x * 4u + wave) * kPgcovNodesPerWave;
    for (uint32_t k = 0; k < kPgcovNodesPerWave; ++k) {
        const uint32_t v = v0 + k;
        if (v >= d.N) break;
        if (!d.active[v]) continue;
        const size_t o = cv_at(d.N, g, v) + lane;
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) {
            const size_t at = o + a * kPgcovLanes;
            c.p[at] = c.z[at] + beta * c.p[at];
        }
    }
}

// K13g.  One lane per entry of a requested block: entry (a, comp) of pair k is component a of node row[k] in column 6 ci[k] + comp, when
// that column is one of this pass.
__global__ __launch_bounds__(256) void k_pgcov_gather(const PgDev d, const PgCovDev c, const uint32_t* __restrict__ ci, const int32_t* __restrict__ row,
                                                      uint32_t n_pairs, double* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)n_pairs * 36u) return;
    const uint32_t k = (uint32_t)(t / 36u), e = (uint32_t)(t % 36u), a = e / 6u, comp = e % 6u;
    const uint32_t j = 6u * ci[k] + comp;
    if (j < c.col0 || j - c.col0 >= c.G * kPgcovLanes) return;
    const uint32_t g = (j - c.col0) / kPgcovLanes, lane = (j - c.col0) % kPgcovLanes;
    out[t] = c.x[cv_at(d.N, g, (uint32_t)row[k]) + a * kPgcovLanes + lane];
}

// ---- the chain preconditioner's apply for column groups (the factor is elm_k_pgchain.hip's, unchanged; the levels are pgc_levels').  One
// workgroup of kPgccovWaves wavefronts per (segment, group), the lane is the column; the same odd-even forward steps, top level and
// back-substitution as K12j .. K12l, but in place on the group's y in global memory between the workgroup's barriers (257 x 6 x 64 doubles
// do not fit LDS); the nodes of a step are dealt to the wavefronts w, w + 16, ...  G, A and B have the same address in every lane.
//   K13h k_pgccov_fwd   per level below the top: the right-hand side into y, reduced; the addition to the segment before into be
//   K13i k_pgccov_top   the top level: forward, the last node, back-substitution
//   K13j k_pgccov_back  per level below the top, downwards
// The level-0 launch of K13i or K13j writes z, on the first apply p = z, and the segment's slot of r^T z per column.
namespace {

constexpr size_t kCovTile = 6u * kPgcovLanes;

// node k of the level lv for this lane: level 0 takes r, a level above the last node of segment k below plus what segment k + 1 added to it
__device__ __forceinline__ void ccov_load_rhs(const PgDev& d, const PgCovDev& c, const PgcLevel& lv, const PgcLevel& lo, int level0, uint32_t g, uint32_t seg,
                                              uint32_t wave, uint32_t lane, double* y_seg, double* e_seg) {
    const double* y_g = c.y + (size_t)g * c.y_pad * kCovTile + lane;
    const double* e_g = c.be + (size_t)g * c.y_segs * kCovTile + lane;
    for (uint32_t k = wave; k < kPgcSeg; k += kPgccovWaves) {
        const uint32_t idx = seg * kPgcSeg + k;
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) {
            double v = 0.0;
            if (level0) {
                if (idx < d.N) v = c.r[cv_at(d.N, g, idx) + a * kPgcovLanes + lane];
            } else if (idx < lv.n) {
                v = y_g[((size_t)lo.off + (size_t)idx * kPgcSeg + (kPgcSeg - 1u)) * kCovTile + a * kPgcovLanes];
                if (idx + 1u < lo.nseg) v = v + e_g[(size_t)(lo.soff + idx + 1u) * kCovTile + a * kPgcovLanes];
            }
            y_seg[(size_t)k * kCovTile + a * kPgcovLanes] = v;
        }
    }
    if (wave == 0u) {
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) e_seg[a * kPgcovLanes] = 0.0;
    }
}

// y: node 0 of the segment for this lane (node k, component a at y[k * kCovTile + 64 a]); e: the slot of the node before the segment
__device__ __forceinline__ void ccov_forward(double* __restrict__ y, double* __restrict__ e, const double* __restrict__ A, const double* __restrict__ B,
                                             uint32_t wave) {
    for (uint32_t t = 0; t < kPgcSteps; ++t) {
        const uint32_t h = 1u << t, cnt = kPgcSeg >> (t + 1u);
        __syncthreads();
        for (uint32_t m = wave; m <= cnt; m += kPgccovWaves) {
            const uint32_t q1 = m << (t + 1u); // q + 1: the slot of the remaining node q
            double* slot = q1 ? y + (size_t)(q1 - 1u) * kCovTile : e;
            double acc[6];
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) acc[a] = slot[a * kPgcovLanes];
            if (m >= 1u) { // q is the right neighbour of q - h
                const uint32_t pl = q1 - 1u - h;
                const double* __restrict__ Bp = B + 36 * (size_t)pl;
                double bp[6];
#pragma unroll
                for (uint32_t b = 0; b < 6u; ++b) bp[b] = y[(size_t)pl * kCovTile + b * kPgcovLanes];
#pragma unroll
                for (uint32_t a = 0; a < 6u; ++a) acc[a] = acc[a] - pg_dot6_col(Bp + a, bp);
            }
            if (m < cnt) { // q is the left neighbour of q + h
                const uint32_t pr = q1 - 1u + h;
                const double* __restrict__ Ap = A + 36 * (size_t)pr;
                double bp[6];
#pragma unroll
                for (uint32_t b = 0; b < 6u; ++b) bp[b] = y[(size_t)pr * kCovTile + b * kPgcovLanes];
#pragma unroll
                for (uint32_t a = 0; a < 6u; ++a) acc[a] = acc[a] - pg_dot6_col(Ap + a, bp);
            }
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) slot[a * kPgcovLanes] = acc[a];
        }
    }
}

// the back-substitution in place: y's last node holds its solution already; xl: the solution of the node before the segment, or null for 0
__device__ __forceinline__ void ccov_backward(double* __restrict__ y, const double* __restrict__ xl0, const double* __restrict__ G,
                                              const double* __restrict__ A, const double* __restrict__ B, uint32_t wave) {
    for (uint32_t t = kPgcSteps; t-- > 0u;) {
        const uint32_t h = 1u << t, cnt = kPgcSeg >> (t + 1u);
        __syncthreads();
        for (uint32_t m = wave; m < cnt; m += kPgccovWaves) {
            const uint32_t p = h - 1u + (m << (t + 1u));
            const double* __restrict__ Gp = G + 36 * (size_t)p;
            const double* __restrict__ Ap = A + 36 * (size_t)p;
            const double* __restrict__ Bp = B + 36 * (size_t)p;
            double bp[6], xl[6], xr[6];
#pragma unroll
            for (uint32_t b = 0; b < 6u; ++b) {
                bp[b] = y[(size_t)p * kCovTile + b * kPgcovLanes];
                xr[b] = y[(size_t)(p + h) * kCovTile + b * kPgcovLanes];
                if (p >= h) xl[b] = y[(size_t)(p - h) * kCovTile + b * kPgcovLanes];
                else xl[b] = xl0 ? xl0[b * kPgcovLanes] : 0.0;
            }
            double x[6];
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) x[a] = (pg_dot6(Gp + a * 6u, bp) - pg_dot6(Ap + a * 6u, xl)) - pg_dot6(Bp + a * 6u, xr);
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) y[(size_t)p * kCovTile + a * kPgcovLanes] = x[a];
        }
    }
}

// level 0, after the back-substitution: z (and p) of the live columns, and the segment's slot of r^T z
__device__ __forceinline__ void ccov_finish(const PgDev& d, const PgCovDev& c, uint32_t g, uint32_t seg, uint32_t wave, uint32_t lane, uint32_t cur, int first,
                                            const double* y_seg, double (*s)[kPgcovLanes]) {
    __syncthreads();
    const bool live = c.stop[(cur * c.G + g) * kPgcovLanes + lane] == 0u;
    double rz = 0.0;
    if (live) {
        for (uint32_t k = wave; k < kPgcSeg; k += kPgccovWaves) {
            const uint32_t v = seg * kPgcSeg + k;
            if (v >= d.N) break;
            const size_t o = cv_at(d.N, g, v) + lane;
#pragma unroll
            for (uint32_t a = 0; a < 6u; ++a) {
                const double z = y_seg[(size_t)k * kCovTile + a * kPgcovLanes];
                c.z[o + a * kPgcovLanes] = z;
                if (first) c.p[o + a * kPgcovLanes] = z;
                rz += c.r[o + a * kPgcovLanes] * z;
            }
        }
    }
    s[wave][lane] = rz;
    __syncthreads();
    if (threadIdx.x < kPgcovLanes && live) {
        double sum = s[0][lane];
#pragma unroll
        for (uint32_t w = 1; w < kPgccovWaves; ++w) sum += s[w][lane];
        c.slot_rz[((size_t)seg * c.G + g) * kPgcovLanes + lane] = sum;
    }
}

} // namespace

// K13h.  grid (the level's segments, G).
__global__ __launch_bounds__(1024) void k_pgccov_fwd(const PgDev d, const PgCovDev c, const PgcDev f, const PgcLevel lv, const PgcLevel lo, int level0, uint32_t it) {
    const uint32_t g = blockIdx.y, seg = blockIdx.x;
    if (c.gstop[(it & 1u) * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const size_t base = (size_t)lv.off + (size_t)seg * kPgcSeg;
    double* y_seg = c.y + ((size_t)g * c.y_pad + base) * kCovTile + lane;
    double* e_seg = c.be + ((size_t)g * c.y_segs + lv.soff + seg) * kCovTile + lane;
    ccov_load_rhs(d, c, lv, lo, level0, g, seg, wave, lane, y_seg, e_seg);
    ccov_forward(y_seg, e_seg, f.A + 36 * base, f.B + 36 * base, wave);
}

// K13i.  grid (1, G): the level of one segment.
__global__ __launch_bounds__(1024) void k_pgccov_top(const PgDev d, const PgCovDev c, const PgcDev f, const PgcLevel lv, const PgcLevel lo, int level0, uint32_t it,
                                                     int first) {
    __shared__ double s[kPgccovWaves][kPgcovLanes];
    const uint32_t g = blockIdx.y, cur = it & 1u;
    if (c.gstop[cur * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const size_t base = (size_t)lv.off;
    double* y_seg = c.y + ((size_t)g * c.y_pad + base) * kCovTile + lane;
    double* e_seg = c.be + ((size_t)g * c.y_segs + lv.soff) * kCovTile + lane;
    ccov_load_rhs(d, c, lv, lo, level0, g, 0u, wave, lane, y_seg, e_seg);
    ccov_forward(y_seg, e_seg, f.A + 36 * base, f.B + 36 * base, wave);
    __syncthreads();
    if (wave == 0u) { // the last node has no neighbour left: its G is the inverse of its block
        const double* __restrict__ Gp = f.G + 36 * (base + kPgcSeg - 1u);
        double* last = y_seg + (size_t)(kPgcSeg - 1u) * kCovTile;
        double b[6], x[6];
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) b[a] = last[a * kPgcovLanes];
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) x[a] = pg_dot6(Gp + a * 6u, b);
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) last[a * kPgcovLanes] = x[a];
    }
    ccov_backward(y_seg, nullptr, f.G + 36 * base, f.A + 36 * base, f.B + 36 * base, wave);
    if (level0) ccov_finish(d, c, g, 0u, wave, lane, cur, first, y_seg, s);
}

// K13j.  grid (the level's segments, G); up: the level above, whose solution is in y.
__global__ __launch_bounds__(1024) void k_pgccov_back(const PgDev d, const PgCovDev c, const PgcDev f, const PgcLevel lv, const PgcLevel up, int level0, uint32_t it,
                                                      int first) {
    __shared__ double s[kPgccovWaves][kPgcovLanes];
    const uint32_t g = blockIdx.y, seg = blockIdx.x, cur = it & 1u;
    if (c.gstop[cur * c.G + g]) return;
    const uint32_t wave = wave_index(), lane = threadIdx.x & 63u;
    const size_t base = (size_t)lv.off + (size_t)seg * kPgcSeg;
    double* y_g = c.y + (size_t)g * c.y_pad * kCovTile + lane;
    double* y_seg = y_g + base * kCovTile;
    if (wave == 0u) { // the segment's last node: solved by the level above
        const double* src = y_g + ((size_t)up.off + seg) * kCovTile;
#pragma unroll
        for (uint32_t a = 0; a < 6u; ++a) y_seg[(size_t)(kPgcSeg - 1u) * kCovTile + a * kPgcovLanes] = src[a * kPgcovLanes];
    }
    const double* xl0 = seg > 0u ? y_g + ((size_t)up.off + seg - 1u) * kCovTile : nullptr;
    ccov_backward(y_seg, xl0, f.G + 36 * base, f.A + 36 * base, f.B + 36 * base, wave);
    if (level0) ccov_finish(d, c, g, seg, wave, lane, cur, first, y_seg, s);
}

// one workgroup per group, after the first apply of a chain: r0^T z0 from the segments' slots, and the words k_pgcov_begin<true> sets itself
__global__ __launch_bounds__(1024) void k_pgcov_begin_rz(const PgDev d, const PgCovDev c, double tol, uint32_t n_slots) {
    __shared__ double s[kPgcovReduceWaves][kPgcovLanes];
    const uint32_t g = blockIdx.x, wave = wave_index(), lane = threadIdx.x & 63u;
    const double rz0 = cov_sum_slots(c.slot_rz, n_slots, c.G, g, wave, lane, s);
    if (threadIdx.x >= kPgcovLanes) return;
    const uint32_t col = g * kPgcovLanes + lane;
    const bool over = tol > 0.0 && !(rz0 > 0.0);
    c.rz[col] = rz0;
    c.rz0[col] = rz0;
    c.rzf[col] = rz0;
    c.stop[col] = over ? 1u : 0u;
    c.converged[col] = over ? 1u : 0u;
    const bool all = __ballot(over) == ~0ull;
    if (lane == 0u) c.gstop[g] = all ? 1u : 0u;
}

namespace {
void launch_pgccov_apply(hipStream_t s, const PgDev& d, const PgCovDev& c, const PgcDev& f, uint32_t it, int first) {
    PgcLevel lv[kPgcMaxLevels];
    const uint32_t nl = pgc_levels(d.N, lv), top = nl - 1;
    for (uint32_t l = 0; l < top; ++l)
        hipLaunchKernelGGL(k_pgccov_fwd, dim3(lv[l].nseg, c.G), dim3(1024), 0, s, d, c, f, lv[l], lv[l ? l - 1 : 0], l == 0 ? 1 : 0, it);
    hipLaunchKernelGGL(k_pgccov_top, dim3(1, c.G), dim3(1024), 0, s, d, c, f, lv[top], lv[top ? top - 1 : 0], top == 0 ? 1 : 0, it, first);
    for (uint32_t l = top; l-- > 0u;)
        hipLaunchKernelGGL(k_pgccov_back, dim3(lv[l].nseg, c.G), dim3(1024), 0, s, d, c, f, lv[l], lv[l + 1], l == 0 ? 1 : 0, it, first);
}
} // namespace

void launch_pgcov_begin(hipStream_t s, const PgDev& d, const PgCovDev& c, const PgcDev* chain, double tol) {
    if (chain) {
        hipLaunchKernelGGL(k_pgcov_begin<false>, dim3(c.G), dim3(64), 0, s, d, c, tol);
        launch_pgccov_apply(s, d, c, *chain, 0u, 1);
        hipLaunchKernelGGL(k_pgcov_begin_rz, dim3(c.G), dim3(1024), 0, s, d, c, tol, pg_blocks(d.N));
    } else {
        hipLaunchKernelGGL(k_pgcov_begin<true>, dim3(c.G), dim3(64), 0, s, d, c, tol);
    }
}

void launch_pgcov_iteration(hipStream_t s, const PgDev& d, const PgCovDev& c, const PgcDev* chain, double lambda, double tol, uint32_t it) {
    const dim3 grid(pgcov_blocks(d.N), c.G);
    hipLaunchKernelGGL(k_pgcov_spmv, grid, dim3(256), 0, s, d, c, lambda, it);
    hipLaunchKernelGGL(k_pgcov_alpha, dim3(c.G), dim3(1024), 0, s, d, c, it);
    if (chain) {
        hipLaunchKernelGGL(k_pgcov_update<false>, grid, dim3(256), 0, s, d, c, it);
        launch_pgccov_apply(s, d, c, *chain, it, 0);
    } else {
        hipLaunchKernelGGL(k_pgcov_update<true>, grid, dim3(256), 0, s, d, c, it);
    }
    hipLaunchKernelGGL(k_pgcov_beta, dim3(c.G), dim3(1024), 0, s, d, c, tol, it, chain ? pg_blocks(d.N) : pgcov_blocks(d.N));
    hipLaunchKernelGGL(k_pgcov_dir, grid, dim3(256), 0, s, d, c, it);
}

void launch_pgcov_gather(hipStream_t s, const PgDev& d, const PgCovDev& c, const uint32_t* ci, const int32_t* row, uint32_t n_pairs, double* out) {
    if (!n_pairs) return;
    hipLaunchKernelGGL(k_pgcov_gather, dim3((uint32_t)(((size_t)n_pairs * 36u + 255u) / 256u)), dim3(256), 0, s, d, c, ci, row, n_pairs, out);
}

} // namespace elm
