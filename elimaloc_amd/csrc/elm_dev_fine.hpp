// elm_dev_fine.hpp -- device code shared by the kernels that read the fine occupancy table of a map (FineTable, elm_internal.hpp): the
// free-space check (elm_k_free.hip), the ray cast (elm_k_ray.hip, section 14), the map evidence (elm_k_evid.hip,
// section 15) and the map growth (elm_k_grow.hip, section 16), with the tables that the growth kernels fill themselves.  Each rule of the
// traversal contract those four share is written here once: the fine cell of a coordinate, the table probe, the neighbourhood cube, the
// pose association, the beam, the job of a chunk, the cell walk and its coarse-mask cache, the walk up to a beam's reach, and the
// workgroup's sum of a chunk partial.  The kernels keep only their own decision at each cell.
#pragma once
#include <hip/hip_runtime.h>

#include "elm_internal.hpp"

namespace elm {

// The contract's fine cell of one world coordinate: (int)floor(q / cell), or q * (1 / cell) where that product is exact.
__device__ __forceinline__ int fine_of(double q, const FineTable& ft) {
    return (int)floor(ft.inv_cell_exact != 0.0 ? q * ft.inv_cell_exact : q / ft.cell);
}

// The 64-bit mask of coarse cell (cx, cy, cz), 0 when the map has no point there, and the table slot of the coarse cell (left alone when
// the cell is absent): the map evidence addresses its counters by slot.
__device__ __forceinline__ unsigned long long fine_probe_slot(const FineTable& ft, int cx, int cy, int cz, uint32_t& slot) {
    uint32_t h = hash3(cx, cy, cz) & ft.mask;
    for (;;) {
        const int4 k = ft.keys[h];
        if (k.w == 0) return 0ull;
        if (k.x == cx && k.y == cy && k.z == cz) {
            slot = h;
            return ft.masks[h];
        }
        h = (h + 1) & ft.mask;
    }
}
__device__ __forceinline__ unsigned long long fine_probe(const FineTable& ft, int cx, int cy, int cz) {
    uint32_t slot = 0;
    return fine_probe_slot(ft, cx, cy, cz, slot);
}
struct FineProbe { // fine_probe as the probe of a MaskCache
    const FineTable& ft;
    __device__ __forceinline__ unsigned long long operator()(int cx, int cy, int cz) const { return fine_probe(ft, cx, cy, cz); }
};

__device__ __forceinline__ uint32_t fine_bit(int fx, int fy, int fz) { return (uint32_t)((((fx & 3) << 2) | (fy & 3)) << 2 | (fz & 3)); }

// ---- the tables a kernel fills itself (map growth, elm_k_grow.hip): open addressing over packed 64-bit keys
// A cell with every |c_r| < 2^20 as one key: 21 bits per axis, biased by 2^20, the top bit set so that 0 is "empty".  Ascending keys are
// ascending (x, y, z).
__host__ __device__ __forceinline__ bool grow_in_range(int x, int y, int z) {
    return x > -kGrowLim && x < kGrowLim && y > -kGrowLim && y < kGrowLim && z > -kGrowLim && z < kGrowLim;
}
__host__ __device__ __forceinline__ unsigned long long grow_key(int x, int y, int z) {
    return (1ull << 63) | ((unsigned long long)(uint32_t)(x + kGrowLim) << 42) | ((unsigned long long)(uint32_t)(y + kGrowLim) << 21) |
           (unsigned long long)(uint32_t)(z + kGrowLim);
}

// The slot of `key` in a table that is stable during the launch (plain loads), or false when the key is absent.  The table is at most
// half full, so an empty slot ends every probe; the loop is bounded by the slot count all the same.
__device__ __forceinline__ bool grow_find(const unsigned long long* __restrict__ keys, uint32_t mask, uint32_t h, unsigned long long key,
                                          uint32_t& slot) {
    h &= mask;
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        const unsigned long long k = keys[h];
        if (k == key) {
            slot = h;
            return true;
        }
        if (k == 0ull) return false;
        h = (h + 1) & mask;
    }
    return false;
}

// The slot of `key` in a table that other lanes fill at the same time: one 64-bit compare-and-swap per slot tried.  It returns empty (the
// slot is now this key's), this key (the slot is shared: lanes of one wave insert the same key together) or another key (the next slot).
// No lock, and no lane ever waits for another lane.  false when the bounded loop runs out (a full table: the host's capacity guard
// excludes it).
__device__ __forceinline__ bool grow_claim(unsigned long long* __restrict__ keys, uint32_t mask, uint32_t h, unsigned long long key,
                                           uint32_t& slot, bool& fresh) {
    h &= mask;
    for (uint32_t tries = 0; tries <= mask; ++tries) {
        const unsigned long long was = atomicCAS(keys + h, 0ull, key);
        if (was == 0ull || was == key) {
            slot = h;
            fresh = was == 0ull;
            return true;
        }
        h = (h + 1) & mask;
    }
    return false;
}

// The mask of the last coarse cell a lane asked for, in registers: consecutive cells of a walk (and consecutive samples of a ray) mostly
// share it, so the table is probed only when the coarse cell (fine cell >> 2 per axis) changes.  probe(cx, cy, cz) gives the mask; a caller
// that needs the cell's slot too keeps it beside the cache and has its probe fill it.
struct MaskCache {
    int cx = 0, cy = 0, cz = 0;
    unsigned long long mask = 0;
    bool have = false;
    // whether fine cell (f0, f1, f2) is set in its coarse cell's mask
    template <class Probe>
    __device__ __forceinline__ bool test(int f0, int f1, int f2, Probe probe) {
        const int x = f0 >> 2, y = f1 >> 2, z = f2 >> 2;
        if (!have || x != cx || y != cy || z != cz) {
            mask = probe(x, y, z);
            cx = x; cy = y; cz = z;
            have = true;
        }
        return (mask >> fine_bit(f0, f1, f2)) & 1ull;
    }
};

// the local coordinates l in 0 .. 3 of coarse cell cc (one axis) whose fine cell lies in [e - C, e + C], as 4 bits; 0 when none does
__device__ __forceinline__ uint32_t axis_bits(int e, int C, int cc) {
    uint32_t b = 0;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int d = (cc << 2) + l - e;
        b |= (d >= -C && d <= C) ? (1u << l) : 0u;
    }
    return b;
}

// Is any cell of the cube of half-width C (1 or 2) around fine cell e occupied in the map?  The cube meets at most two coarse cells per
// axis; the mask of each is probed once and tested against the cube's cells inside it.
__device__ __forceinline__ bool near_occupied(const FineTable& ft, int e0, int e1, int e2, int C) {
    for (int cx = (e0 - C) >> 2; cx <= (e0 + C) >> 2; ++cx)
        for (int cy = (e1 - C) >> 2; cy <= (e1 + C) >> 2; ++cy)
            for (int cz = (e2 - C) >> 2; cz <= (e2 + C) >> 2; ++cz) {
                const unsigned long long m = fine_probe(ft, cx, cy, cz);
                if (!m) continue;
                const uint32_t bx = axis_bits(e0, C, cx), by = axis_bits(e1, C, cy), bz = axis_bits(e2, C, cz);
                uint32_t yz = 0; // bit 4 ly + lz
#pragma unroll
                for (int l = 0; l < 4; ++l) yz |= ((by >> l) & 1u) ? (bz << (4 * l)) : 0u;
                unsigned long long cube = 0; // bit (4 lx + ly) 4 + lz: fine_bit's order
#pragma unroll
                for (int l = 0; l < 4; ++l) cube |= ((bx >> l) & 1u) ? ((unsigned long long)yz << (16 * l)) : 0ull;
                if (m & cube) return true;
            }
    return false;
}

// ---- poses and beams
// The rows of one pose [R | t], workgroup-uniform: 12 doubles (R_r0, R_r1, R_r2, t_r) per row r.
struct PoseRows {
    double r00, r01, r02, t0, r10, r11, r12, t1, r20, r21, r22, t2;
};
__device__ __forceinline__ PoseRows load_pose_rows(const double* R) {
    return PoseRows{R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], R[9], R[10], R[11]};
}
// q = R (x, y, z) + t and w = R (x, y, z): the contract's association, written here only
__device__ __forceinline__ void pose_rotate(const PoseRows& P, double x, double y, double z, double& w0, double& w1, double& w2) {
    w0 = (P.r00 * x + P.r01 * y) + P.r02 * z;
    w1 = (P.r10 * x + P.r11 * y) + P.r12 * z;
    w2 = (P.r20 * x + P.r21 * y) + P.r22 * z;
}
__device__ __forceinline__ void pose_apply(const PoseRows& P, double x, double y, double z, double& q0, double& q1, double& q2) {
    q0 = ((P.r00 * x + P.r01 * y) + P.r02 * z) + P.t0;
    q1 = ((P.r10 * x + P.r11 * y) + P.r12 * z) + P.t1;
    q2 = ((P.r20 * x + P.r21 * y) + P.r22 * z) + P.t2;
}

// Beam i of n packed xyz points seen from origin o: the point p, d = p - o, L2 = |d|^2.  A lane past the end reads point 0 and is not
// valid; cast: a beam with a direction (a NaN fails both comparisons).
struct Beam {
    double px, py, pz, dx, dy, dz, L2;
    bool valid, cast;
};
__device__ __forceinline__ Beam load_beam(const float* __restrict__ pts, uint32_t i, uint32_t n, double ox, double oy, double oz) {
    Beam b;
    b.valid = i < n;
    const uint32_t j = b.valid ? i : 0u;
    b.px = (double)pts[3 * (size_t)j]; b.py = (double)pts[3 * (size_t)j + 1]; b.pz = (double)pts[3 * (size_t)j + 2];
    b.dx = b.px - ox; b.dy = b.py - oy; b.dz = b.pz - oz;
    b.L2 = (b.dx * b.dx + b.dy * b.dy) + b.dz * b.dz;
    b.cast = b.valid && b.L2 > 0.0 && b.L2 < HUGE_VAL;
    return b;
}
// the closed range window [min_r2, max_r2] on a squared length
__device__ __forceinline__ bool in_window(double L2, double min_r2, double max_r2) { return L2 >= min_r2 && L2 <= max_r2; }

// the last job whose first chunk is <= this chunk (jobs without beams own no chunk: the job after them starts at the same chunk)
__device__ __forceinline__ const EvidJob* job_of_chunk(const EvidJob* __restrict__ jobs, uint32_t n_jobs, uint32_t chunk) {
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].chunk0 <= chunk) lo = mid;
        else hi = mid;
    }
    return jobs + lo;
}

// ---- the exact cell walk (the contract is in include/elimaloc_hip.h, "ray casting")
// The exit parameter of cell c along one axis of a cell walk: the far face in the direction of travel, from the integer cell (never
// accumulated).
__device__ __forceinline__ double exit_param(int c, int up, double cell, double s, double w) { return ((double)(c + up) * cell - s) / w; }

// One beam walked fine cell by fine cell at one pose: from s = R o + t along w = R u, standing in cell (c0, c1, c2), entered at t_in.
// Per step: one 3-way minimum (peek), then one integer add and one multiply-subtract-divide for the stepped axis (advance).  Between
// the two the caller decides whether the walk ends: the ray cast looks at the cell it stands in before peek, the evidence walks at the
// cell the step leaves after their end checks.
struct CellWalk {
    double s0, s1, s2, w0, w1, w2, tx0, tx1, tx2, t_in, cell;
    int c0, c1, c2, g0, g1, g2, up0, up1, up2;
    uint32_t steps;
    __device__ __forceinline__ void start(const PoseRows& P, double ox, double oy, double oz, double ux, double uy, double uz, double t_min,
                                          const FineTable& ft) {
        pose_apply(P, ox, oy, oz, s0, s1, s2);
        pose_rotate(P, ux, uy, uz, w0, w1, w2);
        t_in = t_min;
        cell = ft.cell;
        c0 = fine_of(s0 + w0 * t_in, ft); c1 = fine_of(s1 + w1 * t_in, ft); c2 = fine_of(s2 + w2 * t_in, ft);
        g0 = w0 > 0.0 ? 1 : (w0 < 0.0 ? -1 : 0); g1 = w1 > 0.0 ? 1 : (w1 < 0.0 ? -1 : 0); g2 = w2 > 0.0 ? 1 : (w2 < 0.0 ? -1 : 0);
        up0 = g0 > 0 ? 1 : 0; up1 = g1 > 0 ? 1 : 0; up2 = g2 > 0 ? 1 : 0;
        tx0 = g0 ? exit_param(c0, up0, cell, s0, w0) : HUGE_VAL;
        tx1 = g1 ? exit_param(c1, up1, cell, s1, w1) : HUGE_VAL;
        tx2 = g2 ? exit_param(c2, up2, cell, s2, w2) : HUGE_VAL;
        steps = 0;
    }
    // the axis of the next step and the parameter at which the walk enters the next cell (ties: the lowest axis)
    __device__ __forceinline__ int peek(double& t_next) const {
        int ax = 0;
        double tmin = tx0;
        if (tx1 < tmin) { tmin = tx1; ax = 1; }
        if (tx2 < tmin) { tmin = tx2; ax = 2; }
        t_next = fmax(t_in, tmin);
        return ax;
    }
    __device__ __forceinline__ void advance(int ax, double t_next) {
        // (the branches write locals and the members are stored after them: a member stored under the branch is a store the compiler
        // merges into one indexed by ax, which moves the members to scratch)
        int n0 = c0, n1 = c1, n2 = c2;
        double x0 = tx0, x1 = tx1, x2 = tx2;
        if (ax == 0) { n0 += g0; x0 = exit_param(n0, up0, cell, s0, w0); }
        else if (ax == 1) { n1 += g1; x1 = exit_param(n1, up1, cell, s1, w1); }
        else { n2 += g2; x2 = exit_param(n2, up2, cell, s2, w2); }
        c0 = n0; c1 = n1; c2 = n2;
        tx0 = x0; tx1 = x1; tx2 = x2;
        t_in = t_next;
        ++steps;
    }
};

// The walk of the map evidence and the map growth: a beam in the observation window walks from t_min up to a margin before its measured
// end.  visit(c0, c1, c2) sees every cell a step leaves; the cell in which the walk ends (by reach, or truncated by steps) is not visited.
struct ReachWalk {
    bool walked = false, trunc = false;
    uint32_t steps = 0;
};
template <class Visit>
__device__ __forceinline__ ReachWalk walk_to_reach(const FineTable& ft, const EvidParams& ep, const PoseRows& P, const Beam& b, Visit visit) {
    ReachWalk r;
    const double L = sqrt(b.L2);
    const double reach = L - fmax(ep.margin_m, ep.margin_frac * L);
    if (!(reach > ep.t_min)) return r;
    r.walked = true;
    CellWalk w;
    w.start(P, ep.ox, ep.oy, ep.oz, b.dx / L, b.dy / L, b.dz / L, ep.t_min, ft);
    for (;;) {
        double t_next;
        const int ax = w.peek(t_next);
        if (t_next > reach) break; // the walk ends by reach: the cell it stands in is not counted
        if (w.steps >= (uint32_t)ep.max_steps) { // ... by steps
            r.trunc = true;
            break;
        }
        visit(w.c0, w.c1, w.c2); // the current cell is left by this step
        w.advance(ax, t_next);
    }
    r.steps = w.steps;
    return r;
}

// ---- counting
__device__ __forceinline__ uint32_t wave_count(bool b) { return (uint32_t)__popcll(__ballot(b)); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The epilogue of a kernel whose workgroup (4 waves) is one chunk: every wave's W words (wave-uniform) meet in LDS and out[k] = the four
// waves' word k, summed in wave order.
template <int W>
__device__ __forceinline__ void store_chunk_partial(const uint32_t (&v)[W], uint32_t* __restrict__ out) {
    __shared__ uint32_t wcnt[4][W];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    if ((tid & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) wcnt[wave][k] = v[k];
    }
    __syncthreads();
    if (tid < (uint32_t)W) out[tid] = ((wcnt[0][tid] + wcnt[1][tid]) + wcnt[2][tid]) + wcnt[3][tid];
}

// Its counterpart in the sum kernels: word k of the n consecutive chunk partials at p (W words each), summed in chunk order -- the first
// N32 words in 32 bits into a32[k], the others in 64 bits into a64[k - N32] (none: nullptr).
template <int W, int N32>
__device__ __forceinline__ void sum_chunk_partials(const uint32_t* __restrict__ p, uint32_t n, uint32_t* a32, uint64_t* a64) {
#pragma unroll
    for (int k = 0; k < N32; ++k) a32[k] = 0;
#pragma unroll
    for (int k = N32; k < W; ++k) a64[k - N32] = 0;
    for (uint32_t c = 0; c < n; ++c, p += W) {
#pragma unroll
        for (int k = 0; k < N32; ++k) a32[k] += p[k];
#pragma unroll
        for (int k = N32; k < W; ++k) a64[k - N32] += p[k];
    }
}

} // namespace elm
