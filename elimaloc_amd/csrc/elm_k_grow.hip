// elm_k_grow.hip -- map growth: many (scan, pose) observations against the cells the map does NOT hold.  The end points that fall in free
// space away from mapped structure fill a table of candidate fine cells (hit count and fixed-point position sums); then every beam walks
// the evidence walk and counts the candidate cells it passes through (elm_growth_accumulate / _batch; the contract is in
// include/elimaloc_hip.h, "map growth").  Every stored quantity is an integer fed by integer atomics: the result does
// not depend on the order in which the workgroups run.  Three launches on one stream; the kernel boundary is what makes phase 2 see all
// of phase 1.
//   K9a k_grow_end   one (job, 256-beam chunk) per workgroup: the end class of every beam, the candidate inserts
//   K9b k_grow_walk  the same grid: the walk against the candidate tables (it does not read the map's table at all)
//   K9c k_grow_sum   per job, the chunk partials of both kernels summed in chunk order
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

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

// the local coordinates l in 0 .. 3 of coarse cell cc (one axis) that lie in [e - C, e + C], as 4 bits; 0 when none does
__device__ __forceinline__ uint32_t axis_bits(int e, int C, int cc) {
    const int lo = max(e - C, 4 * cc) - 4 * cc, hi = min(e + C, 4 * cc + 3) - 4 * cc;
    return hi >= lo ? ((1u << (hi - lo + 1)) - 1u) << lo : 0u;
}

// is any cell of the cube of half-width C (1 or 2) around fine cell e occupied in the map?  The cube meets at most two coarse cells per
// axis; the mask of each is probed once and tested against the cube's cells inside it.
__device__ __forceinline__ bool near_occupied(const FineTable& ft, int e0, int e1, int e2, int C) {
    const int x0 = (e0 - C) >> 2, x1 = (e0 + C) >> 2, y0 = (e1 - C) >> 2, y1 = (e1 + C) >> 2, z0 = (e2 - C) >> 2, z1 = (e2 + C) >> 2;
    for (int cx = x0; cx <= x1; ++cx) {
        const uint32_t bx = axis_bits(e0, C, cx);
        for (int cy = y0; cy <= y1; ++cy) {
            const uint32_t by = axis_bits(e1, C, cy);
            for (int cz = z0; cz <= z1; ++cz) {
                const unsigned long long m = fine_probe(ft, cx, cy, cz);
                if (m == 0ull) continue;
                const uint32_t bz = axis_bits(e2, C, cz);
                uint32_t yz = 0; // bit 4 ly + lz
#pragma unroll
                for (int l = 0; l < 4; ++l)
                    if ((by >> l) & 1u) yz |= bz << (4 * l);
                unsigned long long cube = 0; // bit (4 lx + ly) 4 + lz: fine_bit's order
#pragma unroll
                for (int l = 0; l < 4; ++l)
                    if ((bx >> l) & 1u) cube |= (unsigned long long)yz << (16 * l);
                if (m & cube) return true;
            }
        }
    }
    return false;
}

__device__ __forceinline__ uint32_t frac_fixed(double v, double fl) {
    const double k = floor((v - fl) * 65536.0);
    return k >= 65535.0 ? 65535u : (uint32_t)k; // the clamp: a tiny negative v has a fraction of exactly 1.0
}

} // namespace

// K9a.  Workgroup = 256 consecutive beams of one job (one per lane), found as k_evid_walk finds it.
__global__ __launch_bounds__(256) void k_grow_end(const FineTable ft, const EvidParams ep, const GrowTables gt, const EvidJob* __restrict__ jobs,
                                                  uint32_t n_jobs, uint32_t* __restrict__ partial) {
    __shared__ uint32_t wcnt[4][kGrowEndWords];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t n = J->n;
    const float* __restrict__ pts = J->pts;
    const double* R = J->rows;
    const PoseRows P{R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], R[9], R[10], R[11]};
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + tid;
    const bool valid = i < n;
    const uint32_t j = valid ? i : 0u;
    const double px = (double)pts[3 * (size_t)j], py = (double)pts[3 * (size_t)j + 1], pz = (double)pts[3 * (size_t)j + 2];
    const double dx = px - ep.ox, dy = py - ep.oy, dz = pz - ep.oz;
    const double L2 = (dx * dx + dy * dy) + dz * dz;
    const bool cast = valid && L2 > 0.0 && L2 < HUGE_VAL; // (a NaN fails both)
    const bool obs = cast && L2 >= ep.obs_min_r2 && L2 <= ep.obs_max_r2;
    bool end_hit = false, end_near = false, end_new = false, end_out = false, dropped = false;
    if (obs) {
        const double q0 = ((P.r00 * px + P.r01 * py) + P.r02 * pz) + P.t0;
        const double q1 = ((P.r10 * px + P.r11 * py) + P.r12 * pz) + P.t1;
        const double q2 = ((P.r20 * px + P.r21 * py) + P.r22 * pz) + P.t2;
        // v = q / cell as fine_of forms it; e = (int)floor(v)
        const bool ex = ft.inv_cell_exact != 0.0;
        const double v0 = ex ? q0 * ft.inv_cell_exact : q0 / ft.cell, v1 = ex ? q1 * ft.inv_cell_exact : q1 / ft.cell;
        const double v2 = ex ? q2 * ft.inv_cell_exact : q2 / ft.cell;
        const double f0 = floor(v0), f1 = floor(v1), f2 = floor(v2);
        const int e0 = (int)f0, e1 = (int)f1, e2 = (int)f2;
        const uint32_t bit = fine_bit(e0, e1, e2);
        if ((fine_probe(ft, e0 >> 2, e1 >> 2, e2 >> 2) >> bit) & 1ull) end_hit = true;
        else if (!grow_in_range(e0, e1, e2)) end_out = true;
        else if (gt.clearance > 0 && near_occupied(ft, e0, e1, e2, gt.clearance)) end_near = true;
        else {
            end_new = true;
            uint32_t slot = 0, cslot = 0;
            bool fresh = false, cfresh = false;
            const int cx = e0 >> 2, cy = e1 >> 2, cz = e2 >> 2;
            if (grow_claim(gt.fkeys, gt.mask, hash3(e0, e1, e2), grow_key(e0, e1, e2), slot, fresh) &&
                grow_claim(gt.ckeys, gt.mask, hash3(cx, cy, cz), grow_key(cx, cy, cz), cslot, cfresh)) {
                if (fresh) (void)atomicAdd(gt.count, 1u);
                (void)atomicAdd(gt.hit + slot, 1u);
                (void)atomicAdd(gt.sums + 3 * (size_t)slot, (unsigned long long)frac_fixed(v0, f0));
                (void)atomicAdd(gt.sums + 3 * (size_t)slot + 1, (unsigned long long)frac_fixed(v1, f1));
                (void)atomicAdd(gt.sums + 3 * (size_t)slot + 2, (unsigned long long)frac_fixed(v2, f2));
                (void)atomicOr(gt.cmasks + cslot, 1ull << bit);
            } else {
                dropped = true;
            }
        }
    }
    const uint32_t c_c = (uint32_t)__popcll(__ballot(cast)), c_o = (uint32_t)__popcll(__ballot(obs)), c_h = (uint32_t)__popcll(__ballot(end_hit));
    const uint32_t c_n = (uint32_t)__popcll(__ballot(end_near)), c_w = (uint32_t)__popcll(__ballot(end_new));
    const uint32_t c_u = (uint32_t)__popcll(__ballot(end_out)), c_d = (uint32_t)__popcll(__ballot(dropped));
    if (lane == 0) {
        uint32_t* w = wcnt[wave];
        w[0] = c_c; w[1] = c_o; w[2] = c_h; w[3] = c_n; w[4] = c_w; w[5] = c_u; w[6] = c_d;
    }
    __syncthreads();
    if (tid < (uint32_t)kGrowEndWords) partial[(size_t)blockIdx.x * kGrowWords + tid] = ((wcnt[0][tid] + wcnt[1][tid]) + wcnt[2][tid]) + wcnt[3][tid];
}

// K9b.  The loop body is k_evid_walk's: per-axis branches, exit_param from the integer cell, the current coarse cell's mask in registers.
// The probed table is the coarse growth table, with plain loads (it is stable during this launch), only when the coarse cell (c >> 2)
// changes; only when the mask bit is set is the fine table probed and one relaxed atomic issued.
__global__ __launch_bounds__(256) void k_grow_walk(const FineTable ft, const EvidParams ep, const GrowTables gt, const EvidJob* __restrict__ jobs,
                                                   uint32_t n_jobs, uint32_t* __restrict__ partial, uint16_t* __restrict__ events_out) {
    __shared__ uint32_t wcnt[4][kGrowWalkWords];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t n = J->n;
    const float* __restrict__ pts = J->pts;
    const double* R = J->rows;
    const PoseRows P{R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], R[9], R[10], R[11]};
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + tid;
    const bool valid = i < n;
    const uint32_t j = valid ? i : 0u;
    const double px = (double)pts[3 * (size_t)j], py = (double)pts[3 * (size_t)j + 1], pz = (double)pts[3 * (size_t)j + 2];
    const double dx = px - ep.ox, dy = py - ep.oy, dz = pz - ep.oz;
    const double L2 = (dx * dx + dy * dy) + dz * dz;
    const bool cast = valid && L2 > 0.0 && L2 < HUGE_VAL;
    const bool obs = cast && L2 >= ep.obs_min_r2 && L2 <= ep.obs_max_r2;
    const double cell = ft.cell; // (the map's table itself is not read: only its cell size)
    bool walked = false, trunc = false;
    uint32_t steps = 0, ev = 0;
    if (obs) {
        const double L = sqrt(L2);
        const double reach = L - fmax(ep.margin_m, ep.margin_frac * L);
        if (reach > ep.t_min) {
            walked = true;
            const double ux = dx / L, uy = dy / L, uz = dz / L;
            const double s0 = ((P.r00 * ep.ox + P.r01 * ep.oy) + P.r02 * ep.oz) + P.t0;
            const double s1 = ((P.r10 * ep.ox + P.r11 * ep.oy) + P.r12 * ep.oz) + P.t1;
            const double s2 = ((P.r20 * ep.ox + P.r21 * ep.oy) + P.r22 * ep.oz) + P.t2;
            const double w0 = (P.r00 * ux + P.r01 * uy) + P.r02 * uz;
            const double w1 = (P.r10 * ux + P.r11 * uy) + P.r12 * uz;
            const double w2 = (P.r20 * ux + P.r21 * uy) + P.r22 * uz;
            double t_in = ep.t_min;
            int c0 = fine_of(s0 + w0 * t_in, ft), c1 = fine_of(s1 + w1 * t_in, ft), c2 = fine_of(s2 + w2 * t_in, ft);
            const int g0 = w0 > 0.0 ? 1 : (w0 < 0.0 ? -1 : 0), g1 = w1 > 0.0 ? 1 : (w1 < 0.0 ? -1 : 0), g2 = w2 > 0.0 ? 1 : (w2 < 0.0 ? -1 : 0);
            const int up0 = g0 > 0 ? 1 : 0, up1 = g1 > 0 ? 1 : 0, up2 = g2 > 0 ? 1 : 0;
            double tx0 = g0 ? exit_param(c0, up0, cell, s0, w0) : HUGE_VAL;
            double tx1 = g1 ? exit_param(c1, up1, cell, s1, w1) : HUGE_VAL;
            double tx2 = g2 ? exit_param(c2, up2, cell, s2, w2) : HUGE_VAL;
            int lcx = 0, lcy = 0, lcz = 0;
            unsigned long long lmask = 0;
            bool have = false;
            for (;;) {
                int ax = 0;
                double tmin = tx0;
                if (tx1 < tmin) { tmin = tx1; ax = 1; }
                if (tx2 < tmin) { tmin = tx2; ax = 2; }
                const double t_next = fmax(t_in, tmin);
                if (t_next > reach) break; // the walk ends by reach: the cell it stands in is not counted
                if (steps >= (uint32_t)ep.max_steps) { // ... by steps
                    trunc = true;
                    break;
                }
                // the current cell is left by this step
                const int cx = c0 >> 2, cy = c1 >> 2, cz = c2 >> 2;
                if (!have || cx != lcx || cy != lcy || cz != lcz) {
                    uint32_t cslot = 0;
                    lmask = grow_in_range(cx, cy, cz) && grow_find(gt.ckeys, gt.mask, hash3(cx, cy, cz), grow_key(cx, cy, cz), cslot) ? gt.cmasks[cslot] : 0ull;
                    lcx = cx; lcy = cy; lcz = cz;
                    have = true;
                }
                if ((lmask >> fine_bit(c0, c1, c2)) & 1ull) { // a candidate (so every |c_r| < 2^20: the key packs)
                    uint32_t slot = 0;
                    if (grow_find(gt.fkeys, gt.mask, hash3(c0, c1, c2), grow_key(c0, c1, c2), slot)) {
                        (void)__hip_atomic_fetch_add(gt.through + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ++ev;
                    }
                }
                t_in = t_next;
                if (ax == 0) { c0 += g0; tx0 = exit_param(c0, up0, cell, s0, w0); }
                else if (ax == 1) { c1 += g1; tx1 = exit_param(c1, up1, cell, s1, w1); }
                else { c2 += g2; tx2 = exit_param(c2, up2, cell, s2, w2); }
                ++steps;
            }
        }
    }
    if (events_out && valid) events_out[i] = (uint16_t)(ev > 65535u ? 65535u : ev);
    const uint32_t c_w = (uint32_t)__popcll(__ballot(walked)), c_t = (uint32_t)__popcll(__ballot(trunc)), c_b = (uint32_t)__popcll(__ballot(ev > 0u));
    const uint32_t c_e = wave_sum(ev), c_s = wave_sum(steps);
    if (lane == 0) {
        uint32_t* w = wcnt[wave];
        w[0] = c_w; w[1] = c_t; w[2] = c_b; w[3] = c_e; w[4] = c_s;
    }
    __syncthreads();
    if (tid < (uint32_t)kGrowWalkWords)
        partial[(size_t)blockIdx.x * kGrowWords + kGrowEndWords + tid] = ((wcnt[0][tid] + wcnt[1][tid]) + wcnt[2][tid]) + wcnt[3][tid];
}

// K9c: stats[j] = the chunk partials of job j, summed in chunk order (the events and the steps in 64 bits)
__global__ __launch_bounds__(256) void k_grow_sum(const uint32_t* __restrict__ partial, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                  elm_growth_stats* __restrict__ stats) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_jobs) return;
    const uint32_t c0 = jobs[j].chunk0, c1 = c0 + (jobs[j].n + 255u) / 256u;
    uint32_t a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t e = 0, s = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t* p = partial + (size_t)c * kGrowWords;
#pragma unroll
        for (int k = 0; k < 10; ++k) a[k] += p[k];
        e += p[10];
        s += p[11];
    }
    elm_growth_stats o;
    o.n_cast = a[0]; o.n_observing = a[1]; o.n_end_hit = a[2]; o.n_end_near = a[3]; o.n_end_new = a[4]; o.n_end_out = a[5]; o.n_dropped = a[6];
    o.n_walked = a[7]; o.n_truncated = a[8]; o.n_through_beams = a[9];
    o.n_through_events = e;
    o.n_steps = s;
    stats[j] = o;
}

void launch_grow(hipStream_t s, const FineTable& ft, const EvidParams& ep, const GrowTables& gt, const EvidJob* jobs, uint32_t n_jobs,
                 uint32_t n_chunks, uint32_t* partial, elm_growth_stats* stats, uint16_t* events) {
    if (!n_jobs) return;
    if (n_chunks) {
        hipLaunchKernelGGL(k_grow_end, dim3(n_chunks), dim3(256), 0, s, ft, ep, gt, jobs, n_jobs, partial);
        hipLaunchKernelGGL(k_grow_walk, dim3(n_chunks), dim3(256), 0, s, ft, ep, gt, jobs, n_jobs, partial, events);
    }
    hipLaunchKernelGGL(k_grow_sum, dim3((n_jobs + 255) / 256), dim3(256), 0, s, partial, jobs, n_jobs, stats);
}

} // namespace elm
