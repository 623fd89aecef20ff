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

__device__ __forceinline__ uint32_t frac_fixed(double v, double fl) {
    const double k = floor((v - fl) * 65536.0);
    return k >= 65535.0 ? 65535u : (uint32_t)k; // the clamp: a tiny negative v has a fraction of exactly 1.0
}

} // namespace

// K9a.  Workgroup = 256 consecutive beams of one job (one per lane), found from the workgroup's chunk (job_of_chunk).
__global__ __launch_bounds__(256) void k_grow_end(const FineTable ft, const EvidParams ep, const GrowTables gt, const EvidJob* __restrict__ jobs,
                                                  uint32_t n_jobs, uint32_t* __restrict__ partial) {
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const PoseRows P = load_pose_rows(J->rows);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    const Beam b = load_beam(J->pts, i, J->n, ep.ox, ep.oy, ep.oz);
    const bool obs = b.cast && in_window(b.L2, ep.obs_min_r2, ep.obs_max_r2);
    bool end_hit = false, end_near = false, end_new = false, end_out = false, dropped = false;
    if (obs) {
        double q0, q1, q2;
        pose_apply(P, b.px, b.py, b.pz, q0, q1, q2);
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
    const uint32_t v[kGrowEndWords] = {wave_count(b.cast), wave_count(obs), wave_count(end_hit), wave_count(end_near),
                                       wave_count(end_new), wave_count(end_out), wave_count(dropped)};
    store_chunk_partial<kGrowEndWords>(v, partial + (size_t)blockIdx.x * kGrowWords);
}

// K9b.  The walk is the map evidence's (walk_to_reach, elm_dev_fine.hpp).  The table behind the MaskCache is the coarse growth table, with
// plain loads (it is stable during this launch; the map's own table is not read at all, only its cell size); only when the mask bit is
// set is the fine table probed and one relaxed atomic issued.
__global__ __launch_bounds__(256) void k_grow_walk(const FineTable ft, const EvidParams ep, const GrowTables gt, const EvidJob* __restrict__ jobs,
                                                   uint32_t n_jobs, uint32_t* __restrict__ partial, uint16_t* __restrict__ events_out) {
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const PoseRows P = load_pose_rows(J->rows);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    const Beam b = load_beam(J->pts, i, J->n, ep.ox, ep.oy, ep.oz);
    const bool obs = b.cast && in_window(b.L2, ep.obs_min_r2, ep.obs_max_r2);
    uint32_t ev = 0;
    ReachWalk r;
    if (obs) {
        MaskCache mc;
        const auto coarse = [&](int cx, int cy, int cz) {
            uint32_t cslot = 0;
            return grow_in_range(cx, cy, cz) && grow_find(gt.ckeys, gt.mask, hash3(cx, cy, cz), grow_key(cx, cy, cz), cslot) ? gt.cmasks[cslot] : 0ull;
        };
        r = walk_to_reach(ft, ep, P, b, [&](int c0, int c1, int c2) {
            if (mc.test(c0, c1, c2, coarse)) { // a candidate (so every |c_r| < 2^20: the key packs)
                uint32_t slot = 0;
                if (grow_find(gt.fkeys, gt.mask, hash3(c0, c1, c2), grow_key(c0, c1, c2), slot)) {
                    (void)__hip_atomic_fetch_add(gt.through + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ++ev;
                }
            }
        });
    }
    if (events_out && b.valid) events_out[i] = (uint16_t)(ev > 65535u ? 65535u : ev);
    const uint32_t v[kGrowWalkWords] = {wave_count(r.walked), wave_count(r.trunc), wave_count(ev > 0u), wave_sum(ev), wave_sum(r.steps)};
    store_chunk_partial<kGrowWalkWords>(v, partial + (size_t)blockIdx.x * kGrowWords + kGrowEndWords);
}

// K9c: stats[j] = the chunk partials of job j, summed in chunk order (the events and the steps in 64 bits)
__global__ __launch_bounds__(256) void k_grow_sum(const uint32_t* __restrict__ partial, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                  elm_growth_stats* __restrict__ stats) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_jobs) return;
    const uint32_t c0 = jobs[j].chunk0, c1 = c0 + (jobs[j].n + 255u) / 256u;
    uint32_t a[10];
    uint64_t s[2]; // the events, the steps
    sum_chunk_partials<kGrowWords, 10>(partial + (size_t)c0 * kGrowWords, c1 - c0, a, s);
    elm_growth_stats o;
    o.n_cast = a[0]; o.n_observing = a[1]; o.n_end_hit = a[2]; o.n_end_near = a[3]; o.n_end_new = a[4]; o.n_end_out = a[5]; o.n_dropped = a[6];
    o.n_walked = a[7]; o.n_truncated = a[8]; o.n_through_beams = a[9];
    o.n_through_events = s[0];
    o.n_steps = s[1];
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
