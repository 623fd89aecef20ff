// elm_k_evid.hip -- map evidence: many (scan, pose) observations walked cell by cell through the fine occupancy of the map, each beam up to
// a margin before its measured end point; per occupied fine cell the beams that passed through it and the beams that ended in it
// (elm_evidence_accumulate / _batch; the contract is in include/elimaloc_hip.h, "map evidence").  Every result is an
// integer, and integer addition commutes: the counters do not depend on the order in which the workgroups run.
//   K8a k_evid_walk  one (job, 256-beam chunk) per workgroup: the counter increments and the chunk's partial of the job's stats
//   K8b k_evid_sum   per job, the chunk partials summed in chunk order
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

// counter[base[slot] + (the occupied cells of the coarse cell below bit)] += 1: relaxed, device scope, the result unused (an integer count
// has no summation order to protect)
__device__ __forceinline__ void count_cell(uint32_t* __restrict__ counter, const uint32_t* __restrict__ base, uint32_t slot,
                                           unsigned long long mask, uint32_t bit) {
    const uint32_t idx = base[slot] + (uint32_t)__popcll(mask & ((1ull << bit) - 1ull));
    (void)__hip_atomic_fetch_add(counter + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace

// K8a.  Workgroup = 256 consecutive beams of one job (one per lane, float64 in registers); the job is found from the workgroup's chunk
// by a search of the jobs' first chunks, and its pose rows are workgroup-uniform.  The loop body is k_ray_cast's: one 3-way minimum, one
// integer add and one multiply-subtract-divide per step, a bit test of the current coarse cell's mask held in registers, a table probe
// only when the coarse cell (c >> 2) changes.  An atomic is issued only when an event happens.
__global__ __launch_bounds__(256) void k_evid_walk(const FineTable ft, const EvidParams ep, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                   const uint32_t* __restrict__ base, uint32_t* __restrict__ through, uint32_t* __restrict__ hit,
                                                   uint32_t* __restrict__ partial, uint16_t* __restrict__ events_out) {
    __shared__ uint32_t wcnt[4][kEvidWords];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    // the last job whose first chunk is <= this chunk (jobs without beams own no chunk: the job after them starts at the same chunk)
    uint32_t lo = 0, hi = n_jobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[mid].chunk0 <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const EvidJob* J = jobs + lo;
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
    const double cell = ft.cell;
    bool end_hit = false, walked = false, trunc = false;
    uint32_t steps = 0, ev = 0;
    if (obs) {
        const double L = sqrt(L2);
        // the end point
        {
            const int e0 = fine_of(((P.r00 * px + P.r01 * py) + P.r02 * pz) + P.t0, ft);
            const int e1 = fine_of(((P.r10 * px + P.r11 * py) + P.r12 * pz) + P.t1, ft);
            const int e2 = fine_of(((P.r20 * px + P.r21 * py) + P.r22 * pz) + P.t2, ft);
            uint32_t slot = 0;
            const unsigned long long m = fine_probe_slot(ft, e0 >> 2, e1 >> 2, e2 >> 2, slot);
            const uint32_t bit = fine_bit(e0, e1, e2);
            if ((m >> bit) & 1ull) {
                end_hit = true;
                count_cell(hit, base, slot, m, bit);
            }
        }
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
            uint32_t lslot = 0;
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
                    lmask = fine_probe_slot(ft, cx, cy, cz, lslot);
                    lcx = cx; lcy = cy; lcz = cz;
                    have = true;
                }
                const uint32_t bit = fine_bit(c0, c1, c2);
                if ((lmask >> bit) & 1ull) {
                    count_cell(through, base, lslot, lmask, bit);
                    ++ev;
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
    const uint32_t c_c = (uint32_t)__popcll(__ballot(cast)), c_o = (uint32_t)__popcll(__ballot(obs)), c_w = (uint32_t)__popcll(__ballot(walked));
    const uint32_t c_t = (uint32_t)__popcll(__ballot(trunc)), c_b = (uint32_t)__popcll(__ballot(ev > 0u));
    const uint32_t c_h = (uint32_t)__popcll(__ballot(end_hit)), c_f = (uint32_t)__popcll(__ballot(obs && !end_hit));
    const uint32_t c_e = wave_sum(ev), c_s = wave_sum(steps);
    if (lane == 0) {
        uint32_t* w = wcnt[wave];
        w[0] = c_c; w[1] = c_o; w[2] = c_w; w[3] = c_t; w[4] = c_b; w[5] = c_h; w[6] = c_f; w[7] = c_e; w[8] = c_s;
    }
    __syncthreads();
    if (tid < (uint32_t)kEvidWords) partial[(size_t)blockIdx.x * kEvidWords + tid] = ((wcnt[0][tid] + wcnt[1][tid]) + wcnt[2][tid]) + wcnt[3][tid];
}

// K8b: stats[j] = the chunk partials of job j, summed in chunk order (the events and the steps in 64 bits)
__global__ __launch_bounds__(256) void k_evid_sum(const uint32_t* __restrict__ partial, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                  elm_evidence_stats* __restrict__ stats) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_jobs) return;
    const uint32_t c0 = jobs[j].chunk0, c1 = c0 + (jobs[j].n + 255u) / 256u;
    uint32_t a[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t e = 0, s = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t* p = partial + (size_t)c * kEvidWords;
#pragma unroll
        for (int k = 0; k < 7; ++k) a[k] += p[k];
        e += p[7];
        s += p[8];
    }
    elm_evidence_stats o;
    o.n_cast = a[0]; o.n_observing = a[1]; o.n_walked = a[2]; o.n_truncated = a[3];
    o.n_through_beams = a[4]; o.n_end_hit = a[5]; o.n_end_free = a[6]; o._pad = 0;
    o.n_through_events = e;
    o.n_steps = s;
    stats[j] = o;
}

void launch_evid_walk(hipStream_t s, const FineTable& ft, const EvidParams& ep, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks,
                      const uint32_t* base, uint32_t* through, uint32_t* hit, uint32_t* partial, elm_evidence_stats* stats, uint16_t* events) {
    if (!n_jobs) return;
    if (n_chunks) hipLaunchKernelGGL(k_evid_walk, dim3(n_chunks), dim3(256), 0, s, ft, ep, jobs, n_jobs, base, through, hit, partial, events);
    hipLaunchKernelGGL(k_evid_sum, dim3((n_jobs + 255) / 256), dim3(256), 0, s, partial, jobs, n_jobs, stats);
}

} // namespace elm
