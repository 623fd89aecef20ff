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
// (job_of_chunk), and its pose rows are workgroup-uniform.  The walk is walk_to_reach over CellWalk, the coarse cell's mask and slot a
// MaskCache (elm_dev_fine.hpp); this kernel's own part is the counting.  An atomic is issued only when an event happens.
__global__ __launch_bounds__(256) void k_evid_walk(const FineTable ft, const EvidParams ep, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                   const uint32_t* __restrict__ base, uint32_t* __restrict__ through, uint32_t* __restrict__ hit,
                                                   uint32_t* __restrict__ partial, uint16_t* __restrict__ events_out) {
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const PoseRows P = load_pose_rows(J->rows);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    const Beam b = load_beam(J->pts, i, J->n, ep.ox, ep.oy, ep.oz);
    const bool obs = b.cast && in_window(b.L2, ep.obs_min_r2, ep.obs_max_r2);
    bool end_hit = false;
    uint32_t ev = 0;
    ReachWalk r;
    if (obs) {
        // the end point
        {
            double q0, q1, q2;
            pose_apply(P, b.px, b.py, b.pz, q0, q1, q2);
            const int e0 = fine_of(q0, ft), e1 = fine_of(q1, ft), e2 = fine_of(q2, ft);
            uint32_t slot = 0;
            const unsigned long long m = fine_probe_slot(ft, e0 >> 2, e1 >> 2, e2 >> 2, slot);
            const uint32_t bit = fine_bit(e0, e1, e2);
            if ((m >> bit) & 1ull) {
                end_hit = true;
                count_cell(hit, base, slot, m, bit);
            }
        }
        MaskCache mc;
        uint32_t slot = 0; // of the cached coarse cell
        const auto probe = [&](int cx, int cy, int cz) { return fine_probe_slot(ft, cx, cy, cz, slot); };
        r = walk_to_reach(ft, ep, P, b, [&](int c0, int c1, int c2) {
            if (mc.test(c0, c1, c2, probe)) {
                count_cell(through, base, slot, mc.mask, fine_bit(c0, c1, c2));
                ++ev;
            }
        });
    }
    if (events_out && b.valid) events_out[i] = (uint16_t)(ev > 65535u ? 65535u : ev);
    const uint32_t v[kEvidWords] = {wave_count(b.cast), wave_count(obs), wave_count(r.walked), wave_count(r.trunc), wave_count(ev > 0u),
                                    wave_count(end_hit), wave_count(obs && !end_hit), wave_sum(ev), wave_sum(r.steps)};
    store_chunk_partial<kEvidWords>(v, partial + (size_t)blockIdx.x * kEvidWords);
}

// K8b: stats[j] = the chunk partials of job j, summed in chunk order (the events and the steps in 64 bits)
__global__ __launch_bounds__(256) void k_evid_sum(const uint32_t* __restrict__ partial, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                  elm_evidence_stats* __restrict__ stats) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_jobs) return;
    const uint32_t c0 = jobs[j].chunk0, c1 = c0 + (jobs[j].n + 255u) / 256u;
    uint32_t a[7];
    uint64_t s[2]; // the events, the steps
    sum_chunk_partials<kEvidWords, 7>(partial + (size_t)c0 * kEvidWords, c1 - c0, a, s);
    elm_evidence_stats o;
    o.n_cast = a[0]; o.n_observing = a[1]; o.n_walked = a[2]; o.n_truncated = a[3];
    o.n_through_beams = a[4]; o.n_end_hit = a[5]; o.n_end_free = a[6]; o._pad = 0;
    o.n_through_events = s[0];
    o.n_steps = s[1];
    stats[j] = o;
}

void launch_evid_walk(hipStream_t s, const FineTable& ft, const EvidParams& ep, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks,
                      const uint32_t* base, uint32_t* through, uint32_t* hit, uint32_t* partial, elm_evidence_stats* stats, uint16_t* events) {
    if (!n_jobs) return;
    if (n_chunks) hipLaunchKernelGGL(k_evid_walk, dim3(n_chunks), dim3(256), 0, s, ft, ep, jobs, n_jobs, base, through, hit, partial, events);
    hipLaunchKernelGGL(k_evid_sum, dim3((n_jobs + 255) / 256), dim3(256), 0, s, partial, jobs, n_jobs, stats);
}

} // namespace elm
