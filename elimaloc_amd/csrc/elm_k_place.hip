// elm_k_place.hip -- place recognition: a rotation-aware binary descriptor of a scan (rings x layers words of 64 sector bits), the
// popcount of a descriptor, the exact match of a query against every database entry at every one of the 64 yaw shifts, and the top-k
// selection per query (elm_places_*; the contract is in include/elimaloc_hip.h, "place recognition").  Every
// result is an integer; OR, integer addition and the maximum of distinct integer keys do not depend on the order in which lanes,
// waves or workgroups run, so the bytes are the same on every run.
//   K11a k_pl_describe  one (job, 256-point chunk) per workgroup: the chunk's bits ORed into the job's descriptor
//   K11b k_pl_bits      one wavefront per descriptor: its popcount
//   K11c k_pl_match     one wavefront per (query, entry) pair, the lane is the shift
//   K11d k_pl_topk      one workgroup per query: top_k passes of a maximum over (dice, entry) keys
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_dev_reduce.hpp"
#include "elm_internal.hpp"

namespace elm {

// K11a.  Workgroup = 256 consecutive points of one job (one per lane, float64 in registers); the job is found from the workgroup's chunk
// (job_of_chunk) and its levelling pose rows are workgroup-uniform.  The descriptor of the chunk is built in LDS (W words, at most
// 4 KB, one 64-bit LDS OR per point that sets a bit) and its non-zero words are ORed into the job's descriptor in global memory, which
// the host zeroed before the launch.  The sector is found as the contract words it: all 64 pairs of crosses, the smallest k that
// satisfies the rule (k is workgroup-uniform in the loop, so the directions come by scalar loads).
__global__ __launch_bounds__(256) void k_pl_describe(const PlaceParams pp, const EvidJob* __restrict__ jobs, uint32_t n_jobs,
                                                     unsigned long long* __restrict__ words, elm_places_stats* __restrict__ stats) {
    __shared__ unsigned long long s_words[kPlaceMaxWords];
    __shared__ uint32_t s_used[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t W = (uint32_t)(pp.n_rings * pp.n_layers);
    for (uint32_t w = tid; w < W; w += 256u) s_words[w] = 0ull;
    __syncthreads();
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t job = (uint32_t)(J - jobs);
    const PoseRows P = load_pose_rows(J->rows);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + tid;
    const bool valid = i < J->n;
    const uint32_t j = valid ? i : 0u;
    const double px = (double)J->pts[3 * (size_t)j], py = (double)J->pts[3 * (size_t)j + 1], pz = (double)J->pts[3 * (size_t)j + 2];
    double qx, qy, qz;
    pose_apply(P, px, py, pz, qx, qy, qz);
    const double r2 = qx * qx + qy * qy;
    // the ring and the layer: the bin whose lower edge is <= the value and whose upper edge is > it (a NaN fails the first test)
    const double* __restrict__ re = pp.tables;
    const double* __restrict__ ze = pp.tables + (pp.n_rings + 1);
    const double* __restrict__ dir = ze + (pp.n_layers + 1);
    bool used = valid && r2 >= re[0] && r2 < re[pp.n_rings] && qz >= ze[0] && qz < ze[pp.n_layers];
    int ring = 0, layer = 0;
    for (int e = 1; e < pp.n_rings; ++e) ring += (r2 >= re[e]) ? 1 : 0; // (the edges ascend strictly: the count of edges passed)
    for (int e = 1; e < pp.n_layers; ++e) layer += (qz >= ze[e]) ? 1 : 0;
    int sector = kPlaceSectors;
    double c0 = dir[0] * qy - dir[1] * qx;
    for (int k = 0; k < kPlaceSectors; ++k) {
        const int k1 = (k + 1) & (kPlaceSectors - 1);
        const double c1 = dir[2 * k1] * qy - dir[2 * k1 + 1] * qx;
        if (sector == kPlaceSectors && c0 >= 0.0 && c1 < 0.0) sector = k;
        c0 = c1;
    }
    used = used && sector < kPlaceSectors;
    if (used) (void)atomicOr(&s_words[ring * pp.n_layers + layer], 1ull << sector);
    const uint32_t n_used = wave_count(used);
    if ((tid & 63u) == 0) s_used[tid >> 6] = n_used;
    __syncthreads();
    unsigned long long* __restrict__ dst = words + (size_t)job * W;
    for (uint32_t w = tid; w < W; w += 256u) {
        const unsigned long long v = s_words[w];
        if (v) (void)atomicOr(dst + w, v);
    }
    if (tid == 0) {
        const uint32_t n = ((s_used[0] + s_used[1]) + s_used[2]) + s_used[3];
        if (n) (void)atomicAdd(&stats[job].n_used, n);
    }
}

// K11b.  One wavefront per descriptor, four per workgroup: n_bits[d] = the popcount of its W words; with stats (the descriptors of a
// describe call, one per job) also the job's n_points and n_bits (n_used is k_pl_describe's).
__global__ __launch_bounds__(256) void k_pl_bits(const unsigned long long* __restrict__ words, uint32_t W, uint32_t n_desc,
                                                 uint32_t* __restrict__ n_bits, const EvidJob* __restrict__ jobs,
                                                 elm_places_stats* __restrict__ stats) {
    const uint32_t d = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (d >= n_desc) return;
    const unsigned long long* __restrict__ a = words + (size_t)d * W;
    uint32_t n = 0;
    for (uint32_t w = lane; w < W; w += 64u) n += (uint32_t)__popcll(a[w]);
    n = wave_sum(n);
    if (lane == 0) {
        n_bits[d] = n;
        if (stats) {
            stats[d].n_points = jobs[d].n;
            stats[d].n_bits = n;
        }
    }
}

// K11c.  One wavefront per (query, entry) pair, four pairs per workgroup; the lane is the shift k.  The words of both descriptors are
// wave-uniform (scalar loads); per word a lane rotates the entry's word left by k -- as a rotate right by s = (64 - k) & 63 on the two
// 32-bit halves: the halves swapped when s >= 32, then two funnel shifts by s & 31 -- ands, and counts the bits of both halves.  The
// winner is the maximum over the lanes of inter << 6 | (63 - k): the largest inter, at the smallest k.
__global__ __launch_bounds__(256) void k_pl_match(const unsigned long long* __restrict__ qwords, const uint32_t* __restrict__ q_bits,
                                                  const unsigned long long* __restrict__ dwords, const uint32_t* __restrict__ d_bits,
                                                  uint32_t W, uint32_t n_entries, elm_place_match* __restrict__ out) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t entry = blockIdx.x * 4u + wave, q = blockIdx.y, lane = threadIdx.x & 63u;
    if (entry >= n_entries) return;
    const unsigned long long* __restrict__ a = qwords + (size_t)q * W;
    const unsigned long long* __restrict__ b = dwords + (size_t)entry * W;
    const uint32_t s = (64u - lane) & 63u, s5 = s & 31u;
    const bool swap = s >= 32u;
    uint32_t inter = 0;
#pragma unroll 4 // (four words per trip: the scalar loads of a trip merge, and their latency is paid once per trip)
    for (uint32_t w = 0; w < W; ++w) {
        const unsigned long long aw = a[w], bw = b[w];
        const uint32_t blo = (uint32_t)bw, bhi = (uint32_t)(bw >> 32);
        const uint32_t x = swap ? bhi : blo, y = swap ? blo : bhi; // {y, x} = the word turned by 0 or 32
        const uint32_t rlo = __builtin_amdgcn_alignbit(y, x, s5), rhi = __builtin_amdgcn_alignbit(x, y, s5);
        inter += (uint32_t)__popc((uint32_t)aw & rlo) + (uint32_t)__popc((uint32_t)(aw >> 32) & rhi);
    }
    // the maximum of the key as the minimum of its complement: the rows by DPP, the four rows by two exchanges
    uint32_t v = ~((inter << 6) | (63u - lane));
    v = group_min_u32<16>(v);
    v = min(v, (uint32_t)__shfl_xor((int)v, 16));
    v = min(v, (uint32_t)__shfl_xor((int)v, 32));
    if (lane == 0) {
        const uint32_t key = ~v, best = key >> 6, k = 63u - (key & 63u);
        const uint32_t den = q_bits[q] + d_bits[entry];
        elm_place_match m;
        m.dice_q16 = den ? (uint32_t)(((unsigned long long)best << 17) / (unsigned long long)den) : 0u;
        m.inter = (uint16_t)best;
        m.shift = (uint16_t)k;
        out[(size_t)q * n_entries + entry] = m;
    }
}

// K11d.  One workgroup per query.  Pass p finds the maximum of dice_q16 << 32 | (0xFFFFFFFF - entry) over the entries that pass the
// threshold and lie outside the excluded id range, strictly below pass p - 1's winner: dice descending, then the entry ascending.
// A key is never 0 (entry < 2^32 - 1), so 0 says that no entry is left.
__global__ __launch_bounds__(256) void k_pl_topk(const elm_place_match* __restrict__ matches, const long long* __restrict__ ids,
                                                 uint32_t n_entries, const elm_places_query_config* __restrict__ cfgs,
                                                 elm_place_candidate* __restrict__ cands, int32_t* __restrict__ n_cands) {
    __shared__ unsigned long long s_best[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const elm_places_query_config c = cfgs[q];
    const elm_place_match* __restrict__ m = matches + (size_t)q * n_entries;
    elm_place_candidate* __restrict__ out = cands + (size_t)q * kPlaceMaxTopK;
    unsigned long long prev = ~0ull;
    int32_t found = 0;
    for (int p = 0; p < c.top_k; ++p) {
        unsigned long long best = 0ull;
        for (uint32_t e = tid; e < n_entries; e += 256u) {
            const uint32_t dice = m[e].dice_q16;
            const long long id = ids[e];
            const unsigned long long key = ((unsigned long long)dice << 32) | (unsigned long long)(0xFFFFFFFFu - e);
            const bool ok = dice >= c.min_dice_q16 && !(id >= c.exclude_id_lo && id <= c.exclude_id_hi) && key < prev;
            if (ok && key > best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other > best ? other : best;
        }
        __syncthreads(); // (the previous pass has read s_best)
        if ((tid & 63u) == 0) s_best[tid >> 6] = best;
        __syncthreads();
        best = s_best[0];
        for (int w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
        if (best == 0ull) break; // workgroup-uniform
        if (tid == 0) {
            const uint32_t e = 0xFFFFFFFFu - (uint32_t)best;
            elm_place_candidate o;
            o.entry = e;
            o.dice_q16 = (uint32_t)(best >> 32);
            o.id = ids[e];
            o.inter = m[e].inter;
            o.shift = m[e].shift;
            o._pad = 0;
            o.yaw_rad = 0.0; // the host's, from the shift
            out[p] = o;
        }
        prev = best;
        ++found;
    }
    if (tid == 0) n_cands[q] = found;
}

void launch_pl_describe(hipStream_t s, const PlaceParams& pp, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks, unsigned long long* words,
                        uint32_t* n_bits, elm_places_stats* stats) {
    if (!n_jobs) return;
    if (n_chunks) hipLaunchKernelGGL(k_pl_describe, dim3(n_chunks), dim3(256), 0, s, pp, jobs, n_jobs, words, stats);
    hipLaunchKernelGGL(k_pl_bits, dim3((n_jobs + 3) / 4), dim3(256), 0, s, words, (uint32_t)(pp.n_rings * pp.n_layers), n_jobs, n_bits, jobs, stats);
}

void launch_pl_bits(hipStream_t s, const unsigned long long* words, uint32_t W, uint32_t n_desc, uint32_t* n_bits) {
    if (!n_desc) return;
    hipLaunchKernelGGL(k_pl_bits, dim3((n_desc + 3) / 4), dim3(256), 0, s, words, W, n_desc, n_bits, (const EvidJob*)nullptr,
                       (elm_places_stats*)nullptr);
}

void launch_pl_match(hipStream_t s, const unsigned long long* qwords, const uint32_t* q_bits, uint32_t n_queries, const unsigned long long* dwords,
                     const uint32_t* d_bits, const long long* ids, uint32_t W, uint32_t n_entries, const elm_places_query_config* cfgs,
                     elm_place_match* matches, elm_place_candidate* cands, int32_t* n_cands) {
    if (!n_queries || !n_entries) return;
    hipLaunchKernelGGL(k_pl_match, dim3((n_entries + 3) / 4, n_queries), dim3(256), 0, s, qwords, q_bits, dwords, d_bits, W, n_entries, matches);
    hipLaunchKernelGGL(k_pl_topk, dim3(n_queries), dim3(256), 0, s, matches, ids, n_entries, cfgs, cands, n_cands);
}

} // namespace elm
