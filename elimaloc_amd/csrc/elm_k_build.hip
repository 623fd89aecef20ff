// elm_k_build.hip -- the device map build (include/elimaloc_hip.h, "device map build"): AddPoints
// (vhm.cpp:270-285) with VoxelBlock::AddPointWithSpacing (vhm.hpp:106-113) replayed on the device, byte for byte what build_host
// (elm_map.cpp) makes of the same input.  The input is one array of packed points: the kept stored points of a base map in bucket
// order (k_bd_keep / k_bd_compact), then the uploaded points.  elm_map_build_device_from fills the same array
// from the device alone: k_bd_keep_within marks the stored points inside a sphere, k_bd_transform writes resident scans at their poses.
//   k_bd_insert     truncated key per point -> scratch open-addressing table (64-bit CAS), atomicMin of the point's index per slot
//   k_bd_opens      1 for the point that opens its voxel (the smallest index of the slot); its exclusive scan over the input order is
//                   the voxel id in first-seen order
//   k_bd_name       the opening point gives its slot the voxel id and unpacks the key
//   k_bd_vid        voxel id and index of every point (the sort's key and payload), raw points per voxel (integer atomicAdd)
//   k_bd_rx_hist / k_bd_rx_scatter   one 8-bit pass of a stable LSD radix sort of the indices by voxel id: per-workgroup histogram,
//                   the scan over (digit, workgroup), ranks inside the workgroup from ballots -- no atomics on the data path
//   k_bd_replay     one wavefront per voxel walks its group in input order; the kept points sit in the lanes (and in memory beyond 64)
//   k_bd_emit / k_bd_ranges   kept points to their place in bucket order, (start, count) per voxel
// k_bd_scan_block / k_bd_offsets / k_bd_scan_add: the exclusive scan all of these share (1024 entries per workgroup, the workgroup
// sums by one workgroup in chunks of 1024 as k_ds_offsets, added back).
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"
#include "elm_dev_scan.hpp"

namespace elm {

constexpr unsigned kBdBlock = 1024;

// ---- exclusive scan -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBdBlock) void k_bd_scan_block(unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ blk) {
    __shared__ unsigned s_wsum[kBdBlock / 64];
    const unsigned i = blockIdx.x * kBdBlock + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned v = i < n ? a[i] : 0u;
    unsigned inc = v; // inclusive scan over the wavefront
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off, 64);
        if (lane >= (unsigned)off) inc += o;
    }
    if (lane == 63u) s_wsum[wave] = inc;
    __syncthreads();
    unsigned wbase = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < kBdBlock / 64; ++w) {
        const unsigned c = s_wsum[w];
        wbase += w < wave ? c : 0u;
        all += c;
    }
    if (i < n) a[i] = wbase + inc - v;
    if (threadIdx.x == 0) blk[blockIdx.x] = all;
}
__global__ __launch_bounds__(1024) void k_bd_offsets(unsigned* blk, unsigned n_blocks, unsigned* total) {
    __shared__ unsigned s[1024];
    chunk_scan_1024(blk, n_blocks, total, s);
}
__global__ __launch_bounds__(kBdBlock) void k_bd_scan_add(unsigned* __restrict__ a, unsigned n, const unsigned* __restrict__ blk) {
    const unsigned i = blockIdx.x * kBdBlock + threadIdx.x;
    if (i < n) a[i] += blk[blockIdx.x];
}
void launch_bd_scan(hipStream_t s, unsigned* a, unsigned n, unsigned* blk, unsigned* total) {
    const unsigned nb = (n + kBdBlock - 1) / kBdBlock;
    if (nb) hipLaunchKernelGGL(k_bd_scan_block, dim3(nb), dim3(kBdBlock), 0, s, a, n, blk);
    hipLaunchKernelGGL(k_bd_offsets, dim3(1), dim3(1024), 0, s, blk, nb, total);
    if (nb > 1) hipLaunchKernelGGL(k_bd_scan_add, dim3(nb), dim3(kBdBlock), 0, s, a, n, (const unsigned*)blk);
}

// ---- the base map's kept points ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bd_keep(const uint8_t* __restrict__ drop, unsigned n, unsigned* __restrict__ pos) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) pos[i] = drop[i] == 0 ? 1u : 0u;
}
// pos[i] = 1 for the stored point inside the closed sphere: ((dx dx + dy dy) + dz dz) <= r2 in float64 from the float32 coordinates (a
// NaN coordinate fails the comparison and is dropped).  No drop bytes exist on this path.
__global__ __launch_bounds__(256) void k_bd_keep_within(const float4* __restrict__ pts, unsigned n, double cx, double cy, double cz, double r2,
                                                        unsigned* __restrict__ pos) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const double dx = (double)p.x - cx, dy = (double)p.y - cy, dz = (double)p.z - cz;
    pos[i] = ((dx * dx + dy * dy) + dz * dz) <= r2 ? 1u : 0u;
}
// drop: the point is kept where its byte is 0, and goes to pos[i].  No drop but pos (the scanned marks of k_bd_keep_within, total their
// sum): the point is kept where the scan steps after it.  Neither: every point, to its own index.
__global__ __launch_bounds__(256) void k_bd_compact(const float4* __restrict__ pts, const uint8_t* __restrict__ drop,
                                                    const unsigned* __restrict__ pos, unsigned n, unsigned total, Pt3* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned dst = i;
    if (drop) {
        if (drop[i] != 0) return;
        dst = pos[i];
    } else if (pos) {
        dst = pos[i];
        if ((i + 1 < n ? pos[i + 1] : total) == dst) return;
    }
    const float4 p = pts[i];
    Pt3 q;
    q.x = p.x; q.y = p.y; q.z = p.z;
    out[dst] = q;
}
// Workgroup = 256 consecutive points of one job (job_of_chunk, as the evidence walk): point i of the job goes to out[pt0[job] + i] as
// float32(R p + t), pose_apply's association in float64, one rounding to nearest at the end.
__global__ __launch_bounds__(256) void k_bd_transform(const EvidJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* __restrict__ pt0,
                                                      Pt3* __restrict__ out) {
    const EvidJob* J = job_of_chunk(jobs, n_jobs, blockIdx.x);
    const uint32_t i = (blockIdx.x - J->chunk0) * 256u + threadIdx.x;
    if (i >= J->n) return;
    const PoseRows P = load_pose_rows(J->rows);
    const float* p = J->pts + 3 * (size_t)i;
    double q0, q1, q2;
    pose_apply(P, (double)p[0], (double)p[1], (double)p[2], q0, q1, q2);
    Pt3 q;
    q.x = (float)q0; q.y = (float)q1; q.z = (float)q2;
    out[(size_t)pt0[J - jobs] + i] = q;
}
void launch_bd_keep(hipStream_t s, const uint8_t* drop, unsigned n, unsigned* pos) {
    hipLaunchKernelGGL(k_bd_keep, dim3((n + 255) / 256), dim3(256), 0, s, drop, n, pos);
}
void launch_bd_keep_within(hipStream_t s, const float4* pts, unsigned n, const double c[3], double r2, unsigned* pos) {
    hipLaunchKernelGGL(k_bd_keep_within, dim3((n + 255) / 256), dim3(256), 0, s, pts, n, c[0], c[1], c[2], r2, pos);
}
void launch_bd_compact(hipStream_t s, const float4* pts, const uint8_t* drop, const unsigned* pos, unsigned n, unsigned total, Pt3* out) {
    hipLaunchKernelGGL(k_bd_compact, dim3((n + 255) / 256), dim3(256), 0, s, pts, drop, pos, n, total, out);
}
void launch_bd_transform(hipStream_t s, const EvidJob* jobs, uint32_t n_jobs, uint32_t n_chunks, const uint32_t* pt0, Pt3* out) {
    if (n_chunks) hipLaunchKernelGGL(k_bd_transform, dim3(n_chunks), dim3(256), 0, s, jobs, n_jobs, pt0, out);
}

// ---- stage 1: key and insert --------------------------------------------------------------------------------
// The stored key: (int)((double)x / vs) per axis, truncation toward zero (vhm.cpp:275), as three 21-bit fields.  A quotient that is
// not finite or not inside (-2^20, 2^20) does not pack: kBdBadInput.  The probe is bounded by the table; a full table (it is sized
// so that this cannot happen) raises kBdTableFull instead of spinning.
__global__ __launch_bounds__(256) void k_bd_insert(const Pt3* __restrict__ in, unsigned n, double vs, unsigned long long* table, unsigned* first,
                                                   unsigned cap_log2, unsigned* __restrict__ slot, unsigned* flags) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Pt3 p = in[i];
    const double qx = (double)p.x / vs, qy = (double)p.y / vs, qz = (double)p.z / vs;
    const double lim = 1048576.0; // 2^20
    slot[i] = 0;
    if (!(qx > -lim && qx < lim && qy > -lim && qy < lim && qz > -lim && qz < lim)) {
        atomicOr(flags, kBdBadInput);
        return;
    }
    const unsigned long long kx = (unsigned long long)((int)qx + 1048576), ky = (unsigned long long)((int)qy + 1048576),
                             kz = (unsigned long long)((int)qz + 1048576);
    const unsigned long long key = (kx << 42) | (ky << 21) | kz;
    const unsigned mask = cap_log2 >= 32u ? 0xFFFFFFFFu : (1u << cap_log2) - 1u; // (2^32 slots: 2^30 points and more)
    unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> (64 - cap_log2));
    bool found = false;
    for (unsigned probe = 0;; ++probe) {
        const unsigned long long prev = atomicCAS(&table[h], ~0ull, key);
        if (prev == ~0ull || prev == key) {
            found = true;
            break;
        }
        if (probe == mask) break; // every slot seen
        h = (h + 1) & mask;
    }
    if (!found) {
        atomicOr(flags, kBdTableFull);
        return;
    }
    atomicMin(&first[h], i);
    slot[i] = h;
}
// ---- stage 2: voxel ids in first-seen order -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bd_opens(const unsigned* __restrict__ first, const unsigned* __restrict__ slot, unsigned n,
                                                  unsigned* __restrict__ opens) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) opens[i] = first[slot[i]] == i ? 1u : 0u;
}
// opens: after its exclusive scan
__global__ __launch_bounds__(256) void k_bd_name(const unsigned* __restrict__ first, const unsigned* __restrict__ slot, unsigned n,
                                                 const unsigned* __restrict__ opens, const unsigned long long* __restrict__ table,
                                                 unsigned* __restrict__ slot_vid, int32_t* __restrict__ keys) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned h = slot[i];
    if (first[h] != i) return;
    const unsigned v = opens[i];
    slot_vid[h] = v;
    const unsigned long long key = table[h];
    keys[3 * (size_t)v] = (int32_t)((key >> 42) & 0x1FFFFFull) - 1048576;
    keys[3 * (size_t)v + 1] = (int32_t)((key >> 21) & 0x1FFFFFull) - 1048576;
    keys[3 * (size_t)v + 2] = (int32_t)(key & 0x1FFFFFull) - 1048576;
}
// ---- stage 3: the sort's input and the raw counts -----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bd_vid(const unsigned* __restrict__ slot, const unsigned* __restrict__ slot_vid, unsigned n,
                                                unsigned* __restrict__ key, unsigned* __restrict__ val, unsigned* raw_cnt) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const unsigned v = slot_vid[slot[i]];
    key[i] = v;
    val[i] = i;
    atomicAdd(&raw_cnt[v], 1u);
}
void launch_bd_insert(hipStream_t s, const Pt3* in, unsigned n, double vs, unsigned long long* table, unsigned* first, unsigned cap_log2,
                      unsigned* slot, unsigned* flags) {
    hipLaunchKernelGGL(k_bd_insert, dim3((n + 255) / 256), dim3(256), 0, s, in, n, vs, table, first, cap_log2, slot, flags);
}
void launch_bd_opens(hipStream_t s, const unsigned* first, const unsigned* slot, unsigned n, unsigned* opens) {
    hipLaunchKernelGGL(k_bd_opens, dim3((n + 255) / 256), dim3(256), 0, s, first, slot, n, opens);
}
void launch_bd_vid(hipStream_t s, const unsigned* first, const unsigned* slot, unsigned n, const unsigned* opens, const unsigned long long* table,
                   unsigned* slot_vid, int32_t* keys, unsigned* key, unsigned* val, unsigned* raw_cnt) {
    hipLaunchKernelGGL(k_bd_name, dim3((n + 255) / 256), dim3(256), 0, s, first, slot, n, opens, table, slot_vid, keys);
    hipLaunchKernelGGL(k_bd_vid, dim3((n + 255) / 256), dim3(256), 0, s, slot, (const unsigned*)slot_vid, n, key, val, raw_cnt);
}

// ---- stage 4: one pass of the stable radix sort ---------------------------------------------------------------------
// hist[digit][workgroup] (digit-major: its exclusive scan in memory order is where the workgroup's run of that digit starts)
__global__ __launch_bounds__(kBdBlock) void k_bd_rx_hist(const unsigned* __restrict__ key, unsigned n, unsigned shift, unsigned nb,
                                                         unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[256];
    if (threadIdx.x < 256u) s_h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned i = blockIdx.x * kBdBlock + threadIdx.x;
    if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u); // integer counts in LDS: the sums do not depend on the order
    __syncthreads();
    if (threadIdx.x < 256u) hist[(size_t)threadIdx.x * nb + blockIdx.x] = s_h[threadIdx.x];
}
// Lanes of a wavefront with the same digit find each other with 8 ballots; the rank of a point inside its workgroup's run of the digit
// = the points of the digit in the waves before + the lower lanes of its group: input order, so the pass is stable.
__global__ __launch_bounds__(kBdBlock) void k_bd_rx_scatter(const unsigned* __restrict__ key, const unsigned* __restrict__ val, unsigned n,
                                                            unsigned shift, unsigned nb, const unsigned* __restrict__ start,
                                                            unsigned* __restrict__ key_out, unsigned* __restrict__ val_out) {
    __shared__ unsigned s_cnt[kBdBlock / 64][256];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (unsigned k = tid; k < (kBdBlock / 64) * 256u; k += kBdBlock) (&s_cnt[0][0])[k] = 0;
    __syncthreads();
    const unsigned i = blockIdx.x * kBdBlock + tid;
    const bool valid = i < n;
    const unsigned k = valid ? key[i] : 0u, d = (k >> shift) & 255u;
    unsigned long long grp = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        grp &= bit ? bal : ~bal;
    }
    const unsigned below = (unsigned)__popcll(grp & ((1ull << lane) - 1ull));
    if (valid && below == 0) s_cnt[wave][d] = (unsigned)__popcll(grp); // one lane per (wave, digit)
    __syncthreads();
    if (tid < 256u) { // exclusive prefix over the waves
        unsigned run = 0;
#pragma unroll
        for (unsigned w = 0; w < kBdBlock / 64; ++w) {
            const unsigned c = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
    if (valid) {
        const unsigned pos = start[(size_t)d * nb + blockIdx.x] + s_cnt[wave][d] + below;
        key_out[pos] = k;
        val_out[pos] = val[i];
    }
}
size_t bd_rx_hist_words(unsigned n) { return (size_t)((n + kBdBlock - 1) / kBdBlock) * 256; }
void launch_bd_rx_hist(hipStream_t s, const unsigned* key, unsigned n, unsigned shift, unsigned* hist) {
    const unsigned nb = (n + kBdBlock - 1) / kBdBlock;
    hipLaunchKernelGGL(k_bd_rx_hist, dim3(nb), dim3(kBdBlock), 0, s, key, n, shift, nb, hist);
}
void launch_bd_rx_scatter(hipStream_t s, const unsigned* key, const unsigned* val, unsigned n, unsigned shift, const unsigned* start,
                          unsigned* key_out, unsigned* val_out) {
    const unsigned nb = (n + kBdBlock - 1) / kBdBlock;
    hipLaunchKernelGGL(k_bd_rx_scatter, dim3(nb), dim3(kBdBlock), 0, s, key, val, n, shift, nb, start, key_out, val_out);
}

// ---- stage 5: the replay ----------------------------------------------------------------------------------------
// One wavefront per voxel.  Its group order[off[v] .. off[v + 1]) is read 64 candidates at a time (one per lane) and replayed one by
// one in input order; kept point k < 64 sits in lane k, kept points beyond are read back through order[], into whose front the kept
// indices are compacted (position off[v] + kept is never ahead of the candidate being replayed, and the 64 candidates of a step are in
// registers before any of them is replayed).  A candidate is kept iff no kept point is nearer than res:
// sqrt((dx * dx + dy * dy) + dz * dz) < res in float64 from the float32 coordinates, the reference's expression (vhm.hpp:109); the
// first point of a voxel meets no kept point and is always kept.  The group is not read beyond the point that reaches the cap.
__global__ __launch_bounds__(256) void k_bd_replay(const Pt3* __restrict__ in, unsigned* order, const unsigned* __restrict__ off, unsigned n_vox,
                                                   unsigned n, unsigned cap, double res, unsigned* __restrict__ kcnt, unsigned* __restrict__ kstart) {
    const unsigned lane = threadIdx.x & 63u, v = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (v >= n_vox) return; // the whole wavefront
    const unsigned start = off[v], end = v + 1 < n_vox ? off[v + 1] : n;
    unsigned kept = 0;
    double mx = 0.0, my = 0.0, mz = 0.0; // kept point `lane`
    for (unsigned base = start; base < end && kept < cap; base += 64u) {
        const unsigned j = base + lane;
        unsigned idx = 0;
        Pt3 p;
        p.x = p.y = p.z = 0.f;
        if (j < end) {
            idx = order[j];
            p = in[idx];
        }
        const unsigned cnt = min(64u, end - base);
        for (unsigned t = 0; t < cnt && kept < cap; ++t) {
            const unsigned ci = (unsigned)__shfl((int)idx, (int)t, 64);
            const double cx = (double)__shfl(p.x, (int)t, 64), cy = (double)__shfl(p.y, (int)t, 64), cz = (double)__shfl(p.z, (int)t, 64);
            bool near = false;
            if (lane < kept) { // (lane < 64: the kept points in lanes)
                const double dx = mx - cx, dy = my - cy, dz = mz - cz;
                near = sqrt((dx * dx + dy * dy) + dz * dz) < res;
            }
            for (unsigned k = 64u + lane; k < kept; k += 64u) {
                const Pt3 q = in[order[start + k]];
                const double dx = (double)q.x - cx, dy = (double)q.y - cy, dz = (double)q.z - cz;
                near = near || sqrt((dx * dx + dy * dy) + dz * dz) < res;
            }
            if (__ballot(near) == 0ull) {
                if (lane == kept) {
                    mx = cx; my = cy; mz = cz;
                }
                if (lane == 0) order[start + kept] = ci;
                if (kept >= 64u) __threadfence_block(); // read back by another lane of this wavefront at a later candidate
                ++kept;
            }
        }
    }
    if (lane == 0) {
        kcnt[v] = kept;
        kstart[v] = kept; // scanned in place afterwards
    }
}
// ---- stage 6: kept points in bucket order ---------------------------------------------------------------------------
// vid: the sorted keys (position j of the grouping belongs to voxel vid[j])
__global__ __launch_bounds__(256) void k_bd_emit(const Pt3* __restrict__ in, const unsigned* __restrict__ order, const unsigned* __restrict__ vid,
                                                 const unsigned* __restrict__ off, const unsigned* __restrict__ kcnt,
                                                 const unsigned* __restrict__ kstart, unsigned n, float4* __restrict__ out) {
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const unsigned v = vid[j], k = j - off[v];
    if (k >= kcnt[v]) return;
    const Pt3 p = in[order[j]];
    out[kstart[v] + k] = make_float4(p.x, p.y, p.z, 0.f);
}
__global__ __launch_bounds__(256) void k_bd_ranges(const unsigned* __restrict__ kcnt, const unsigned* __restrict__ kstart, unsigned n_vox,
                                                   uint2* __restrict__ ranges) {
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v < n_vox) ranges[v] = make_uint2(kstart[v], kcnt[v]);
}
void launch_bd_replay(hipStream_t s, const Pt3* in, unsigned* order, const unsigned* off, unsigned n_vox, unsigned n, unsigned cap, double res,
                      unsigned* kcnt, unsigned* kstart) {
    hipLaunchKernelGGL(k_bd_replay, dim3((n_vox + 3) / 4), dim3(256), 0, s, in, order, off, n_vox, n, cap, res, kcnt, kstart);
}
void launch_bd_emit(hipStream_t s, const Pt3* in, const unsigned* order, const unsigned* vid, const unsigned* off, const unsigned* kcnt,
                    const unsigned* kstart, unsigned n_vox, unsigned n, float4* out, uint2* ranges) {
    hipLaunchKernelGGL(k_bd_emit, dim3((n + 255) / 256), dim3(256), 0, s, in, order, vid, off, kcnt, kstart, n, out);
    hipLaunchKernelGGL(k_bd_ranges, dim3((n_vox + 255) / 256), dim3(256), 0, s, kcnt, kstart, n_vox, ranges);
}

} // namespace elm
