// elm_k_reloc.hip -- relocalization: voxel-occupancy scores of many candidate poses of one scan (elm_map_score_poses / elm_relocalize;
// DESIGN.md section 11).  score(T) = the number of counted scan points whose STORED key (truncated, vhm.cpp:275) under T is a
// voxel of the map: it reads only the voxel set, so it is exact and the same for every search-index form.
//   K5a k_reloc_bitmap   one bit per voxel of a key box (the union of the hypotheses' key ranges), filled by hash probes
//   K5b k_reloc_score    (point chunk x hypothesis block) partial counts, in three forms of the occupancy lookup (template FORM):
//                        0 = the bitmap staged in LDS, 1 = the bitmap read from global memory (L2-resident), 2 = hash probes only;
//                        in forms 0 / 1 a key outside the box is probed, so every form returns the same counts
//   K5c k_reloc_sum      per hypothesis, the chunk partials summed in chunk order
#include <hip/hip_runtime.h>

#include "elm_internal.hpp"
#include "elm_dev_fine.hpp"
#include "elm_dev_pairs.hpp"

namespace elm {

// K5a: bit (c & 63) of word c >> 6 = cell c of the box occupied; cell c = (cx * ny + cy) * nz + cz.  A wave covers 64 consecutive cells
// (the launch is in whole workgroups of 256, so lane 0 of a wave holds a multiple of 64): one ballot, one 8-byte vector store.
__global__ __launch_bounds__(256) void k_reloc_bitmap(const DevMap m, const RelocBox b, uint64_t n_cells, unsigned long long* __restrict__ bits) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool occ = false;
    if (c < n_cells) {
        const uint64_t r = c / b.nz;
        const uint32_t cz = (uint32_t)(c - r * b.nz);
        const uint32_t cy = (uint32_t)(r % b.ny);
        const uint32_t cx = (uint32_t)(r / b.ny);
        occ = probe_voxel(m, b.x0 + (int)cx, b.y0 + (int)cy, b.z0 + (int)cz).vid >= 0;
    }
    const unsigned long long w = __ballot(occ);
    if ((threadIdx.x & 63u) == 0 && c < n_cells) bits[c >> 6] = w;
}

// The score contract's key of one transformed coordinate: (int)(q / voxel_size), or q * (1 / voxel_size) where that product is exact
// (power-of-two voxel sizes, DevMap::inv_vs_exact), which gives the same bits.  Shared by the score, the leaf scores and the bounds.
__device__ __forceinline__ int reloc_key(double q, const DevMap& m) { return m.inv_vs_exact != 0.0 ? (int)(q * m.inv_vs_exact) : (int)(q / m.voxel_size); }

// One row of the rotation applied to a scan point in the score contract's association, ((R_r0 x + R_r1 y) + R_r2 z) (float64, no
// contraction); the score adds t_r to it, the bounds add the ends of a node's t range -- the monotonicity argument of DESIGN.md section 12
// needs both to start from this same value.
__device__ __forceinline__ double reloc_rotate(double a0, double a1, double a2, double x, double y, double z) { return (a0 * x + a1 * y) + a2 * z; }

// Whether key (kx, ky, kz) is a voxel of the map: the occupancy bitmap of box b (FORM 0: in LDS, 1: in global memory) inside the box, a hash
// probe outside it (FORM 2: always) -- the same answer in every form.
template <int FORM>
__device__ __forceinline__ bool reloc_point_hit(const DevMap& m, const RelocBox& b, const uint32_t* bits, int kx, int ky, int kz) {
    const uint32_t cx = (uint32_t)(kx - b.x0), cy = (uint32_t)(ky - b.y0), cz = (uint32_t)(kz - b.z0);
    if (FORM < 2 && cx < b.nx && cy < b.ny && cz < b.nz) {
        const uint32_t c = (cx * b.ny + cy) * b.nz + cz; // < 2^32: the host uses forms 0 / 1 only for such boxes
        return (bits[c >> 5] >> (c & 31u)) & 1u;
    }
    return probe_voxel(m, kx, ky, kz).vid >= 0;
}

// K5b.  Workgroup = kRelocHyp consecutive hypotheses x one chunk of kRelocChunk points; every lane keeps kRelocPPL points in registers
// (float64) and the workgroup loops over its hypotheses, whose poses are workgroup-uniform (scalar loads).  Per hypothesis each wave counts
// its hits with ballot + popcount; the four waves combine through LDS and one lane per hypothesis stores the workgroup's partial.
// poses: 12 doubles per hypothesis, the top three rows of T (row-major: R_r0, R_r1, R_r2, t_r).  The arithmetic is the score contract's:
// q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r in float64 (no contraction: -ffp-contract=off), k = (int)(q / voxel_size) -- or q * (1 / voxel_size)
// where that product is exact (power-of-two voxel sizes, DevMap::inv_vs_exact), which gives the same bits.
template <int FORM>
__global__ __launch_bounds__(256) void k_reloc_score(const DevMap m, const float* __restrict__ pts, uint32_t n, const double* __restrict__ poses,
                                                     uint32_t n_poses, const RelocBox b, const uint32_t* __restrict__ bits, uint32_t n_words,
                                                     uint32_t n_chunks, uint32_t* __restrict__ partial) {
    extern __shared__ uint32_t lds[]; // [kRelocHyp * 4] wave counts, then (FORM 0) the bitmap's n_words words
    uint32_t* wcnt = lds;
    uint32_t* lbits = lds + kRelocHyp * 4;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t chunk = blockIdx.x % n_chunks, h0 = (blockIdx.x / n_chunks) * kRelocHyp;
    double px[kRelocPPL], py[kRelocPPL], pz[kRelocPPL];
    bool valid[kRelocPPL];
#pragma unroll
    for (int k = 0; k < kRelocPPL; ++k) {
        const uint32_t i = chunk * kRelocChunk + (uint32_t)k * 256u + tid;
        valid[k] = i < n;
        const uint32_t j = valid[k] ? i : 0u;
        px[k] = (double)pts[3 * (size_t)j];
        py[k] = (double)pts[3 * (size_t)j + 1];
        pz[k] = (double)pts[3 * (size_t)j + 2];
    }
    if (FORM == 0) {
        for (uint32_t w = tid; w < n_words; w += 256u) lbits[w] = bits[w];
        __syncthreads();
    }
    const uint32_t hn = min((uint32_t)kRelocHyp, n_poses - h0);
    for (uint32_t hl = 0; hl < hn; ++hl) {
        const double* P = poses + (size_t)(h0 + hl) * 12;
        const double r00 = P[0], r01 = P[1], r02 = P[2], t0 = P[3];
        const double r10 = P[4], r11 = P[5], r12 = P[6], t1 = P[7];
        const double r20 = P[8], r21 = P[9], r22 = P[10], t2 = P[11];
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < kRelocPPL; ++k) {
            const double x = px[k], y = py[k], z = pz[k];
            const bool hit = valid[k] && reloc_point_hit<FORM>(m, b, FORM == 0 ? lbits : bits, reloc_key(reloc_rotate(r00, r01, r02, x, y, z) + t0, m),
                                                                reloc_key(reloc_rotate(r10, r11, r12, x, y, z) + t1, m),
                                                                reloc_key(reloc_rotate(r20, r21, r22, x, y, z) + t2, m));
            cnt += (uint32_t)__popcll(__ballot(hit));
        }
        if ((tid & 63u) == 0) wcnt[hl * 4 + wave] = cnt;
    }
    __syncthreads();
    if (tid < hn) partial[(size_t)(h0 + tid) * n_chunks + chunk] = ((wcnt[tid * 4] + wcnt[tid * 4 + 1]) + wcnt[tid * 4 + 2]) + wcnt[tid * 4 + 3];
}

// K5c: scores[h] = the chunk partials of hypothesis h, summed in chunk order
__global__ __launch_bounds__(256) void k_reloc_sum(const uint32_t* __restrict__ partial, uint32_t n_chunks, uint32_t n_poses, uint32_t* __restrict__ scores) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n_poses) return;
    uint32_t s;
    sum_chunk_partials<1, 1>(partial + (size_t)h * n_chunks, n_chunks, &s, nullptr);
    scores[h] = s;
}

void launch_reloc_bitmap(hipStream_t s, const DevMap& m, const RelocBox& b, uint64_t n_cells, unsigned long long* bits) {
    if (!n_cells) return;
    hipLaunchKernelGGL(k_reloc_bitmap, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, s, m, b, n_cells, bits);
}

void launch_reloc_score(hipStream_t s, int form, const DevMap& m, const float* pts, uint32_t n, const double* poses, uint32_t n_poses,
                        const RelocBox& b, const uint32_t* bits, uint32_t n_words, uint32_t* partial, uint32_t* scores) {
    if (!n || !n_poses) return;
    const uint32_t n_chunks = (n + kRelocChunk - 1) / kRelocChunk;
    const uint32_t n_hblk = (n_poses + kRelocHyp - 1) / kRelocHyp;
    const dim3 grid(n_chunks * n_hblk), blk(256);
    const size_t lds = (size_t)kRelocHyp * 4 * sizeof(uint32_t) + (form == 0 ? (size_t)n_words * sizeof(uint32_t) : 0);
    if (form == 0) hipLaunchKernelGGL(k_reloc_score<0>, grid, blk, lds, s, m, pts, n, poses, n_poses, b, bits, n_words, n_chunks, partial);
    else if (form == 1) hipLaunchKernelGGL(k_reloc_score<1>, grid, blk, lds, s, m, pts, n, poses, n_poses, b, bits, n_words, n_chunks, partial);
    else hipLaunchKernelGGL(k_reloc_score<2>, grid, blk, lds, s, m, pts, n, poses, n_poses, b, bits, n_words, n_chunks, partial);
    hipLaunchKernelGGL(k_reloc_sum, dim3((n_poses + 255) / 256), dim3(256), 0, s, partial, n_chunks, n_poses, scores);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// global relocalization
//   K5d k_ground_heights     the ground field g(x, y) of a batch of xy queries through the map's 2-D bin index, elm_map_find_ground_height's
//                            arithmetic: the 5 lowest z of the points with dx*dx + dy*dy <= 25 kept sorted in registers, summed ascending
//   K5e k_reloc_window_or    one axis of a level's window bitmap from the previous level's (separable sliding OR, word-wise over z)
//   K5f k_reloc_bound        upper bounds of search nodes (k_reloc_score's shape: float64 points in registers, one uniform node per step)
//   K5g k_reloc_leaf_rows    the pose rows of lattice leaves, built as the host builds the lattice poses

__global__ __launch_bounds__(256) void k_ground_heights(const GroundIndex gi, const double* __restrict__ xy, uint32_t n, double* __restrict__ z,
                                                        int32_t* __restrict__ found) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const double x = xy[2 * (size_t)q], y = xy[2 * (size_t)q + 1];
    double lo[5] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, HUGE_VAL, HUGE_VAL};
    uint32_t cnt = 0;
    if (isfinite(x) && isfinite(y) && gi.nbx > 0) {
        // bins within two of the query's (a point within 5 m lies in one: 2 * kGroundBin > 5 + the rounding of the bin arithmetic)
        const double fx = floor((x - gi.x0) / gi.bin), fy = floor((y - gi.y0) / gi.bin);
        const int bx0 = (int)fmin(fmax(fx - 2.0, 0.0), (double)gi.nbx), bx1 = (int)fmax(fmin(fx + 2.0, (double)gi.nbx - 1.0), -1.0);
        const int by0 = (int)fmin(fmax(fy - 2.0, 0.0), (double)gi.nby), by1 = (int)fmax(fmin(fy + 2.0, (double)gi.nby - 1.0), -1.0);
        for (int bx = bx0; bx <= bx1; ++bx)
            for (int by = by0; by <= by1; ++by) {
                // skip a bin whose rectangle lies farther than 5 m (with a margin far above the rounding of these terms)
                const double ex = fmax(fmax(gi.x0 + bx * gi.bin - x, x - (gi.x0 + (bx + 1) * gi.bin)), 0.0);
                const double ey = fmax(fmax(gi.y0 + by * gi.bin - y, y - (gi.y0 + (by + 1) * gi.bin)), 0.0);
                if (ex * ex + ey * ey > 25.5) continue;
                const uint32_t b = (uint32_t)bx * (uint32_t)gi.nby + (uint32_t)by;
                const uint32_t e = gi.start[b + 1];
                for (uint32_t i = gi.start[b]; i < e; ++i) {
                    const float4 p = gi.pts[i];
                    const double dx = (double)p.x - x, dy = (double)p.y - y;
                    if (dx * dx + dy * dy <= 25.0) {
                        ++cnt;
                        double v = (double)p.z;
#pragma unroll
                        for (int r = 0; r < 5; ++r) {
                            const double a = lo[r];
                            const bool lt = v < a;
                            lo[r] = lt ? v : a;
                            v = lt ? a : v;
                        }
                    }
                }
            }
    }
    if (cnt > 3) {
        const uint32_t N = min(cnt, 5u);
        double s = 0.0;
#pragma unroll
        for (uint32_t r = 0; r < 5; ++r)
            if (r < N) s += lo[r];
        z[q] = s / (double)N;
        found[q] = 1;
    } else {
        z[q] = 0.0;
        found[q] = 0;
    }
}

// K5e: out(c) = OR of in over [c, c + w) along the axis, where every word of in already ORs a window of width wp: reads at the offsets
// 0, wp, 2 wp, ... below w - wp, then w - wp (each window inside [c, c + w), together covering it).  One thread per 32-bit word.
__global__ __launch_bounds__(256) void k_reloc_window_or(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t nx, uint32_t ny,
                                                         uint32_t nzw, int axis, uint32_t wp, uint32_t w) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t total = (uint64_t)nx * ny * nzw;
    if (t >= total) return;
    const uint32_t wz = (uint32_t)(t % nzw);
    const uint64_t col = t / nzw;
    const uint32_t cy = (uint32_t)(col % ny), cx = (uint32_t)(col / ny);
    const uint32_t c = axis == 0 ? cx : cy, n = axis == 0 ? nx : ny;
    uint32_t acc = 0;
    for (uint32_t d = 0;; d += wp) {
        const uint32_t off = d + wp < w ? d : w - wp;
        if (c + off < n) {
            const uint64_t src = axis == 0 ? ((uint64_t)(c + off) * ny + cy) * nzw + wz : ((uint64_t)cx * ny + (c + off)) * nzw + wz;
            acc |= in[src];
        }
        if (off == w - wp) break;
    }
    out[t] = acc;
}

// K5f.  Workgroup = kRelocHyp consecutive nodes x one chunk of kRelocChunk points (k_reloc_score's shape).  Per point and node the x, y, z
// ranges of q = a + t over the node (a = the rotated point, fl(a + t) monotone in t) give key ranges; the point counts when
//   the x or y key range is wider than the window w (the window would not cover it), or its z range exceeds kz_cap keys, or
//   the window at (key(a_x + xlo), key(a_y + ylo)) -- clamped to the box, which only widens it -- is occupied at a kz of the z range.
__global__ __launch_bounds__(256) void k_reloc_bound(const DevMap m, const float* __restrict__ pts, uint32_t n, const RelocNode* __restrict__ nodes,
                                                     uint32_t n_nodes, const double* __restrict__ rot, const RelocBox b,
                                                     const uint32_t* __restrict__ bits, uint32_t w, uint32_t kz_cap, uint32_t n_chunks,
                                                     uint32_t* __restrict__ partial) {
    __shared__ uint32_t wcnt[kRelocHyp * 4];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t chunk = blockIdx.x % n_chunks, h0 = (blockIdx.x / n_chunks) * kRelocHyp;
    const uint32_t nzw = b.nz >> 5;
    double px[kRelocPPL], py[kRelocPPL], pz[kRelocPPL];
    bool valid[kRelocPPL];
#pragma unroll
    for (int k = 0; k < kRelocPPL; ++k) {
        const uint32_t i = chunk * kRelocChunk + (uint32_t)k * 256u + tid;
        valid[k] = i < n;
        const uint32_t j = valid[k] ? i : 0u;
        px[k] = (double)pts[3 * (size_t)j];
        py[k] = (double)pts[3 * (size_t)j + 1];
        pz[k] = (double)pts[3 * (size_t)j + 2];
    }
    const uint32_t hn = min((uint32_t)kRelocHyp, n_nodes - h0);
    for (uint32_t hl = 0; hl < hn; ++hl) {
        const RelocNode nd = nodes[h0 + hl];
        const double* R = rot + (size_t)nd.k * 9;
        const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < kRelocPPL; ++k) {
            const double x = px[k], y = py[k], z = pz[k];
            const double ax = reloc_rotate(r00, r01, r02, x, y, z), ay = reloc_rotate(r10, r11, r12, x, y, z), az = reloc_rotate(r20, r21, r22, x, y, z);
            const int kx0 = reloc_key(ax + nd.xlo, m), kx1 = reloc_key(ax + nd.xhi, m);
            const int ky0 = reloc_key(ay + nd.ylo, m), ky1 = reloc_key(ay + nd.yhi, m);
            const int kz0 = reloc_key(az + nd.zlo, m), kz1 = reloc_key(az + nd.zhi, m);
            bool hit = false;
            if (valid[k]) {
                if ((uint32_t)(kx1 - kx0) >= w || (uint32_t)(ky1 - ky0) >= w) hit = true;
                else if (kx1 >= b.x0 && ky1 >= b.y0 && kz1 >= b.z0 && kx0 - b.x0 < (int)b.nx && ky0 - b.y0 < (int)b.ny &&
                         kz0 - b.z0 < (int)b.nz) {
                    const uint32_t cz0 = (uint32_t)max(kz0 - b.z0, 0), cz1 = (uint32_t)min(kz1 - b.z0, (int)b.nz - 1);
                    if (cz1 - cz0 >= kz_cap) hit = true;
                    else {
                        const uint32_t cx = (uint32_t)max(kx0 - b.x0, 0), cy = (uint32_t)max(ky0 - b.y0, 0);
                        const uint32_t* col = bits + ((size_t)cx * b.ny + cy) * nzw;
                        for (uint32_t wd = cz0 >> 5; wd <= (cz1 >> 5) && !hit; ++wd) {
                            const uint32_t lo_b = wd == (cz0 >> 5) ? (cz0 & 31u) : 0u, hi_b = wd == (cz1 >> 5) ? (cz1 & 31u) : 31u;
                            const uint32_t mask = (0xFFFFFFFFu >> (31u - hi_b)) & (0xFFFFFFFFu << lo_b);
                            hit = (col[wd] & mask) != 0u;
                        }
                    }
                }
            }
            cnt += (uint32_t)__popcll(__ballot(hit));
        }
        if ((tid & 63u) == 0) wcnt[hl * 4 + wave] = cnt;
    }
    __syncthreads();
    if (tid < hn) partial[(size_t)(h0 + tid) * n_chunks + chunk] = ((wcnt[tid * 4] + wcnt[tid * 4 + 1]) + wcnt[tid * 4 + 2]) + wcnt[tid * 4 + 3];
}

// K5g: the pose rows (R_r0, R_r1, R_r2, t_r) of lattice leaf hyps[l]; t = (x_min + (double)i * step, y_min + (double)j * step, gz[i NY + j])
__global__ __launch_bounds__(256) void k_reloc_leaf_rows(const uint32_t* __restrict__ hyps, uint32_t n, const double* __restrict__ rot, double x_min,
                                                         double y_min, double step, uint32_t NX, uint32_t NY, const double* __restrict__ gz,
                                                         double* __restrict__ rows) {
    const uint32_t l = blockIdx.x * 256u + threadIdx.x;
    if (l >= n) return;
    const uint32_t h = hyps[l];
    const uint32_t j = h % NY, i = (h / NY) % NX, k = h / NY / NX;
    const double* R = rot + (size_t)k * 9;
    const double t[3] = {x_min + (double)i * step, y_min + (double)j * step, gz[(size_t)i * NY + j]};
    double* P = rows + (size_t)l * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P[r * 4] = R[r * 3];
        P[r * 4 + 1] = R[r * 3 + 1];
        P[r * 4 + 2] = R[r * 3 + 2];
        P[r * 4 + 3] = t[r];
    }
}

void launch_ground_heights(hipStream_t s, const GroundIndex& gi, const double* xy, uint32_t n, double* z, int32_t* found) {
    if (!n) return;
    hipLaunchKernelGGL(k_ground_heights, dim3((n + 255) / 256), dim3(256), 0, s, gi, xy, n, z, found);
}

void launch_reloc_window_or(hipStream_t s, const uint32_t* in, uint32_t* out, uint32_t nx, uint32_t ny, uint32_t nzw, int axis, uint32_t wp, uint32_t w) {
    const uint64_t total = (uint64_t)nx * ny * nzw;
    if (!total) return;
    hipLaunchKernelGGL(k_reloc_window_or, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, nx, ny, nzw, axis, wp, w);
}

void launch_reloc_bound(hipStream_t s, const DevMap& m, const float* pts, uint32_t n, const RelocNode* nodes, uint32_t n_nodes, const double* rot,
                        const RelocBox& b, const uint32_t* bits, uint32_t w, uint32_t kz_cap, uint32_t* partial, uint32_t* bounds) {
    if (!n || !n_nodes) return;
    const uint32_t n_chunks = (n + kRelocChunk - 1) / kRelocChunk;
    const uint32_t n_blk = (n_nodes + kRelocHyp - 1) / kRelocHyp;
    hipLaunchKernelGGL(k_reloc_bound, dim3(n_chunks * n_blk), dim3(256), 0, s, m, pts, n, nodes, n_nodes, rot, b, bits, w, kz_cap, n_chunks, partial);
    hipLaunchKernelGGL(k_reloc_sum, dim3((n_nodes + 255) / 256), dim3(256), 0, s, partial, n_chunks, n_nodes, bounds);
}

void launch_reloc_leaf_rows(hipStream_t s, const uint32_t* hyps, uint32_t n, const double* rot, double x_min, double y_min, double step,
                            uint32_t NX, uint32_t NY, const double* gz, double* rows) {
    if (!n) return;
    hipLaunchKernelGGL(k_reloc_leaf_rows, dim3((n + 255) / 256), dim3(256), 0, s, hyps, n, rot, x_min, y_min, step, NX, NY, gz, rows);
}

} // namespace elm
