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
    const double vs = m.voxel_size, inv = m.inv_vs_exact;
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
            const double q0 = ((r00 * x + r01 * y) + r02 * z) + t0;
            const double q1 = ((r10 * x + r11 * y) + r12 * z) + t1;
            const double q2 = ((r20 * x + r21 * y) + r22 * z) + t2;
            int kx, ky, kz;
            if (inv != 0.0) { kx = (int)(q0 * inv); ky = (int)(q1 * inv); kz = (int)(q2 * inv); }
            else { kx = (int)(q0 / vs); ky = (int)(q1 / vs); kz = (int)(q2 / vs); }
            bool hit = false;
            if (valid[k]) {
                const uint32_t cx = (uint32_t)(kx - b.x0), cy = (uint32_t)(ky - b.y0), cz = (uint32_t)(kz - b.z0);
                if (FORM < 2 && cx < b.nx && cy < b.ny && cz < b.nz) {
                    const uint32_t c = (cx * b.ny + cy) * b.nz + cz; // < 2^32: the host uses forms 0 / 1 only for such boxes
                    const uint32_t word = (FORM == 0) ? lbits[c >> 5] : bits[c >> 5];
                    hit = (word >> (c & 31u)) & 1u;
                } else {
                    hit = probe_voxel(m, kx, ky, kz).vid >= 0;
                }
            }
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
    uint32_t s = 0;
    for (uint32_t c = 0; c < n_chunks; ++c) s += partial[(size_t)h * n_chunks + c];
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

} // namespace elm
