// elm_k_gridbuild.hip -- the device build of the P2P / GICP cell grid (include/elimaloc_hip.h, "device index build"; DESIGN.md section
// 19): DevMap::grid_blk / grid_idx / grid_start (and grid_tiles) from the stored points where they lie, byte for byte what
// grid_block_layout (elm_grid_layout.hpp) makes of the same points on the host.
//   k_gb_box          half-voxel cell of every coordinate (grid_cell_of), min / max per axis: workgroup reduction, integer atomics
//   k_gb_entry_dense  entry = linear cell; the sort's key and payload; integer atomicAdd into the one table of entries + 4 words
//   k_gb_tile_z / k_gb_tile_cnt / k_gb_tiles / k_gb_entry_tiled   the two-level form: z range per tile (integer atomicMin / atomicMax),
//                     64 * (nz + 1) entries per occupied tile (their 64-bit total is checked on the host before the 32-bit scan is
//                     used), the tile table, entry_of
//   k_gb_blocks / k_gb_start_fin   counts -> blocks of four in place; after the exclusive scan: + 1 (block 0 is padding), the four
//                     trailing words, the zero run of the two-level form's first 64 entries
//   k_gb_pad          every block and slot at its padding value, 16 bytes per lane, coalesced
//   k_gb_fill         one lane per point, in sorted order: rank = sorted position - first position of its entry, found in the sorted
//                     keys themselves (a backward gallop, then a bisection: at most 2 log2(n) loads however many points share a cell)
// The order inside an entry is the order of a STABLE sort by entry of (entry, point number) -- k_bd_rx_hist / k_bd_rx_scatter of
// elm_k_build.hip -- so it is a function of the input alone; the atomics above only count, take minima and maxima.
// Compiled like elm_k_build.hip: -ffp-contract=off, no fast-math (grid_cell_of's division and comparisons are the contract).
#include <hip/hip_runtime.h>

#include "elm_internal.hpp"

namespace elm {

constexpr unsigned kGbBlock = 256;

__device__ __forceinline__ void gb_cell3(const float4 p, double vs, int& cx, int& cy, int& cz) {
    cx = grid_cell_of((double)p.x, vs);
    cy = grid_cell_of((double)p.y, vs);
    cz = grid_cell_of((double)p.z, vs);
}

// box[0..2] = min, box[3..5] = max (initialised to INT32_MAX / INT32_MIN by the host)
__global__ __launch_bounds__(kGbBlock) void k_gb_box(const float4* __restrict__ pts, unsigned n, double vs, int* box) {
    __shared__ int s_r[kGbBlock / 64][6];
    int lx = INT32_MAX, ly = INT32_MAX, lz = INT32_MAX, hx = INT32_MIN, hy = INT32_MIN, hz = INT32_MIN;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kGbBlock + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * kGbBlock) {
        int cx, cy, cz;
        gb_cell3(pts[i], vs, cx, cy, cz);
        lx = min(lx, cx); ly = min(ly, cy); lz = min(lz, cz);
        hx = max(hx, cx); hy = max(hy, cy); hz = max(hz, cz);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lx = min(lx, __shfl_xor(lx, off, 64)); ly = min(ly, __shfl_xor(ly, off, 64)); lz = min(lz, __shfl_xor(lz, off, 64));
        hx = max(hx, __shfl_xor(hx, off, 64)); hy = max(hy, __shfl_xor(hy, off, 64)); hz = max(hz, __shfl_xor(hz, off, 64));
    }
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_r[wave][0] = lx; s_r[wave][1] = ly; s_r[wave][2] = lz;
        s_r[wave][3] = hx; s_r[wave][4] = hy; s_r[wave][5] = hz;
    }
    __syncthreads();
    if (threadIdx.x < 6u) {
        int v = s_r[0][threadIdx.x];
#pragma unroll
        for (unsigned w = 1; w < kGbBlock / 64; ++w) v = threadIdx.x < 3u ? min(v, s_r[w][threadIdx.x]) : max(v, s_r[w][threadIdx.x]);
        if (threadIdx.x < 3u) atomicMin(&box[threadIdx.x], v);
        else atomicMax(&box[threadIdx.x], v);
    }
}

// dense form: the linear cell in 64 bits, stored as 32 (the host has refused cells > 0xFFFFFFF0)
__global__ __launch_bounds__(kGbBlock) void k_gb_entry_dense(const float4* __restrict__ pts, unsigned n, double vs, int x0, int y0, int z0,
                                                             unsigned long long ny, unsigned long long nz, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ val, unsigned* cnt) {
    const unsigned i = blockIdx.x * kGbBlock + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    gb_cell3(pts[i], vs, cx, cy, cz);
    const unsigned long long l = ((unsigned long long)(cx - x0) * ny + (unsigned long long)(cy - y0)) * nz + (unsigned long long)(cz - z0);
    key[i] = (unsigned)l;
    val[i] = i;
    atomicAdd(&cnt[(unsigned)l], 1u); // integer counts: the sums do not depend on the order
}

// two-level form: z range per tile (zmin initialised to 0xFFFFFFFF, zmax to 0)
__global__ __launch_bounds__(kGbBlock) void k_gb_tile_z(const float4* __restrict__ pts, unsigned n, double vs, int x0, int y0, int z0,
                                                        unsigned long long tny, unsigned* zmin, unsigned* zmax) {
    const unsigned i = blockIdx.x * kGbBlock + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    gb_cell3(pts[i], vs, cx, cy, cz);
    cx -= x0; cy -= y0; cz -= z0;
    const unsigned long long t = (unsigned long long)(cx >> kTileShift) * tny + (unsigned long long)(cy >> kTileShift);
    atomicMin(&zmin[t], (unsigned)cz);
    atomicMax(&zmax[t], (unsigned)cz);
}
// entries per tile (0: empty) and their total in 64 bits
__global__ __launch_bounds__(kGbBlock) void k_gb_tile_cnt(const unsigned* __restrict__ zmin, const unsigned* __restrict__ zmax, unsigned n_tiles,
                                                          unsigned* __restrict__ tcnt, unsigned long long* total) {
    __shared__ unsigned long long s_sum[kGbBlock / 64];
    const unsigned t = blockIdx.x * kGbBlock + threadIdx.x;
    unsigned c = 0;
    if (t < n_tiles) {
        const unsigned lo = zmin[t];
        if (lo != 0xFFFFFFFFu) c = (unsigned)(kTile * kTile) * (zmax[t] - lo + 2u); // nz + 1 entries per column
        tcnt[t] = c;
    }
    unsigned long long sum = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
#pragma unroll
        for (unsigned w = 0; w < kGbBlock / 64; ++w) all += s_sum[w];
        if (all) atomicAdd(total, all);
    }
}
// tcnt: after its exclusive scan
__global__ __launch_bounds__(kGbBlock) void k_gb_tiles(const unsigned* __restrict__ zmin, const unsigned* __restrict__ zmax,
                                                       const unsigned* __restrict__ tcnt, unsigned n_tiles, uint2* __restrict__ tiles) {
    const unsigned t = blockIdx.x * kGbBlock + threadIdx.x;
    if (t >= n_tiles) return;
    const unsigned lo = zmin[t];
    tiles[t] = lo == 0xFFFFFFFFu ? make_uint2(0u, 0u) : make_uint2((unsigned)(kTile * kTile) + tcnt[t], lo | ((zmax[t] - lo + 1u) << 16));
}
__global__ __launch_bounds__(kGbBlock) void k_gb_entry_tiled(const float4* __restrict__ pts, unsigned n, double vs, int x0, int y0, int z0,
                                                             unsigned long long tny, const uint2* __restrict__ tiles,
                                                             unsigned* __restrict__ key, unsigned* __restrict__ val, unsigned* cnt) {
    const unsigned i = blockIdx.x * kGbBlock + threadIdx.x;
    if (i >= n) return;
    int cx, cy, cz;
    gb_cell3(pts[i], vs, cx, cy, cz);
    cx -= x0; cy -= y0; cz -= z0;
    const uint2 te = tiles[(unsigned long long)(cx >> kTileShift) * tny + (unsigned long long)(cy >> kTileShift)];
    const unsigned tz0 = te.y & 0xFFFFu, nz = te.y >> 16;
    const unsigned e = te.x + (unsigned)(((cx & (kTile - 1)) << kTileShift) | (cy & (kTile - 1))) * (nz + 1u) + ((unsigned)cz - tz0);
    key[i] = e;
    val[i] = i;
    atomicAdd(&cnt[e], 1u);
}

// counts -> blocks of four, in place
__global__ __launch_bounds__(kGbBlock) void k_gb_blocks(unsigned* __restrict__ a, unsigned entries) {
    const unsigned i = blockIdx.x * kGbBlock + threadIdx.x;
    if (i < entries) a[i] = (a[i] + 3u) >> 2;
}
// a: the exclusive scan of the blocks; *total: their sum (n_blk - 1)
__global__ __launch_bounds__(kGbBlock) void k_gb_start_fin(unsigned* __restrict__ a, unsigned entries, unsigned zero_head,
                                                           const unsigned* __restrict__ total) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kGbBlock + threadIdx.x;
    if (i >= (unsigned long long)entries + 4ull) return;
    unsigned v;
    if (i < entries) v = i < zero_head ? 0u : a[i] + 1u;
    else v = *total + 1u;
    a[i] = v;
}

// q16 < 4 * n_blk: three 16-byte quarters of coordinates and one of point numbers per block
__global__ __launch_bounds__(kGbBlock) void k_gb_pad(float4* __restrict__ blk4, uint4* __restrict__ idx4, unsigned long long n_blk) {
    const float c = 1e18f; // kGridPadCoord
    for (unsigned long long j = (unsigned long long)blockIdx.x * kGbBlock + threadIdx.x; j < 4ull * n_blk; j += (unsigned long long)gridDim.x * kGbBlock) {
        if (j < 3ull * n_blk) blk4[j] = make_float4(c, c, c, c);
        else idx4[j - 3ull * n_blk] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu); // kGridPadPoint
    }
}

// skey / sval: (entry, point number) sorted by entry, stable.  The block array may pass 4 GB: 64-bit offsets; slots stay below 2^31.
__global__ __launch_bounds__(kGbBlock) void k_gb_fill(const float4* __restrict__ pts, const unsigned* __restrict__ skey,
                                                      const unsigned* __restrict__ sval, unsigned n, const unsigned* __restrict__ start,
                                                      float* __restrict__ blk, unsigned* __restrict__ idx) {
    const unsigned p = blockIdx.x * kGbBlock + threadIdx.x;
    if (p >= n) return;
    const unsigned e = skey[p];
    // the first position f of entry e: skey[hi] == e throughout
    unsigned hi = p, lo = 0, step = 1;
    bool bracket = true; // skey[lo] < e
    for (;;) {
        if (hi < step) {
            if (skey[0] == e) { hi = 0; bracket = false; }
            break;
        }
        const unsigned q = hi - step;
        if (skey[q] == e) { hi = q; step <<= 1; }
        else { lo = q; break; }
    }
    if (bracket)
        while (hi - lo > 1u) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (skey[mid] == e) hi = mid;
            else lo = mid;
        }
    const unsigned u = sval[p];
    const size_t slot = 4 * (size_t)start[e] + (size_t)(p - hi);
    const float4 q = pts[u];
    float* b = blk + (slot >> 2) * 12 + (slot & 3);
    b[0] = q.x; b[4] = q.y; b[8] = q.z;
    idx[slot] = u;
}

static unsigned gb_grid(unsigned long long items, unsigned cap) {
    const unsigned long long nb = (items + kGbBlock - 1) / kGbBlock;
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}
void launch_gb_box(hipStream_t s, const float4* pts, unsigned n, double vs, int* box) {
    hipLaunchKernelGGL(k_gb_box, dim3(gb_grid(n, 2048)), dim3(kGbBlock), 0, s, pts, n, vs, box);
}
void launch_gb_entry_dense(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t ny, uint64_t nz, unsigned* key,
                           unsigned* val, unsigned* cnt) {
    hipLaunchKernelGGL(k_gb_entry_dense, dim3(gb_grid(n, ~0u)), dim3(kGbBlock), 0, s, pts, n, vs, lo[0], lo[1], lo[2], (unsigned long long)ny,
                       (unsigned long long)nz, key, val, cnt);
}
void launch_gb_tile_z(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t tny, unsigned* zmin, unsigned* zmax) {
    hipLaunchKernelGGL(k_gb_tile_z, dim3(gb_grid(n, ~0u)), dim3(kGbBlock), 0, s, pts, n, vs, lo[0], lo[1], lo[2], (unsigned long long)tny, zmin, zmax);
}
void launch_gb_tile_cnt(hipStream_t s, const unsigned* zmin, const unsigned* zmax, unsigned n_tiles, unsigned* tcnt, unsigned long long* total) {
    hipLaunchKernelGGL(k_gb_tile_cnt, dim3(gb_grid(n_tiles, ~0u)), dim3(kGbBlock), 0, s, zmin, zmax, n_tiles, tcnt, total);
}
void launch_gb_tiles(hipStream_t s, const unsigned* zmin, const unsigned* zmax, const unsigned* tcnt, unsigned n_tiles, uint2* tiles) {
    hipLaunchKernelGGL(k_gb_tiles, dim3(gb_grid(n_tiles, ~0u)), dim3(kGbBlock), 0, s, zmin, zmax, tcnt, n_tiles, tiles);
}
void launch_gb_entry_tiled(hipStream_t s, const float4* pts, unsigned n, double vs, const int32_t lo[3], uint64_t tny, const uint2* tiles,
                           unsigned* key, unsigned* val, unsigned* cnt) {
    hipLaunchKernelGGL(k_gb_entry_tiled, dim3(gb_grid(n, ~0u)), dim3(kGbBlock), 0, s, pts, n, vs, lo[0], lo[1], lo[2], (unsigned long long)tny, tiles,
                       key, val, cnt);
}
void launch_gb_blocks(hipStream_t s, unsigned* a, unsigned entries) {
    hipLaunchKernelGGL(k_gb_blocks, dim3(gb_grid(entries, ~0u)), dim3(kGbBlock), 0, s, a, entries);
}
void launch_gb_start_fin(hipStream_t s, unsigned* a, unsigned entries, unsigned zero_head, const unsigned* total) {
    hipLaunchKernelGGL(k_gb_start_fin, dim3(gb_grid((unsigned long long)entries + 4, ~0u)), dim3(kGbBlock), 0, s, a, entries, zero_head, total);
}
void launch_gb_pad(hipStream_t s, GridBlk* blk, uint32_t* idx, uint64_t n_blk) {
    hipLaunchKernelGGL(k_gb_pad, dim3(gb_grid(4ull * n_blk, 1u << 16)), dim3(kGbBlock), 0, s, (float4*)blk, (uint4*)idx, (unsigned long long)n_blk);
}
void launch_gb_fill(hipStream_t s, const float4* pts, const unsigned* skey, const unsigned* sval, unsigned n, const unsigned* start, GridBlk* blk,
                    uint32_t* idx) {
    hipLaunchKernelGGL(k_gb_fill, dim3(gb_grid(n, ~0u)), dim3(kGbBlock), 0, s, pts, skey, sval, n, start, (float*)blk, idx);
}

} // namespace elm
