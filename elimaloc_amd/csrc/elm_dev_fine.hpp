// elm_dev_fine.hpp -- device code shared by the kernels that read the fine occupancy table of a map (FineTable, elm_internal.hpp): the
// free-space check (elm_k_free.hip), the ray cast (elm_k_ray.hip, section 14), the map evidence (elm_k_evid.hip,
// section 15) and the map growth (elm_k_grow.hip, section 16), with the tables that the growth kernels fill themselves.
#pragma once
#include <hip/hip_runtime.h>

#include "elm_internal.hpp"

namespace elm {

// The contract's fine cell of one world coordinate: (int)floor(q / cell), or q * (1 / cell) where that product is exact.
__device__ __forceinline__ int fine_of(double q, const FineTable& ft) {
    return (int)floor(ft.inv_cell_exact != 0.0 ? q * ft.inv_cell_exact : q / ft.cell);
}

// The 64-bit mask of coarse cell (cx, cy, cz); 0 when the map has no point there.
__device__ __forceinline__ unsigned long long fine_probe(const FineTable& ft, int cx, int cy, int cz) {
    uint32_t h = hash3(cx, cy, cz) & ft.mask;
    for (;;) {
        const int4 k = ft.keys[h];
        if (k.w == 0) return 0ull;
        if (k.x == cx && k.y == cy && k.z == cz) return ft.masks[h];
        h = (h + 1) & ft.mask;
    }
}

// The same probe, also giving the table slot of the coarse cell (left alone when the cell is absent): the map evidence addresses its
// counters by slot.
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

// The exit parameter of cell c along one axis of a cell walk: the far face in the direction of travel, from the integer cell (never
// accumulated).
__device__ __forceinline__ double exit_param(int c, int up, double cell, double s, double w) { return ((double)(c + up) * cell - s) / w; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// The rows of one pose [R | t], workgroup-uniform: 12 doubles (R_r0, R_r1, R_r2, t_r) per row r.
struct PoseRows {
    double r00, r01, r02, t0, r10, r11, r12, t1, r20, r21, r22, t2;
};

} // namespace elm
