// elm_dev_scan.hpp -- the exclusive prefix sum one 1024-thread workgroup runs over an array of any length, shared by the device
// VoxelDownsample (elm_k_scan.hip, k_ds_offsets) and the device map build (elm_k_build.hip, k_bd_offsets).
#pragma once
#include <hip/hip_runtime.h>

namespace elm {

// In-place exclusive scan of a[0 .. n) by ONE workgroup of 1024 threads, in chunks of 1024 entries with a running carry; *total = the sum.
// s: 1024 words of LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ void chunk_scan_1024(unsigned* a, unsigned n, unsigned* total, unsigned* s) {
    unsigned carry = 0;
    for (unsigned base = 0; base < n; base += 1024) {
        const unsigned j = base + threadIdx.x;
        const unsigned v = j < n ? a[j] : 0u;
        s[threadIdx.x] = v;
        __syncthreads();
        for (unsigned off = 1; off < 1024; off <<= 1) {
            const unsigned t = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        if (j < n) a[j] = carry + s[threadIdx.x] - v;
        const unsigned chunk_total = s[1023];
        __syncthreads();
        carry += chunk_total;
    }
    if (threadIdx.x == 0) *total = carry;
}

} // namespace elm
