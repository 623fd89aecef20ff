// elm_k_loops.hip -- the loop consistency check (elm_loops_consistency; the contract is in include/elimaloc_hip_loops.h; DESIGN.md
// section 24): the L x L pair terms as a bit matrix, and the greedy clique over it.  Float64 without contraction in the pair term, integers
// after it.  No atomics, no inline assembly, no scratch; plain launches on the context's stream.
//   K14a k_lc_adjacency  one wavefront per 64-bit word of one row: every lane its pair, the word is the wave's ballot
//   K14b k_lc_degree     one wavefront per loop: its neighbours inside the candidate set (popcounts, an integer wave sum)
//   K14c k_lc_pick       one workgroup: the candidate of the largest (degree, lowest index), the member byte, the next candidate set
// A greedy step reads the candidate set and the stop word of its parity and writes those of the other parity, so nothing a launch reads
// is written in it; a set stop word makes the rest of a queued batch return at once.
#include <hip/hip_runtime.h>

#include "elm_dev_loops.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

__device__ __forceinline__ void lc_load12(const double* __restrict__ p, double out[12]) {
#pragma unroll
    for (int q = 0; q < 12; ++q) out[q] = p[q];
}

} // namespace

// K14a.  Wavefront (row, w) owns word w of row `row`: lane c is column 64 w + c.  The pair is always evaluated as (k, l) = (the lower,
// the higher index), so both triangles get the same bits and the same s without a transpose.  The row's ends and variances are the
// same for the whole wavefront (the wavefront's number is made uniform, so they are loaded once, by scalar loads); those of the lane's
// own loop, the four poses of the pair and its two measurements are gathered by the lane.  A lane on the diagonal or past L computes a pair of valid loops (its column is
// clamped) and is masked out of the ballot, so the padding bits and the diagonal are zero.
__global__ __launch_bounds__(256) void k_lc_adjacency(const LcDev d, double q_t, double q_r, double gamma) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + wave;
    if (wid >= d.L * d.W) return;
    const uint32_t row = wid / d.W, w = wid - row * d.W;
    const uint32_t col_raw = w * 64u + lane;
    const bool valid = col_raw < d.L && col_raw != row;
    const uint32_t col = col_raw < d.L ? col_raw : d.L - 1u;
    const bool row_low = row < col;
    const uint32_t k = row_low ? row : col, l = row_low ? col : row;
    const int32_t a_row = d.a[row], b_row = d.b[row], a_col = d.a[col], b_col = d.b[col];
    const double vt_row = d.var_t[row], vr_row = d.var_r[row], vt_col = d.var_t[col], vr_col = d.var_r[col];
    const int32_t ak = row_low ? a_row : a_col, bk = row_low ? b_row : b_col, al = row_low ? a_col : a_row, bl = row_low ? b_col : b_row;
    double Pak[12], Pbk[12], PZk[12], Pal[12], Pbl[12], PZl[12], e[6];
    lc_load12(d.poses + 12 * (size_t)ak, Pak);
    lc_load12(d.poses + 12 * (size_t)bk, Pbk);
    lc_load12(d.Z + 12 * (size_t)k, PZk);
    lc_load12(d.poses + 12 * (size_t)al, Pal);
    lc_load12(d.poses + 12 * (size_t)bl, Pbl);
    lc_load12(d.Z + 12 * (size_t)l, PZl);
    lc_pair_e(Pak, Pbk, PZk, Pal, Pbl, PZl, e);
    const int32_t da = ak > al ? ak - al : al - ak, db = bk > bl ? bk - bl : bl - bk;
    // (a sum of two variances does not depend on which of them is k's)
    const double s = lc_pair_s(e, vt_row, vt_col, vr_row, vr_col, (double)(da + db), q_t, q_r);
    const unsigned long long word = __ballot(valid && s <= gamma); // a NaN compares false: not adjacent
    if (lane == 0u) d.adj[wid] = word;                              // wid = row * W + w
    if (d.s && col_raw < d.L) d.s[(size_t)row * d.L + col_raw] = col_raw == row ? 0.0 : s;
}

// K14b.  Wavefront v: -1 for a loop outside the candidate set, else the popcount of adj[v] & cand, lanes striding the words.
__global__ __launch_bounds__(256) void k_lc_degree(const LcDev d, uint32_t it, int32_t* __restrict__ deg) {
    const uint32_t p = it & 1u;
    if (d.state->stop[p]) return;
    const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (v >= d.L) return;
    const unsigned long long* __restrict__ cand = d.cand + (size_t)p * d.W;
    if (!((cand[v >> 6] >> (v & 63u)) & 1ull)) {
        if (lane == 0u) deg[v] = -1;
        return;
    }
    const unsigned long long* __restrict__ row = d.adj + (size_t)v * d.W;
    int n = 0;
    for (uint32_t w = lane; w < d.W; w += 64u) n += __popcll(row[w] & cand[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0u) deg[v] = n;
}

// K14c.  The largest key degree * 2^32 + (0xFFFFFFFF - v) over all loops (lane t takes t, t + 256, ..., then a fixed tree in LDS): the
// most neighbours, the lowest index among equals.  A negative key means that no loop is a candidate: the stop word is set.
__global__ __launch_bounds__(256) void k_lc_pick(const LcDev d, uint32_t it, const int32_t* __restrict__ deg) {
    __shared__ long long buf[256];
    const uint32_t p = it & 1u, tid = threadIdx.x;
    if (d.state->stop[p]) {
        if (tid == 0u) d.state->stop[p ^ 1u] = 1u;
        return;
    }
    long long best = -1;
    for (uint32_t v = tid; v < d.L; v += 256u) {
        const long long key = (long long)deg[v] * 4294967296ll + (long long)(0xFFFFFFFFu - v);
        best = key > best ? key : best;
    }
    buf[tid] = best;
    __syncthreads();
#pragma unroll
    for (uint32_t h = 128u; h > 0u; h >>= 1) {
        if (tid < h) buf[tid] = buf[tid] > buf[tid + h] ? buf[tid] : buf[tid + h];
        __syncthreads();
    }
    best = buf[0];
    if (best < 0) {
        if (tid == 0u) d.state->stop[p ^ 1u] = 1u;
        return;
    }
    const uint32_t v = 0xFFFFFFFFu - (uint32_t)((unsigned long long)best & 0xFFFFFFFFull);
    const unsigned long long* __restrict__ cand = d.cand + (size_t)p * d.W;
    unsigned long long* __restrict__ next = d.cand + (size_t)(p ^ 1u) * d.W;
    const unsigned long long* __restrict__ row = d.adj + (size_t)v * d.W;
    for (uint32_t w = tid; w < d.W; w += 256u) next[w] = cand[w] & row[w];
    if (tid == 0u) {
        d.member[v] = 1;
        d.state->size = it + 1u;
        d.state->stop[p ^ 1u] = 0u;
    }
}

void launch_lc_adjacency(hipStream_t s, const LcDev& d, double q_t, double q_r, double gamma) {
    if (!d.L) return;
    hipLaunchKernelGGL(k_lc_adjacency, dim3((d.L * d.W + 3u) / 4u), dim3(256), 0, s, d, q_t, q_r, gamma);
}

void launch_lc_step(hipStream_t s, const LcDev& d, uint32_t it) {
    if (!d.L) return;
    int32_t* deg = it == 0u ? d.deg0 : d.deg;
    hipLaunchKernelGGL(k_lc_degree, dim3((d.L + 3u) / 4u), dim3(256), 0, s, d, it, deg);
    hipLaunchKernelGGL(k_lc_pick, dim3(1), dim3(256), 0, s, d, it, (const int32_t*)deg);
}

} // namespace elm
