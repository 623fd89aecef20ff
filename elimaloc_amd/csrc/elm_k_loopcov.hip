// elm_k_loopcov.hip -- the loop consistency check with a propagated covariance (elm_loopcov_chain, elm_loopcov_consistency; the contract is
// in include/elimaloc_hip_loopcov.h).  Float64 without contraction.  No atomics, no inline assembly, no scratch;
// plain launches on the context's stream.  The greedy clique is that of elm_k_loops.hip.
//   K15a k_lcv_terms      one lane per pose: the term P_{v-1} of the step into it (0 for pose 0), component-major
//   K15b k_lcv_scan       one workgroup per 1 024 elements of one of the 21 rows: an inclusive prefix sum in a fixed tree, and the block's total
//   K15c k_lcv_addback    adds the scanned totals of the blocks before it to every element
//   K15d k_lcv_expand     one lane per pose: W_v as a full 6 x 6 and, when asked for, S_v
//   K15e k_lcv_records    one lane per loop: Y_a, Y_b, Z, W_a, W_b, Sigma, component-major
//   K15f k_lcv_adjacency  one wavefront per 64-bit word of one row: every lane its pair, the word is the wave's ballot
//   K15g k_lcv_rowcount   one wavefront per row: the pairs of the row whose s is NaN
#include <hip/hip_runtime.h>

#include "elm_dev_loopcov.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

__device__ __forceinline__ void lcv_load12(const double* __restrict__ p, double out[12]) {
#pragma unroll
    for (int q = 0; q < 12; ++q) out[q] = p[q];
}

} // namespace

// K15a.  Wc[c][i] = P_{i-1}[c] for i >= 1 and 0 for i = 0: the inclusive prefix sum of it is W.
__global__ __launch_bounds__(256) void k_lcv_terms(const LcvChain c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c.n) return;
    double P[kLcvSym];
    if (i == 0u) {
#pragma unroll
        for (int q = 0; q < kLcvSym; ++q) P[q] = 0.0;
    } else {
        double P0[12], Pn[12], Q[kLcvSym];
        lcv_load12(c.poses, P0);
        lcv_load12(c.poses + 12 * (size_t)i, Pn);
        const double* __restrict__ q = c.Q + (c.q_count == 1u ? (size_t)0 : (size_t)kLcvSym * (i - 1u));
#pragma unroll
        for (int k = 0; k < kLcvSym; ++k) Q[k] = q[k];
        lcv_step_term(P0, Pn, Q, P);
    }
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) c.Wc[(size_t)q * c.n + i] = P[q];
}

// K15b.  Workgroup (blk, row): the inclusive prefix sum of elements blk * 1024 .. of row `row` (stride `stride`, `count` elements), in
// place.  The tree: a shift-and-add scan over the 64 lanes of each wavefront (offsets 1, 2, 4, .. 32), then the totals of the wavefronts
// before it added in sequence.  tot (when not null) takes the block's total at [row][blk].
__global__ __launch_bounds__(1024) void k_lcv_scan(double* __restrict__ data, uint32_t count, uint32_t stride, double* __restrict__ tot, uint32_t nb) {
    __shared__ double wave_tot[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = blockIdx.x * kLcvScanBlock + tid;
    double* __restrict__ row = data + (size_t)blockIdx.y * stride;
    double x = i < count ? row[i] : 0.0;
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const double up = __shfl_up(x, off, 64);
        if (lane >= off) x = up + x;
    }
    if (lane == 63u) wave_tot[wave] = x;
    __syncthreads();
    double before = 0.0;
    for (uint32_t w = 0; w < wave; ++w) before += wave_tot[w];
    x = before + x;
    if (i < count) row[i] = x;
    if (tot && tid == kLcvScanBlock - 1u) tot[(size_t)blockIdx.y * nb + blockIdx.x] = x;
}

// K15c.  Element i of a block after the first takes the scanned total of the blocks before it.
__global__ __launch_bounds__(256) void k_lcv_addback(const LcvChain c) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c.n || i < kLcvScanBlock) return;
    const size_t at = (size_t)blockIdx.y * c.n + i;
    c.Wc[at] = c.tot[(size_t)blockIdx.y * c.nb + (i / kLcvScanBlock - 1u)] + c.Wc[at];
}

// K15d.
__global__ __launch_bounds__(256) void k_lcv_expand(const LcvChain c, double* __restrict__ W_out, double* __restrict__ S_out) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= c.n) return;
    double W[kLcvSym];
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) W[q] = c.Wc[(size_t)q * c.n + v];
    double* __restrict__ w = W_out + 36 * (size_t)v;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) w[r * 6 + q] = W[lcv_sx(r, q)];
    if (!S_out) return;
    double P0[12], Pv[12], S[kLcvSym];
    lcv_load12(c.poses, P0);
    lcv_load12(c.poses + 12 * (size_t)v, Pv);
    lcv_local(P0, Pv, W, S);
    double* __restrict__ o = S_out + 36 * (size_t)v;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) o[r * 6 + q] = S[lcv_sx(r, q)];
}

// K15e.  Loop k's record: entry q at rec[q * Lp + k], so that the 64 loops of a wavefront of K15f are read side by side.
__global__ __launch_bounds__(256) void k_lcv_records(const LcvChain c, const LcvDev d) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= d.L) return;
    const uint32_t a = (uint32_t)d.a[k], b = (uint32_t)d.b[k];
    double P0[12], P[12], R[9], t[3];
    lcv_load12(c.poses, P0);
    double* __restrict__ out = d.rec + k;
    lcv_load12(c.poses + 12 * (size_t)a, P);
    lc_between(P0, P, R, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) out[(size_t)(kLcvRecYa + r * 4 + q) * d.Lp] = R[r * 3 + q];
        out[(size_t)(kLcvRecYa + r * 4 + 3) * d.Lp] = t[r];
    }
    lcv_load12(c.poses + 12 * (size_t)b, P);
    lc_between(P0, P, R, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) out[(size_t)(kLcvRecYb + r * 4 + q) * d.Lp] = R[r * 3 + q];
        out[(size_t)(kLcvRecYb + r * 4 + 3) * d.Lp] = t[r];
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) out[(size_t)(kLcvRecZ + q) * d.Lp] = d.Z[12 * (size_t)k + q];
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) {
        out[(size_t)(kLcvRecWa + q) * d.Lp] = c.Wc[(size_t)q * c.n + a];
        out[(size_t)(kLcvRecWb + q) * d.Lp] = c.Wc[(size_t)q * c.n + b];
        out[(size_t)(kLcvRecSigma + q) * d.Lp] = d.Sigma[(size_t)kLcvSym * k + q];
    }
}

// K15f.  The structure of k_lc_adjacency (elm_k_loops.hip): wavefront (row, w) owns word w of row `row`, lane c is column 64 w + c, the
// pair is always evaluated as (k, l) = (the lower, the higher index).  The row's record is the same for the whole wavefront (its number
// is made uniform, so the record comes by scalar loads); the lane's own is read from the component-major records, 64 loops side by side.
// A lane on the diagonal or past L computes a pair of valid loops (its column is clamped) and is masked out of both ballots.
__global__ __launch_bounds__(256) void k_lcv_adjacency(const LcvDev d, double gamma) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t wid = blockIdx.x * 4u + wave;
    if (wid >= d.L * d.W) return;
    const uint32_t row = wid / d.W, w = wid - row * d.W;
    const uint32_t col_raw = w * 64u + lane;
    const bool valid = col_raw < d.L && col_raw != row;
    const uint32_t col = col_raw < d.L ? col_raw : d.L - 1u;
    const bool row_low = row < col;
    const int32_t a_row = d.a[row], b_row = d.b[row], a_col = d.a[col], b_col = d.b[col];
    const double* __restrict__ rr = d.rec + row;
    const double* __restrict__ rc = d.rec + col;
    // The stages of lcv_pair with the loads of each stage placed before it (the scheduler is kept from moving them up: all 198 values
    // of the two records live at once cost 400 registers).
    double e[6], cov[kLcvSym], S[kLcvSym];
    LcvFrames F;
    {
        double Yak[12], Ybk[12], PZk[12], Yal[12], Ybl[12], PZl[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const double ya_r = rr[(size_t)(kLcvRecYa + q) * d.Lp], ya_c = rc[(size_t)(kLcvRecYa + q) * d.Lp];
            const double yb_r = rr[(size_t)(kLcvRecYb + q) * d.Lp], yb_c = rc[(size_t)(kLcvRecYb + q) * d.Lp];
            const double z_r = rr[(size_t)(kLcvRecZ + q) * d.Lp], z_c = rc[(size_t)(kLcvRecZ + q) * d.Lp];
            Yak[q] = row_low ? ya_r : ya_c;
            Yal[q] = row_low ? ya_c : ya_r;
            Ybk[q] = row_low ? yb_r : yb_c;
            Ybl[q] = row_low ? yb_c : yb_r;
            PZk[q] = row_low ? z_r : z_c;
            PZl[q] = row_low ? z_c : z_r;
        }
        lcv_pair_frames(Yak, Ybk, PZk, Yal, Ybl, PZl, e, F);
    }
    __builtin_amdgcn_sched_barrier(0);
    // C(u, v) = W_max(u,v) - W_min(u,v), which does not depend on which loop is k
    const bool a_up = a_row > a_col, b_up = b_row > b_col;
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) {
        const double wa_r = rr[(size_t)(kLcvRecWa + q) * d.Lp], wa_c = rc[(size_t)(kLcvRecWa + q) * d.Lp];
        S[q] = a_up ? wa_r - wa_c : wa_c - wa_r;
    }
    lcv_sandwich(F.RA, F.tA, S, cov);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) {
        const double s_r = rr[(size_t)(kLcvRecSigma + q) * d.Lp], s_c = rc[(size_t)(kLcvRecSigma + q) * d.Lp];
        S[q] = row_low ? s_c : s_r; // Sigma_l
    }
    lcv_pair_add(F.Rl, F.tl, S, cov);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) {
        const double wb_r = rr[(size_t)(kLcvRecWb + q) * d.Lp], wb_c = rc[(size_t)(kLcvRecWb + q) * d.Lp];
        S[q] = b_up ? wb_r - wb_c : wb_c - wb_r;
    }
    lcv_pair_add(F.RB, F.tB, S, cov);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < kLcvSym; ++q) {
        const double s_r = rr[(size_t)(kLcvRecSigma + q) * d.Lp], s_c = rc[(size_t)(kLcvRecSigma + q) * d.Lp];
        S[q] = row_low ? s_r : s_c; // Sigma_k
    }
    const double s = lcv_pair_finish(S, e, cov);
    const unsigned long long word = __ballot(valid && s <= gamma); // a NaN compares false: not adjacent
    const unsigned long long nans = __ballot(valid && s != s);
    if (lane == 0u) {
        d.adj[wid] = word; // wid = row * W + w
        d.nanc[wid] = (uint8_t)__popcll(nans);
    }
    if (d.s && col_raw < d.L) d.s[(size_t)row * d.L + col_raw] = col_raw == row ? 0.0 : s;
}

// K15g.  Wavefront v: the sum of row v's NaN counts, lanes striding the words, an integer wave sum.
__global__ __launch_bounds__(256) void k_lcv_rowcount(const LcvDev d) {
    const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (v >= d.L) return;
    const uint8_t* __restrict__ row = d.nanc + (size_t)v * d.W;
    int n = 0;
    for (uint32_t w = lane; w < d.W; w += 64u) n += (int)row[w];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0u) d.nan_row[v] = n;
}

void launch_lcv_chain(hipStream_t s, const LcvChain& c) {
    if (!c.n) return;
    hipLaunchKernelGGL(k_lcv_terms, dim3((c.n + 255u) / 256u), dim3(256), 0, s, c);
    hipLaunchKernelGGL(k_lcv_scan, dim3(c.nb, kLcvSym), dim3(kLcvScanBlock), 0, s, c.Wc, c.n, c.n, c.tot, c.nb);
    if (c.nb > 1u) {
        hipLaunchKernelGGL(k_lcv_scan, dim3(1, kLcvSym), dim3(kLcvScanBlock), 0, s, c.tot, c.nb, c.nb, (double*)nullptr, 1u);
        hipLaunchKernelGGL(k_lcv_addback, dim3((c.n + 255u) / 256u, kLcvSym), dim3(256), 0, s, c);
    }
}

void launch_lcv_expand(hipStream_t s, const LcvChain& c, double* W_out, double* S_out) {
    if (!c.n) return;
    hipLaunchKernelGGL(k_lcv_expand, dim3((c.n + 255u) / 256u), dim3(256), 0, s, c, W_out, S_out);
}

void launch_lcv_adjacency(hipStream_t s, const LcvChain& c, const LcvDev& d, double gamma) {
    if (!d.L) return;
    hipLaunchKernelGGL(k_lcv_records, dim3((d.L + 255u) / 256u), dim3(256), 0, s, c, d);
    hipLaunchKernelGGL(k_lcv_adjacency, dim3((d.L * d.W + 3u) / 4u), dim3(256), 0, s, d, gamma);
    hipLaunchKernelGGL(k_lcv_rowcount, dim3((d.L + 3u) / 4u), dim3(256), 0, s, d);
}

} // namespace elm
