// elm_k_free.hip -- free-space check: the rays of one scan tested against the fine occupancy of the map at many poses
// (elm_map_check_free_space).  Every result is an integer count, so the answer is the same on every run.
//   K6a k_free_rays   (ray chunk x pose block) partials: per pose the counted / pierced / end-occupied / supported rays and the samples /
//                     occupied samples of the chunk, and (optionally) every ray's occupied samples
//   K6b k_free_sum    per pose, the chunk partials summed in chunk order
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"

namespace elm {

namespace {

// One sample of a ray: a = o + u (k step), q = R a + t, whether q's fine cell is occupied.  mc keeps the last coarse cell probed:
// consecutive samples mostly share it (8 per cell along an axis at the defaults).
__device__ __forceinline__ bool sample_hit(const FineTable& ft, const FreeParams& fp, const PoseRows& P, double ux, double uy, double uz, int k,
                                           MaskCache& mc) {
    const double s = (double)k * fp.step;
    double q0, q1, q2;
    pose_apply(P, fp.ox + ux * s, fp.oy + uy * s, fp.oz + uz * s, q0, q1, q2);
    return mc.test(fine_of(q0, ft), fine_of(q1, ft), fine_of(q2, ft), FineProbe{ft});
}

} // namespace

// K6a.  Workgroup = 256 consecutive rays (one per lane, float64 in registers) x kFreePoses consecutive poses, whose rows are
// workgroup-uniform.  The ray's length, direction and sample count do not depend on the pose: they are formed once.
//   FORM 0: a lane walks its own ray; the last coarse cell's mask stays in registers (MaskCache), a probe only when the cell changes.
//   FORM 1: a wave walks its 64 rays one after the other, lane l taking samples k0 + l, k0 + l + 64, ...: no lane waits for a longer ray,
//           but neighbouring samples sit in different lanes, so nearly every sample is a probe.
// Per pose each wave counts with ballot + popcount (and one shuffle sum for the occupied samples); the four waves meet in LDS and one lane
// per pose stores the workgroup's partial.
template <int FORM>
__global__ __launch_bounds__(256) void k_free_rays(const FineTable ft, const FreeParams fp, const float* __restrict__ pts, uint32_t n,
                                                   const double* __restrict__ rows, uint32_t n_poses, uint32_t n_chunks, uint32_t* __restrict__ partial,
                                                   uint16_t* __restrict__ hits_out) {
    __shared__ uint32_t wcnt[kFreePoses][4][4]; // per pose and wave: pierced, end-occupied, supported, occupied samples
    __shared__ uint32_t wray[4][2];             // per wave: counted rays, samples (the same for every pose)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % n_chunks, h0 = (blockIdx.x / n_chunks) * kFreePoses;
    const uint32_t i = chunk * 256u + tid;
    const Beam b = load_beam(pts, i, n, fp.ox, fp.oy, fp.oz);
    const bool valid = b.valid;
    const bool counted = valid && in_window(b.L2, fp.min_r2, fp.max_r2) && b.L2 > 0.0; // (not b.cast: max_r2 may be infinite)
    const double L = sqrt(b.L2);
    const double reach = L - fmax(fp.margin_m, fp.margin_frac * L);
    int K = 0;
    if (counted && reach > 0.0) K = (int)fmin(floor(reach / fp.step), (double)fp.max_samples);
    const double ux = b.dx / L, uy = b.dy / L, uz = b.dz / L;
    const uint32_t n_s = K >= fp.k0 ? (uint32_t)(K - fp.k0 + 1) : 0u;
    {
        const uint32_t c = wave_count(counted), s = wave_sum(n_s);
        if (lane == 0) {
            wray[wave][0] = c;
            wray[wave][1] = s;
        }
    }
    const uint32_t hn = min((uint32_t)kFreePoses, n_poses - h0);
    for (uint32_t hl = 0; hl < hn; ++hl) {
        const PoseRows P = load_pose_rows(rows + (size_t)(h0 + hl) * 12);
        uint32_t hits = 0;
        MaskCache mc;
        if (FORM == 0) {
            for (int k = fp.k0; k <= K; ++k) hits += sample_hit(ft, fp, P, ux, uy, uz, k, mc) ? 1u : 0u;
        } else {
            for (int r = 0; r < 64; ++r) {
                const int Kr = __shfl(K, r);
                if (Kr < fp.k0) continue; // wave-uniform
                const double rx = __shfl(ux, r), ry = __shfl(uy, r), rz = __shfl(uz, r);
                uint32_t c = 0;
                for (int kb = fp.k0; kb <= Kr; kb += 64) {
                    const int k = kb + (int)lane;
                    const bool hit = k <= Kr && sample_hit(ft, fp, P, rx, ry, rz, k, mc);
                    c += wave_count(hit);
                }
                if ((int)lane == r) hits = c;
            }
        }
        bool end_occ = false, sup = false;
        if (counted) {
            double q0, q1, q2;
            pose_apply(P, b.px, b.py, b.pz, q0, q1, q2);
            const int fx = fine_of(q0, ft), fy = fine_of(q1, ft), fz = fine_of(q2, ft);
            end_occ = (fine_probe(ft, fx >> 2, fy >> 2, fz >> 2) >> fine_bit(fx, fy, fz)) & 1ull;
            sup = end_occ || near_occupied(ft, fx, fy, fz, 1); // the cell or one of its 26 neighbours
        }
        if (hits_out && valid) hits_out[(size_t)(h0 + hl) * n + i] = (uint16_t)min(hits, 65535u);
        const uint32_t c_p = wave_count(hits >= (uint32_t)fp.min_hits), c_e = wave_count(end_occ), c_s = wave_count(sup);
        const uint32_t c_h = wave_sum(hits);
        if (lane == 0) {
            wcnt[hl][wave][0] = c_p;
            wcnt[hl][wave][1] = c_e;
            wcnt[hl][wave][2] = c_s;
            wcnt[hl][wave][3] = c_h;
        }
    }
    __syncthreads();
    if (tid < hn) {
        uint32_t* out = partial + ((size_t)(h0 + tid) * n_chunks + chunk) * kFreeWords;
        out[0] = ((wray[0][0] + wray[1][0]) + wray[2][0]) + wray[3][0];
        out[4] = ((wray[0][1] + wray[1][1]) + wray[2][1]) + wray[3][1];
        out[1] = ((wcnt[tid][0][0] + wcnt[tid][1][0]) + wcnt[tid][2][0]) + wcnt[tid][3][0];
        out[2] = ((wcnt[tid][0][1] + wcnt[tid][1][1]) + wcnt[tid][2][1]) + wcnt[tid][3][1];
        out[3] = ((wcnt[tid][0][2] + wcnt[tid][1][2]) + wcnt[tid][2][2]) + wcnt[tid][3][2];
        out[5] = ((wcnt[tid][0][3] + wcnt[tid][1][3]) + wcnt[tid][2][3]) + wcnt[tid][3][3];
    }
}

// K6b: stats[h] = the chunk partials of pose h, summed in chunk order
__global__ __launch_bounds__(256) void k_free_sum(const uint32_t* __restrict__ partial, uint32_t n_chunks, uint32_t n_poses,
                                                  elm_freespace_stats* __restrict__ stats) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n_poses) return;
    uint32_t a[4];
    uint64_t s[2];
    sum_chunk_partials<kFreeWords, 4>(partial + (size_t)h * n_chunks * kFreeWords, n_chunks, a, s);
    elm_freespace_stats o;
    o.n_counted = a[0]; o.n_pierced = a[1]; o.n_end_occupied = a[2]; o.n_supported = a[3];
    o.n_samples = s[0];
    o.n_hit_samples = s[1];
    stats[h] = o;
}

void launch_free_space(hipStream_t s, int form, const FineTable& ft, const FreeParams& fp, const float* pts, uint32_t n, const double* rows,
                       uint32_t n_poses, uint32_t* partial, elm_freespace_stats* stats, uint16_t* hits) {
    if (!n || !n_poses) return;
    const uint32_t n_chunks = (n + 255u) / 256u;
    const uint32_t n_blk = (n_poses + kFreePoses - 1) / kFreePoses;
    if (form == 0) hipLaunchKernelGGL(k_free_rays<0>, dim3(n_chunks * n_blk), dim3(256), 0, s, ft, fp, pts, n, rows, n_poses, n_chunks, partial, hits);
    else hipLaunchKernelGGL(k_free_rays<1>, dim3(n_chunks * n_blk), dim3(256), 0, s, ft, fp, pts, n, rows, n_poses, n_chunks, partial, hits);
    hipLaunchKernelGGL(k_free_sum, dim3((n_poses + 255) / 256), dim3(256), 0, s, partial, n_chunks, n_poses, stats);
}

} // namespace elm
