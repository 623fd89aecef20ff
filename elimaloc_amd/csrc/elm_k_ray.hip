// elm_k_ray.hip -- ray casting: the beams of one scan walked cell by cell through the fine occupancy of the map at many poses
// (elm_map_raycast; the contract is in include/elimaloc_hip.h, "ray casting").  Every count is an integer and every
// range one division result, so the answer is the same on every run.
//   K7a k_ray_cast   (beam chunk x pose block) partials: per pose the cast / hit / missed / truncated / compared / matching / through / front
//                    beams and the steps of the chunk, and (optionally) every beam's range_in, range_out, hit cell and flag
//   K7b k_ray_sum    per pose, the chunk partials summed in chunk order
#include <hip/hip_runtime.h>

#include "elm_dev_fine.hpp"
#include "elm_internal.hpp"

namespace elm {

// K7a.  Workgroup = 256 consecutive beams (one per lane, float64 in registers) x pose_block consecutive poses, whose rows are
// workgroup-uniform.  The beam's length, direction, cast / compared state and tolerance do not depend on the pose: they are formed once.
// The walk is CellWalk and the coarse cell's mask MaskCache (elm_dev_fine.hpp); this kernel's own part is the decision at each cell: a
// beam enters its first run of occupied cells (range_in) and leaves it (range_out), or ends by range or by steps.  Per pose each wave
// counts with ballot + popcount (and one shuffle sum for the steps); the four waves meet in LDS and one lane per pose stores the partial.
__global__ __launch_bounds__(256) void k_ray_cast(const FineTable ft, const RayParams rp, const float* __restrict__ pts, uint32_t n,
                                                  const double* __restrict__ rows, uint32_t n_poses, uint32_t n_chunks, uint32_t pose_block,
                                                  uint32_t* __restrict__ partial, double* __restrict__ rin_out, double* __restrict__ rout_out,
                                                  int32_t* __restrict__ cell_out, uint8_t* __restrict__ flag_out) {
    __shared__ uint32_t wcnt[kRayMaxPoses][4][7]; // per pose and wave: hit, miss, truncated, match, through, front, steps
    __shared__ uint32_t wray[4][2];               // per wave: cast, compared beams (the same for every pose)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t chunk = blockIdx.x % n_chunks, h0 = (blockIdx.x / n_chunks) * pose_block;
    const uint32_t i = chunk * 256u + tid;
    const Beam b = load_beam(pts, i, n, rp.ox, rp.oy, rp.oz);
    const bool valid = b.valid, cast = b.cast;
    const bool compared = cast && in_window(b.L2, rp.cmp_min_r2, rp.cmp_max_r2);
    const double L = sqrt(b.L2);
    const double ux = b.dx / L, uy = b.dy / L, uz = b.dz / L;
    const double tol = fmax(rp.tol_m, rp.tol_frac * L);
    {
        const uint32_t c = wave_count(cast), m = wave_count(compared);
        if (lane == 0) {
            wray[wave][0] = c;
            wray[wave][1] = m;
        }
    }
    const uint32_t hn = min(pose_block, n_poses - h0);
    for (uint32_t hl = 0; hl < hn; ++hl) {
        const PoseRows P = load_pose_rows(rows + (size_t)(h0 + hl) * 12);
        uint32_t flag = 0, steps_hit = 0;
        double rin = -1.0, rout = -1.0;
        int hx = 0, hy = 0, hz = 0;
        if (cast) {
            CellWalk w;
            w.start(P, rp.ox, rp.oy, rp.oz, ux, uy, uz, rp.t_min, ft);
            MaskCache mc;
            bool in_run = false;
            for (;;) {
                const bool occ = mc.test(w.c0, w.c1, w.c2, FineProbe{ft});
                if (!in_run) {
                    if (occ) {
                        in_run = true;
                        flag = 1;
                        rin = w.t_in;
                        hx = w.c0; hy = w.c1; hz = w.c2;
                        steps_hit = w.steps;
                    }
                } else if (!occ) {
                    rout = w.t_in;
                    break;
                }
                double t_next;
                const int ax = w.peek(t_next);
                if (t_next > rp.t_max) { // the walk ends by range
                    if (in_run) rout = rp.t_max;
                    else { flag = 2; steps_hit = w.steps; }
                    break;
                }
                if (w.steps >= (uint32_t)rp.max_steps) { // ... by steps
                    if (in_run) rout = w.t_in;
                    else { flag = 3; steps_hit = w.steps; }
                    break;
                }
                w.advance(ax, t_next);
            }
        }
        const bool hit = flag == 1;
        const bool match = compared && hit && rin - tol <= L && L <= rout + tol;
        const bool through = compared && hit && L > rout + tol;
        const bool front = compared && !match && !through;
        if (valid) {
            const size_t o = (size_t)(h0 + hl) * n + i;
            if (rin_out) rin_out[o] = rin;
            if (rout_out) rout_out[o] = rout;
            if (cell_out) {
                cell_out[3 * o] = hx;
                cell_out[3 * o + 1] = hy;
                cell_out[3 * o + 2] = hz;
            }
            if (flag_out) flag_out[o] = (uint8_t)flag;
        }
        const uint32_t c_h = wave_count(hit), c_m = wave_count(flag == 2), c_t = wave_count(flag == 3);
        const uint32_t c_a = wave_count(match), c_p = wave_count(through), c_f = wave_count(front);
        const uint32_t c_s = wave_sum(steps_hit);
        if (lane == 0) {
            uint32_t* wc = wcnt[hl][wave];
            wc[0] = c_h; wc[1] = c_m; wc[2] = c_t; wc[3] = c_a; wc[4] = c_p; wc[5] = c_f; wc[6] = c_s;
        }
    }
    __syncthreads();
    if (tid < hn) {
        uint32_t* out = partial + ((size_t)(h0 + tid) * n_chunks + chunk) * kRayWords;
        out[0] = ((wray[0][0] + wray[1][0]) + wray[2][0]) + wray[3][0];
        out[4] = ((wray[0][1] + wray[1][1]) + wray[2][1]) + wray[3][1];
        out[1] = ((wcnt[tid][0][0] + wcnt[tid][1][0]) + wcnt[tid][2][0]) + wcnt[tid][3][0];
        out[2] = ((wcnt[tid][0][1] + wcnt[tid][1][1]) + wcnt[tid][2][1]) + wcnt[tid][3][1];
        out[3] = ((wcnt[tid][0][2] + wcnt[tid][1][2]) + wcnt[tid][2][2]) + wcnt[tid][3][2];
        out[5] = ((wcnt[tid][0][3] + wcnt[tid][1][3]) + wcnt[tid][2][3]) + wcnt[tid][3][3];
        out[6] = ((wcnt[tid][0][4] + wcnt[tid][1][4]) + wcnt[tid][2][4]) + wcnt[tid][3][4];
        out[7] = ((wcnt[tid][0][5] + wcnt[tid][1][5]) + wcnt[tid][2][5]) + wcnt[tid][3][5];
        out[8] = ((wcnt[tid][0][6] + wcnt[tid][1][6]) + wcnt[tid][2][6]) + wcnt[tid][3][6];
    }
}

// K7b: stats[h] = the chunk partials of pose h, summed in chunk order (the steps in 64 bits)
__global__ __launch_bounds__(256) void k_ray_sum(const uint32_t* __restrict__ partial, uint32_t n_chunks, uint32_t n_poses,
                                                 elm_raycast_stats* __restrict__ stats) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n_poses) return;
    uint32_t a[8];
    uint64_t s;
    sum_chunk_partials<kRayWords, 8>(partial + (size_t)h * n_chunks * kRayWords, n_chunks, a, &s);
    elm_raycast_stats o;
    o.n_cast = a[0]; o.n_hit = a[1]; o.n_miss = a[2]; o.n_truncated = a[3];
    o.n_compared = a[4]; o.n_match = a[5]; o.n_through = a[6]; o.n_front = a[7];
    o.n_steps = s;
    stats[h] = o;
}

void launch_ray_cast(hipStream_t s, uint32_t pose_block, const FineTable& ft, const RayParams& rp, const float* pts, uint32_t n, const double* rows,
                     uint32_t n_poses, uint32_t* partial, elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag) {
    if (!n || !n_poses) return;
    pose_block = pose_block < 1u ? 1u : (pose_block > (uint32_t)kRayMaxPoses ? (uint32_t)kRayMaxPoses : pose_block);
    const uint32_t n_chunks = (n + 255u) / 256u;
    const uint32_t n_blk = (n_poses + pose_block - 1) / pose_block;
    hipLaunchKernelGGL(k_ray_cast, dim3(n_chunks * n_blk), dim3(256), 0, s, ft, rp, pts, n, rows, n_poses, n_chunks, pose_block, partial, range_in,
                       range_out, cell, flag);
    hipLaunchKernelGGL(k_ray_sum, dim3((n_poses + 255) / 256), dim3(256), 0, s, partial, n_chunks, n_poses, stats);
}

} // namespace elm
