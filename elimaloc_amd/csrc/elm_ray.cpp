// elm_ray.cpp -- ray casting (include/elimaloc_hip.h, "ray casting"): the argument checks, the pose rows, the launches
// of elm_k_ray.hip on the map's fine occupancy table (built and cached by elm_map.cpp) and the download, through the call of one scan at
// many poses that elm_query.hpp shares with the free-space check.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

extern "C" void elm_raycast_config_default(elm_raycast_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->sub = 4;
    c->max_steps = 4096;
    c->min_range_m = 1.0;
    c->max_range_m = 100.0;
    c->cmp_min_range_m = 2.0;
    c->cmp_max_range_m = 50.0;
    c->tol_m = 0.5;
    c->tol_frac = 0.02;
}

namespace {

bool config_ok(const elm_raycast_config* c) {
    if (!c || !sub_ok(c->sub) || c->max_steps < 1 || c->max_steps > kRayMaxSteps) return false;
    if (!fin_ge0(c->min_range_m) || !(isfinite(c->max_range_m) && c->max_range_m >= c->min_range_m)) return false;
    if (!fin_ge0(c->cmp_min_range_m) || !(isfinite(c->cmp_max_range_m) && c->cmp_max_range_m >= c->cmp_min_range_m)) return false;
    return fin_ge0(c->tol_m) && fin_ge0(c->tol_frac) && finite3(c->origin);
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int cast_impl(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, uint32_t n_poses, const elm_raycast_config* c,
              elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag) {
    PoseQuery q;
    int rc = open_pose_query(ctx, map, c->sub, scan, q);
    if (rc != ELM_OK) return rc;
    RayParams rp{};
    rp.ox = c->origin[0]; rp.oy = c->origin[1]; rp.oz = c->origin[2];
    rp.t_min = c->min_range_m;
    rp.t_max = c->max_range_m;
    rp.cmp_min_r2 = c->cmp_min_range_m * c->cmp_min_range_m;
    rp.cmp_max_r2 = c->cmp_max_range_m * c->cmp_max_range_m;
    rp.tol_m = c->tol_m;
    rp.tol_frac = c->tol_frac;
    rp.max_steps = c->max_steps;
    // the per-beam arrays share one scratch slot: range_in | range_out | cell | flag, each part present only when asked for
    const size_t beams = (size_t)n_poses * q.n;
    const size_t b_in = range_in ? beams * sizeof(double) : 0, b_out = range_out ? beams * sizeof(double) : 0;
    const size_t b_cell = cell ? beams * 3 * sizeof(int32_t) : 0, b_flag = flag ? beams : 0;
    const size_t o_out = up256(b_in), o_cell = o_out + up256(b_out), o_flag = o_cell + up256(b_cell), arr_bytes = o_flag + up256(b_flag);
    return run_pose_query(
        ctx, q, poses16, n_poses, kRayWords, stats, arr_bytes, "ray cast",
        [&](hipStream_t st, const double* d_rows, uint32_t* d_part, elm_raycast_stats* d_stats, char* d_arr) {
            launch_ray_cast(st, (uint32_t)elm_host::ray_pose_block(kRayPosesDefault), *q.ft, rp, q.d_pts, (uint32_t)q.n, d_rows, n_poses, d_part, d_stats,
                            b_in ? (double*)d_arr : nullptr, b_out ? (double*)(d_arr + o_out) : nullptr, b_cell ? (int32_t*)(d_arr + o_cell) : nullptr,
                            b_flag ? (uint8_t*)(d_arr + o_flag) : nullptr);
        },
        [&](hipStream_t st, const char* d_arr) {
            hipError_t e = hipSuccess;
            if (b_in) e = hipMemcpyAsync(range_in, d_arr, b_in, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && b_out) e = hipMemcpyAsync(range_out, d_arr + o_out, b_out, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && b_cell) e = hipMemcpyAsync(cell, d_arr + o_cell, b_cell, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && b_flag) e = hipMemcpyAsync(flag, d_arr + o_flag, b_flag, hipMemcpyDeviceToHost, st);
            return e;
        });
}

} // namespace

extern "C" int elm_map_raycast(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses, const elm_raycast_config* c,
                               elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag) {
    const char* what = "elm_map_raycast";
    int rc = check_pose_query(ctx, map, scan, poses16, n_poses, config_ok(c), stats, what);
    if (rc != ELM_OK || n_poses == 0) return rc;
    return guard_alloc(ctx, what, [&] { return cast_impl(ctx, map, scan, poses16, (uint32_t)n_poses, c, stats, range_in, range_out, cell, flag); });
}
