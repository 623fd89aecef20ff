// elm_ray.cpp -- ray casting (include/elimaloc_hip.h, "ray casting"): the argument checks, the pose rows, the launches
// of elm_k_ray.hip on the map's fine occupancy table (built and cached by elm_api.cpp) and the download.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "elm_hostapi.hpp"
#include "elm_internal.hpp"

using namespace elm;

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

bool fin_ge0(double v) { return isfinite(v) && v >= 0.0; }

bool config_ok(const elm_raycast_config* c) {
    if (!c || !(c->sub == 1 || c->sub == 2 || c->sub == 4) || c->max_steps < 1 || c->max_steps > kRayMaxSteps) return false;
    if (!fin_ge0(c->min_range_m) || !(isfinite(c->max_range_m) && c->max_range_m >= c->min_range_m)) return false;
    if (!fin_ge0(c->cmp_min_range_m) || !(isfinite(c->cmp_max_range_m) && c->cmp_max_range_m >= c->cmp_min_range_m)) return false;
    if (!fin_ge0(c->tol_m) || !fin_ge0(c->tol_frac)) return false;
    return isfinite(c->origin[0]) && isfinite(c->origin[1]) && isfinite(c->origin[2]);
}

// one rank, no exchange (as the other map queries)
int check_plain(elm_ctx* ctx, const char* what) {
    if ((elm_host::ctx_group(ctx) && !elm_multi::in_worker()) || elm_host::ctx_exchange_attached(ctx)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": one rank only (not on a device group, nor with a communicator or hook attached)");
        return ELM_ERR_UNSUPPORTED;
    }
    return ELM_OK;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int cast_impl(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, uint32_t n_poses, const elm_raycast_config* c,
              elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag) {
    if (hipSetDevice(elm_host::ctx_device(ctx)) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(map, c->sub, &ft, nullptr);
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
    size_t n = 0;
    const float* d_pts = elm_host::scan_dev_points(scan, &n);
    if (n == 0) {
        memset(stats, 0, (size_t)n_poses * sizeof(*stats));
        return ELM_OK;
    }
    std::vector<double> rows((size_t)n_poses * 12);
    for (uint32_t h = 0; h < n_poses; ++h)
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 4; ++q) rows[12 * (size_t)h + r * 4 + q] = poses16[16 * (size_t)h + q * 4 + r];
    const uint32_t n_chunks = (uint32_t)((n + 255) / 256);
    // the per-beam arrays share one scratch slot: range_in | range_out | cell | flag, each part present only when asked for
    const size_t beams = (size_t)n_poses * n;
    const size_t b_in = range_in ? beams * sizeof(double) : 0, b_out = range_out ? beams * sizeof(double) : 0;
    const size_t b_cell = cell ? beams * 3 * sizeof(int32_t) : 0, b_flag = flag ? beams : 0;
    const size_t o_out = up256(b_in), o_cell = o_out + up256(b_out), o_flag = o_cell + up256(b_cell), arr_bytes = o_flag + up256(b_flag);
    double* d_rows = (double*)elm_host::ctx_reloc_scratch(ctx, 1, rows.size() * sizeof(double), &rc);
    uint32_t* d_part = d_rows ? (uint32_t*)elm_host::ctx_reloc_scratch(ctx, 3, (size_t)n_poses * n_chunks * kRayWords * sizeof(uint32_t), &rc) : nullptr;
    elm_raycast_stats* d_stats = d_part ? (elm_raycast_stats*)elm_host::ctx_reloc_scratch(ctx, 4, (size_t)n_poses * sizeof(elm_raycast_stats), &rc) : nullptr;
    char* d_arr = d_stats && arr_bytes ? (char*)elm_host::ctx_reloc_scratch(ctx, 13, arr_bytes, &rc) : nullptr;
    if (!d_stats || (arr_bytes && !d_arr)) return rc;
    double* d_in = b_in ? (double*)d_arr : nullptr;
    double* d_out = b_out ? (double*)(d_arr + o_out) : nullptr;
    int32_t* d_cell = b_cell ? (int32_t*)(d_arr + o_cell) : nullptr;
    uint8_t* d_flag = b_flag ? (uint8_t*)(d_arr + o_flag) : nullptr;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        launch_ray_cast(st, (uint32_t)elm_host::ray_pose_block(kRayPosesDefault), *ft, rp, d_pts, (uint32_t)n, d_rows, n_poses, d_part, d_stats, d_in,
                        d_out, d_cell, d_flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, (size_t)n_poses * sizeof(elm_raycast_stats), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && b_in) e = hipMemcpyAsync(range_in, d_in, b_in, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && b_out) e = hipMemcpyAsync(range_out, d_out, b_out, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && b_cell) e = hipMemcpyAsync(cell, d_cell, b_cell, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && b_flag) e = hipMemcpyAsync(flag, d_flag, b_flag, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        elm_host::ctx_set_error(ctx, std::string("ray cast: ") + hipGetErrorString(e));
        return ELM_ERR_DEVICE;
    }
    return ELM_OK;
}

} // namespace

extern "C" int elm_map_raycast(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses, const elm_raycast_config* c,
                               elm_raycast_stats* stats, double* range_in, double* range_out, int32_t* cell, uint8_t* flag) {
    if (!ctx || !map || !scan || n_poses < 0 || !config_ok(c) || (n_poses > 0 && (!poses16 || !stats))) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, "elm_map_raycast");
    if (rc != ELM_OK) return rc;
    if (elm_host::map_ctx(map) != ctx || elm_host::scan_ctx(scan) != ctx || elm_host::ctx_in_flight(ctx)) return ELM_ERR_INVALID;
    for (int h = 0; h < n_poses; ++h)
        for (int i = 0; i < 16; ++i)
            if (!isfinite(poses16[16 * (size_t)h + i])) return ELM_ERR_INVALID;
    if (n_poses == 0) return ELM_OK;
    try {
        return cast_impl(ctx, map, scan, poses16, (uint32_t)n_poses, c, stats, range_in, range_out, cell, flag);
    } catch (const std::bad_alloc&) {
        elm_host::ctx_set_error(ctx, "elm_map_raycast: host allocation failed");
        return ELM_ERR_ALLOC;
    }
}
