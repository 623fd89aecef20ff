// elm_free.cpp -- free-space check (include/elimaloc_hip.h, "free-space check"): the argument checks, the fine
// occupancy table of the map (built and cached by elm_map.cpp), the launches of elm_k_free.hip and the download, through the call of one
// scan at many poses that elm_query.hpp shares with the ray cast.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

extern "C" void elm_freespace_config_default(elm_freespace_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->sub = 4;
    c->min_hits = 2;
    c->max_samples = 1024;
    c->step_m = 0.0; // cell / 2 of the map the call is made on
    c->start_m = 1.0;
    c->min_range_m = 2.0;
    c->max_range_m = 50.0;
    c->end_margin_m = 1.0;
    c->end_margin_frac = 0.2;
}

namespace {

bool config_ok(const elm_freespace_config* c) {
    if (!c || !sub_ok(c->sub) || c->min_hits < 1 || c->max_samples < 1 || c->max_samples > 65536) return false;
    if (!fin_ge0(c->step_m) || !fin_ge0(c->start_m)) return false;
    if (!fin_ge0(c->min_range_m) || !(isfinite(c->max_range_m) && c->max_range_m >= c->min_range_m)) return false;
    return fin_ge0(c->end_margin_m) && fin_ge0(c->end_margin_frac) && finite3(c->origin);
}

int check_impl(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, uint32_t n_poses, const elm_freespace_config* c,
               elm_freespace_stats* stats, uint16_t* hits) {
    PoseQuery q;
    int rc = open_pose_query(ctx, map, c->sub, scan, q);
    if (rc != ELM_OK) return rc;
    FreeParams fp{};
    fp.ox = c->origin[0]; fp.oy = c->origin[1]; fp.oz = c->origin[2];
    fp.step = c->step_m > 0.0 ? c->step_m : q.ft->cell / 2.0;
    fp.min_r2 = c->min_range_m * c->min_range_m;
    fp.max_r2 = c->max_range_m * c->max_range_m;
    fp.margin_m = c->end_margin_m;
    fp.margin_frac = c->end_margin_frac;
    const double k0 = floor(c->start_m / fp.step) + 1.0;
    fp.k0 = (int32_t)std::min(k0, 1073741824.0); // beyond every K (<= 65536): no samples
    fp.max_samples = c->max_samples;
    fp.min_hits = c->min_hits;
    const size_t hits_bytes = hits ? (size_t)n_poses * q.n * sizeof(uint16_t) : 0;
    return run_pose_query(
        ctx, q, poses16, n_poses, kFreeWords, stats, hits_bytes, "free-space check",
        [&](hipStream_t st, const double* d_rows, uint32_t* d_part, elm_freespace_stats* d_stats, char* d_hits) {
            launch_free_space(st, elm_host::free_space_form(), *q.ft, fp, q.d_pts, (uint32_t)q.n, d_rows, n_poses, d_part, d_stats, (uint16_t*)d_hits);
        },
        [&](hipStream_t st, const char* d_hits) { return hits ? hipMemcpyAsync(hits, d_hits, hits_bytes, hipMemcpyDeviceToHost, st) : hipSuccess; });
}

} // namespace

extern "C" int elm_map_fine_cells(elm_ctx* ctx, const elm_map* map, int sub, int32_t* cells3, size_t cap, size_t* n) {
    if (!ctx || !map || !sub_ok(sub) || !n || (cap && !cells3)) return ELM_ERR_INVALID;
    if (map->ctx != ctx) return ELM_ERR_INVALID;
    return guard_alloc(ctx, "elm_map_fine_cells", [&] {
        if (hipSetDevice(ctx->device) != hipSuccess) return (int)ELM_ERR_DEVICE;
        std::vector<int32_t> cells;
        int rc = elm_host::map_fine_cells(map, sub, cells);
        if (rc != ELM_OK) return rc;
        *n = cells.size() / 3;
        const size_t k = std::min(cap, *n);
        if (k) memcpy(cells3, cells.data(), k * 3 * sizeof(int32_t));
        return (int)ELM_OK;
    });
}

extern "C" int elm_map_check_free_space(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                                        const elm_freespace_config* c, elm_freespace_stats* stats, uint16_t* hits) {
    const char* what = "elm_map_check_free_space";
    int rc = check_pose_query(ctx, map, scan, poses16, n_poses, config_ok(c), stats, what);
    if (rc != ELM_OK || n_poses == 0) return rc;
    return guard_alloc(ctx, what, [&] { return check_impl(ctx, map, scan, poses16, (uint32_t)n_poses, c, stats, hits); });
}
