// elm_free.cpp -- free-space check (include/elimaloc_hip.h, "free-space check"): the argument checks, the fine
// occupancy table of the map (built and cached by elm_api.cpp), the launches of elm_k_free.hip and the download.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "elm_hostapi.hpp"
#include "elm_internal.hpp"

using namespace elm;

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

bool sub_ok(int sub) { return sub == 1 || sub == 2 || sub == 4; }

bool config_ok(const elm_freespace_config* c) {
    if (!c || !sub_ok(c->sub) || c->min_hits < 1 || c->max_samples < 1 || c->max_samples > 65536) return false;
    if (!(isfinite(c->step_m) && c->step_m >= 0.0) || !(isfinite(c->start_m) && c->start_m >= 0.0)) return false;
    if (!(isfinite(c->min_range_m) && c->min_range_m >= 0.0) || !(isfinite(c->max_range_m) && c->max_range_m >= c->min_range_m)) return false;
    if (!(isfinite(c->end_margin_m) && c->end_margin_m >= 0.0) || !(isfinite(c->end_margin_frac) && c->end_margin_frac >= 0.0)) return false;
    return isfinite(c->origin[0]) && isfinite(c->origin[1]) && isfinite(c->origin[2]);
}

// one rank, no exchange (as the relocalization calls)
int check_plain(elm_ctx* ctx, const char* what) {
    if ((elm_host::ctx_group(ctx) && !elm_multi::in_worker()) || elm_host::ctx_exchange_attached(ctx)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": one rank only (not on a device group, nor with a communicator or hook attached)");
        return ELM_ERR_UNSUPPORTED;
    }
    return ELM_OK;
}

int check_impl(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, uint32_t n_poses, const elm_freespace_config* c,
               elm_freespace_stats* stats, uint16_t* hits) {
    if (hipSetDevice(elm_host::ctx_device(ctx)) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(map, c->sub, &ft, nullptr);
    if (rc != ELM_OK) return rc;
    FreeParams fp{};
    fp.ox = c->origin[0]; fp.oy = c->origin[1]; fp.oz = c->origin[2];
    fp.step = c->step_m > 0.0 ? c->step_m : ft->cell / 2.0;
    fp.min_r2 = c->min_range_m * c->min_range_m;
    fp.max_r2 = c->max_range_m * c->max_range_m;
    fp.margin_m = c->end_margin_m;
    fp.margin_frac = c->end_margin_frac;
    const double k0 = floor(c->start_m / fp.step) + 1.0;
    fp.k0 = (int32_t)std::min(k0, 1073741824.0); // beyond every K (<= 65536): no samples
    fp.max_samples = c->max_samples;
    fp.min_hits = c->min_hits;
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
    const size_t hits_bytes = hits ? (size_t)n_poses * n * sizeof(uint16_t) : 0;
    double* d_rows = (double*)elm_host::ctx_reloc_scratch(ctx, 1, rows.size() * sizeof(double), &rc);
    uint32_t* d_part = d_rows ? (uint32_t*)elm_host::ctx_reloc_scratch(ctx, 3, (size_t)n_poses * n_chunks * kFreeWords * sizeof(uint32_t), &rc) : nullptr;
    elm_freespace_stats* d_stats = d_part ? (elm_freespace_stats*)elm_host::ctx_reloc_scratch(ctx, 4, (size_t)n_poses * sizeof(elm_freespace_stats), &rc) : nullptr;
    uint16_t* d_hits = d_stats && hits ? (uint16_t*)elm_host::ctx_reloc_scratch(ctx, 13, hits_bytes, &rc) : nullptr;
    if (!d_stats || (hits && !d_hits)) return rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        launch_free_space(st, elm_host::free_space_form(), *ft, fp, d_pts, (uint32_t)n, d_rows, n_poses, d_part, d_stats, d_hits);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, (size_t)n_poses * sizeof(elm_freespace_stats), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && hits) e = hipMemcpyAsync(hits, d_hits, hits_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        elm_host::ctx_set_error(ctx, std::string("free-space check: ") + hipGetErrorString(e));
        return ELM_ERR_DEVICE;
    }
    return ELM_OK;
}

} // namespace

extern "C" int elm_map_fine_cells(elm_ctx* ctx, const elm_map* map, int sub, int32_t* cells3, size_t cap, size_t* n) {
    if (!ctx || !map || !sub_ok(sub) || !n || (cap && !cells3)) return ELM_ERR_INVALID;
    if (elm_host::map_ctx(map) != ctx) return ELM_ERR_INVALID;
    try {
        if (hipSetDevice(elm_host::ctx_device(ctx)) != hipSuccess) return ELM_ERR_DEVICE;
        std::vector<int32_t> cells;
        int rc = elm_host::map_fine_cells(map, sub, cells);
        if (rc != ELM_OK) return rc;
        *n = cells.size() / 3;
        const size_t k = std::min(cap, *n);
        if (k) memcpy(cells3, cells.data(), k * 3 * sizeof(int32_t));
        return ELM_OK;
    } catch (const std::bad_alloc&) {
        elm_host::ctx_set_error(ctx, "elm_map_fine_cells: host allocation failed");
        return ELM_ERR_ALLOC;
    }
}

extern "C" int elm_map_check_free_space(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                                        const elm_freespace_config* c, elm_freespace_stats* stats, uint16_t* hits) {
    if (!ctx || !map || !scan || n_poses < 0 || !config_ok(c) || (n_poses > 0 && (!poses16 || !stats))) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, "elm_map_check_free_space");
    if (rc != ELM_OK) return rc;
    if (elm_host::map_ctx(map) != ctx || elm_host::scan_ctx(scan) != ctx || elm_host::ctx_in_flight(ctx)) return ELM_ERR_INVALID;
    for (int h = 0; h < n_poses; ++h)
        for (int i = 0; i < 16; ++i)
            if (!isfinite(poses16[16 * (size_t)h + i])) return ELM_ERR_INVALID;
    if (n_poses == 0) return ELM_OK;
    try {
        return check_impl(ctx, map, scan, poses16, (uint32_t)n_poses, c, stats, hits);
    } catch (const std::bad_alloc&) {
        elm_host::ctx_set_error(ctx, "elm_map_check_free_space: host allocation failed");
        return ELM_ERR_ALLOC;
    }
}
