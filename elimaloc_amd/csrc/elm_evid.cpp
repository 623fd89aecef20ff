// elm_evid.cpp -- map evidence (include/elimaloc_hip.h, "map evidence"): the evidence object (two device counters
// per occupied fine cell of a map, addressed through a per-slot prefix of the fine table's mask popcounts), the argument checks, the job
// table and the launches of elm_k_evid.hip through the call of many jobs that elm_query.hpp shares with the map growth, and the downloads.
// Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

struct elm_evidence {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (as maps and scans keep it)
    const elm_map* map = nullptr;
    int sub = 0;
    uint32_t n_cells = 0;
    uint32_t* d_base = nullptr;    // [table slots] the first counter of every slot
    uint32_t* d_through = nullptr; // [n_cells] in slot order, within a slot in bit order
    uint32_t* d_hit = nullptr;
    std::vector<int32_t> cells3;   // [n_cells][3] ascending (x, y, z): elm_map_fine_cells' order
    std::vector<uint32_t> perm;    // perm[k] = the counter of the k-th cell of that order
    uint64_t total_beams = 0;      // beams handed to accumulate calls since creation / reset
};

extern "C" void elm_evidence_config_default(elm_evidence_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->sub = 4;
    c->max_steps = 4096;
    c->min_range_m = 1.0;
    c->obs_min_range_m = 2.0;
    c->obs_max_range_m = 50.0;
    c->end_margin_m = 1.0;
    c->end_margin_frac = 0.2;
}

extern "C" void elm_evidence_rule_default(elm_evidence_rule* r) {
    if (!r) return;
    r->min_through = 3;
    r->through_per_hit = 4;
}

namespace {

void evidence_free(elm_evidence* ev) {
    if (!ev) return;
    if (elm_host::ctx_is_alive(ev->ctx, ev->ctx_id)) (void)hipSetDevice(ev->ctx->device); // a context destroyed first: just release
    if (ev->d_base) (void)hipFree(ev->d_base);
    if (ev->d_through) (void)hipFree(ev->d_through);
    if (ev->d_hit) (void)hipFree(ev->d_hit);
    delete ev;
}

int create_impl(elm_ctx* ctx, const elm_map* map, int sub, elm_evidence** out) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(map, sub, &ft, nullptr);
    if (rc != ELM_OK) return rc;
    // the table as the kernels see it: the counters are laid out in its slot order
    const size_t cap = (size_t)ft->mask + 1;
    std::vector<int4> keys(cap);
    std::vector<unsigned long long> masks(cap);
    hipError_t e = hipMemcpy(keys.data(), ft->keys, cap * sizeof(int4), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(masks.data(), ft->masks, cap * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return dev_error(ctx, "elm_evidence_create", e);
    std::vector<uint32_t> base(cap);
    uint64_t total = 0;
    for (size_t h = 0; h < cap; ++h) {
        base[h] = (uint32_t)total;
        if (keys[h].w) total += (uint64_t)__builtin_popcountll(masks[h]);
    }
    if (total > 0xFFFFFFF0ull) {
        elm_host::ctx_set_error(ctx, "elm_evidence_create: too many cells");
        return ELM_ERR_UNSUPPORTED;
    }
    elm_evidence* ev = new elm_evidence();
    ev->ctx = ctx;
    ev->ctx_id = ctx->id;
    ev->map = map;
    ev->sub = sub;
    ev->n_cells = (uint32_t)total;
    // cell -> counter, sorted into elm_map_fine_cells' order
    std::vector<std::array<int32_t, 4>> cells;
    cells.reserve((size_t)total);
    for (size_t h = 0; h < cap; ++h) {
        if (!keys[h].w) continue;
        uint32_t k = base[h];
        for (int bit = 0; bit < 64; ++bit)
            if ((masks[h] >> bit) & 1ull)
                cells.push_back({keys[h].x * 4 + (bit >> 4), keys[h].y * 4 + ((bit >> 2) & 3), keys[h].z * 4 + (bit & 3), (int32_t)k++});
    }
    std::sort(cells.begin(), cells.end(), [](const std::array<int32_t, 4>& a, const std::array<int32_t, 4>& b) {
        return a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : a[2] < b[2]);
    });
    ev->cells3.resize(3 * cells.size());
    ev->perm.resize(cells.size());
    for (size_t k = 0; k < cells.size(); ++k) {
        memcpy(&ev->cells3[3 * k], cells[k].data(), 3 * sizeof(int32_t));
        ev->perm[k] = (uint32_t)cells[k][3];
    }
    const size_t cb = std::max<size_t>((size_t)total * sizeof(uint32_t), 256);
    e = hipMalloc((void**)&ev->d_base, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&ev->d_through, cb);
    if (e == hipSuccess) e = hipMalloc((void**)&ev->d_hit, cb);
    if (e == hipSuccess) e = hipMemcpy(ev->d_base, base.data(), cap * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(ev->d_through, 0, cb);
    if (e == hipSuccess) e = hipMemset(ev->d_hit, 0, cb);
    if (e != hipSuccess) {
        evidence_free(ev);
        return dev_error(ctx, "elm_evidence_create", e);
    }
    *out = ev;
    return ELM_OK;
}

int accumulate_impl(elm_ctx* ctx, elm_evidence* ev, const elm_scan* const* scans, const double* poses16, uint32_t n_jobs,
                    const elm_evidence_config* c, elm_evidence_stats* stats, uint16_t* events) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(ev->map, ev->sub, &ft, nullptr);
    if (rc != ELM_OK) return rc;
    const JobTable jobs = build_jobs(scans, poses16, n_jobs);
    const EvidParams ep = walk_params(*c);
    return run_jobs(
        ctx, jobs, ev->total_beams, "map evidence", "counters", kEvidWords, stats, events,
        [&](hipStream_t st, const EvidJob* d_jobs, uint32_t n_chunks, uint32_t* d_part, elm_evidence_stats* d_stats, uint16_t* d_ev) {
            launch_evid_walk(st, *ft, ep, d_jobs, n_jobs, n_chunks, ev->d_base, ev->d_through, ev->d_hit, d_part, d_stats, d_ev);
        },
        [](hipStream_t) { return hipSuccess; });
}

int accumulate_checked(elm_ctx* ctx, elm_evidence* ev, const elm_scan* const* scans, const double* poses16, int n_jobs,
                       const elm_evidence_config* c, elm_evidence_stats* stats, uint16_t* events, const char* what) {
    int rc = check_accumulate(ctx, ev, scans, poses16, n_jobs, c, walk_config_ok(c), what);
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, what, [&] { return accumulate_impl(ctx, ev, scans, poses16, (uint32_t)n_jobs, c, stats, events); });
}

} // namespace

extern "C" int elm_evidence_create(elm_ctx* ctx, const elm_map* map, int sub, elm_evidence** out) {
    if (!ctx || !map || !out || !sub_ok(sub)) return ELM_ERR_INVALID;
    *out = nullptr;
    int rc = check_plain(ctx, "elm_evidence_create");
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    return guard_alloc(ctx, "elm_evidence_create", [&] { return create_impl(ctx, map, sub, out); });
}

extern "C" void elm_evidence_destroy(elm_evidence* ev) { evidence_free(ev); }

extern "C" int elm_evidence_reset(elm_ctx* ctx, elm_evidence* ev) {
    int rc = check_object(ctx, ev, "elm_evidence_reset");
    if (rc != ELM_OK) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipSuccess;
    if (ev->n_cells) {
        e = hipMemsetAsync(ev->d_through, 0, (size_t)ev->n_cells * sizeof(uint32_t), st);
        if (e == hipSuccess) e = hipMemsetAsync(ev->d_hit, 0, (size_t)ev->n_cells * sizeof(uint32_t), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return dev_error(ctx, "elm_evidence_reset", e);
    ev->total_beams = 0;
    return ELM_OK;
}

extern "C" int elm_evidence_accumulate(elm_ctx* ctx, elm_evidence* ev, const elm_scan* scan, const double T16[16], const elm_evidence_config* cfg,
                                       elm_evidence_stats* stats, uint16_t* events) {
    if (!scan) return ELM_ERR_INVALID;
    return accumulate_checked(ctx, ev, &scan, T16, 1, cfg, stats, events, "elm_evidence_accumulate");
}

extern "C" int elm_evidence_accumulate_batch(elm_ctx* ctx, elm_evidence* ev, const elm_scan* const* scans, const double* poses16, int n_jobs,
                                             const elm_evidence_config* cfg, elm_evidence_stats* stats) {
    return accumulate_checked(ctx, ev, scans, poses16, n_jobs, cfg, stats, nullptr, "elm_evidence_accumulate_batch");
}

namespace {

// the counters in elm_map_fine_cells' order
int download_counts(elm_ctx* ctx, const elm_evidence* ev, std::vector<uint32_t>& through, std::vector<uint32_t>& hit) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const size_t n = ev->n_cells;
    std::vector<uint32_t> t(n), h(n);
    through.resize(n);
    hit.resize(n);
    if (!n) return ELM_OK;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(t.data(), ev->d_through, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), ev->d_hit, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev_error(ctx, "map evidence: download", e);
    for (size_t k = 0; k < n; ++k) {
        through[k] = t[ev->perm[k]];
        hit[k] = h[ev->perm[k]];
    }
    return ELM_OK;
}

} // namespace

extern "C" int elm_evidence_counts(elm_ctx* ctx, const elm_evidence* ev, uint32_t* through, uint32_t* hit, size_t cap, size_t* n) {
    if (!n) return ELM_ERR_INVALID;
    int rc = check_object(ctx, ev, "elm_evidence_counts");
    if (rc != ELM_OK) return rc;
    *n = ev->n_cells;
    const size_t k = std::min<size_t>(cap, ev->n_cells);
    if (!k || (!through && !hit)) return ELM_OK;
    return guard_alloc(ctx, "elm_evidence_counts", [&] {
        std::vector<uint32_t> t, h;
        int rc = download_counts(ctx, ev, t, h);
        if (rc != ELM_OK) return rc;
        if (through) memcpy(through, t.data(), k * sizeof(uint32_t));
        if (hit) memcpy(hit, h.data(), k * sizeof(uint32_t));
        return (int)ELM_OK;
    });
}

extern "C" int elm_evidence_stale_points(elm_ctx* ctx, const elm_evidence* ev, const elm_evidence_rule* rule, uint8_t* flags, size_t cap, size_t* n) {
    if (!n || !rule || (!flags && cap)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, ev, "elm_evidence_stale_points");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_evidence_stale_points", [&] {
        std::vector<int32_t> f;
        int rc = elm_host::map_point_fine_cells(ev->map, ev->sub, f);
        if (rc != ELM_OK) return rc;
        const size_t n_pts = f.size() / 3;
        *n = n_pts;
        const size_t k = std::min(cap, n_pts);
        if (!k) return (int)ELM_OK;
        std::vector<uint32_t> t, h;
        rc = download_counts(ctx, ev, t, h);
        if (rc != ELM_OK) return rc;
        std::vector<uint8_t> stale(ev->n_cells);
        for (size_t q = 0; q < stale.size(); ++q)
            stale[q] = t[q] >= rule->min_through && (uint64_t)t[q] >= (uint64_t)rule->through_per_hit * (uint64_t)h[q];
        const std::array<int32_t, 3>* cells = (const std::array<int32_t, 3>*)ev->cells3.data();
        for (size_t i = 0; i < k; ++i) {
            const std::array<int32_t, 3> c{f[3 * i], f[3 * i + 1], f[3 * i + 2]};
            const std::array<int32_t, 3>* it = std::lower_bound(cells, cells + ev->n_cells, c);
            flags[i] = (it != cells + ev->n_cells && *it == c) ? stale[it - cells] : 0; // (every stored point's cell is in the table)
        }
        return (int)ELM_OK;
    });
}
