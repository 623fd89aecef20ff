// elm_grow.cpp -- map growth (include/elimaloc_hip.h, "map growth"): the growth object (two open-addressing tables
// on the device that the kernels of elm_k_grow.hip fill: candidate fine cells with their counters, and the coarse cells' masks), the
// capacity guard, the job table and the launches through the call of many jobs that elm_query.hpp shares with the map evidence, the
// downloads and the rule; and the objects of the appeared cells ("map growth: objects"): the union-find state
// that the kernels of elm_k_obj.hip work on, allocated when objects are first asked for, the sorted object list and the two ways back
// from a cell and from a beam to its object.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

struct elm_growth {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (as maps and scans keep it)
    const elm_map* map = nullptr;
    int sub = 0;
    size_t capacity = 0;
    size_t slots = 0;          // a power of two >= 2 * capacity
    GrowTables t{};            // device arrays of `slots` entries each (sums: 3 per slot), and the candidate count
    uint64_t count = 0;        // the candidates, exact after every call
    uint64_t total_beams = 0;  // beams handed to accumulate calls since creation / reset
    // the objects (elm_growth_find_objects): nothing is allocated before the first call
    ObjTables o{};                 // device state: parent / root_id per slot, records / list / rank per candidate
    ObjRecord* o_out = nullptr;    // the listed records side by side, for the download
    size_t o_out_cap = 0;
    bool o_held = false;           // a result is held: from a find until the next accumulate, reset or find
    std::vector<elm_growth_object> objects; // ascending label
    std::vector<int32_t> rank;     // per record: the object's index, or -2 (the host's copy of o.rank)
    elm_growth_object_stats o_stats{};
};

extern "C" void elm_growth_config_default(elm_growth_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->sub = 4;
    c->max_steps = 4096;
    c->min_range_m = 1.0;
    c->obs_min_range_m = 2.0;
    c->obs_max_range_m = 50.0;
    c->end_margin_m = 1.0;
    c->end_margin_frac = 0.2;
    c->clearance_cells = 1;
}

extern "C" void elm_growth_rule_default(elm_growth_rule* r) {
    if (!r) return;
    r->min_hit = 3;
    r->hit_per_through = 4;
}

namespace {

constexpr size_t kGrowMaxCapacity = (size_t)1 << 30;

bool config_ok(const elm_growth_config* c) { return walk_config_ok(c) && c->clearance_cells >= 0 && c->clearance_cells <= 2; }

void growth_free(elm_growth* g) {
    if (!g) return;
    if (elm_host::ctx_is_alive(g->ctx, g->ctx_id)) (void)hipSetDevice(g->ctx->device); // a context destroyed first: just release
    void* arrays[] = {g->t.ckeys, g->t.cmasks, g->t.fkeys, g->t.hit, g->t.through, g->t.sums, g->t.count, g->o.parent, g->o.root_id,
                      g->o.rec, g->o.listed, g->o.rank, g->o.counters, g->o_out};
    for (void* p : arrays)
        if (p) (void)hipFree(p);
    delete g;
}

// every table entry and the candidate count to zero, in stream order
hipError_t clear_tables(const elm_growth* g, hipStream_t st) {
    const size_t s = g->slots;
    hipError_t e = hipMemsetAsync(g->t.ckeys, 0, s * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.cmasks, 0, s * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.fkeys, 0, s * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.hit, 0, s * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.through, 0, s * sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.sums, 0, 3 * s * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(g->t.count, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

int create_impl(elm_ctx* ctx, const elm_map* map, int sub, size_t capacity, elm_growth** out) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(map, sub, &ft, nullptr); // built now when it is not there yet
    if (rc != ELM_OK) return rc;
    elm_growth* g = new elm_growth();
    g->ctx = ctx;
    g->ctx_id = ctx->id;
    g->map = map;
    g->sub = sub;
    g->capacity = capacity;
    g->slots = 2;
    while (g->slots < 2 * capacity) g->slots <<= 1;
    g->t.mask = (uint32_t)(g->slots - 1);
    const size_t s = g->slots;
    hipError_t e = hipMalloc((void**)&g->t.ckeys, s * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.cmasks, s * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.fkeys, s * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.hit, s * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.through, s * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.sums, 3 * s * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&g->t.count, 256);
    if (e == hipSuccess) e = clear_tables(g, (hipStream_t)elm_ctx_stream(ctx));
    if (e != hipSuccess) {
        growth_free(g);
        return dev_error(ctx, "elm_growth_create", e);
    }
    *out = g;
    return ELM_OK;
}

int accumulate_impl(elm_ctx* ctx, elm_growth* g, const elm_scan* const* scans, const double* poses16, uint32_t n_jobs,
                    const elm_growth_config* c, elm_growth_stats* stats, uint16_t* events) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(g->map, g->sub, &ft, nullptr);
    if (rc != ELM_OK) return rc;
    const JobTable jobs = build_jobs(scans, poses16, n_jobs);
    // the table can never fill: one beam makes at most one candidate
    if (g->count + jobs.beams > (uint64_t)g->capacity) {
        elm_host::ctx_set_error(ctx, "map growth: candidates + beams of the call exceed the capacity; download the cells and reset, or create a larger object");
        return ELM_ERR_UNSUPPORTED;
    }
    const EvidParams ep = walk_params(*c);
    GrowTables gt = g->t;
    gt.clearance = c->clearance_cells;
    g->o_held = false; // the counters move: the objects held are those of the table as it was
    uint32_t count = 0;
    rc = run_jobs(
        ctx, jobs, g->total_beams, "map growth", "cells", kGrowWords, stats, events,
        [&](hipStream_t st, const EvidJob* d_jobs, uint32_t n_chunks, uint32_t* d_part, elm_growth_stats* d_stats, uint16_t* d_ev) {
            launch_grow(st, *ft, ep, gt, d_jobs, n_jobs, n_chunks, d_part, d_stats, d_ev);
        },
        // the count comes back with the stats
        [&](hipStream_t st) { return hipMemcpyAsync(&count, g->t.count, sizeof(uint32_t), hipMemcpyDeviceToHost, st); });
    if (rc == ELM_OK && jobs.chunks) g->count = count;
    return rc;
}

int accumulate_checked(elm_ctx* ctx, elm_growth* g, const elm_scan* const* scans, const double* poses16, int n_jobs,
                       const elm_growth_config* c, elm_growth_stats* stats, uint16_t* events, const char* what) {
    int rc = check_accumulate(ctx, g, scans, poses16, n_jobs, c, config_ok(c), what);
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, what, [&] { return accumulate_impl(ctx, g, scans, poses16, (uint32_t)n_jobs, c, stats, events); });
}

// the candidates in ascending (x, y, z) order, which is the ascending order of their keys
struct Cells {
    std::vector<int32_t> cells3;
    std::vector<uint32_t> hit, through;
    std::vector<uint64_t> sums3;
};

int download_cells(elm_ctx* ctx, const elm_growth* g, Cells& out) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    if (!g->count) return ELM_OK;
    const size_t s = g->slots;
    std::vector<unsigned long long> keys(s), sums(3 * s);
    std::vector<uint32_t> hit(s), through(s);
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(keys.data(), g->t.fkeys, s * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hit.data(), g->t.hit, s * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(through.data(), g->t.through, s * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sums.data(), g->t.sums, 3 * s * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev_error(ctx, "map growth: download", e);
    std::vector<uint32_t> order;
    order.reserve((size_t)g->count);
    for (size_t h = 0; h < s; ++h)
        if (keys[h]) order.push_back((uint32_t)h);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    const size_t n = order.size();
    out.cells3.resize(3 * n);
    out.hit.resize(n);
    out.through.resize(n);
    out.sums3.resize(3 * n);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t h = order[k];
        for (int r = 0; r < 3; ++r) {
            out.cells3[3 * k + r] = (int32_t)((keys[h] >> (21 * (2 - r))) & 0x1FFFFFull) - kGrowLim;
            out.sums3[3 * k + r] = sums[3 * (size_t)h + r];
        }
        out.hit[k] = hit[h];
        out.through[k] = through[h];
    }
    return ELM_OK;
}


// ---- objects
void key_to_cell(unsigned long long key, int32_t* c3) {
    for (int r = 0; r < 3; ++r) c3[r] = (int32_t)((key >> (21 * (2 - r))) & 0x1FFFFFull) - kGrowLim;
}

// the per-slot state once, the per-candidate state for at least `count` records (grown, never shrunk)
hipError_t obj_reserve(elm_growth* g) {
    hipError_t e = hipSuccess;
    if (!g->o.parent) {
        e = hipMalloc((void**)&g->o.parent, g->slots * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&g->o.root_id, g->slots * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&g->o.counters, 256);
    }
    const size_t want = std::max<size_t>((size_t)g->count, 1);
    if (e == hipSuccess && g->o.rec_cap < want) {
        void* old[] = {g->o.rec, g->o.listed, g->o.rank};
        for (void* p : old)
            if (p) (void)hipFree(p);
        g->o.rec = nullptr; g->o.listed = nullptr; g->o.rank = nullptr;
        g->o.rec_cap = 0;
        e = hipMalloc((void**)&g->o.rec, want * sizeof(ObjRecord));
        if (e == hipSuccess) e = hipMalloc((void**)&g->o.listed, want * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&g->o.rank, want * sizeof(int32_t));
        if (e == hipSuccess) g->o.rec_cap = (uint32_t)want;
    }
    return e;
}

int find_objects_impl(elm_ctx* ctx, elm_growth* g, const elm_growth_object_rule* rule, elm_growth_object_stats* stats) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const char* what = "elm_growth_find_objects";
    g->o_held = false;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = obj_reserve(g);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    uint32_t cnt[kObjCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemsetAsync(g->o.counters, 0, kObjCounters * sizeof(uint32_t), st);
    if (e == hipSuccess)
        e = launched([&] { launch_obj_find(st, g->t, g->o, rule->min_hit, rule->hit_per_through, rule->connectivity, rule->min_cells, (uint32_t)g->count); });
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, g->o.counters, sizeof(cnt), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    const uint32_t n_roots = cnt[1], n_listed = cnt[2];
    if (cnt[6] || n_roots > g->count || n_listed > n_roots) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": more components than candidate cells (the object's count is stale after a failed call; reset it)");
        return ELM_ERR_DEVICE;
    }
    // the listed records come down, are sorted by label, and every record's rank goes up for the beam call
    if (g->o_out_cap < n_listed) {
        if (g->o_out) (void)hipFree(g->o_out);
        g->o_out = nullptr;
        g->o_out_cap = 0;
        e = hipMalloc((void**)&g->o_out, (size_t)n_listed * sizeof(ObjRecord));
        if (e != hipSuccess) return dev_error(ctx, what, e);
        g->o_out_cap = n_listed;
    }
    std::vector<ObjRecord> rec(n_listed);
    std::vector<uint32_t> listed(n_listed);
    if (n_listed) {
        e = launched([&] { launch_obj_gather(st, g->o, n_listed, g->o_out); });
        if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), g->o_out, (size_t)n_listed * sizeof(ObjRecord), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(listed.data(), g->o.listed, (size_t)n_listed * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return dev_error(ctx, what, e);
    }
    std::vector<uint32_t> order(n_listed);
    for (uint32_t j = 0; j < n_listed; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rec[a].label < rec[b].label; });
    g->objects.assign(n_listed, elm_growth_object{});
    g->rank.assign(n_roots, -2);
    for (uint32_t k = 0; k < n_listed; ++k) {
        const ObjRecord& r = rec[order[k]];
        elm_growth_object& ob = g->objects[k];
        key_to_cell(r.label, ob.label);
        ob.n_cells = r.n_cells;
        for (int q = 0; q < 3; ++q) {
            ob.lo[q] = r.lo[q];
            ob.hi[q] = r.hi[q];
            ob.cell_sum[q] = r.cell_sum[q];
        }
        ob.hit = r.hit;
        ob.through = r.through;
        if (listed[order[k]] >= n_roots) return dev_error(ctx, what, hipErrorUnknown);
        g->rank[listed[order[k]]] = (int32_t)k;
    }
    if (n_roots) {
        e = hipMemcpyAsync(g->o.rank, g->rank.data(), (size_t)n_roots * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return dev_error(ctx, what, e);
    }
    elm_growth_object_stats s{};
    s.n_members = cnt[0];
    s.n_objects = n_listed;
    s.n_small = cnt[3];
    s.n_small_cells = cnt[4];
    s.max_cells = cnt[5];
    g->o_stats = s;
    g->o_held = true;
    if (stats) *stats = s;
    return ELM_OK;
}

// a read call on the objects: the object checks, and a result must be held
int check_objects_held(elm_ctx* ctx, const elm_growth* g, const char* what) {
    int rc = check_object(ctx, g, what);
    if (rc != ELM_OK) return rc;
    if (!g->o_held) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": no objects are held (elm_growth_find_objects first; an accumulate or reset drops them)");
        return ELM_ERR_INVALID;
    }
    return ELM_OK;
}

// one value per candidate cell in elm_growth_cells' order
int cell_objects_impl(elm_ctx* ctx, const elm_growth* g, std::vector<int32_t>& out) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    if (!g->count) return ELM_OK;
    const size_t s = g->slots;
    std::vector<unsigned long long> keys(s);
    std::vector<uint32_t> parent(s), root_id(s);
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(keys.data(), g->t.fkeys, s * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(parent.data(), g->o.parent, s * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(root_id.data(), g->o.root_id, s * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dev_error(ctx, "map growth: objects: download", e);
    std::vector<uint32_t> order;
    order.reserve((size_t)g->count);
    for (size_t h = 0; h < s; ++h)
        if (keys[h]) order.push_back((uint32_t)h);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    out.resize(order.size());
    for (size_t k = 0; k < order.size(); ++k) {
        const uint32_t root = parent[order[k]];
        int32_t v = -1;
        if (root != kObjNone) {
            const uint32_t id = root < s ? root_id[root] : 0xFFFFFFFFu;
            if (id >= g->rank.size()) return dev_error(ctx, "map growth: objects: download", hipErrorUnknown);
            v = g->rank[id];
        }
        out[k] = v;
    }
    return ELM_OK;
}

int beam_objects_impl(elm_ctx* ctx, const elm_growth* g, const elm_scan* scan, const double T16[16], const elm_growth_config* c, int32_t* obj) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const char* what = "elm_growth_beam_objects";
    const FineTable* ft = nullptr;
    int rc = elm_host::map_fine_table(g->map, g->sub, &ft, nullptr);
    if (rc != ELM_OK) return rc;
    EvidJob job{};
    const size_t n = scan->n;
    job.pts = (const float*)scan->d_pts;
    job.n = scan->n;
    pose_rows12(T16, job.rows);
    if (!n) return ELM_OK;
    QueryScratch scr{ctx};
    int32_t* d_out = scr.take<int32_t>(elm_host::kScrBeamArrays, n);
    if (scr.rc != ELM_OK) return scr.rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = launched([&] { launch_obj_beams(st, *ft, walk_params(*c), g->t, g->o, job, d_out); });
    if (e == hipSuccess) e = hipMemcpyAsync(obj, d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? ELM_OK : dev_error(ctx, what, e);
}

} // namespace

extern "C" int elm_growth_create(elm_ctx* ctx, const elm_map* map, int sub, size_t capacity, elm_growth** out) {
    if (!ctx || !map || !out || !sub_ok(sub) || capacity < 1 || capacity > kGrowMaxCapacity) return ELM_ERR_INVALID;
    *out = nullptr;
    int rc = check_plain(ctx, "elm_growth_create");
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    return guard_alloc(ctx, "elm_growth_create", [&] { return create_impl(ctx, map, sub, capacity, out); });
}

extern "C" void elm_growth_destroy(elm_growth* g) { growth_free(g); }

extern "C" int elm_growth_reset(elm_ctx* ctx, elm_growth* g) {
    int rc = check_object(ctx, g, "elm_growth_reset");
    if (rc != ELM_OK) return rc;
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const hipError_t e = clear_tables(g, (hipStream_t)elm_ctx_stream(ctx));
    if (e != hipSuccess) return dev_error(ctx, "elm_growth_reset", e);
    g->count = 0;
    g->total_beams = 0;
    g->o_held = false;
    return ELM_OK;
}

extern "C" int elm_growth_accumulate(elm_ctx* ctx, elm_growth* g, const elm_scan* scan, const double T16[16], const elm_growth_config* cfg,
                                     elm_growth_stats* stats, uint16_t* events) {
    if (!scan) return ELM_ERR_INVALID;
    return accumulate_checked(ctx, g, &scan, T16, 1, cfg, stats, events, "elm_growth_accumulate");
}

extern "C" int elm_growth_accumulate_batch(elm_ctx* ctx, elm_growth* g, const elm_scan* const* scans, const double* poses16, int n_jobs,
                                           const elm_growth_config* cfg, elm_growth_stats* stats) {
    return accumulate_checked(ctx, g, scans, poses16, n_jobs, cfg, stats, nullptr, "elm_growth_accumulate_batch");
}

extern "C" int elm_growth_cells(elm_ctx* ctx, const elm_growth* g, int32_t* cells3, uint32_t* hit, uint32_t* through, uint64_t* sums3, size_t cap,
                                size_t* n) {
    if (!n) return ELM_ERR_INVALID;
    int rc = check_object(ctx, g, "elm_growth_cells");
    if (rc != ELM_OK) return rc;
    *n = (size_t)g->count;
    const size_t k = std::min<size_t>(cap, (size_t)g->count);
    if (!k || (!cells3 && !hit && !through && !sums3)) return ELM_OK;
    return guard_alloc(ctx, "elm_growth_cells", [&] {
        Cells c;
        int rc = download_cells(ctx, g, c);
        if (rc != ELM_OK) return rc;
        if (cells3) memcpy(cells3, c.cells3.data(), 3 * k * sizeof(int32_t));
        if (hit) memcpy(hit, c.hit.data(), k * sizeof(uint32_t));
        if (through) memcpy(through, c.through.data(), k * sizeof(uint32_t));
        if (sums3) memcpy(sums3, c.sums3.data(), 3 * k * sizeof(uint64_t));
        return (int)ELM_OK;
    });
}

extern "C" int elm_growth_appeared_points(elm_ctx* ctx, const elm_growth* g, const elm_growth_rule* rule, double* xyz64, size_t cap, size_t* n) {
    if (!n || !rule || (!xyz64 && cap)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, g, "elm_growth_appeared_points");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_growth_appeared_points", [&] {
        const FineTable* ft = nullptr;
        int rc = elm_host::map_fine_table(g->map, g->sub, &ft, nullptr);
        if (rc != ELM_OK) return rc;
        const double cell = ft->cell;
        Cells c;
        rc = download_cells(ctx, g, c);
        if (rc != ELM_OK) return rc;
        size_t m = 0;
        for (size_t k = 0; k < c.hit.size(); ++k) {
            const uint32_t h = c.hit[k], t = c.through[k];
            if (!(h >= rule->min_hit && (uint64_t)h >= (uint64_t)rule->hit_per_through * (uint64_t)t)) continue;
            if (m < cap)
                for (int r = 0; r < 3; ++r)
                    xyz64[3 * m + r] = ((double)c.cells3[3 * k + r] + ((double)c.sums3[3 * k + r] / (double)h + 0.5) / 65536.0) * cell;
            ++m;
        }
        *n = m;
        return (int)ELM_OK;
    });
}

extern "C" void elm_growth_object_rule_default(elm_growth_object_rule* r) {
    if (!r) return;
    r->min_hit = 3;
    r->hit_per_through = 4;
    r->connectivity = 26;
    r->min_cells = 1;
}

extern "C" int elm_growth_find_objects(elm_ctx* ctx, elm_growth* g, const elm_growth_object_rule* rule, elm_growth_object_stats* stats) {
    if (!rule || (rule->connectivity != 6 && rule->connectivity != 18 && rule->connectivity != 26) || rule->min_cells < 1) return ELM_ERR_INVALID;
    int rc = check_object(ctx, g, "elm_growth_find_objects");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_growth_find_objects", [&] { return find_objects_impl(ctx, g, rule, stats); });
}

extern "C" int elm_growth_objects(elm_ctx* ctx, const elm_growth* g, elm_growth_object* objs, size_t cap, size_t* n) {
    if (!n || (!objs && cap)) return ELM_ERR_INVALID;
    int rc = check_objects_held(ctx, g, "elm_growth_objects");
    if (rc != ELM_OK) return rc;
    *n = g->objects.size();
    const size_t k = std::min(cap, g->objects.size());
    if (k) memcpy(objs, g->objects.data(), k * sizeof(elm_growth_object));
    return ELM_OK;
}

extern "C" int elm_growth_cell_objects(elm_ctx* ctx, const elm_growth* g, int32_t* obj, size_t cap, size_t* n) {
    if (!n || (!obj && cap)) return ELM_ERR_INVALID;
    int rc = check_objects_held(ctx, g, "elm_growth_cell_objects");
    if (rc != ELM_OK) return rc;
    *n = (size_t)g->count;
    const size_t k = std::min<size_t>(cap, (size_t)g->count);
    if (!k) return ELM_OK;
    return guard_alloc(ctx, "elm_growth_cell_objects", [&] {
        std::vector<int32_t> v;
        int rc = cell_objects_impl(ctx, g, v);
        if (rc != ELM_OK) return rc;
        memcpy(obj, v.data(), std::min(k, v.size()) * sizeof(int32_t));
        return (int)ELM_OK;
    });
}

extern "C" int elm_growth_beam_objects(elm_ctx* ctx, const elm_growth* g, const elm_scan* scan, const double T16[16], const elm_growth_config* cfg,
                                       int32_t* obj) {
    if (!scan || !obj) return ELM_ERR_INVALID;
    int rc = check_accumulate(ctx, g, &scan, T16, 1, cfg, config_ok(cfg), "elm_growth_beam_objects");
    if (rc != ELM_OK) return rc;
    rc = check_objects_held(ctx, g, "elm_growth_beam_objects");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_growth_beam_objects", [&] { return beam_objects_impl(ctx, g, scan, T16, cfg, obj); });
}
