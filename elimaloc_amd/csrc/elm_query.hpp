// elm_query.hpp -- the host side that the calls on the context's query scratch share: the free-space check (elm_free.cpp), the ray cast
// (elm_ray.cpp), the map evidence (elm_evid.cpp), the map growth (elm_grow.cpp) and relocalization (elm_reloc.cpp).  On the call skeleton
// of elm_call.hpp (included here): the small argument checks and the scratch taker; the call of one scan at many poses (ray cast,
// free-space check); the call of many (scan, pose) jobs on an object that counts (evidence, growth).  Host-side C++17, everything inline.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "elm_call.hpp"

namespace elm_query {

inline bool sub_ok(int sub) { return sub == 1 || sub == 2 || sub == 4; }
inline bool fin_ge0(double v) { return isfinite(v) && v >= 0.0; }
inline bool finite3(const double v[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
inline bool poses_finite(const double* poses16, size_t n) {
    for (size_t i = 0; i < 16 * n; ++i)
        if (!isfinite(poses16[i])) return false;
    return true;
}
inline bool range_ok(size_t first, size_t count, size_t size) { return first <= size && count <= size - first; }
inline bool finite36(const double* M) {
    for (int q = 0; q < 36; ++q)
        if (!isfinite(M[q])) return false;
    return true;
}
inline bool symmetric36(const double* M) {
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (M[i * 6 + j] != M[j * 6 + i]) return false;
    return true;
}
// one column-major 4 x 4 pose as the kernels read it: (R_r0, R_r1, R_r2, t_r) per row r
inline void pose_rows12(const double* T16, double* out12) {
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 4; ++q) out12[r * 4 + q] = T16[q * 4 + r];
}

// The context's scratch slots (elm_hostapi.hpp), taken one after another: after the first failure take() returns nullptr without asking
// further, and rc holds that failure.
struct QueryScratch {
    elm_ctx* ctx;
    int rc = ELM_OK;
    template <class T>
    T* take(elm_host::ScratchSlot s, size_t count) {
        return rc == ELM_OK ? (T*)elm_host::ctx_reloc_scratch(ctx, s, count * sizeof(T), &rc) : nullptr;
    }
};

// ---- one scan at many poses (ray cast, free-space check)
// The argument checks of the entry point, config_ok being the call's own verdict on its config.  ELM_OK: go on, unless n_poses is 0.
inline int check_pose_query(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses, bool config_ok,
                            const void* stats, const char* what) {
    if (!ctx || !map || !scan || n_poses < 0 || !config_ok || (n_poses > 0 && (!poses16 || !stats))) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || scan->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    return poses_finite(poses16, (size_t)n_poses) ? ELM_OK : ELM_ERR_INVALID;
}

struct PoseQuery {
    const elm::FineTable* ft = nullptr;
    const float* d_pts = nullptr; // the scan's n resident points
    size_t n = 0;
};
// the device made current, the map's fine table for sub and the scan's points
inline int open_pose_query(elm_ctx* ctx, const elm_map* map, int sub, const elm_scan* scan, PoseQuery& q) {
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    int rc = elm_host::map_fine_table(map, sub, &q.ft, nullptr);
    if (rc != ELM_OK) return rc;
    q.d_pts = (const float*)scan->d_pts;
    q.n = scan->n;
    return ELM_OK;
}
// The call itself: the pose rows go up (kScrRows), launch(stream, d_rows, d_part, d_stats, d_arr) queues the kernels on the partials
// (kScrPartials: part_words per pose and 256-beam chunk), the stats (kScrStats) and the per-beam outputs (kScrBeamArrays: arr_bytes, or
// nullptr when none is asked for), the stats come down, download(stream, d_arr) queues the per-beam copies, and the stream is joined.  A
// scan without points: zero stats.
template <class Stats, class Launch, class Download>
int run_pose_query(elm_ctx* ctx, const PoseQuery& q, const double* poses16, uint32_t n_poses, int part_words, Stats* stats, size_t arr_bytes,
                   const char* what, Launch launch, Download download) {
    if (q.n == 0) {
        memset(stats, 0, (size_t)n_poses * sizeof(*stats));
        return ELM_OK;
    }
    std::vector<double> rows((size_t)n_poses * 12);
    for (uint32_t h = 0; h < n_poses; ++h) pose_rows12(poses16 + 16 * (size_t)h, &rows[12 * (size_t)h]);
    const uint32_t n_chunks = (uint32_t)((q.n + 255) / 256);
    QueryScratch scr{ctx};
    double* d_rows = scr.take<double>(elm_host::kScrRows, rows.size());
    uint32_t* d_part = scr.take<uint32_t>(elm_host::kScrPartials, (size_t)n_poses * n_chunks * part_words);
    Stats* d_stats = scr.take<Stats>(elm_host::kScrStats, n_poses);
    char* d_arr = arr_bytes ? scr.take<char>(elm_host::kScrBeamArrays, arr_bytes) : nullptr;
    if (scr.rc != ELM_OK) return scr.rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launched([&] { launch(st, d_rows, d_part, d_stats, d_arr); });
    if (e == hipSuccess) e = hipMemcpyAsync(stats, d_stats, (size_t)n_poses * sizeof(Stats), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = download(st, d_arr);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? ELM_OK : dev_error(ctx, what, e);
}

// ---- many (scan, pose) jobs on an object that counts (evidence, growth).  The object has ctx, ctx_id, sub and total_beams; its config
// has the fields the two public configs share.
// the checks every call on an existing object shares
template <class Obj>
int check_object(elm_ctx* ctx, const Obj* o, const char* what) {
    if (!ctx || !o) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    if (o->ctx != ctx || o->ctx_id != ctx->id || ctx->in_flight) return ELM_ERR_INVALID;
    return ELM_OK;
}

template <class Cfg>
bool walk_config_ok(const Cfg* c) {
    if (!c || !sub_ok(c->sub) || c->max_steps < 1 || c->max_steps > elm::kRayMaxSteps) return false;
    if (!fin_ge0(c->min_range_m) || !fin_ge0(c->obs_min_range_m) || !(isfinite(c->obs_max_range_m) && c->obs_max_range_m >= c->obs_min_range_m)) return false;
    return fin_ge0(c->end_margin_m) && fin_ge0(c->end_margin_frac) && finite3(c->origin);
}

template <class Cfg>
elm::EvidParams walk_params(const Cfg& c) {
    elm::EvidParams ep{};
    ep.ox = c.origin[0]; ep.oy = c.origin[1]; ep.oz = c.origin[2];
    ep.t_min = c.min_range_m;
    ep.obs_min_r2 = c.obs_min_range_m * c.obs_min_range_m;
    ep.obs_max_r2 = c.obs_max_range_m * c.obs_max_range_m;
    ep.margin_m = c.end_margin_m;
    ep.margin_frac = c.end_margin_frac;
    ep.max_steps = c.max_steps;
    return ep;
}

// the argument checks of an accumulate call, config_ok being the call's own verdict on its config
template <class Obj, class Cfg>
int check_accumulate(elm_ctx* ctx, const Obj* o, const elm_scan* const* scans, const double* poses16, int n_jobs, const Cfg* c, bool config_ok,
                     const char* what) {
    if (!ctx || !o || !scans || !poses16 || n_jobs < 1 || n_jobs > elm::kEvidMaxJobs || !config_ok) return ELM_ERR_INVALID;
    int rc = check_object(ctx, o, what);
    if (rc != ELM_OK) return rc;
    if (c->sub != o->sub) return ELM_ERR_INVALID;
    for (int j = 0; j < n_jobs; ++j)
        if (!scans[j] || scans[j]->ctx != ctx) return ELM_ERR_INVALID;
    return poses_finite(poses16, (size_t)n_jobs) ? ELM_OK : ELM_ERR_INVALID;
}

struct JobTable {
    std::vector<elm::EvidJob> jobs; // ascending chunk0
    uint64_t beams = 0, chunks = 0; // of all jobs
};
inline JobTable build_jobs(const elm_scan* const* scans, const double* poses16, uint32_t n_jobs) {
    JobTable t;
    t.jobs.resize(n_jobs);
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const size_t n = scans[j]->n;
        t.jobs[j].pts = (const float*)scans[j]->d_pts;
        t.jobs[j].n = scans[j]->n;
        t.jobs[j].chunk0 = (uint32_t)t.chunks;
        pose_rows12(poses16 + 16 * (size_t)j, t.jobs[j].rows);
        t.beams += n;
        t.chunks += (n + 255) / 256;
    }
    return t;
}

// The call itself, after the guard that no counter can wrap (one beam adds at most 1 to any counter, and the object never takes more
// than 2^32 - 1 beams; `what` and `items` word its refusal).  The job table goes up (kScrRows), launch(stream, d_jobs, n_chunks, d_part,
// d_stats, d_events) queues the kernels on the partials (kScrPartials: part_words per chunk), the stats (kScrStats) and the first job's
// per-beam events (kScrBeamArrays, nullptr when not asked for); the stats come down when asked for, then(stream) queues what else the
// call reads back, the events come down and the stream is joined.
template <class Stats, class Launch, class Then>
int run_jobs(elm_ctx* ctx, const JobTable& t, uint64_t& total_beams, const char* what, const char* items, int part_words, Stats* stats,
             uint16_t* events, Launch launch, Then then) {
    if (total_beams + t.beams > 0xFFFFFFFFull) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": more than 2^32 - 1 beams accumulated; download the " + items + " and reset");
        return ELM_ERR_UNSUPPORTED;
    }
    const size_t n_jobs = t.jobs.size();
    if (stats) memset(stats, 0, n_jobs * sizeof(*stats));
    if (t.chunks == 0) return ELM_OK;
    const size_t n_ev = events ? t.jobs[0].n : 0;
    QueryScratch scr{ctx};
    elm::EvidJob* d_jobs = scr.take<elm::EvidJob>(elm_host::kScrRows, n_jobs);
    uint32_t* d_part = scr.take<uint32_t>(elm_host::kScrPartials, (size_t)t.chunks * part_words);
    Stats* d_stats = scr.take<Stats>(elm_host::kScrStats, n_jobs);
    uint16_t* d_ev = n_ev ? scr.take<uint16_t>(elm_host::kScrBeamArrays, n_ev) : nullptr;
    if (scr.rc != ELM_OK) return scr.rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    hipError_t e = hipMemcpyAsync(d_jobs, t.jobs.data(), n_jobs * sizeof(elm::EvidJob), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launched([&] { launch(st, d_jobs, (uint32_t)t.chunks, d_part, d_stats, d_ev); });
    if (e == hipSuccess) total_beams += t.beams; // the launch is queued: the counters will take these beams
    if (e == hipSuccess && stats) e = hipMemcpyAsync(stats, d_stats, n_jobs * sizeof(Stats), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = then(st);
    if (e == hipSuccess && n_ev) e = hipMemcpyAsync(events, d_ev, n_ev * sizeof(uint16_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st); // the job table on the host is read by the copy until here
    return e == hipSuccess ? ELM_OK : dev_error(ctx, what, e);
}

} // namespace elm_query
