// elm_place.cpp -- place recognition (include/elimaloc_hip.h, "place recognition"): the descriptor tables, the places
// object (a database of descriptors, their popcounts and ids resident on the device, of a capacity fixed at creation), the argument
// checks, and the launches of elm_k_place.hip on the job table and the scratch taker that elm_query.hpp shares with the map queries,
// every entry point with device work inside elm_call.hpp's on_stream.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

struct elm_places {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (as maps and scans keep it)
    elm_places_config cfg{};
    uint32_t W = 0, capacity = 0, size = 0;
    double* d_tables = nullptr;            // ring_edge2, z_edge, dir
    unsigned long long* d_words = nullptr; // [capacity][W]
    uint32_t* d_bits = nullptr;            // [capacity]
    long long* d_ids = nullptr;            // [capacity]
    std::vector<int64_t> ids;              // [size]: the host's copy
};

extern "C" void elm_places_config_default(elm_places_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->n_rings = 16;
    c->n_layers = 8;
    c->r_min_m = 2.0;
    c->r_max_m = 42.0;
    c->z_min_m = -3.0;
    c->z_max_m = 9.0;
}

namespace {

constexpr int kPlaceMaxCapacity = 65536;

bool ascending(const std::vector<double>& t) {
    for (size_t i = 0; i < t.size(); ++i)
        if (!isfinite(t[i]) || (i && !(t[i] > t[i - 1]))) return false;
    return true;
}

// the three tables of the contract; false: a bad config or a table that is not finite and strictly increasing
bool place_tables(const elm_places_config* c, std::vector<double>& re, std::vector<double>& ze, std::vector<double>& dir) {
    if (!c || c->n_rings < 1 || c->n_rings > 32 || c->n_layers < 1 || c->n_layers > 16) return false;
    if (!isfinite(c->r_min_m) || !isfinite(c->r_max_m) || !isfinite(c->z_min_m) || !isfinite(c->z_max_m)) return false;
    const int nr = c->n_rings, nl = c->n_layers;
    re.resize(nr + 1);
    ze.resize(nl + 1);
    for (int i = 0; i <= nr; ++i) {
        const double e = i == nr ? c->r_max_m : c->r_min_m + ((c->r_max_m - c->r_min_m) * (double)i) / (double)nr;
        re[i] = e * e;
    }
    for (int j = 0; j <= nl; ++j) ze[j] = j == nl ? c->z_max_m : c->z_min_m + ((c->z_max_m - c->z_min_m) * (double)j) / (double)nl;
    if (c->r_min_m < 0.0 || !ascending(re) || !ascending(ze)) return false;
    dir.assign(2 * kPlaceSectors, 0.0);
    dir[0] = 1.0;
    for (int k = 1; k < 8; ++k) {
        const double a = (2.0 * M_PI * (double)k) / 64.0;
        dir[2 * k] = cos(a);
        dir[2 * k + 1] = sin(a);
    }
    dir[16] = dir[17] = cos(M_PI / 4.0);
    for (int k = 0; k < 8; ++k) { // about the diagonal
        dir[2 * (16 - k)] = dir[2 * k + 1];
        dir[2 * (16 - k) + 1] = dir[2 * k];
    }
    for (int k = 17; k < kPlaceSectors; ++k) { // a quarter turn of dir[k - 16]; a zero is stored as +0.0
        dir[2 * k] = -dir[2 * (k - 16) + 1] + 0.0;
        dir[2 * k + 1] = dir[2 * (k - 16)] + 0.0;
    }
    return true;
}

void places_free(elm_places* pl) {
    if (!pl) return;
    if (elm_host::ctx_is_alive(pl->ctx, pl->ctx_id)) (void)hipSetDevice(pl->ctx->device); // a context destroyed first: just release
    if (pl->d_tables) (void)hipFree(pl->d_tables);
    if (pl->d_words) (void)hipFree(pl->d_words);
    if (pl->d_bits) (void)hipFree(pl->d_bits);
    if (pl->d_ids) (void)hipFree(pl->d_ids);
    delete pl;
}

int create_impl(elm_ctx* ctx, const elm_places_config* cfg, uint32_t capacity, const std::vector<double>& re, const std::vector<double>& ze,
                const std::vector<double>& dir, elm_places** out) {
    elm_places* pl = new elm_places();
    pl->ctx = ctx;
    pl->ctx_id = ctx->id;
    pl->cfg = *cfg;
    pl->W = (uint32_t)(cfg->n_rings * cfg->n_layers);
    pl->capacity = capacity;
    pl->ids.reserve(capacity);
    std::vector<double> tab(re);
    tab.insert(tab.end(), ze.begin(), ze.end());
    tab.insert(tab.end(), dir.begin(), dir.end());
    hipError_t e = hipMalloc((void**)&pl->d_tables, tab.size() * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->d_words, (size_t)capacity * pl->W * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->d_bits, std::max<size_t>((size_t)capacity * sizeof(uint32_t), 256));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->d_ids, std::max<size_t>((size_t)capacity * sizeof(long long), 256));
    if (e == hipSuccess) e = hipMemcpy(pl->d_tables, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        places_free(pl);
        return dev_error(ctx, "elm_places_create", e);
    }
    *out = pl;
    return ELM_OK;
}

bool query_configs_ok(const elm_places_query_config* q, int n) {
    if (!q) return false;
    for (int i = 0; i < n; ++i)
        if (q[i].top_k < 1 || q[i].top_k > kPlaceMaxTopK) return false;
    return true;
}

// the checks of a call that takes jobs, before anything is dereferenced but the caller's arrays, then the object's and the scans'
int check_jobs(elm_ctx* ctx, const elm_places* pl, const elm_scan* const* scans, const double* levels16, int n_jobs, bool rest_ok, const char* what) {
    if (!ctx || !pl || !scans || n_jobs < 1 || n_jobs > kEvidMaxJobs || !rest_ok) return ELM_ERR_INVALID;
    if (levels16 && !poses_finite(levels16, (size_t)n_jobs)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pl, what);
    if (rc != ELM_OK) return rc;
    for (int j = 0; j < n_jobs; ++j)
        if (!scans[j] || scans[j]->ctx != ctx) return ELM_ERR_INVALID;
    return ELM_OK;
}

JobTable level_jobs(const elm_scan* const* scans, const double* levels16, uint32_t n_jobs) {
    if (levels16) return build_jobs(scans, levels16, n_jobs);
    std::vector<double> eye((size_t)16 * n_jobs, 0.0);
    for (uint32_t j = 0; j < n_jobs; ++j) eye[16 * (size_t)j] = eye[16 * (size_t)j + 5] = eye[16 * (size_t)j + 10] = eye[16 * (size_t)j + 15] = 1.0;
    return build_jobs(scans, eye.data(), n_jobs);
}

// Queues the describe of the jobs into d_words [n_jobs][W] / d_bits [n_jobs] and the stats' way down (when asked for); the caller joins
// the stream while the job table lives.
int queue_describe(elm_ctx* ctx, const elm_places* pl, const JobTable& t, unsigned long long* d_words, uint32_t* d_bits, elm_places_stats* stats,
                   hipStream_t st, const char* what) {
    const size_t n_jobs = t.jobs.size();
    QueryScratch scr{ctx};
    EvidJob* d_jobs = scr.take<EvidJob>(elm_host::kScrRows, n_jobs);
    elm_places_stats* d_stats = scr.take<elm_places_stats>(elm_host::kScrStats, n_jobs);
    if (scr.rc != ELM_OK) return scr.rc;
    const PlaceParams pp{pl->cfg.n_rings, pl->cfg.n_layers, pl->d_tables};
    hipError_t e = hipMemcpyAsync(d_jobs, t.jobs.data(), n_jobs * sizeof(EvidJob), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_words, 0, n_jobs * pl->W * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, n_jobs * sizeof(elm_places_stats), st);
    if (e == hipSuccess) e = launched([&] { launch_pl_describe(st, pp, d_jobs, (uint32_t)n_jobs, (uint32_t)t.chunks, d_words, d_bits, d_stats); });
    if (e == hipSuccess && stats) e = hipMemcpyAsync(stats, d_stats, n_jobs * sizeof(elm_places_stats), hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? ELM_OK : dev_error(ctx, what, e);
}

double yaw_of_shift(uint32_t k) { return k < 32u ? -(2.0 * M_PI * (double)k) / 64.0 : (2.0 * M_PI * (double)(64u - k)) / 64.0; }

// Queues the match of Q query descriptors (d_qwords / d_qbits) against the database and the results' way down, and joins the stream.
int match_and_join(elm_ctx* ctx, const elm_places* pl, const unsigned long long* d_qwords, const uint32_t* d_qbits, uint32_t Q,
                   const elm_places_query_config* cfgs, elm_place_candidate* cands, int32_t* n_cands, elm_place_match* matches, hipStream_t st,
                   const char* what) {
    const uint32_t N = pl->size;
    memset(n_cands, 0, Q * sizeof(int32_t));
    hipError_t e = hipSuccess;
    if (N) {
        const size_t cand_bytes = (size_t)Q * kPlaceMaxTopK * sizeof(elm_place_candidate), cfg_bytes = (size_t)Q * sizeof(elm_places_query_config);
        QueryScratch scr{ctx};
        elm_place_match* d_m = scr.take<elm_place_match>(elm_host::kScrPlaceMatches, (size_t)Q * N);
        char* d_c = scr.take<char>(elm_host::kScrPlaceCands, cand_bytes + cfg_bytes + Q * sizeof(int32_t));
        if (scr.rc != ELM_OK) return scr.rc;
        elm_place_candidate* d_cands = (elm_place_candidate*)d_c;
        elm_places_query_config* d_cfgs = (elm_places_query_config*)(d_c + cand_bytes);
        int32_t* d_n = (int32_t*)(d_c + cand_bytes + cfg_bytes);
        e = hipMemcpyAsync(d_cfgs, cfgs, cfg_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(d_cands, 0, cand_bytes, st); // k_pl_topk writes the first n_cands[q] of a query only
        if (e == hipSuccess)
            e = launched([&] { launch_pl_match(st, d_qwords, d_qbits, Q, pl->d_words, pl->d_bits, pl->d_ids, pl->W, N, d_cfgs, d_m, d_cands, d_n); });
        if (e == hipSuccess) e = hipMemcpyAsync(n_cands, d_n, Q * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(cands, d_cands, cand_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && matches) e = hipMemcpyAsync(matches, d_m, (size_t)Q * N * sizeof(elm_place_match), hipMemcpyDeviceToHost, st);
    }
    const int rc = join(ctx, st, e, what);
    if (rc != ELM_OK) return rc;
    for (uint32_t q = 0; q < Q; ++q)
        for (int32_t c = 0; c < n_cands[q]; ++c) {
            elm_place_candidate& o = cands[(size_t)q * kPlaceMaxTopK + c];
            o.yaw_rad = yaw_of_shift(o.shift);
        }
    return ELM_OK;
}

} // namespace

extern "C" int elm_places_tables(const elm_places_config* cfg, double* ring_edge2, double* z_edge, double* dir) {
    std::vector<double> re, ze, d;
    if (!place_tables(cfg, re, ze, d)) return ELM_ERR_INVALID;
    if (ring_edge2) memcpy(ring_edge2, re.data(), re.size() * sizeof(double));
    if (z_edge) memcpy(z_edge, ze.data(), ze.size() * sizeof(double));
    if (dir) memcpy(dir, d.data(), d.size() * sizeof(double));
    return ELM_OK;
}

extern "C" int elm_places_create(elm_ctx* ctx, const elm_places_config* cfg, int capacity, elm_places** out) {
    if (!ctx || !cfg || !out || capacity < 1 || capacity > kPlaceMaxCapacity) return ELM_ERR_INVALID;
    *out = nullptr;
    std::vector<double> re, ze, dir;
    if (!place_tables(cfg, re, ze, dir)) return ELM_ERR_INVALID;
    const int rc = check_call(ctx, "elm_places_create");
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, "elm_places_create", [&](hipStream_t) { return create_impl(ctx, cfg, (uint32_t)capacity, re, ze, dir, out); });
}

extern "C" void elm_places_destroy(elm_places* pl) { places_free(pl); }

extern "C" int elm_places_reset(elm_ctx* ctx, elm_places* pl) {
    int rc = check_object(ctx, pl, "elm_places_reset");
    if (rc != ELM_OK) return rc;
    pl->size = 0;
    pl->ids.clear();
    return ELM_OK;
}

extern "C" int elm_places_size(elm_ctx* ctx, const elm_places* pl, size_t* n) {
    if (!n) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pl, "elm_places_size");
    if (rc != ELM_OK) return rc;
    *n = pl->size;
    return ELM_OK;
}

extern "C" int elm_places_describe(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, int n_jobs,
                                   uint64_t* words_out, elm_places_stats* stats) {
    const char* what = "elm_places_describe";
    int rc = check_jobs(ctx, pl, scans, levels16, n_jobs, words_out != nullptr, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const JobTable t = level_jobs(scans, levels16, (uint32_t)n_jobs);
        const size_t n_words = (size_t)n_jobs * pl->W;
        QueryScratch scr{ctx};
        char* d_w = scr.take<char>(elm_host::kScrPlaceWords, n_words * sizeof(unsigned long long) + (size_t)n_jobs * sizeof(uint32_t));
        if (scr.rc != ELM_OK) return scr.rc;
        int rc = queue_describe(ctx, pl, t, (unsigned long long*)d_w, (uint32_t*)(d_w + n_words * sizeof(unsigned long long)), stats, st, what);
        if (rc != ELM_OK) return rc;
        // (the job table on the host is read by the copy until the join)
        return join(ctx, st, hipMemcpyAsync(words_out, d_w, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, st), what);
    });
}

extern "C" int elm_places_add(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, const int64_t* ids, int n_jobs,
                              elm_places_stats* stats) {
    const char* what = "elm_places_add";
    int rc = check_jobs(ctx, pl, scans, levels16, n_jobs, ids != nullptr, what);
    if (rc != ELM_OK) return rc;
    if ((size_t)pl->size + (size_t)n_jobs > pl->capacity) return refuse_full(ctx, what, "entries", pl->size, (size_t)n_jobs, pl->capacity);
    return on_stream(ctx, what, [&](hipStream_t st) {
        const JobTable t = level_jobs(scans, levels16, (uint32_t)n_jobs);
        pl->ids.reserve((size_t)pl->size + (size_t)n_jobs);
        // the rows past `size` are nobody's until the call has succeeded
        int rc = queue_describe(ctx, pl, t, pl->d_words + (size_t)pl->size * pl->W, pl->d_bits + pl->size, stats, st, what);
        if (rc != ELM_OK) return rc;
        rc = join(ctx, st, hipMemcpyAsync(pl->d_ids + pl->size, ids, (size_t)n_jobs * sizeof(int64_t), hipMemcpyHostToDevice, st), what);
        if (rc != ELM_OK) return rc;
        pl->ids.insert(pl->ids.end(), ids, ids + n_jobs);
        pl->size += (uint32_t)n_jobs;
        return (int)ELM_OK;
    });
}

extern "C" int elm_places_add_words(elm_ctx* ctx, elm_places* pl, const uint64_t* words, const int64_t* ids, size_t n) {
    const char* what = "elm_places_add_words";
    if (!ctx || !pl || (n && (!words || !ids))) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pl, what);
    if (rc != ELM_OK) return rc;
    if (n > (size_t)(pl->capacity - pl->size)) return refuse_full(ctx, what, "entries", pl->size, n, pl->capacity);
    if (!n) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        pl->ids.reserve((size_t)pl->size + n);
        unsigned long long* d_w = pl->d_words + (size_t)pl->size * pl->W;
        hipError_t e = hipMemcpyAsync(d_w, words, n * pl->W * sizeof(uint64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pl->d_ids + pl->size, ids, n * sizeof(int64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launched([&] { launch_pl_bits(st, d_w, pl->W, (uint32_t)n, pl->d_bits + pl->size); });
        const int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        pl->ids.insert(pl->ids.end(), ids, ids + n);
        pl->size += (uint32_t)n;
        return (int)ELM_OK;
    });
}

extern "C" int elm_places_download(elm_ctx* ctx, const elm_places* pl, size_t first, size_t count, uint64_t* words, int64_t* ids, uint32_t* n_bits) {
    const char* what = "elm_places_download";
    int rc = check_object(ctx, pl, what);
    if (rc != ELM_OK) return rc;
    if (!range_ok(first, count, pl->size)) return ELM_ERR_INVALID;
    if (!count) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        hipError_t e = hipSuccess;
        if (words) e = hipMemcpyAsync(words, pl->d_words + first * pl->W, count * pl->W * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && n_bits) e = hipMemcpyAsync(n_bits, pl->d_bits + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        const int rc = join(ctx, st, e, what);
        if (rc == ELM_OK && ids) memcpy(ids, pl->ids.data() + first, count * sizeof(int64_t));
        return rc;
    });
}

extern "C" int elm_places_match_words(elm_ctx* ctx, elm_places* pl, const uint64_t* words, int n_queries, const elm_places_query_config* query_cfg,
                                      elm_place_candidate* cands, int32_t* n_cands, elm_place_match* matches) {
    const char* what = "elm_places_match_words";
    if (!ctx || !pl || !words || !cands || !n_cands || n_queries < 1 || n_queries > kEvidMaxJobs || !query_configs_ok(query_cfg, n_queries))
        return ELM_ERR_INVALID;
    int rc = check_object(ctx, pl, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const uint32_t Q = (uint32_t)n_queries;
        const size_t w_bytes = (size_t)Q * pl->W * sizeof(unsigned long long);
        QueryScratch scr{ctx};
        char* d_w = scr.take<char>(elm_host::kScrPlaceWords, w_bytes + Q * sizeof(uint32_t));
        if (scr.rc != ELM_OK) return scr.rc;
        uint32_t* d_qbits = (uint32_t*)(d_w + w_bytes);
        hipError_t e = hipMemcpyAsync(d_w, words, w_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launched([&] { launch_pl_bits(st, (const unsigned long long*)d_w, pl->W, Q, d_qbits); });
        if (e != hipSuccess) return dev_error(ctx, what, e);
        return match_and_join(ctx, pl, (const unsigned long long*)d_w, d_qbits, Q, query_cfg, cands, n_cands, matches, st, what);
    });
}

extern "C" int elm_places_query(elm_ctx* ctx, elm_places* pl, const elm_scan* const* scans, const double* levels16, int n_queries,
                                const elm_places_query_config* query_cfg, elm_place_candidate* cands, int32_t* n_cands, elm_place_match* matches,
                                elm_places_stats* stats) {
    const char* what = "elm_places_query";
    const bool rest_ok = cands && n_cands && n_queries >= 1 && n_queries <= kEvidMaxJobs && query_configs_ok(query_cfg, n_queries);
    int rc = check_jobs(ctx, pl, scans, levels16, n_queries, rest_ok, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const uint32_t Q = (uint32_t)n_queries;
        const JobTable t = level_jobs(scans, levels16, Q);
        const size_t w_bytes = (size_t)Q * pl->W * sizeof(unsigned long long);
        QueryScratch scr{ctx};
        char* d_w = scr.take<char>(elm_host::kScrPlaceWords, w_bytes + Q * sizeof(uint32_t));
        if (scr.rc != ELM_OK) return scr.rc;
        uint32_t* d_qbits = (uint32_t*)(d_w + w_bytes);
        int rc = queue_describe(ctx, pl, t, (unsigned long long*)d_w, d_qbits, stats, st, what);
        if (rc != ELM_OK) return rc;
        return match_and_join(ctx, pl, (const unsigned long long*)d_w, d_qbits, Q, query_cfg, cands, n_cands, matches, st, what);
    });
}
