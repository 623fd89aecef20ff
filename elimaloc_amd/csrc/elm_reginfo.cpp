// elm_reginfo.cpp -- registration information (include/elimaloc_hip_reginfo.h): the argument checks, the job table
// and the launches of elm_k_reginfo.hip around the pair search of elm_map_get_correspondences (elm_host::query_pairs_enqueue), on the call
// skeleton of elm_call.hpp / elm_query.hpp; and the host's call of the pair terms.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "elm_dev_reginfo.hpp"
#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

extern "C" void elm_reginfo_config_default(elm_reginfo_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->metric = ELM_REGINFO_METRIC_METHOD;
}

namespace {

bool config_ok(const elm_reginfo_config* c) {
    if (c->metric != ELM_REGINFO_METRIC_METHOD && c->metric != ELM_REGINFO_METRIC_PLANE) return false;
    return fin_ge0(c->sigma2) && fin_ge0(c->length_scale_m) && fin_ge0(c->min_eigen_ratio) && c->min_eigen_ratio < 1.0;
}

template <int METHOD, int METRIC>
bool pair_terms(const double* rows, const double* p, const double* mu, const double* S, const double* nrm, double th, RegInfoPair& o) {
    return reginfo_pair<METHOD, METRIC>(rows, p[0], p[1], p[2], mu[0], mu[1], mu[2], S, nrm, th, o);
}

struct RegInfoJobs {
    std::vector<RegInfoJob> jobs; // ascending chunk0
    uint64_t points = 0, chunks = 0;
};
RegInfoJobs build_reginfo_jobs(const elm_scan* const* scans, const double* poses16, uint32_t n_jobs) {
    RegInfoJobs t;
    t.jobs.resize(n_jobs);
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const size_t n = scans[j]->n;
        t.jobs[j].pts = (const float*)scans[j]->d_pts;
        t.jobs[j].n = scans[j]->n;
        t.jobs[j].chunk0 = (uint32_t)t.chunks;
        t.jobs[j].pt0 = t.points;
        pose_rows12(poses16 + 16 * (size_t)j, t.jobs[j].rows);
        t.points += n;
        t.chunks += (n + 255) / 256;
    }
    return t;
}

int information_impl(elm_ctx* ctx, const elm_map* map, const elm_scan* const* scans, const double* poses16, uint32_t n_jobs,
                     const elm_reg_config* reg, const elm_reginfo_config* cfg, elm_reginfo_result* results) {
    const char* what = "elm_register_information";
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    const int method = reg->icp_method;
    const bool plane = cfg->metric == ELM_REGINFO_METRIC_PLANE;
    memset(results, 0, (size_t)n_jobs * sizeof(*results));
    for (uint32_t j = 0; j < n_jobs; ++j) {
        results[j].n_points = (int32_t)scans[j]->n;
        results[j].status = ELM_REGINFO_NO_PAIRS | ELM_REGINFO_DEGENERATE;
    }
    if (map->dm.n_vox == 0) return ELM_OK;
    int rc = elm_host::check_covariances(ctx, map, method);
    if (rc == ELM_OK && plane) rc = elm_host::check_covariances(ctx, map, ELM_GICP);
    if (rc != ELM_OK) return rc;
    const RegInfoJobs t = build_reginfo_jobs(scans, poses16, n_jobs);
    if (t.chunks == 0) return ELM_OK;
    const int qwhat = method == ELM_VGICP ? 1 : method == ELM_AVGICP ? 2 : 0;
    const size_t per = qwhat == 2 ? 8 : 1;
    QueryScratch scr{ctx};
    RegInfoJob* d_jobs = scr.take<RegInfoJob>(elm_host::kScrRows, n_jobs);
    double* d_query = scr.take<double>(elm_host::kScrPoints, (size_t)t.points * 3);
    int32_t* d_pairs = scr.take<int32_t>(elm_host::kScrBeamArrays, (size_t)t.points * per);
    double* d_part = scr.take<double>(elm_host::kScrPartials, (size_t)t.chunks * kRiWords);
    elm_reginfo_result* d_res = scr.take<elm_reginfo_result>(elm_host::kScrStats, n_jobs);
    if (scr.rc != ELM_OK) return scr.rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    ScanDesc hd{}; // read by the search's descriptor copy until the stream is joined
    hipError_t e = hipMemcpyAsync(d_jobs, t.jobs.data(), (size_t)n_jobs * sizeof(RegInfoJob), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launched([&] { launch_reginfo_transform(st, d_jobs, n_jobs, (uint32_t)t.chunks, d_query); });
    if (e == hipSuccess) {
        rc = elm_host::query_pairs_enqueue(ctx, map, qwhat, d_query, (size_t)t.points, reg->max_search_dist, d_pairs, &hd);
        if (rc != ELM_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        e = launched([&] {
            launch_reginfo_terms(st, map->dm, method, cfg->metric, reg->max_search_dist, d_jobs, n_jobs, (uint32_t)t.chunks, d_pairs, d_part);
            launch_reginfo_finish(st, d_jobs, n_jobs, d_part, *cfg, d_res);
        });
    }
    if (e == hipSuccess) e = hipMemcpyAsync(results, d_res, (size_t)n_jobs * sizeof(*results), hipMemcpyDeviceToHost, st);
    return join(ctx, st, e, what); // the job table and the descriptor on the host are read by their copies until here
}

} // namespace

extern "C" int elm_register_information(elm_ctx* ctx, const elm_map* map, const elm_scan* const* scans, const double* poses16, int n_jobs,
                                        const elm_reg_config* reg, const elm_reginfo_config* cfg, elm_reginfo_result* results) {
    const char* what = "elm_register_information";
    if (!ctx || !map || !scans || !poses16 || !reg || !cfg || !results || n_jobs < 1 || n_jobs > ELM_REGINFO_MAX_JOBS) return ELM_ERR_INVALID;
    if (!config_ok(cfg) || reg->icp_method < ELM_P2P || reg->icp_method > ELM_AVGICP) return ELM_ERR_INVALID;
    if (!(isfinite(reg->max_search_dist) && reg->max_search_dist > 0.0)) return ELM_ERR_INVALID;
    if (cfg->metric == ELM_REGINFO_METRIC_PLANE && (reg->icp_method == ELM_VGICP || reg->icp_method == ELM_AVGICP)) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    uint64_t points = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (!scans[j] || scans[j]->ctx != ctx) return ELM_ERR_INVALID;
        points += scans[j]->n;
    }
    if (points > 0x7FFFFF00ull || !poses_finite(poses16, (size_t)n_jobs)) return ELM_ERR_INVALID;
    if (reg->use_radar_cov != 0) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": use_radar_cov is not supported (source covariances are not part of the information)");
        return ELM_ERR_UNSUPPORTED;
    }
    return guard_alloc(ctx, what, [&] { return information_impl(ctx, map, scans, poses16, (uint32_t)n_jobs, reg, cfg, results); });
}

extern "C" int elm_reginfo_pair_terms(const double* T16, const double* p, const double* mu, const double* S9, const double* normal3, double th,
                                      int method, int metric, double* w, double* JtMJ36, double* JtMe6, double* eMe) {
    if (!T16 || !p || !mu || method < ELM_P2P || method > ELM_AVGICP || !(isfinite(th) && th > 0.0)) return ELM_ERR_INVALID;
    const bool plane = metric == ELM_REGINFO_METRIC_PLANE;
    if (!plane && metric != ELM_REGINFO_METRIC_METHOD) return ELM_ERR_INVALID;
    if (plane && (!normal3 || method == ELM_VGICP || method == ELM_AVGICP)) return ELM_ERR_INVALID;
    double rows[12];
    pose_rows12(T16, rows);
    RegInfoPair o;
    memset(&o, 0, sizeof(o));
    bool in;
    if (plane) in = method == ELM_P2P ? pair_terms<ELM_P2P, ELM_REGINFO_METRIC_PLANE>(rows, p, mu, S9, normal3, th, o)
                                      : pair_terms<ELM_GICP, ELM_REGINFO_METRIC_PLANE>(rows, p, mu, S9, normal3, th, o);
    else if (method == ELM_P2P) in = pair_terms<ELM_P2P, ELM_REGINFO_METRIC_METHOD>(rows, p, mu, S9, normal3, th, o);
    else if (method == ELM_GICP) in = pair_terms<ELM_GICP, ELM_REGINFO_METRIC_METHOD>(rows, p, mu, S9, normal3, th, o);
    else if (method == ELM_VGICP) in = pair_terms<ELM_VGICP, ELM_REGINFO_METRIC_METHOD>(rows, p, mu, S9, normal3, th, o);
    else in = pair_terms<ELM_AVGICP, ELM_REGINFO_METRIC_METHOD>(rows, p, mu, S9, normal3, th, o);
    if (!in) memset(&o, 0, sizeof(o));
    if (w) *w = o.w;
    if (JtMJ36)
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) JtMJ36[i * 6 + j] = JtMJ36[j * 6 + i] = o.Ht[ri_tri(i, j)];
    if (JtMe6) memcpy(JtMe6, o.gt, sizeof(o.gt));
    if (eMe) *eMe = o.chi;
    return ELM_OK;
}
