// elm_api.cpp -- registration: the choice of kernels per call (choose_path), the correspondence and align calls, the per-iteration
// launch sequence of every elm_register* driver, and the device pass of the node callback.  Host-side C++17.  (What else this file held
// is in elm_ctx.cpp, elm_map.cpp, elm_index.cpp and elm_scan.cpp; the structs behind the handles are in elm_host_types.hpp.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <string>
#include <vector>

#include "elm_host_types.hpp"
#include "elm_la.hpp"

using namespace elm;
using namespace elm_host;

// ------------------------------------------------------------------------------------------------------
// registration
// ------------------------------------------------------------------------------------------------------
static int prof_mark(elm_ctx* ctx) { // records the next pooled event on the context stream
    if (!ctx->profiling) return ELM_OK;
    if (ctx->events_used == (int)ctx->events.size()) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableSystemFence)); // timing only: no system-scope fence between launches
        ctx->events.push_back(e);
    }
    HIPCHK(ctx, hipEventRecord(ctx->events[ctx->events_used++], ctx->stream));
    return ELM_OK;
}

// use_radar_cov (reg.hpp:186-217) changes the arithmetic of the covariance methods only: AlignCloudsLocal (P2P) never reads a covariance.
// ELM_CHECK=strict_pairs: the covariance-weighted methods run the reference's own per-pair arithmetic -- (R^-1 C R^-T)^-1 by 3x3 products and an
// inverse per pair, all 36 entries of J^T M J, LDLT on the lower triangle: the radar kernels with a zero source term -- instead of the
// world-frame / fused forms: the in-product checker of the fast forms (a plain walk, no streams: 12-27 times slower at 131 072-point
// scans, profiles/r04k_strict_rate.txt).
// Unset (the default): every map runs the fast kernels; a map with a flagged covariance of the method's own kind whose stored inverse is
// not symmetric (layout_flags bits 7 / 8, counted by k_point_cov / k_voxel_cov) additionally carries the antisymmetric part of J^T M J in
// side records (choose_path, asym_side_store) -- exact like the per-pair arithmetic.
static int strict_pairs() { // 1: per-pair kernels always, -1: fast kernels, side records by map
    return check_mode("strict_pairs") ? 1 : -1; // (read per call: a registration call, not a launch)
}
// pcm.cpp:92-100: the covariance methods need their covariances computed (the index builders read them)
int elm_host::check_covariances(elm_ctx* ctx, const elm_map* map, int method) {
    if (!map || map->dm.n_vox == 0) return ELM_OK;
    if ((method == ELM_VGICP || method == ELM_AVGICP) && !map->info.has_voxel_cov) {
        ctx->last_error = "VGICP/AVGICP need elm_map_cal_voxel_cov_all() (pcm.cpp:92-95)";
        return ELM_ERR_INVALID;
    }
    if (method == ELM_GICP && !map->info.has_point_cov) {
        ctx->last_error = "GICP needs elm_map_cal_point_cov_all() (pcm.cpp:97-100)";
        return ELM_ERR_INVALID;
    }
    return ELM_OK;
}
struct PathChoice {
    bool radar = false, asym = false, use_grid = false, use_cells = false, use_vnbr = false;
};
// Which kernels one registration call runs.  `radar`: the per-pair kernels (use_radar_cov, or ELM_CHECK=strict_pairs).  Otherwise the search
// index (built on first use) -- dense / two-level cell grid, neighbourhood lists, voxel-mean lists, or the plain walk -- and `asym`: the
// map holds a flagged covariance of the method's kind whose stored inverse is not symmetric, and the fast kernels carry the antisymmetric
// part of J^T M J in side records (RegParams::asym; grid and voxel-list kernels, unfused reduction).  Such a map on one of the fall-back
// indices (lists / plain walk: maps the grid cannot hold, ELM_KERNEL=...) still takes the per-pair kernels.  The one check of the
// covariances every registration driver relies on (check_covariances) runs here.
static int choose_path(elm_ctx* ctx, const elm_map* map, const elm_reg_config* cfg, PathChoice* pc) {
    *pc = PathChoice();
    const int method = cfg->icp_method;
    if (method < ELM_P2P || method > ELM_AVGICP) return ELM_ERR_INVALID;
    if (!map || map->dm.n_vox == 0) return ELM_OK;
    int rc0;
    if ((rc0 = check_covariances(ctx, map, method)) != ELM_OK) return rc0;
    const int mode = strict_pairs();
    if (method != ELM_P2P && (cfg->use_radar_cov != 0 || mode == 1)) { pc->radar = true; return ELM_OK; }
    int rc;
    const bool use_nbr = ctx->kernel_mode != 2 && (method == ELM_P2P || method == ELM_GICP);
    pc->use_grid = use_nbr && ctx->kernel_mode == 4 && map->has_grid;
    if (use_nbr && !pc->use_grid && !map->has_nbr)
        if ((rc = build_search_index(const_cast<elm_map*>(map), &pc->use_grid)) != ELM_OK) return rc;
    pc->use_cells = use_nbr && !pc->use_grid && map->has_cells;
    pc->use_vnbr = ctx->kernel_mode != 2 && (method == ELM_VGICP || method == ELM_AVGICP);
    if (pc->use_vnbr)
        if ((rc = build_voxel_neighbourhoods(const_cast<elm_map*>(map), method == ELM_AVGICP)) != ELM_OK) return rc;
    const bool asym_map = mode < 0 && method != ELM_P2P && (method == ELM_GICP ? map->n_asym_pts != 0 : map->n_asym_vox != 0);
    if (asym_map) {
        if (pc->use_grid || pc->use_vnbr || pc->use_cells) pc->asym = true; // (use_cells: P2P / GICP on the neighbourhood lists -- GICP's kernel
                                                                            // there writes the side records too)
        else {
            // The one slow corner left: asymmetric covariances on a map whose search runs the PLAIN WALK (ELM_KERNEL=direct, or lists that
            // could not be cell-sorted) -- that kernel carries no side records, so the covariance methods run the per-pair kernels (exact,
            // 12-27 times slower).  Said ONCE per map, and visible in elm_reg_result.path.
            pc->radar = true; pc->use_grid = pc->use_cells = pc->use_vnbr = false;
            elm_map* mm = const_cast<elm_map*>(map);
            if (!mm->warned_slow_path) {
                mm->warned_slow_path = true;
                fprintf(stderr, "[elimaloc] map %p: %u point / %u voxel covariances are asymmetric (rank-deficient neighbourhoods) and its search index is a "
                                "fall-back form (%s): method %d runs the per-pair kernels, 12-27 times slower than the grid kernels (elm_reg_result.path = %d)\n",
                        (const void*)map, map->n_asym_pts, map->n_asym_vox, ctx->kernel_mode == 2 ? "ELM_KERNEL=direct" : "lists without cell order", method, ELM_PATH_PAIRS);
            }
        }
    }
    return ELM_OK;
}
static int path_code(const PathChoice& pc) {
    return pc.radar ? ELM_PATH_PAIRS : ((pc.use_grid ? ELM_PATH_GRID : pc.use_cells ? ELM_PATH_LISTS : pc.use_vnbr ? ELM_PATH_VOXEL_LISTS : ELM_PATH_WALK) | (pc.asym ? ELM_PATH_SIDE_RECORDS : 0));
}
// VoxelHashMap::GetCorrespondencePoints / GetCorrespondencesCov / GetCorrespondencesAllCov (vhm.cpp:31-206) as calls of their own: the pairs
// themselves, in input order, as (source index, target index).  The search is the production one -- the QUERY instantiations of the grid /
// voxel-list kernels (the code the fused accumulate kernels run, minus the sums) -- or, without such an index (ELM_KERNEL=direct / lists, a
// refused grid) and with ELM_CHECK=query_direct, the plain walk.
static int get_correspondences_impl(elm_ctx* ctx, const elm_map* map, int what, const double* xyz, size_t n, double max_dist,
                                    uint32_t* src_index, int32_t* tgt_index, size_t cap, size_t* n_pairs);
// the search of that call on query points in HBM (elm_host_types.hpp): also what elm_register_information pairs its points with
int elm_host::query_pairs_enqueue(elm_ctx* ctx, const elm_map* map, int what, const double* d_q, size_t n, double max_dist, int32_t* d_out,
                                  ScanDesc* hd) {
    const int method = what == 0 ? ELM_P2P : what == 1 ? ELM_VGICP : ELM_AVGICP;
    bool production = false;
    const bool force_direct = check_mode("query_direct");
    if (map->dm.n_vox != 0) {
        int rc;
        if (what != 0 && (rc = check_covariances(ctx, map, method)) != ELM_OK) return rc;
        if (!force_direct && ctx->kernel_mode != 2) {
            if (what == 0) {
                bool g = ctx->kernel_mode == 4 && map->has_grid;
                if (!g && ctx->kernel_mode == 4 && !map->has_nbr)
                    if ((rc = build_search_index(const_cast<elm_map*>(map), &g)) != ELM_OK) return rc;
                production = g;
            } else {
                if ((rc = build_voxel_neighbourhoods(const_cast<elm_map*>(map), what == 2)) != ELM_OK) return rc;
                production = map->has_vnbr;
            }
        }
    }
    const size_t per = what == 2 ? 8 : 1;
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_q2, sizeof(ScanDesc))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_q3, sizeof(ScanState))) != ELM_OK) return rc;
    ScanDesc* d_desc = (ScanDesc*)ctx->d_q2.p;
    ScanState* d_state = (ScanState*)ctx->d_q3.p;
    HIPCHK(ctx, hipMemsetAsync(d_out, 0xFF, n * per * sizeof(int32_t), ctx->stream)); // (AllCov: < 0 = no pair with that neighbour)
    if (production) {
        *hd = ScanDesc{};
        hd->pts = nullptr; hd->n = (uint32_t)n; hd->n_total = (uint32_t)n; hd->blk_begin = 0; hd->blk_end = (uint32_t)((n + kBlock - 1) / kBlock);
        HIPCHK(ctx, hipMemcpyAsync(d_desc, hd, sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_state, 0, sizeof(ScanState), ctx->stream)); // done = 0; the pose is not read by a query
        RegParams rp{};
        rp.th = max_dist; rp.th2 = max_dist * max_dist;
        rp.method = method; rp.max_iter = 1;
        rp.query = d_q; rp.q_out = d_out;
        if (what == 0) launch_accumulate_grid(ctx->stream, map->dm, d_desc, 1, (int)hd->blk_end, d_state, nullptr, rp);
        else launch_accumulate_vnbr(ctx->stream, map->dm, d_desc, 1, (int)hd->blk_end, d_state, nullptr, rp);
    } else {
        launch_query_direct(ctx->stream, map->dm, what, d_q, n, max_dist * max_dist, d_out);
    }
    HIPCHK(ctx, hipGetLastError());
    return ELM_OK;
}
// (the host staging of these two calls is sized by the caller's n: an allocation failure is a status, never an exception through the C ABI)
extern "C" int elm_map_get_correspondences(elm_ctx* ctx, const elm_map* map, int what, const double* xyz, size_t n, double max_dist,
                                           uint32_t* src_index, int32_t* tgt_index, size_t cap, size_t* n_pairs) {
    try {
        return get_correspondences_impl(ctx, map, what, xyz, n, max_dist, src_index, tgt_index, cap, n_pairs);
    } catch (const std::bad_alloc&) {
        if (ctx) ctx->last_error = "elm_map_get_correspondences: host allocation failed";
        return ELM_ERR_ALLOC;
    }
}
static int get_correspondences_impl(elm_ctx* ctx, const elm_map* map, int what, const double* xyz, size_t n, double max_dist,
                                    uint32_t* src_index, int32_t* tgt_index, size_t cap, size_t* n_pairs) {
    if (!ctx || !map || what < 0 || what > 2 || (n && !xyz) || !n_pairs || map->ctx != ctx) return ELM_ERR_INVALID;
    *n_pairs = 0;
    if (n == 0) return ELM_OK;
    if (n > 0x7FFFFF00ull) return ELM_ERR_INVALID;
    if (ctx->in_flight) return ELM_ERR_INVALID; // the context's stream and query scratch belong to the batch in flight
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t per = what == 2 ? 8 : 1;
    std::vector<int32_t> out(n * per);
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_q0, n * 3 * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_q1, n * per * sizeof(int32_t))) != ELM_OK) return rc;
    double* d_q = (double*)ctx->d_q0.p;
    int32_t* d_out = (int32_t*)ctx->d_q1.p;
    HIPCHK(ctx, hipMemcpyAsync(d_q, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ScanDesc hd{};
    if ((rc = query_pairs_enqueue(ctx, map, what, d_q, n, max_dist, d_out, &hd)) != ELM_OK) {
        (void)hipStreamSynchronize(ctx->stream); // (the upload reads the caller's array until here)
        return rc;
    }
    HIPCHK(ctx, hipMemcpyAsync(out.data(), d_out, n * per * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (also: the stack copy of the descriptor has been read)
    // marshalling: the reference's result vectors hold the pairs in input order (tbb::parallel_reduce joins its ranges in order)
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (what == 2) {
            for (int r = 0; r < 7; ++r) {
                const int32_t v = out[8 * i + r];
                if (v < 0) continue;
                if (k < cap) { if (src_index) src_index[k] = (uint32_t)i; if (tgt_index) tgt_index[k] = v; }
                ++k;
            }
        } else {
            const int32_t v = out[i];
            if (v < -1) continue;
            if (k < cap) { if (src_index) src_index[k] = (uint32_t)i; if (tgt_index) tgt_index[k] = v; }
            ++k;
        }
    }
    *n_pairs = k; // (the count even when cap was too small: call again with more room)
    return ELM_OK;
}

// Registration::AlignCloudsLocal (method ELM_P2P; reg.cpp:15-66), ::AlignCloudsLocalPointCov (ELM_GICP; :68-152) and
// ::AlignCloudsLocalVoxelCov (ELM_VGICP / ELM_AVGICP; :154-225) on pairs the caller holds: accumulate on the device with the reference's
// per-pair arithmetic, solve, return the step.
static int align_clouds_local_impl(elm_ctx* ctx, int method, const double* src_local, const double* tgt_xyz, const double* tgt_cov9,
                                   const double* src_cov9, size_t n, const double last_icp_pose[16], double trans_th,
                                   const elm_reg_config* cfg, double T_out[16], double local_cov[36], double* fitness_score);
extern "C" int elm_align_clouds_local(elm_ctx* ctx, int method, const double* src_local, const double* tgt_xyz, const double* tgt_cov9,
                                      const double* src_cov9, size_t n, const double last_icp_pose[16], double trans_th,
                                      const elm_reg_config* cfg, double T_out[16], double local_cov[36], double* fitness_score) {
    try {
        return align_clouds_local_impl(ctx, method, src_local, tgt_xyz, tgt_cov9, src_cov9, n, last_icp_pose, trans_th, cfg, T_out, local_cov, fitness_score);
    } catch (const std::bad_alloc&) {
        if (ctx) ctx->last_error = "elm_align_clouds_local: host allocation failed";
        return ELM_ERR_ALLOC;
    }
}
static int align_clouds_local_impl(elm_ctx* ctx, int method, const double* src_local, const double* tgt_xyz, const double* tgt_cov9,
                                   const double* src_cov9, size_t n, const double last_icp_pose[16], double trans_th,
                                   const elm_reg_config* cfg, double T_out[16], double local_cov[36], double* fitness_score) {
    if (!ctx || !last_icp_pose || !T_out || method < ELM_P2P || method > ELM_AVGICP || (n && (!src_local || !tgt_xyz))) return ELM_ERR_INVALID;
    if (n && method != ELM_P2P && !tgt_cov9) return ELM_ERR_INVALID;
    if (n > 0x7FFFFF00ull) return ELM_ERR_INVALID; // (the same bound as elm_map_get_correspondences: the pairs of one scan)
    if (ctx->in_flight) return ELM_ERR_INVALID;    // the context's stream and scratch belong to the batch in flight
    elm_reg_config dflt;
    if (!cfg) { elm_reg_config_default(&dflt); cfg = &dflt; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    AlignArgs a{};
    {
        double R[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r * 3 + c] = last_icp_pose[c * 4 + r];
        elm::inv3(R, a.Rinv); // (the 3x3 cofactor inverse of the rotation block, as the registration's own state keeps it)
        for (int r = 0; r < 3; ++r)
            a.tinv[r] = -((a.Rinv[r * 3] * last_icp_pose[12] + a.Rinv[r * 3 + 1] * last_icp_pose[13]) + a.Rinv[r * 3 + 2] * last_icp_pose[14]);
    }
    a.th = trans_th; a.th2 = trans_th * trans_th;
    a.lm_lambda = cfg->lm_lambda;
    a.method = method == ELM_AVGICP ? ELM_VGICP : method;
    a.use_src_cov = (cfg->use_radar_cov != 0 && src_cov9 && method != ELM_P2P) ? 1 : 0;
    // staging: positions as they are, covariances column-major -> row-major
    const bool cov = method != ELM_P2P;
    std::vector<double> stage_t, stage_s; // one per upload: both are read by asynchronous copies until the synchronisation below
    auto transposed = [&](const double* c9, std::vector<double>& stage) {
        stage.resize(n * 9);
        for (size_t i = 0; i < n; ++i)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) stage[9 * i + r * 3 + c] = c9[9 * i + c * 3 + r];
        return stage.data();
    };
    int rc;
    const size_t nb = std::max<size_t>(n, 1);
    if ((rc = dev_reserve(ctx, ctx->d_q0, nb * 3 * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_q1, nb * 3 * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_q2, (size_t)1024 * kRadarRecord * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_q3, kAlignOut * sizeof(double))) != ELM_OK) return rc;
    double *d_src = (double*)ctx->d_q0.p, *d_tgt = (double*)ctx->d_q1.p, *d_part = (double*)ctx->d_q2.p, *d_out = (double*)ctx->d_q3.p;
    double *d_cov = nullptr, *d_scov = nullptr;
    // uploads on the context's stream, like the launch behind them (the stream is non-blocking: nothing orders it after the null stream)
    if (n) HIPCHK(ctx, hipMemcpyAsync(d_src, src_local, n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (n) HIPCHK(ctx, hipMemcpyAsync(d_tgt, tgt_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (cov && n) {
        if ((rc = dev_reserve(ctx, ctx->d_q4, n * 9 * sizeof(double))) != ELM_OK) return rc;
        d_cov = (double*)ctx->d_q4.p;
        HIPCHK(ctx, hipMemcpyAsync(d_cov, transposed(tgt_cov9, stage_t), n * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (a.use_src_cov) {
            if ((rc = dev_reserve(ctx, ctx->d_q5, n * 9 * sizeof(double))) != ELM_OK) return rc;
            d_scov = (double*)ctx->d_q5.p;
            HIPCHK(ctx, hipMemcpyAsync(d_scov, transposed(src_cov9, stage_s), n * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    double out[kAlignOut];
    launch_align_pairs(ctx->stream, d_src, d_tgt, d_cov, d_scov, n, a, d_part, d_out);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T_out, out, 16 * sizeof(double));
    if (local_cov && method == ELM_GICP) memcpy(local_cov, out + 16, 36 * sizeof(double)); // (the reference writes local_cov in AlignCloudsLocalPointCov only)
    if (fitness_score) *fitness_score = out[52];
    return ELM_OK;
}

// ctx->rp of a registration call: `blocks` workgroups over `n_scans` scans / slots, uniform_blocks > 0 when each owns that many.  The
// side records of an asymmetric map (pc.asym): the scans' reduced side sums sit right behind the packed sums in d_sums (one exchange
// carries both).  radar_var is read by k_accumulate_radar alone, which runs only when rp.radar != 0.
static int set_reg_params(elm_ctx* ctx, const elm_reg_config* cfg, const PathChoice& pc, uint32_t blocks, int n_scans, uint32_t uniform_blocks) {
    RegParams rp;
    memset(&rp, 0, sizeof(rp));
    rp.th = cfg->max_search_dist;
    rp.th2 = cfg->max_search_dist * cfg->max_search_dist;
    rp.lm_lambda = cfg->lm_lambda;
    rp.term_thr = cfg->icp_termination_threshold_m;
    rp.min_overlap = cfg->min_overlap_ratio;
    rp.max_fitness = cfg->max_fitness_score;
    rp.method = cfg->icp_method;
    rp.max_iter = cfg->max_iteration;
    rp.uniform_blocks = uniform_blocks;
    rp.radar = pc.radar ? (cfg->use_radar_cov != 0 ? 1 : 2) : 0; // 2: the radar kernels without a source covariance (ELM_CHECK=strict_pairs)
    rp.stats = ctx->work_counters ? 1 : 0;
    rp.radar_var[0] = cfg->range_variance_m;
    rp.radar_var[1] = cfg->azimuth_variance_deg;
    rp.radar_var[2] = cfg->elevation_variance_deg;
    if (pc.asym) {
        int rc;
        if ((rc = dev_reserve(ctx, ctx->d_asym, (size_t)std::max<uint32_t>(blocks, 1) * kAsymRecord * sizeof(double))) != ELM_OK) return rc;
        rp.asym = (double*)ctx->d_asym.p;
        rp.asym_sums = (double*)ctx->d_sums.p + (size_t)n_scans * kSums;
    }
    rp.rank_check = ((ctx->comm || ctx->hook) && !rp.radar && !rp.stats) ? 1 : 0;
    ctx->rp = rp;
    return ELM_OK;
}

// the misuse every registration driver refuses: a map of another context, an unknown method, a batch still in flight
static bool reg_args_ok(const elm_ctx* ctx, const elm_map* map, const elm_reg_config* cfg) {
    return map->ctx == ctx && cfg->icp_method >= ELM_P2P && cfg->icp_method <= ELM_AVGICP && !ctx->in_flight;
}


static size_t trace_bytes(int count) { return (size_t)count * ELM_MAX_ITER_TRACE * sizeof(elm_iter_trace); }
// the iteration traces of `count` registrations: device (zeroed on the context stream) and host copies
static int reserve_trace(elm_ctx* ctx, int count, elm_iter_trace** d_trace) {
    const size_t tb = trace_bytes(count);
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_trace, tb)) != ELM_OK) return rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_trace, &ctx->h_trace_cap, tb)) != ELM_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_trace.p, 0, tb, ctx->stream));
    *d_trace = (elm_iter_trace*)ctx->d_trace.p;
    return ELM_OK;
}

// One ICP iteration's correspondence + accumulation launch for `n_scans` scans / slots, bracketed by two profiling marks (the
// solve span starts at the second).
static int enqueue_accumulate(elm_ctx* ctx, const elm_map* map, const ScanDesc* dsc, int n_scans, uint32_t blocks, ScanState* st,
                              const RegParams& rp, const PathChoice& pc, double* partials = nullptr) {
    int rc;
    if ((rc = prof_mark(ctx)) != ELM_OK) return rc;
    if (!partials) partials = (double*)ctx->d_partials.p;
    if (blocks) {
        if (rp.radar) launch_accumulate_radar(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rp);
        else if (pc.use_grid) launch_accumulate_grid(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rp);
        else if (pc.use_cells) launch_accumulate_cell(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rp);
        else if (pc.use_vnbr && rp.method == ELM_AVGICP && map->dm.vface_flagged) {
            // the fused walk on a map with flagged voxels: one flag per workgroup (all zero between launches: the fix-up launch clears what
            // the walk sets)
            RegParams rq = rp;
            const size_t need = (size_t)blocks * sizeof(uint32_t);
            if (need > ctx->d_flagged.cap) {
                if ((rc = dev_reserve(ctx, ctx->d_flagged, need + need / 2)) != ELM_OK) return rc;
                HIPCHK(ctx, hipMemsetAsync(ctx->d_flagged.p, 0, ctx->d_flagged.cap, ctx->stream));
            }
            rq.flagged = (need <= ctx->d_flagged.cap) ? (uint32_t*)ctx->d_flagged.p : nullptr;
            launch_accumulate_vnbr(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rq);
        }
        else if (pc.use_vnbr) launch_accumulate_vnbr(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rp);
        else launch_accumulate_direct(ctx->stream, map->dm, dsc, n_scans, (int)blocks, st, partials, rp);
    }
    return prof_mark(ctx);
}
// folds the recorded events [acc_0, solve_0, acc_1, solve_1, ..., end] into the profile totals
static int prof_collect(elm_ctx* ctx) {
    if (ctx->profiling && ctx->events_used >= 3) {
        for (int k = 0; k + 1 < ctx->events_used; ++k) {
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->events[k], ctx->events[k + 1]));
            if ((k & 1) == 0) { ctx->prof.accumulate_ms += ms; ctx->prof.accumulate_launches++; if (ctx->keep_iter_ms) ctx->iter_acc_ms.push_back(ms); }
            else { ctx->prof.solve_ms += ms; ctx->prof.solve_steps++; }
        }
    }
    ctx->events_used = 0;
    return ELM_OK;
}

// n_dev != nullptr (batch == 1): the scan's size lives in device memory (produced by the downsample kernels on this stream);
// scans[0]->n is its upper bound (grid size).  The result's point counts then come from the device state.
int elm_host::batch_enqueue_impl(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch, const double* T0, const elm_reg_config* cfg,
                                  int want_trace, const unsigned* n_dev) {
    if (!ctx || !map || !scans || batch <= 0 || !T0 || !cfg) return ELM_ERR_INVALID;
    if (!reg_args_ok(ctx, map, cfg)) return ELM_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int method = cfg->icp_method;
    const bool map_empty = map->dm.n_vox == 0;
    if (ctx->iter_key_map != (const void*)map || ctx->iter_key_method != method || ctx->iter_key_batch != batch) {
        // (a registration that ran to max_iteration on another map / method / batch shape must not push THIS call's first early-stop
        // check to its count)
        ctx->iter_key_map = map; ctx->iter_key_method = method; ctx->iter_key_batch = batch;
        for (int k = 0; k < 8; ++k) ctx->iter_ring[k] = 0;
        ctx->iter_hint = 0;
    }
    int rc;
    PathChoice pc;
    if ((rc = choose_path(ctx, map, cfg, &pc)) != ELM_OK) return rc;
    ctx->path = (map && map->dm.n_vox) ? path_code(pc) : 0;
    const bool radar = pc.radar;
    // batch descriptors
    const size_t stage_bytes = (size_t)batch * (sizeof(ScanDesc) + 16 * sizeof(double));
    if ((rc = pinned_reserve(ctx, &ctx->h_desc, &ctx->h_desc_cap, std::max<size_t>(stage_bytes, 4096))) != ELM_OK) return rc;
    ScanDesc* hd = (ScanDesc*)ctx->h_desc;
    double* hT = (double*)((char*)ctx->h_desc + (size_t)batch * sizeof(ScanDesc));
    uint32_t blocks = 0;
    uint32_t uniform_blocks = batch > 0 && scans[0] ? (scans[0]->n + kBlock - 1) / kBlock : 0;
    for (int b = 0; b < batch; ++b) {
        if (!scans[b] || scans[b]->ctx != ctx) return ELM_ERR_INVALID;
        const uint32_t nb = (scans[b]->n + kBlock - 1) / kBlock;
        if (nb != uniform_blocks) uniform_blocks = 0;
        hd[b].pts = scans[b]->d_pts;
        hd[b].n = scans[b]->n;
        hd[b].n_total = scans[b]->n_total;
        hd[b].blk_begin = blocks;
        blocks += nb;
        hd[b].blk_end = blocks;
    }
    memcpy(hT, T0, (size_t)batch * 16 * sizeof(double));
    // the counter of still-iterating scans sits right behind the states (StateTail): an early-stop check reads both with ONE copy, and
    // when the counter is zero the final states are already on the host
    const size_t st_bytes = (size_t)batch * sizeof(ScanState) + sizeof(StateTail);
    if ((rc = dev_reserve(ctx, ctx->d_scans, (size_t)batch * sizeof(ScanDesc))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_T0, (size_t)batch * 16 * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_state, st_bytes)) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_partials, (size_t)std::max<uint32_t>(blocks, 1) * (radar ? kRadarRecord : kSums) * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_sums, (size_t)batch * (radar ? kRadarRecord : kSums + kAsymRecord) * sizeof(double))) != ELM_OK) return rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_state, &ctx->h_state_cap, st_bytes)) != ELM_OK) return rc;
    ctx->results_ready = false;
    elm_iter_trace* d_trace = nullptr;
    if (want_trace && (rc = reserve_trace(ctx, batch, &d_trace)) != ELM_OK) return rc;
    const bool packed_init = batch <= kInitPack;
    if (!packed_init) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_scans.p, hd, (size_t)batch * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_T0.p, hT, (size_t)batch * 16 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = set_reg_params(ctx, cfg, pc, blocks, batch, uniform_blocks)) != ELM_OK) return rc;
    const RegParams& rp = ctx->rp;

    ScanState* st = (ScanState*)ctx->d_state.p;
    const ScanDesc* dsc = (const ScanDesc*)ctx->d_scans.p;
    int* d_active = &state_tail(st, batch)->active;
    (void)hipGetLastError();
    if (packed_init) { // descriptors and guesses as kernel arguments: no H2D copies, no memset
        InitPack pack;
        memset(&pack, 0, sizeof(pack));
        for (int b = 0; b < batch; ++b) {
            pack.d[b] = hd[b];
            memcpy(pack.T0[b], T0 + (size_t)b * 16, 16 * sizeof(double));
        }
        launch_init_pack(ctx->stream, (ScanDesc*)ctx->d_scans.p, st, pack, batch, map_empty ? 1 : 0, d_active, n_dev);
    } else {
        HIPCHK(ctx, hipMemsetAsync(d_active, 0, 2 * sizeof(int), ctx->stream));
        launch_init_state(ctx->stream, st, (const double*)ctx->d_T0.p, batch, map_empty ? 1 : 0, d_active);
    }
    const bool distributed = (ctx->comm != nullptr) || (ctx->hook != nullptr);
    ctx->events_used = 0;
    if (!map_empty) {
        for (int it = 0; it < cfg->max_iteration; ++it) {
            if ((rc = enqueue_accumulate(ctx, map, dsc, batch, blocks, st, rp, pc)) != ELM_OK) return rc;
            if (distributed) {
                launch_solve(ctx->stream, dsc, batch, st, (const double*)ctx->d_partials.p, (double*)ctx->d_sums.p, rp, d_trace, 1, d_active); // reduce only
                // (use_radar_cov on several ranks: the all-reduce carries the radar kernel's 64 sums per scan instead of the 32 of the packed layout)
                if ((rc = exchange(ctx, (double*)ctx->d_sums.p, (size_t)batch * (radar ? kRadarRecord : (rp.asym ? kSums + kAsymRecord : kSums)))) != ELM_OK) return rc;
                launch_solve(ctx->stream, dsc, batch, st, (const double*)ctx->d_partials.p, (double*)ctx->d_sums.p, rp, d_trace, 2, d_active);
            } else {
                launch_solve(ctx->stream, dsc, batch, st, (const double*)ctx->d_partials.p, (double*)ctx->d_sums.p, rp, d_trace, 0, d_active);
            }
            // Early stop: every scan of the batch has met the reference's termination rule (or a gate).  The counter is
            // derived from the (all-reduced) sums, so every rank reads the same value and stops at the same iteration.
            // The first check is placed where the previous batch finished; an unknown history never checks.
            const int done_iters = it + 1;
            if (ctx->iter_hint > 0 && done_iters >= ctx->iter_hint && done_iters < cfg->max_iteration &&
                ((done_iters - ctx->iter_hint) % 2) == 0) {
                HIPCHK(ctx, hipMemcpyAsync(ctx->h_state, st, st_bytes, hipMemcpyDeviceToHost, ctx->stream)); // states + tail
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                if (state_tail(ctx->h_state, batch)->active == 0) {
                    ctx->results_ready = true; // every scan has finished: these ARE the final states
                    break;
                }
            }
        }
        if ((rc = prof_mark(ctx)) != ELM_OK) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    if (!ctx->results_ready) HIPCHK(ctx, hipMemcpyAsync(ctx->h_state, st, st_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (want_trace) HIPCHK(ctx, hipMemcpyAsync(ctx->h_trace, ctx->d_trace.p, trace_bytes(batch), hipMemcpyDeviceToHost, ctx->stream));
    ctx->batch = batch;
    ctx->want_trace = want_trace != 0;
    ctx->in_flight = true;
    return ELM_OK;
}
extern "C" int elm_register_batch_enqueue(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch,
                                          const double* T0, const elm_reg_config* cfg, int want_trace) {
    if (group_call(ctx)) { ctx->last_error = "elm_register_batch_enqueue: not available on a device group (use elm_register_batch / _stream)"; return ELM_ERR_UNSUPPORTED; }
    return batch_enqueue_impl(ctx, map, scans, batch, T0, cfg, want_trace, nullptr);
}

static void state_to_result(const ScanState& h, const RegParams& rp, elm_reg_result& r, int path = 0) {
    memset(&r, 0, sizeof(r));
    r.path = path;
    memcpy(r.T, h.T, sizeof(r.T));
    memcpy(r.local_cov, h.local_cov, sizeof(r.local_cov));
    r.d_fitness = h.fitness;
    r.is_success = h.success;
    r.fitness_score = h.success ? h.fitness : 0.0; // written only on success (reg.cpp:415)
    r.iterations = h.iters;
    r.gate = h.gate;
    r.n_corr_last = h.n_corr_last;
    r.point_iterations = h.pt_iters;
    r.n_cand_total = h.cand_total;
    r.n_occ_total = h.occ_total;
    r.fallback_blocks = h.fallback_blocks;
    r.n_tested_total = h.tested_total;
    if (rp.max_iter <= 0 && h.gate == 0) r.is_success = 1; // no iteration ran: fitness gate on the initial 0.0 passes
}
// the results of the call's `count` registrations from their final states in h_state and, with `trace`, their iteration traces
static void hand_back(const elm_ctx* ctx, int count, elm_reg_result* results, elm_iter_trace* trace) {
    const ScanState* hs = (const ScanState*)ctx->h_state;
    for (int b = 0; results && b < count; ++b) state_to_result(hs[b], ctx->rp, results[b], ctx->path);
    if (trace) memcpy(trace, ctx->h_trace, trace_bytes(count));
}

extern "C" int elm_register_batch_finish(elm_ctx* ctx, elm_reg_result* results, elm_iter_trace* trace) {
    if (!ctx || !ctx->in_flight) return ELM_ERR_INVALID;
    ctx->in_flight = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->results_ready || ctx->want_trace || ctx->profiling) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    {
        int prc = prof_collect(ctx);
        if (prc != ELM_OK) return prc;
    }
    const ScanState* hs = (const ScanState*)ctx->h_state;
    if (ctx->rp.rank_check && state_tail(ctx->h_state, ctx->batch)->rank_mismatch != 0) {
        ctx->last_error = "the ranks iterated different registrations in one slot (rank-agreement check of the exchanged sums)";
        return ELM_ERR_COMM;
    }
    hand_back(ctx, ctx->batch, results, ctx->want_trace ? trace : nullptr);
    {
        int mx = 0;
        for (int b = 0; b < ctx->batch; ++b) mx = std::max(mx, (int)hs[b].iters);
        // where the next batch's first early-stop check goes: the LONGEST of the last eight batches.  (The previous batch's own count
        // mispredicts a stream whose registrations alternate between 2 and 3 iterations every other call: a check one iteration early
        // costs a host round trip in the middle of the registration, ~25 us, a check one iteration late one pair of launches that
        // return at once, ~10 us -- profiles/r04_single_timeline.txt.)
        ctx->iter_ring[ctx->iter_ring_pos++ & 7] = mx;
        int h = 0;
        for (int k = 0; k < 8; ++k) h = std::max(h, ctx->iter_ring[k]);
        ctx->iter_hint = h;
    }
    return ELM_OK;
}

extern "C" int elm_register_batch(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch, const double* T0,
                                  const elm_reg_config* cfg, elm_reg_result* results, elm_iter_trace* trace) {
    if (group_call(ctx)) return elm_multi::reg_batch(ctx, map, scans, batch, T0, cfg, 0, results, trace);
    int rc = elm_register_batch_enqueue(ctx, map, scans, batch, T0, cfg, trace != nullptr);
    if (rc != ELM_OK) return rc;
    return elm_register_batch_finish(ctx, results, trace);
}

// The queue of a slot stream in d_queue: the registrations' items, their initial guesses, the control block and, 64-byte aligned, their
// final states.  h_desc stages the same head [items | guesses | control] -- one copy -- and the slot descriptors at out_off.
struct SlotQueue {
    size_t ctrl_off, out_off;
    QueueItem* d_q; double* d_qT0; StreamCtrl* d_ctrl; ScanState* d_out; // in d_queue
    QueueItem* hq; double* hT; StreamCtrl* hc; ScanDesc* hd;              // in h_desc
};
// what a stream of `count` registrations through S slots of cap_blocks workgroups each reserves: the host staging, the slot descriptors
// and states, the partial records and sums, the queue, the host copy of the final states and the completion counters
static int reserve_slot_queue(elm_ctx* ctx, int count, int S, uint32_t cap_blocks, SlotQueue* q) {
    const size_t t0_off = (size_t)count * sizeof(QueueItem);
    q->ctrl_off = t0_off + (size_t)count * 16 * sizeof(double);
    q->out_off = q->ctrl_off + ((sizeof(StreamCtrl) + 63) / 64) * 64;
    const size_t d_bytes = (size_t)S * sizeof(ScanDesc);
    const uint32_t blocks = cap_blocks * (uint32_t)S;
    int rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_desc, &ctx->h_desc_cap, std::max<size_t>(q->out_off + d_bytes, 4096))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_scans, d_bytes)) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_state, (size_t)S * sizeof(ScanState))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_partials, (size_t)std::max<uint32_t>(blocks, 1) * kSums * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_sums, (size_t)S * (kSums + kAsymRecord) * sizeof(double))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_queue, q->out_off + (size_t)count * sizeof(ScanState))) != ELM_OK) return rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_state, &ctx->h_state_cap, (size_t)count * sizeof(ScanState))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_active, 256)) != ELM_OK) return rc;
    if (!ctx->h_active) HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_active, 64, hipHostMallocDefault));
    char* d = (char*)ctx->d_queue.p;
    char* h = (char*)ctx->h_desc;
    q->d_q = (QueueItem*)d;
    q->d_qT0 = (double*)(d + t0_off);
    q->d_ctrl = (StreamCtrl*)(d + q->ctrl_off);
    q->d_out = (ScanState*)(d + q->out_off);
    q->hq = (QueueItem*)h;
    q->hT = (double*)(h + t0_off);
    q->hc = (StreamCtrl*)(h + q->ctrl_off);
    q->hd = (ScanDesc*)(h + q->out_off);
    return ELM_OK;
}

// Continuous batching: `count` registrations through `slots` slots.  Every ICP iteration is one accumulate launch over the
// slots, the solve, and a refill kernel that hands finished slots the next pending registration on the device -- so the
// launches stay full until the queue is empty (a lockstep batch ends in launches with a handful of live scans, which are
// latency bound).  Per-registration arithmetic is unchanged: results are bit-identical to elm_register_batch.
extern "C" int elm_register_stream(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int count, const double* T0,
                                   const elm_reg_config* cfg, int slots, elm_reg_result* results, elm_iter_trace* trace) {
    if (!ctx || !map || !scans || count <= 0 || !T0 || !cfg || slots <= 0) return ELM_ERR_INVALID;
    if (group_call(ctx)) return elm_multi::reg_batch(ctx, map, scans, count, T0, cfg, slots, results, trace);
    if (map->dm.n_vox == 0 || cfg->max_iteration <= 0) // nothing iterates: the lockstep path handles the degenerate cases
        return elm_register_batch(ctx, map, scans, count, T0, cfg, results, trace);
    if (!reg_args_ok(ctx, map, cfg)) return ELM_ERR_INVALID;
    int rc;
    PathChoice pc;
    if ((rc = choose_path(ctx, map, cfg, &pc)) != ELM_OK) return rc;
    ctx->path = (map && map->dm.n_vox) ? path_code(pc) : 0;
    if (pc.radar) {
        // use_radar_cov: lockstep batches of `slots` registrations (k_accumulate_radar is not a slot kernel; a radar scan is a few hundred
        // returns).  Per-registration arithmetic is that of elm_register_batch.
        for (int b0 = 0; b0 < count; b0 += slots) {
            const int n = std::min(slots, count - b0);
            const int rc = elm_register_batch(ctx, map, scans + b0, n, T0 + (size_t)b0 * 16, cfg, results ? results + b0 : nullptr,
                                              trace ? trace + (size_t)b0 * ELM_MAX_ITER_TRACE : nullptr);
            if (rc != ELM_OK) return rc;
        }
        return ELM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int S = std::min(std::min(slots, count), stream_max_slots());
    uint32_t max_n = 0;
    for (int b = 0; b < count; ++b) {
        if (!scans[b] || scans[b]->ctx != ctx) return ELM_ERR_INVALID;
        max_n = std::max(max_n, scans[b]->n);
    }
    const uint32_t cap_blocks = (max_n + kBlock - 1) / kBlock;
    const uint32_t blocks = cap_blocks * (uint32_t)S;
    SlotQueue q;
    if ((rc = reserve_slot_queue(ctx, count, S, cap_blocks, &q)) != ELM_OK) return rc;
    for (int b = 0; b < count; ++b) { q.hq[b].pts = scans[b]->d_pts; q.hq[b].n = scans[b]->n; q.hq[b].n_total = scans[b]->n_total; }
    memcpy(q.hT, T0, (size_t)count * 16 * sizeof(double));
    *q.hc = StreamCtrl{/*next*/ 0, /*completed*/ 0, /*total*/ count, /*ready*/ count, /*done_iter*/ -1};
    // slot descriptors with fixed block ranges sized for the largest scan
    for (int s = 0; s < S; ++s) {
        q.hd[s].pts = nullptr; q.hd[s].n = 0; q.hd[s].n_total = 0;
        q.hd[s].blk_begin = cap_blocks * (uint32_t)s; q.hd[s].blk_end = cap_blocks * (uint32_t)(s + 1);
    }
    elm_iter_trace* d_trace = nullptr;
    if (trace && (rc = reserve_trace(ctx, count, &d_trace)) != ELM_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(q.d_q, q.hq, q.ctrl_off + sizeof(StreamCtrl), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_scans.p, q.hd, (size_t)S * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_active.p, 0, 2 * sizeof(int), ctx->stream));
    if ((rc = set_reg_params(ctx, cfg, pc, blocks, S, cap_blocks)) != ELM_OK) return rc; // every slot owns cap_blocks workgroups
    const RegParams& rp = ctx->rp;

    ScanState* st = (ScanState*)ctx->d_state.p;
    ScanDesc* dsc = (ScanDesc*)ctx->d_scans.p;
    int* d_active = (int*)ctx->d_active.p;
    const bool distributed = (ctx->comm != nullptr) || (ctx->hook != nullptr);
    (void)hipGetLastError();
    launch_stream_refill(ctx->stream, dsc, st, S, q.d_q, q.d_qT0, q.d_out, q.d_ctrl, 1);
    ctx->events_used = 0;
    // Iterations needed: unknown in advance (it depends on when each registration converges).  The previous call with the
    // same shape is the prediction: enqueue that many without looking, then read the completed counter after every
    // further iteration.  All ranks read the same counter (it derives from all-reduced sums) and stop together.
    const int hard_limit = ((count + S - 1) / S + 1) * cfg->max_iteration;
    const bool same_shape = ctx->stream_hint_count == count && ctx->stream_hint_slots == S;
    const int predicted = same_shape ? ctx->stream_hint_iters : 0;
    double* const partials = (double*)ctx->d_partials.p;
    double* const sums = (double*)ctx->d_sums.p;
    int it = 0;
    for (; it < hard_limit; ++it) {
        if ((rc = enqueue_accumulate(ctx, map, dsc, S, blocks, st, rp, pc, partials)) != ELM_OK) return rc;
        if (distributed) {
            // reduce -> all-reduce -> solve -> refill: four launches + one collective per iteration.  (Side sums of a map with an asymmetric
            // covariance sit right behind the packed sums: one exchange carries both.)  The refill launch walks the slots in slot order and
            // hands the finished ones the next pending registrations -- first come, first served like the single-rank stream, yet identical
            // on every rank (the finished flags derive from the all-reduced sums), so no slot idles while the queue has work.
            launch_solve(ctx->stream, dsc, S, st, partials, sums, rp, d_trace, 1, d_active);
            if ((rc = exchange(ctx, sums, (size_t)S * (rp.asym ? kSums + kAsymRecord : kSums))) != ELM_OK) return rc;
            const StreamArgs sv = {dsc, q.d_q, q.d_qT0, q.d_out, q.d_ctrl, 0, /*save_only*/ 1, 0, it}; // the solve saves + counts, the refill assigns
            launch_solve(ctx->stream, dsc, S, st, partials, sums, rp, d_trace, 2, d_active, &sv);
            launch_stream_refill(ctx->stream, dsc, st, S, q.d_q, q.d_qT0, q.d_out, q.d_ctrl, 0, /*save*/ 0);
        } else {
            // single rank: the solve hands finished slots their next registration itself (no refill launch)
            const StreamArgs sa = {dsc, q.d_q, q.d_qT0, q.d_out, q.d_ctrl, 0, 0, 0, it};
            launch_solve(ctx->stream, dsc, S, st, partials, sums, rp, d_trace, 0, d_active, &sa);
        }
        const int done_iters = it + 1;
        const bool look = predicted > 0 ? done_iters >= predicted : (done_iters >= (count + S - 1) / S && (done_iters % 2) == 0);
        if (look) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_active, &q.d_ctrl->completed, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (*ctx->h_active == count) { ++it; break; }
        }
    }
    if ((rc = prof_mark(ctx)) != ELM_OK) return rc;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_state, q.d_out, (size_t)count * sizeof(ScanState), hipMemcpyDeviceToHost, ctx->stream));
    if (trace) HIPCHK(ctx, hipMemcpyAsync(ctx->h_trace, ctx->d_trace.p, trace_bytes(count), hipMemcpyDeviceToHost, ctx->stream));
    ctx->h_active[2] = 0;
    if (rp.rank_check) HIPCHK(ctx, hipMemcpyAsync(ctx->h_active + 2, d_active + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->h_active[3] = -1;
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_active + 3, &q.d_ctrl->done_iter, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = prof_collect(ctx)) != ELM_OK) return rc;
    if (ctx->h_active[2] != 0) {
        ctx->last_error = "the ranks iterated different registrations in one slot (rank-agreement check of the exchanged sums)";
        return ELM_ERR_COMM;
    }
    ctx->stream_hint_count = count;
    ctx->stream_hint_slots = S;
    // what the next call of this shape enqueues before it first looks: the iterations this one NEEDED (the device notes the iteration
    // whose solve finished the last registration) -- not the count at which the host happened to look, which can only grow: a call
    // with poor initial guesses would leave every later call of the shape enqueueing its iteration count in empty launches
    ctx->stream_hint_iters = (ctx->h_active[3] >= 0) ? std::min(it, ctx->h_active[3] + 1) : it;
    hand_back(ctx, count, results, trace);
    return ELM_OK;
}

constexpr int kStageSets = 3; // staging sets of a host-fed stream: the DMA of group g + 2 may run while group g is still being ordered
static int ensure_side_streams(elm_ctx* ctx) {
    if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->order_stream) {
        // the ordering kernel runs beside the accumulate launches of the compute stream: highest priority, so that its few workgroups
        // are dispatched as soon as a CU has room instead of behind the tail of a 65 536-workgroup launch
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = hi = 0; (void)hipGetLastError(); }
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->order_stream, hipStreamNonBlocking, hi));
    }
    if (!ctx->poll_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->poll_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&ctx->ev_iter[0], &ctx->ev_iter[1], &ctx->ev_iter[2], &ctx->ev_iter[3]})
        if (!*e) HIPCHK(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return ELM_OK;
}
static void sync_all_streams(elm_ctx* ctx) {
    for (hipStream_t st : {ctx->copy_stream, ctx->order_stream, ctx->poll_stream, ctx->stream})
        if (st) (void)hipStreamSynchronize(st);
}

// elm_register_stream with the scans still in HOST memory when the call starts (the per-call contract of RunRegister, reg.cpp:274-290:
// the caller hands over a point vector, not a device handle).  Three things overlap:
//   copy stream    H2D of the packed xyz of the next group of scans into one of kStageSets (3) staging sets (page-locked sources: one DMA per
//                  group when the group is contiguous in host memory)
//   order stream   k_scan_order over the group (staging -> the registration's own place in the arena, Hilbert order), then the
//                  group's arrival is published in ctrl->ready
//   compute stream the ICP iterations of the registrations that have arrived: a slot that finishes (or idles) claims the next
//                  arrived registration in the solve kernel, exactly as in elm_register_stream
// Results are bit-identical to elm_register_stream on the same scans uploaded with elm_scan_upload (same ordering kernel).
extern "C" int elm_register_stream_host(elm_ctx* ctx, const elm_map* map, const float* const* scan_xyz, const uint32_t* n_pts, int count,
                                        const double* T0, const elm_reg_config* cfg, int slots, elm_reg_result* results, elm_iter_trace* trace) {
    if (!ctx || !map || !scan_xyz || !n_pts || count <= 0 || !T0 || !cfg || slots <= 0) return ELM_ERR_INVALID;
    if (!reg_args_ok(ctx, map, cfg)) return ELM_ERR_INVALID;
    if (ctx->comm || ctx->hook) {
        ctx->last_error = "host-fed streams run on one rank (slot assignment follows scan arrival, which differs between ranks)";
        return ELM_ERR_UNSUPPORTED;
    }
    uint32_t max_n = 0;
    for (int b = 0; b < count; ++b) {
        if ((!scan_xyz[b] && n_pts[b]) || n_pts[b] > 0x7FFFFFFFu) return ELM_ERR_INVALID;
        max_n = std::max(max_n, n_pts[b]);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    PathChoice pc;
    if ((rc = choose_path(ctx, map, cfg, &pc)) != ELM_OK) return rc;
    ctx->path = (map && map->dm.n_vox) ? path_code(pc) : 0;
    if (map->dm.n_vox == 0 || cfg->max_iteration <= 0 || max_n == 0 || pc.radar) {
        // nothing iterates (or use_radar_cov: see elm_register_stream): upload and let the lockstep path handle the degenerate cases
        std::vector<elm_scan*> sc((size_t)count, nullptr);
        rc = ELM_OK;
        for (int b = 0; b < count && rc == ELM_OK; ++b) rc = elm_scan_upload(ctx, scan_xyz[b], n_pts[b], n_pts[b], &sc[b]);
        if (rc == ELM_OK) rc = elm_register_batch(ctx, map, sc.data(), count, T0, cfg, results, trace);
        for (elm_scan* x : sc) elm_scan_destroy(x);
        return rc;
    }
    if ((rc = ensure_side_streams(ctx)) != ELM_OK) return rc;
    if ((rc = ensure_hilbert(ctx)) != ELM_OK) return rc;
    const int S = std::min(std::min(slots, count), stream_max_slots());
    const uint32_t cap_blocks = (max_n + kBlock - 1) / kBlock;
    const uint32_t blocks = cap_blocks * (uint32_t)S;
    // upload groups: ~32 MB of points each, at most 64 scans (one ordering workgroup per scan)
    const size_t scan_stride = (((size_t)max_n * sizeof(Pt3)) + 255) & ~(size_t)255;
    const int G = (int)std::min<size_t>(std::min<size_t>(64, (size_t)count), std::max<size_t>(1, ((size_t)32 << 20) / scan_stride));
    const int n_groups = (count + G - 1) / G;
    // the arena: every registration's ordered scan has its own place for the whole call
    std::vector<size_t> off((size_t)count + 1, 0);
    for (int b = 0; b < count; ++b) off[b + 1] = off[b] + ((((size_t)n_pts[b] * sizeof(Pt3)) + 255) & ~(size_t)255);
    if ((rc = dev_reserve(ctx, ctx->d_arena, std::max<size_t>(off[count], 256))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_raw, (size_t)kStageSets * G * scan_stride)) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_order_tmp, (size_t)kStageSets * G * max_n * sizeof(uint32_t))) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_order_jobs, (size_t)count * sizeof(OrderJob))) != ELM_OK) return rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_jobs, &ctx->h_jobs_cap, std::max<size_t>((size_t)count * sizeof(OrderJob), 4096))) != ELM_OK) return rc;
    OrderJob* hj = (OrderJob*)ctx->h_jobs;
    for (int b = 0; b < count; ++b) {
        const int set = (b / G) % kStageSets, j = b % G;
        hj[b].src = (const Pt3*)((char*)ctx->d_raw.p + ((size_t)set * G + j) * scan_stride);
        hj[b].dst = (Pt3*)((char*)ctx->d_arena.p + off[b]);
        hj[b].tmp = (uint32_t*)ctx->d_order_tmp.p + ((size_t)set * G + j) * max_n;
        hj[b].n = n_pts[b];
        hj[b]._pad = 0;
    }
    // queue, guesses, control block, result states (ready = 0: the registrations arrive while the stream runs)
    SlotQueue q;
    if ((rc = reserve_slot_queue(ctx, count, S, cap_blocks, &q)) != ELM_OK) return rc;
    for (int b = 0; b < count; ++b) { q.hq[b].pts = hj[b].dst; q.hq[b].n = n_pts[b]; q.hq[b].n_total = n_pts[b]; }
    memcpy(q.hT, T0, (size_t)count * 16 * sizeof(double));
    *q.hc = StreamCtrl{/*next*/ 0, /*completed*/ 0, /*total*/ count, /*ready*/ 0, /*done_iter*/ -1};
    elm_iter_trace* d_trace = nullptr;
    if (trace && (rc = reserve_trace(ctx, count, &d_trace)) != ELM_OK) return rc;
    if ((rc = set_reg_params(ctx, cfg, pc, blocks, S, cap_blocks)) != ELM_OK) return rc; // (no comm / hook here: rank_check stays 0)
    const RegParams& rp = ctx->rp;

#define HF_CHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            ctx->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            sync_all_streams(ctx);                                                                     \
            return ELM_ERR_DEVICE;                                                                     \
        }                                                                                              \
    } while (0)
    HF_CHK(hipMemcpyAsync(q.d_q, q.hq, q.ctrl_off + sizeof(StreamCtrl), hipMemcpyHostToDevice, ctx->stream));
    HF_CHK(hipMemcpyAsync(ctx->d_order_jobs.p, hj, (size_t)count * sizeof(OrderJob), hipMemcpyHostToDevice, ctx->stream));
    HF_CHK(hipMemsetAsync(ctx->d_active.p, 0, 2 * sizeof(int), ctx->stream));
    ScanState* st = (ScanState*)ctx->d_state.p;
    ScanDesc* dsc = (ScanDesc*)ctx->d_scans.p;
    int* d_active = (int*)ctx->d_active.p;
    (void)hipGetLastError();
    launch_slots_idle(ctx->stream, dsc, st, S, cap_blocks);
    // the side streams start behind the control block's initialisation (and behind whatever the compute stream still reads from
    // the arena / staging of an earlier call)
    HF_CHK(hipEventRecord(ctx->ev_iter[0], ctx->stream));
    HF_CHK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_iter[0], 0));
    HF_CHK(hipStreamWaitEvent(ctx->order_stream, ctx->ev_iter[0], 0));
    ctx->events_used = 0;
    const OrderJob* d_jobs = (const OrderJob*)ctx->d_order_jobs.p;
    int g_enq = 0;
    // one pair of events per upload group (a pool that only grows): group g's "copied" and "ordered"
    while ((int)ctx->ev_groups.size() < 2 * n_groups) {
        hipEvent_t e;
        HF_CHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ev_groups.push_back(e);
    }
    hipStream_t copy_stream = ctx->copy_stream, order_stream = ctx->order_stream;
    auto enqueue_group = [&](int g) -> hipError_t {
        const int set = g % kStageSets, r0 = g * G, r1 = std::min(count, r0 + G);
        hipEvent_t ev_copied = ctx->ev_groups[2 * g], ev_ordered = ctx->ev_groups[2 * g + 1];
        hipError_t e = hipSuccess;
        if (g >= kStageSets) e = hipStreamWaitEvent(copy_stream, ctx->ev_groups[2 * (g - kStageSets) + 1], 0); // the set's previous ordering kernel has read it
        char* base = (char*)ctx->d_raw.p + (size_t)set * G * scan_stride;
        // one DMA for the whole group when it is contiguous in host memory and in the staging set
        bool contiguous = (size_t)max_n * sizeof(Pt3) == scan_stride;
        for (int r = r0; r < r1 && contiguous; ++r)
            contiguous = n_pts[r] == max_n && (r == r0 || scan_xyz[r] == scan_xyz[r - 1] + 3 * (size_t)max_n);
        if (contiguous) {
            if (e == hipSuccess) e = hipMemcpyAsync(base, scan_xyz[r0], (size_t)(r1 - r0) * scan_stride, hipMemcpyHostToDevice, copy_stream);
        } else {
            for (int r = r0; r < r1 && e == hipSuccess; ++r)
                if (n_pts[r]) e = hipMemcpyAsync(base + (size_t)(r - r0) * scan_stride, scan_xyz[r], (size_t)n_pts[r] * sizeof(Pt3), hipMemcpyHostToDevice, copy_stream);
        }
        if (e == hipSuccess) e = hipEventRecord(ev_copied, copy_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(order_stream, ev_copied, 0);
        if (e == hipSuccess) {
            launch_scan_order(order_stream, d_jobs + r0, r1 - r0, ctx->d_hilbert);
            launch_publish_ready(order_stream, q.d_ctrl, r1);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev_ordered, order_stream);
        return e;
    };
    // Iterations are enqueued a few ahead of the device (an event per iteration throttles the host); the number of finished
    // registrations is read on a stream of its own, so that looking never waits for the iterations in flight.
    const StreamArgs sa = {dsc, q.d_q, q.d_qT0, q.d_out, q.d_ctrl, 1, 0, 0, 0};
    int it = 0, done_seen = 0, idle_turns = 0, g_done = 0;
    const int idle_limit = 4000000; // ~ minutes of polling without a single registration finishing: a lost upload, give up
    const int groups_ahead = 2 * kStageSets; // uploads enqueued but not yet ordered: enough to keep the DMA engine fed; a long backlog
                                             // of queued copies and cross-stream waits slows the runtime's submission path down
    for (;;) {
        while (g_done < g_enq && hipEventQuery(ctx->ev_groups[2 * g_done + 1]) == hipSuccess) ++g_done;
        (void)hipGetLastError(); // hipErrorNotReady of the query
        for (int k = 0; k < 2 && g_enq < n_groups && g_enq - g_done < groups_ahead; ++k, ++g_enq) HF_CHK(enqueue_group(g_enq));
        if (it >= 4) HF_CHK(hipEventSynchronize(ctx->ev_iter[it & 3]));
        if ((rc = enqueue_accumulate(ctx, map, dsc, S, blocks, st, rp, pc)) != ELM_OK) { sync_all_streams(ctx); return rc; }
        launch_solve(ctx->stream, dsc, S, st, (const double*)ctx->d_partials.p, (double*)ctx->d_sums.p, rp, d_trace, 0, d_active, &sa);
        HF_CHK(hipEventRecord(ctx->ev_iter[it & 3], ctx->stream));
        ++it;
        HF_CHK(hipMemcpyAsync(ctx->h_active, &q.d_ctrl->completed, sizeof(int), hipMemcpyDeviceToHost, ctx->poll_stream));
        HF_CHK(hipStreamSynchronize(ctx->poll_stream));
        const int c = *ctx->h_active;
        if (c >= count) break;
        idle_turns = (c == done_seen) ? idle_turns + 1 : 0;
        done_seen = c;
        if (idle_turns > idle_limit) {
            ctx->last_error = "host-fed stream made no progress";
            sync_all_streams(ctx);
            return ELM_ERR_DEVICE;
        }
    }
    if ((rc = prof_mark(ctx)) != ELM_OK) { sync_all_streams(ctx); return rc; }
    HF_CHK(hipGetLastError());
    HF_CHK(hipMemcpyAsync(ctx->h_state, q.d_out, (size_t)count * sizeof(ScanState), hipMemcpyDeviceToHost, ctx->stream));
    if (trace) HF_CHK(hipMemcpyAsync(ctx->h_trace, ctx->d_trace.p, trace_bytes(count), hipMemcpyDeviceToHost, ctx->stream));
    HF_CHK(hipStreamSynchronize(ctx->stream));
#undef HF_CHK
    if ((rc = prof_collect(ctx)) != ELM_OK) return rc;
    hand_back(ctx, count, results, trace);
    return ELM_OK;
}

// RunRegister on host buffers; n_total > n: this context holds a SHARD of an n_total-point scan (a rank of a process-per-GPU job, or a
// rank of a device group: elm_multi.cpp) -- the sums are exchanged, the overlap gate is taken against n_total.  quiet: no log text (only one
// rank of a job prints what RunRegister prints).
static int register_impl(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, size_t n_total, const double T0[16],
                         const elm_reg_config* cfg, double T_out[16], int* is_success, double* fitness_score,
                         double local_cov[36], elm_reg_result* result, elm_iter_trace* trace, bool quiet) {
    if (!ctx || !map || !T0 || !cfg || n_total < n) return ELM_ERR_INVALID;
    elm_scan* s = nullptr;
    // the caller's point order (see scan_upload_impl); no wait between the upload and the iterations: the pinned staging buffer is
    // not touched again before elm_register_batch has synchronised the stream
    int rc = scan_upload_impl(ctx, scan_xyz, n, n_total, false, false, &s);
    if (rc != ELM_OK) return rc;
    elm_reg_result res;
    // b_debug_print (reg.cpp:343-347, 396-403): the reference's per-iteration and total timing lines need the iteration trace and one
    // hipEvent pair per accumulate launch; the default (0) records neither -- and prints nothing unless a gate fails
    const bool dbg = cfg->b_debug_print != 0;
    std::vector<elm_iter_trace> own_trace;
    elm_iter_trace* tr = trace;
    const bool was_profiling = ctx->profiling;
    const elm_profile saved_prof = ctx->prof;
    std::chrono::steady_clock::time_point t_begin;
    if (dbg) {
        if (!tr) { own_trace.resize(ELM_MAX_ITER_TRACE); tr = own_trace.data(); }
        ctx->profiling = true;
        ctx->keep_iter_ms = true;
        ctx->iter_acc_ms.clear();
        t_begin = std::chrono::steady_clock::now();
    }
    rc = elm_register_batch(ctx, map, &s, 1, T0, cfg, &res, tr);
    if (dbg) {
        ctx->profiling = was_profiling;
        ctx->keep_iter_ms = false;
        if (!was_profiling) ctx->prof = saved_prof; // the caller did not ask for a profile: its totals are untouched
    }
    if (rc != ELM_OK) (void)hipStreamSynchronize(ctx->stream); // the upload may still be reading the pinned staging buffer
    elm_scan_destroy(s);
    if (rc != ELM_OK) return rc;
    if ((dbg || res.gate != 0) && !quiet) {
        // what RunRegister writes to stdout (elm_format_register_log): warnings always, the timing lines with b_debug_print
        const double total_ms = dbg ? std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count() / 1000.0 : 0.0;
        std::vector<double> corr(ctx->iter_acc_ms);
        corr.resize((size_t)std::max(res.iterations, 0), 0.0);
        // sized from the text itself (up to ELM_MAX_ITER_TRACE per-iteration lines of ~95 bytes: a fixed 4 KB buffer cut the totals off)
        const size_t need = elm_format_register_log(cfg, &res, n_total, dbg ? tr : nullptr, dbg ? corr.data() : nullptr, total_ms, nullptr, 0);
        std::vector<char> text(need + 1);
        elm_format_register_log(cfg, &res, n_total, dbg ? tr : nullptr, dbg ? corr.data() : nullptr, total_ms, text.data(), text.size());
        fputs(text.data(), stdout);
        fflush(stdout);
    }
    if (T_out) memcpy(T_out, res.T, sizeof(res.T));
    if (is_success) *is_success = res.is_success;
    if (fitness_score && res.is_success) *fitness_score = res.fitness_score; // untouched on failure, like the reference
    if (local_cov) memcpy(local_cov, res.local_cov, sizeof(res.local_cov));
    if (result) *result = res;
    return ELM_OK;
}
extern "C" int elm_register(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T0[16],
                            const elm_reg_config* cfg, double T_out[16], int* is_success, double* fitness_score,
                            double local_cov[36], elm_reg_result* result, elm_iter_trace* trace) {
    if (group_call(ctx)) return elm_multi::reg(ctx, map, scan_xyz, n, T0, cfg, T_out, is_success, fitness_score, local_cov, result, trace);
    return register_impl(ctx, map, scan_xyz, n, n, T0, cfg, T_out, is_success, fitness_score, local_cov, result, trace, false);
}
extern "C" int elm_register_shard(elm_ctx* ctx, const elm_map* map, const float* shard_xyz, size_t n, size_t n_total, const double T0[16],
                                  const elm_reg_config* cfg, elm_reg_result* result, elm_iter_trace* trace, int quiet) {
    if (!result) return ELM_ERR_INVALID;
    if (group_call(ctx)) return ELM_ERR_INVALID; // a group shards for itself
    return register_impl(ctx, map, shard_xyz, n, n_total, T0, cfg, nullptr, nullptr, nullptr, nullptr, result, trace, quiet != 0);
}

// ---- the device pass of the node callback (elm_glue.cpp) ---------------------------------------------------------------------
namespace elm_host {
// page-locked scratch of the context: the callback filters the raw cloud straight into it, laid out as the device wants it
// ([kCbTableBytes of deskew tables][xyz]), so that one DMA moves tables and points
void* callback_staging(elm_ctx* ctx, size_t bytes) {
    if (!ctx || hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    if (pinned_reserve(ctx, &ctx->h_stage, &ctx->h_stage_cap, std::max<size_t>(bytes, 4096)) != ELM_OK) return nullptr;
    return ctx->h_stage;
}
// DeskewPoint for every point -> VoxelDownsample -> RunRegister in ONE device pass: DMA of [tables | xyz] and of the per-point
// times, k_deskew, the k_ds_* kernels, k_init_pack (the scan's size stays on the device) and the ICP iterations are enqueued
// back to back; the host waits once, for the result.  stage = callback_staging(): tables at 0 (time, rot_x, rot_y, rot_z, 2000
// doubles each), xyz at kCbTableBytes.  *unpackable = 1: a voxel key does not fit the device table -> the caller's host path.
int callback_register(elm_ctx* ctx, const elm_map* map, const void* stage, const float* rel_time, size_t n, const elm_deskew_tables* tab,
                      double voxel_size, const double T0[16], const elm_reg_config* cfg, elm_reg_result* result, uint64_t* n_source,
                      int* unpackable) {
    if (!ctx || !map || !stage || stage != ctx->h_stage || !rel_time || !tab || !T0 || !cfg || !result || !n_source || !unpackable || n == 0 ||
        n > 0x7FFFFFFFull)
        return ELM_ERR_INVALID;
    if (group_call(ctx)) return ELM_ERR_UNSUPPORTED; // (a device group: the callback takes its stage-by-stage path -- deskew and downsample on the
                                                     // lead device, the registration sharded over the ranks; elm_glue.cpp)
    *unpackable = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    const size_t pts_bytes = n * 3 * sizeof(float);
    if ((rc = dev_reserve(ctx, ctx->d_stage_pts, kCbTableBytes + n * 7 * sizeof(float) + 64)) != ELM_OK) return rc;
    char* base = (char*)ctx->d_stage_pts.p;
    double* d_tab = (double*)base;
    float* d_xyz = (float*)(base + kCbTableBytes);
    float* d_time = d_xyz + 3 * n;
    float* d_out = d_time + n;
    HIPCHK(ctx, hipMemcpyAsync(base, stage, kCbTableBytes + pts_bytes, hipMemcpyHostToDevice, ctx->stream));
    const float* d_und = d_xyz; // run_deskew = 0: the cloud as it is (pcm.cpp:513-525)
    if (tab->b_run_deskew) {
        HIPCHK(ctx, hipMemcpyAsync(d_time, rel_time, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        (void)hipGetLastError();
        launch_deskew(ctx->stream, d_xyz, d_time, (uint32_t)n, deskew_args(tab, d_tab, kCbTableRows), d_out);
        HIPCHK(ctx, hipGetLastError());
        d_und = d_out;
    }
    elm_scan* sc = nullptr;
    unsigned* d_total = nullptr;
    if ((rc = downsample_enqueue(ctx, d_und, n, voxel_size, &sc, &d_total)) != ELM_OK) return rc;
    rc = batch_enqueue_impl(ctx, map, &sc, 1, T0, cfg, 0, d_total);
    if (rc == ELM_OK) rc = elm_register_batch_finish(ctx, result, nullptr);
    else (void)hipStreamSynchronize(ctx->stream);
    elm_scan_destroy(sc);
    if (rc != ELM_OK) return rc;
    const StateTail* ht = state_tail(ctx->h_state, 1);
    *n_source = ht->ds_kept;
    *unpackable = ht->ds_overflow ? 1 : 0;
    return ELM_OK;
}
} // namespace elm_host
