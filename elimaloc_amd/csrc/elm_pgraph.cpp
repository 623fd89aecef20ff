// elm_pgraph.cpp -- the pose graph (include/elimaloc_hip.h, "pose graph"): the object (nodes, edges, the
// linearization and the solver's vectors resident on the device, of capacities fixed at creation), the argument checks, the incidence
// lists (a stable counting sort of (edge, side) by node, redone when the edge set has changed), the conjugate-gradient driver that
// queues pcg_check_every iterations between two reads of the device's state (elm_call.hpp's run_batched), the Levenberg-Marquardt loop
// around it, and the linear initialization (include/elimaloc_hip_posegraph_init.h; DESIGN.md section 23: its preconditions and its two
// stages on the same driver; with the priors in it include/elimaloc_hip_posegraph_init_prior.h and DESIGN.md section 28: the plan of
// elm_pginit_classes.hpp, the gauge nodes, the alignment).  The object itself is elm_pgraph_host.hpp's, which the covariances (elm_pgcov.cpp) and the priors
// (elm_pgprior.cpp: their calls and arrays; their launches are queued here, with the linearization and the cost) share.  The launches
// are those of elm_k_pgraph.hip, elm_k_pgchain.hip, elm_k_pginit.hip, elm_k_pgprior.hip and elm_k_pginitp.hip.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_pginit_classes.hpp"
#include "elm_pgraph_host.hpp"

using namespace elm;
using namespace elm_query;
using namespace elm_pgraph_host;

extern "C" void elm_posegraph_config_default(elm_posegraph_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_iterations = 20;
    c->pcg_max_iterations = 2000;
    c->pcg_check_every = 32;
    c->lambda_init = 1e-4;
    c->lambda_up = 10.0;
    c->lambda_down = 0.1;
    c->lambda_min = 1e-12;
    c->lambda_max = 1e8;
    c->cost_rel_tol = 1e-12;
    c->step_tol = 1e-10;
    c->pcg_rel_tol = 1e-8;
    c->huber_k = 0.0;
}

namespace {

bool config_ok(const elm_posegraph_config* c) {
    if (!c || c->max_iterations < 1 || c->pcg_max_iterations < 1 || c->pcg_check_every < 1) return false;
    if (!fin_ge0(c->lambda_init) || !fin_ge0(c->lambda_min) || !fin_ge0(c->lambda_max) || c->lambda_min > c->lambda_max) return false;
    if (!(isfinite(c->lambda_up) && c->lambda_up >= 1.0) || !(isfinite(c->lambda_down) && c->lambda_down > 0.0 && c->lambda_down <= 1.0)) return false;
    return fin_ge0(c->cost_rel_tol) && fin_ge0(c->step_tol) && fin_ge0(c->pcg_rel_tol) && fin_ge0(c->huber_k);
}

void pg_free(elm_posegraph* pg) {
    if (!pg) return;
    if (elm_host::ctx_is_alive(pg->ctx, pg->ctx_id)) (void)hipSetDevice(pg->ctx->device); // a context destroyed first: just release
    if (pg->blob) (void)hipFree(pg->blob);
    if (pg->prior_blob) (void)hipFree(pg->prior_blob);
    delete pg;
}

// the device arrays of the object from its one allocation
void carve(elm_posegraph* pg, Carver& c) {
    const size_t Nc = pg->n_cap, Ec = pg->e_cap;
    PgDev& d = pg->dev;
    pg->poses = c.take<double>(12 * Nc);
    pg->trial = c.take<double>(12 * Nc);
    pg->d_fixed = c.take<uint8_t>(Nc);
    pg->d_ei = c.take<int32_t>(Ec);
    pg->d_ej = c.take<int32_t>(Ec);
    pg->d_Z = c.take<double>(12 * Ec);
    pg->d_info = c.take<double>(36 * Ec);
    pg->d_inc_start = c.take<uint32_t>(Nc + 1);
    pg->d_inc = c.take<uint32_t>(2 * Ec);
    pg->d_hubs = c.take<uint32_t>(pg_max_hubs(Ec));
    d.r = c.take<double>(6 * Ec);
    d.A = c.take<double>(36 * Ec);
    d.B = c.take<double>(36 * Ec);
    d.s = c.take<double>(Ec);
    d.w = c.take<double>(Ec);
    d.gi = c.take<double>(6 * Ec);
    d.gj = c.take<double>(6 * Ec);
    d.Hii = c.take<double>(36 * Ec);
    d.Hij = c.take<double>(36 * Ec);
    d.Hjj = c.take<double>(36 * Ec);
    d.Hd = c.take<double>(36 * Nc);
    d.g = c.take<double>(6 * Nc);
    d.Minv = c.take<double>(36 * Nc);
    d.active = c.take<uint8_t>(Nc);
    d.x = c.take<double>(6 * Nc);
    d.rr = c.take<double>(6 * Nc);
    d.z = c.take<double>(6 * Nc);
    d.p = c.take<double>(6 * Nc);
    d.q = c.take<double>(6 * Nc);
    d.part_pq = c.take<double>(pg_pq_slots((uint32_t)Nc, (uint32_t)pg_max_hubs(Ec)));
    d.part_rz = c.take<double>(pg_blocks((uint32_t)Nc));
    d.part_cost = c.take<double>(3 * (size_t)pg_blocks((uint32_t)Ec));
    d.part_max = c.take<double>(pg_blocks((uint32_t)Nc));
    d.state = c.take<PgState>(1);
    d.out = c.take<PgOut>(1);
    d.e_stride = (uint32_t)Ec;
    d.ei = pg->d_ei;
    d.ej = pg->d_ej;
    d.Z = pg->d_Z;
    d.info = pg->d_info;
    d.fixed = pg->d_fixed;
    d.inc_start = pg->d_inc_start;
    d.inc = pg->d_inc;
    d.hubs = pg->d_hubs;
    // the chain preconditioner's factor and vectors: every level padded to whole segments, for the capacity's levels
    PgcLevel lv[kPgcMaxLevels];
    const uint32_t nl = pgc_levels((uint32_t)Nc, lv);
    const size_t pad = (size_t)lv[nl - 1].off + (size_t)lv[nl - 1].nseg * kPgcSeg, segs = (size_t)lv[nl - 1].soff + lv[nl - 1].nseg;
    PgcDev& k = pg->chain;
    pg->d_ce = c.take<uint32_t>(Nc);
    k.G = c.take<double>(36 * pad);
    k.A = c.take<double>(36 * pad);
    k.B = c.take<double>(36 * pad);
    k.Lw = c.take<double>(36 * pad);
    k.De = c.take<double>(36 * segs);
    k.y = c.take<double>(6 * pad);
    k.bl = c.take<double>(6 * segs);
    k.be = c.take<double>(6 * segs);
    k.ce = pg->d_ce;
}

int create_impl(elm_ctx* ctx, hipStream_t st, uint32_t n_cap, uint32_t e_cap, elm_posegraph** out) {
    elm_posegraph* pg = new elm_posegraph();
    pg->ctx = ctx;
    pg->ctx_id = ctx->id;
    pg->n_cap = n_cap;
    pg->e_cap = e_cap;
    DeviceBlob blob(st);
    hipError_t e = blob.alloc([&](Carver& c) { carve(pg, c); });
    // zeroed on the context's stream and joined: a memset on the null stream may still be running when the first upload on the
    // context's (non-blocking) stream lands, and would then wipe it
    if (e == hipSuccess) e = hipMemsetAsync(blob.p, 0, blob.bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        pg_free(pg);
        return dev_error(ctx, "elm_posegraph_create", e);
    }
    pg->blob = blob.release();
    *out = pg;
    return ELM_OK;
}

void rows12_to_pose16(const double* P, double* T16) {
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 4; ++q) T16[q * 4 + r] = P[r * 4 + q];
    T16[3] = T16[7] = T16[11] = 0.0;
    T16[15] = 1.0;
}

// the incidence lists of the current edge set: per node its (edge, side) entries in ascending edge index, and the hubs
hipError_t upload_csr(elm_posegraph* pg, hipStream_t st, std::vector<uint32_t>& start, std::vector<uint32_t>& inc, std::vector<uint32_t>& hubs) {
    const uint32_t N = pg->N, E = pg->E;
    start.assign((size_t)N + 1, 0u);
    for (uint32_t e = 0; e < E; ++e) {
        ++start[(size_t)pg->ei[e] + 1];
        ++start[(size_t)pg->ej[e] + 1];
    }
    for (uint32_t v = 0; v < N; ++v) start[v + 1] += start[v];
    inc.assign(2 * (size_t)E + 1, 0u);
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t e = 0; e < E; ++e) { // edges ascending: every list ends up ascending
        inc[at[pg->ei[e]]++] = e << 1;
        inc[at[pg->ej[e]]++] = (e << 1) | 1u;
    }
    hubs.clear();
    for (uint32_t v = 0; v < N; ++v)
        if (start[v + 1] - start[v] > kPgHubDegree) hubs.push_back(v);
    pg->n_hubs = (uint32_t)hubs.size();
    hubs.push_back(0u);
    // the chain edge of v: the lowest-index edge between v and v + 1, in either direction (whether both ends are active is the
    // device's to say, from the flags and the diagonal blocks of the solve)
    std::vector<uint32_t> ce(N ? N : 1u, kPgcNoEdge);
    for (uint32_t e = E; e-- > 0u;) { // descending: the lowest index is written last
        const int32_t a = pg->ei[e], b = pg->ej[e];
        if (b == a + 1) ce[a] = e << 1;
        else if (a == b + 1) ce[b] = (e << 1) | 1u;
    }
    hipError_t e = hipMemcpyAsync(pg->d_ce, ce.data(), ce.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pg->d_inc_start, start.data(), start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && E) e = hipMemcpyAsync(pg->d_inc, inc.data(), 2 * (size_t)E * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pg->d_hubs, hubs.data(), hubs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st); // the host vectors are read until here
    return e;
}

// Queues the linearization at the current poses with the damping lambda.  With priors the node kernel runs twice: its summing entry
// leaves the edges' H_vv and g_v, the priors are added onto them, and its read-back entry redoes the active rule, the damping and the
// inverse on the completed block (k_pg_nodes itself is untouched, and without priors the launches are exactly those of before).
hipError_t queue_linearize(elm_posegraph* pg, hipStream_t st, double huber_k, double lambda, bool for_solve) {
    hipError_t e = ensure_csr(pg, st);
    if (e == hipSuccess) e = ensure_prior_rows(pg, st);
    if (e != hipSuccess) return e;
    pg->lin_huber = huber_k;
    const PgDev& d = dev_view(pg);
    const PgPriorDev* pr = prior_view(pg);
    const PgcDev* c = for_solve ? chain(pg) : nullptr;
    return launched([&] {
        launch_pg_linearize(st, d, pg->poses, huber_k);
        if (!pr) {
            launch_damping(st, d, c, lambda, 1);
            return;
        }
        launch_pgp_linearize(st, *pr, pg->poses, pg->prior_huber);
        launch_pg_nodes(st, d, lambda, 1);
        launch_pgp_nodes(st, d, *pr);
        launch_damping(st, d, c, lambda, 0);
    });
}

// The conjugate gradients on the current linearization and damping (launch_damping has run with this lambda and chain(pg)):
// check_every iterations are queued, then the state comes down once.
int run_pcg(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, double lambda, double tol, int max_it, int check_every, PcgStats& stats, const char* what) {
    const PgDev& d = dev_view(pg);
    stats = PcgStats{};
    if (!pg->N) return ELM_OK;
    const PgcDev* c = chain(pg);
    PgState state{};
    hipError_t e = launched([&] { launch_pg_pcg_begin(st, d, c, tol); });
    if (e == hipSuccess)
        e = run_batched(
            st, check_every, max_it, [&](uint32_t it) { launch_pg_pcg_iteration(st, d, c, lambda, tol, it); }, (const PgState*)d.state, &state,
            [&](uint32_t it) { return state.stop[it & 1u] != 0; });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    stats.iterations = (int32_t)state.iters;
    stats.converged = (int32_t)state.converged;
    stats.rel_residual = state.rz0 > 0.0 ? sqrt(state.rz[state.iters & 1u]) / sqrt(state.rz0) : 0.0;
    return ELM_OK;
}

// the cost record at `poses` (and the largest |x| of the retraction queued before it); the priors count unless the caller ignores them
int cost_at(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, const double* poses, double huber_k, int want_grad, PgOut& out, const char* what,
            bool with_priors = true) {
    const PgDev& d = dev_view(pg);
    const PgPriorDev* pr = with_priors ? prior_view(pg) : nullptr;
    hipError_t e = launched([&] { launch_pg_cost(st, d, pr, poses, huber_k, pg->prior_huber, want_grad); });
    if (e == hipSuccess) e = hipMemcpyAsync(&out, d.out, sizeof(PgOut), hipMemcpyDeviceToHost, st);
    return join(ctx, st, e, what);
}

int optimize_impl(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, const elm_posegraph_config& c, elm_posegraph_result* res, elm_posegraph_trace* trace,
                  int trace_cap) {
    const char* what = "elm_posegraph_optimize";
    elm_posegraph_result R{};
    double lambda = c.lambda_init;
    pg->lin_valid = false;
    hipError_t e = queue_linearize(pg, st, c.huber_k, lambda, true);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    PgOut o{};
    int rc = cost_at(ctx, pg, st, pg->poses, c.huber_k, 0, o, what);
    if (rc != ELM_OK) return rc;
    pg->lin_valid = true;
    double F = o.cost;
    R.cost_initial = R.cost_final = F;
    R.lambda_final = lambda;
    R.stop_reason = F == 0.0 ? ELM_PG_STOP_COST_ZERO : ELM_PG_STOP_MAX_ITERATIONS;
    while (R.stop_reason == ELM_PG_STOP_MAX_ITERATIONS && R.solves < c.max_iterations) {
        PcgStats s;
        rc = run_pcg(ctx, pg, st, lambda, c.pcg_rel_tol, c.pcg_max_iterations, c.pcg_check_every, s, what);
        if (rc != ELM_OK) return rc;
        const PgDev& d = dev_view(pg);
        e = launched([&] { launch_pg_retract(st, d, pg->poses, pg->trial); });
        if (e != hipSuccess) return dev_error(ctx, what, e);
        rc = cost_at(ctx, pg, st, pg->trial, c.huber_k, 0, o, what);
        if (rc != ELM_OK) return rc;
        const double F_new = o.cost, used = lambda;
        const bool accept = F_new < F;
        ++R.solves;
        R.pcg_iterations_total += s.iterations;
        bool stop = false;
        if (accept) {
            ++R.accepted;
            std::swap(pg->poses, pg->trial);
            pg->lin_valid = false; // the linearization is that of the poses before the step until it is redone below
            const double dec = F - F_new, F_old = F;
            F = F_new;
            lambda = std::max(lambda * c.lambda_down, c.lambda_min);
            if (F == 0.0) R.stop_reason = ELM_PG_STOP_COST_ZERO, stop = true;
            else if (dec <= c.cost_rel_tol * F_old) R.stop_reason = ELM_PG_STOP_COST_TOL, stop = true;
            else if (o.dmax <= c.step_tol) R.stop_reason = ELM_PG_STOP_STEP_TOL, stop = true;
            else if (R.solves >= c.max_iterations) stop = true;
            if (!stop) {
                e = queue_linearize(pg, st, c.huber_k, lambda, true);
                if (e != hipSuccess) return dev_error(ctx, what, e);
                pg->lin_valid = true;
            }
        } else {
            ++R.rejected;
            if (o.dmax <= c.step_tol) R.stop_reason = ELM_PG_STOP_STEP_TOL, stop = true;
            else if (lambda >= c.lambda_max) R.stop_reason = ELM_PG_STOP_LAMBDA_MAX, stop = true;
            else {
                lambda = std::min(lambda * c.lambda_up, c.lambda_max);
                e = launched([&] { launch_damping(st, d, chain(pg), lambda, 0); }); // (the chain factor is redone with it)
                if (e != hipSuccess) return dev_error(ctx, what, e);
            }
        }
        if (trace && R.solves <= trace_cap) {
            elm_posegraph_trace& t = trace[R.solves - 1];
            t.cost = F_new;
            t.lambda = used;
            t.accepted = accept ? 1 : 0;
            t.pcg_iterations = s.iterations;
        }
        if (stop) break;
    }
    rc = join(ctx, st, hipSuccess, what);
    if (rc != ELM_OK) return rc;
    R.cost_final = F;
    R.lambda_final = lambda;
    if (res) *res = R;
    return ELM_OK;
}

bool init_config_ok(const elm_posegraph_init_config* c) {
    return c && isfinite(c->pcg_rel_tol) && c->pcg_rel_tol > 0.0 && c->pcg_max_iterations >= 1 && c->pcg_check_every >= 1 && c->stages >= 1 &&
           c->stages <= (ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS);
}

// The preconditions on the nodes and the edge weights that both initializations share: "" when they hold, else the text.
std::string init_edge_refusal(const elm_posegraph* pg, int stages) {
    if (!pg->N) return "no node in the graph";
    for (uint32_t e = 0; e < pg->E; ++e) {
        if ((stages & ELM_PG_INIT_ROT) && !(pg->wr[e] > 0.0)) return "edge " + std::to_string(e) + " has no positive rotation weight trace(Omega_ww) / 3";
        if ((stages & ELM_PG_INIT_TRANS) && !(pg->wt[e] > 0.0))
            return "edge " + std::to_string(e) + " has no positive translation weight trace(Omega_vv) / 3";
    }
    return "";
}

// The preconditions of elm_posegraph_initialize that need the graph: "" when they hold, else the text for elm_last_error.  The
// components come from a union-find over the host's copy of the edges (path halving, the smaller index the root).
std::string init_refusal(const elm_posegraph* pg, int stages) {
    const std::string edges = init_edge_refusal(pg, stages);
    if (!edges.empty()) return edges;
    std::vector<uint32_t> root(pg->N);
    for (uint32_t v = 0; v < pg->N; ++v) root[v] = v;
    auto find = [&](uint32_t v) {
        while (root[v] != v) v = root[v] = root[root[v]];
        return v;
    };
    for (uint32_t e = 0; e < pg->E; ++e) {
        const uint32_t a = find((uint32_t)pg->ei[e]), b = find((uint32_t)pg->ej[e]);
        if (a != b) root[std::max(a, b)] = std::min(a, b);
    }
    std::vector<uint8_t> anchored(pg->N, 0), has_edge(pg->N, 0);
    for (uint32_t v = 0; v < pg->N; ++v)
        if (pg->fixed[v]) anchored[find(v)] = 1;
    for (uint32_t e = 0; e < pg->E; ++e) has_edge[find((uint32_t)pg->ei[e])] = 1;
    for (uint32_t v = 0; v < pg->N; ++v)
        if (has_edge[v] && !anchored[v]) return "the connected component of node " + std::to_string(v) + " has edges but no fixed node (singular at lambda = 0)";
    return "";
}

// One stage of the initialization: its edge terms at `at`, the undamped node sums (with the chain factor), the conjugate gradients.
// pr: null, or the priors whose terms of `stage` (0: rotations, 1: translations) under the weights `weight` are added onto the node sums
// by queue_linearize's launch pattern; without them the launches are those of before.
int init_stage(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, const elm_posegraph_init_config& c,
               void (*launch_terms)(hipStream_t, const PgDev&, const double*), const double* at, const PgPriorDev* pr, const double* weight, int stage,
               PcgStats& s, const char* what) {
    const PgDev& d = dev_view(pg);
    hipError_t e = launched([&] {
        launch_terms(st, d, at);
        if (!pr) {
            launch_damping(st, d, chain(pg), 0.0, 1);
            return;
        }
        launch_pgip_terms(st, *pr, at, weight, stage);
        launch_pg_nodes(st, d, 0.0, 1);
        launch_pgp_nodes(st, d, *pr);
        launch_damping(st, d, chain(pg), 0.0, 0);
    });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    return run_pcg(ctx, pg, st, 0.0, c.pcg_rel_tol, c.pcg_max_iterations, c.pcg_check_every, s, what);
}

// What elm_posegraph_initialize_priors adds to a run of the initialization (null for elm_posegraph_initialize, which ignores priors).
struct InitPriorRun {
    const elm_pginit::Plan* plan;
    double align_min_ratio;
    elm_posegraph_init_prior_result* ext; // everything but `base`
    double *v_pre_out, *align_out;
    int align_capacity;
};

// The gauge nodes held as if fixed on the device; the object's own flags are put back when the guard is released or leaves.
struct GaugeHold {
    elm_posegraph* pg;
    hipStream_t st;
    bool held = false;
    hipError_t upload(const std::vector<uint8_t>& fx) {
        hipError_t e = hipMemcpyAsync(pg->d_fixed, fx.data(), fx.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st); // the host vector is read until here
        return e;
    }
    hipError_t hold(const std::vector<uint32_t>& gauge) {
        std::vector<uint8_t> fx(pg->fixed);
        for (uint32_t v : gauge) fx[v] = 1;
        held = true;
        return upload(fx);
    }
    hipError_t release() {
        if (!held) return hipSuccess;
        held = false;
        return upload(pg->fixed);
    }
    ~GaugeHold() { (void)release(); }
};

// the priors' Huber threshold off for the call's costs, and back as it was however the call ends
struct PriorHuberOff {
    double& k;
    const double old;
    explicit PriorHuberOff(double& ref) : k(ref), old(ref) { k = 0.0; }
    void back() { k = old; }
    ~PriorHuberOff() { back(); }
};

int initialize_impl(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, const elm_posegraph_init_config& c, elm_posegraph_init_result* res, double* rows_out,
                    double* v_out, const InitPriorRun* run, const char* what) {
    const size_t N = pg->N;
    const bool rot = (c.stages & ELM_PG_INIT_ROT) != 0, trans = (c.stages & ELM_PG_INIT_TRANS) != 0;
    elm_posegraph_init_result R{};
    hipError_t e = ensure_csr(pg, st);
    if (e == hipSuccess && run) e = ensure_prior_rows(pg, st);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    // With priors in the run: their view, the three weight arrays and the aligned components' lists in the call's one allocation.
    // Without a prior in the object pv is null and every launch below is elm_posegraph_initialize's.
    const PgPriorDev* pv = run ? prior_view(pg) : nullptr;
    const size_t P = pv ? pg->P : 0, A = pv ? run->plan->aligned() : 0;
    DeviceBlob blob(st);
    double *d_w = nullptr, *d_sums = nullptr, *d_xf = nullptr;
    uint32_t *d_first = nullptr, *d_list = nullptr;
    int32_t* d_comp = nullptr;
    GaugeHold gauge{pg, st};
    if (pv) {
        const elm_pginit::Plan& pl = *run->plan;
        e = blob.alloc([&](Carver& cv) {
            d_w = cv.take<double>(3 * P);
            d_first = cv.take<uint32_t>(A + 1);
            d_list = cv.take<uint32_t>(pl.list.size());
            d_comp = cv.take<int32_t>(A ? N : 0);
            d_sums = cv.take<double>(16 * A);
            d_xf = cv.take<double>(21 * A);
        });
        if (e == hipSuccess) e = hipMemcpyAsync(d_w, pl.w_rot.data(), P * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_w + P, pl.w_pre.data(), P * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_w + 2 * P, pl.w_last.data(), P * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && A) e = hipMemcpyAsync(d_first, pl.list_first.data(), (A + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && A) e = hipMemcpyAsync(d_list, pl.list.data(), pl.list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && A) e = hipMemcpyAsync(d_comp, pl.node_comp.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && A) e = gauge.hold(pl.gauge); // held through S1 and S2
        if (e != hipSuccess) return dev_error(ctx, what, e);
    }
    const double *w_rot = d_w, *w_pre = d_w + P, *w_last = d_w + 2 * P;
    PgOut o{};
    // elm_posegraph_initialize ignores priors, here and in its stages; with a run they count, both Huber thresholds off
    double no_threshold = 0.0;
    PriorHuberOff huber_off(run ? pg->prior_huber : no_threshold);
    int rc = cost_at(ctx, pg, st, pg->poses, 0.0, 0, o, what, run != nullptr);
    if (rc != ELM_OK) return rc;
    R.cost_before = o.cost;
    // From here the contribution arrays, the node sums and the flags are those of the stages: a linearization that was valid is put
    // back below unless the poses change.
    const bool was_valid = pg->lin_valid;
    pg->lin_valid = false;
    const PgDev& d = dev_view(pg);
    double* const rows = d.q; // [N][6]: the conjugate gradients' q is free between two solves
    PcgStats s;
    if (rot) {
        rc = init_stage(ctx, pg, st, c, launch_pgi_rot_terms, pg->poses, pv, w_rot, 0, s, what);
        if (rc != ELM_OK) return rc;
        R.rot_iterations = s.iterations;
        R.rot_converged = s.converged;
        R.rot_rel_residual = s.rel_residual;
        const uint32_t nb = pg_blocks(pg->N);
        std::vector<double> counts(nb);
        e = launched([&] { launch_pgi_rot_apply(st, d, pg->poses, pg->trial, rows, d.part_rz); });
        if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d.part_rz, nb * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && rows_out) e = hipMemcpyAsync(rows_out, rows, 6 * N * sizeof(double), hipMemcpyDeviceToHost, st);
        rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        double n = 0.0;
        for (uint32_t k = 0; k < nb; ++k) n += counts[k]; // whole numbers in slot order
        R.degenerate_nodes = (int32_t)n;
    } else {
        e = hipMemcpyAsync(pg->trial, pg->poses, 12 * N * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return dev_error(ctx, what, e);
        if (rows_out) { // the current rows
            std::vector<double> P(12 * N);
            rc = join(ctx, st, hipMemcpyAsync(P.data(), pg->poses, 12 * N * sizeof(double), hipMemcpyDeviceToHost, st), what);
            if (rc != ELM_OK) return rc;
            for (size_t v = 0; v < N; ++v)
                for (int q = 0; q < 6; ++q) rows_out[6 * v + q] = P[12 * v + (q < 3 ? q : q + 1)];
        }
    }
    // one translation solve at the trial poses under the weights `weight`, applied; `out` [N][3] takes the upper three of the solution
    auto trans_stage = [&](const double* weight, double* out) -> int {
        int rc = init_stage(ctx, pg, st, c, launch_pgi_trans_terms, pg->trial, pv, weight, 1, s, what);
        if (rc != ELM_OK) return rc;
        std::vector<double> host(out ? 6 * N : 0); // the solution [N][6]
        hipError_t e = launched([&] { launch_pgi_trans_apply(st, d, pg->trial); });
        if (e == hipSuccess && out) e = hipMemcpyAsync(host.data(), d.x, 6 * N * sizeof(double), hipMemcpyDeviceToHost, st);
        rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        if (out)
            for (size_t v = 0; v < N; ++v)
                for (int q = 0; q < 3; ++q) out[3 * v + q] = host[6 * v + q];
        return ELM_OK;
    };
    int deficient = 0;
    if (run) {
        *run->ext = elm_posegraph_init_prior_result{};
        if (run->v_pre_out && !A) std::fill(run->v_pre_out, run->v_pre_out + 3 * N, 0.0);
    }
    if (trans) {
        rc = trans_stage(A ? w_pre : w_last, A ? run->v_pre_out : v_out);
        if (rc != ELM_OK) return rc;
        R.trans_iterations = s.iterations;
        R.trans_converged = s.converged;
        R.trans_rel_residual = s.rel_residual;
    } else if (v_out) {
        std::fill(v_out, v_out + 3 * N, 0.0);
    }
    if (A) { // (both stages were requested: the plan aligns nothing otherwise)
        elm_posegraph_init_prior_result& X = *run->ext;
        X.pre_iterations = R.trans_iterations;
        X.pre_converged = R.trans_converged;
        X.pre_rel_residual = R.trans_rel_residual;
        X.aligned_components = (int32_t)A;
        e = gauge.release();
        if (e != hipSuccess) return dev_error(ctx, what, e);
        std::vector<double> sums(16 * A), out_rows(ELM_PG_INIT_ALIGN_ROW * A), xf(21 * A);
        e = launched([&] { launch_pgip_align_sums(st, *pv, pg->trial, w_last, d_first, d_list, (uint32_t)A, d_sums); });
        if (e == hipSuccess) e = hipMemcpyAsync(sums.data(), d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        for (size_t k = 0; k < A; ++k) {
            double* row = &out_rows[ELM_PG_INIT_ALIGN_ROW * k];
            elm_pginit::align_row(&sums[16 * k], row);
            memcpy(&xf[21 * k], row + 16, 9 * sizeof(double));
            memcpy(&xf[21 * k + 9], row, 6 * sizeof(double));
            const double s1 = row[25], s2 = row[26], ratio = s1 > 0.0 ? s2 / s1 : 0.0;
            if (!(s2 > run->align_min_ratio * s1)) ++deficient;
            X.min_align_ratio = k ? std::min(X.min_align_ratio, ratio) : ratio;
        }
        X.rank_deficient_components = deficient;
        if (run->align_out)
            memcpy(run->align_out, out_rows.data(), ELM_PG_INIT_ALIGN_ROW * std::min(A, (size_t)run->align_capacity) * sizeof(double));
        e = hipMemcpyAsync(d_xf, xf.data(), xf.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launched([&] { launch_pgip_align_apply(st, pg->N, d_comp, d_xf, pg->trial); });
        if (e != hipSuccess) return dev_error(ctx, what, e);
        rc = trans_stage(w_last, v_out); // S3: the gauge nodes released, every prior in (its join also ends the reads of xf)
        if (rc != ELM_OK) return rc;
        R.trans_iterations = s.iterations;
        R.trans_converged = s.converged;
        R.trans_rel_residual = s.rel_residual;
    }
    rc = cost_at(ctx, pg, st, pg->trial, 0.0, 0, o, what, run != nullptr);
    if (rc != ELM_OK) return rc;
    huber_off.back();
    R.cost_after = o.cost;
    R.applied = ((!rot || R.rot_converged) && (!trans || R.trans_converged) && (!A || run->ext->pre_converged) && !deficient) ? 1 : 0;
    if (R.applied) {
        std::swap(pg->poses, pg->trial);
    } else if (was_valid) {
        // The same kernels on the same poses: the same bytes as before the call in what a linearization shows (the contribution arrays,
        // the undamped diagonal blocks and the gradient, the sums and the flags).  The damped blocks, their inverses and the chain factor
        // are NOT those of the caller's last lambda: they are left at lambda = 0 without a factor.  That is invisible only because
        // elm_posegraph_solve queues launch_damping with its own lambda before its conjugate gradients and optimize_impl linearizes
        // anew; a later caller that read the inverses or the factor without doing so would have to restore them here.
        e = queue_linearize(pg, st, pg->lin_huber, 0.0, false);
        rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        pg->lin_valid = true;
    }
    *res = R;
    return ELM_OK;
}

} // namespace

hipError_t elm_pgraph_host::ensure_csr(elm_posegraph* pg, hipStream_t st) {
    if (!pg->csr_dirty) return hipSuccess;
    std::vector<uint32_t> start, inc, hubs;
    hipError_t e = upload_csr(pg, st, start, inc, hubs);
    if (e == hipSuccess) pg->csr_dirty = false;
    return e;
}

extern "C" int elm_posegraph_edge_terms(const double* Ti16, const double* Tj16, const double* Z16, double* r, double* A, double* B) {
    if (!Ti16 || !Tj16 || !Z16 || !poses_finite(Ti16, 1) || !poses_finite(Tj16, 1) || !poses_finite(Z16, 1)) return ELM_ERR_INVALID;
    double Pi[12], Pj[12], PZ[12], rr[6], AA[36], BB[36];
    pose_rows12(Ti16, Pi);
    pose_rows12(Tj16, Pj);
    pose_rows12(Z16, PZ);
    pg_edge_terms(Pi, Pj, PZ, rr, AA, BB);
    if (r) memcpy(r, rr, sizeof(rr));
    if (A) memcpy(A, AA, sizeof(AA));
    if (B) memcpy(B, BB, sizeof(BB));
    return ELM_OK;
}

extern "C" int elm_posegraph_create(elm_ctx* ctx, int node_capacity, int edge_capacity, elm_posegraph** out) {
    if (!ctx || !out || node_capacity < 1 || node_capacity > ELM_POSEGRAPH_MAX_NODES || edge_capacity < 1 || edge_capacity > ELM_POSEGRAPH_MAX_EDGES)
        return ELM_ERR_INVALID;
    *out = nullptr;
    const int rc = check_call(ctx, "elm_posegraph_create");
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, "elm_posegraph_create", [&](hipStream_t st) { return create_impl(ctx, st, (uint32_t)node_capacity, (uint32_t)edge_capacity, out); });
}

extern "C" void elm_posegraph_destroy(elm_posegraph* pg) { pg_free(pg); }

extern "C" int elm_posegraph_reset(elm_ctx* ctx, elm_posegraph* pg) {
    int rc = check_object(ctx, pg, "elm_posegraph_reset");
    if (rc != ELM_OK) return rc;
    pg->N = pg->E = 0;
    pg->fixed.clear();
    pg->ei.clear();
    pg->ej.clear();
    pg->wr.clear();
    pg->wt.clear();
    pg->csr_dirty = true;
    pg->P = 0; // the priors go with their nodes; their capacity and threshold stay
    pg->pnode.clear();
    pg->pwr.clear();
    pg->pwt.clear();
    pg->prior_rows_dirty = true;
    pg->lin_valid = false;
    return ELM_OK;
}

extern "C" int elm_posegraph_set_preconditioner(elm_ctx* ctx, elm_posegraph* pg, int kind) {
    if (!ctx || !pg || (kind != ELM_PG_PRECOND_BLOCK_JACOBI && kind != ELM_PG_PRECOND_CHAIN)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_set_preconditioner");
    if (rc != ELM_OK) return rc;
    pg->precond = kind; // every solve redoes the damped blocks and the factor: the linearization stays valid
    return ELM_OK;
}

extern "C" int elm_posegraph_get_preconditioner(elm_ctx* ctx, const elm_posegraph* pg, int* kind) {
    if (!kind) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_get_preconditioner");
    if (rc != ELM_OK) return rc;
    *kind = pg->precond;
    return ELM_OK;
}

extern "C" int elm_posegraph_size(elm_ctx* ctx, const elm_posegraph* pg, size_t* n_nodes, size_t* n_edges) {
    if (!n_nodes || !n_edges) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_size");
    if (rc != ELM_OK) return rc;
    *n_nodes = pg->N;
    *n_edges = pg->E;
    return ELM_OK;
}

extern "C" int elm_posegraph_add_nodes(elm_ctx* ctx, elm_posegraph* pg, const double* poses16, const uint8_t* fixed, size_t n) {
    const char* what = "elm_posegraph_add_nodes";
    if (!ctx || !pg || (n && !poses16)) return ELM_ERR_INVALID;
    if (n > (size_t)ELM_POSEGRAPH_MAX_NODES || !poses_finite(poses16, n)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (n > (size_t)(pg->n_cap - pg->N)) return refuse_full(ctx, what, "nodes", pg->N, n, pg->n_cap);
    if (!n) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(12 * n);
        for (size_t k = 0; k < n; ++k) pose_rows12(poses16 + 16 * k, &rows[12 * k]);
        std::vector<uint8_t> fx(n, 0);
        if (fixed)
            for (size_t k = 0; k < n; ++k) fx[k] = fixed[k] ? 1 : 0;
        pg->fixed.reserve((size_t)pg->N + n);
        hipError_t e = hipMemcpyAsync(pg->poses + 12 * (size_t)pg->N, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_fixed + pg->N, fx.data(), n, hipMemcpyHostToDevice, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        pg->fixed.insert(pg->fixed.end(), fx.begin(), fx.end());
        pg->N += (uint32_t)n;
        pg->csr_dirty = true;
        pg->lin_valid = false;
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_set_poses(elm_ctx* ctx, elm_posegraph* pg, size_t first, size_t count, const double* poses16) {
    const char* what = "elm_posegraph_set_poses";
    if (!ctx || !pg || (count && !poses16)) return ELM_ERR_INVALID;
    if (count > (size_t)ELM_POSEGRAPH_MAX_NODES || !poses_finite(poses16, count)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!range_ok(first, count, pg->N)) return ELM_ERR_INVALID;
    if (!count) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(12 * count);
        for (size_t k = 0; k < count; ++k) pose_rows12(poses16 + 16 * k, &rows[12 * k]);
        pg->lin_valid = false;
        return join(ctx, st, hipMemcpyAsync(pg->poses + 12 * first, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st), what);
    });
}

extern "C" int elm_posegraph_get_poses(elm_ctx* ctx, const elm_posegraph* pg, size_t first, size_t count, double* poses16) {
    const char* what = "elm_posegraph_get_poses";
    if (!ctx || !pg || (count && !poses16)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!range_ok(first, count, pg->N)) return ELM_ERR_INVALID;
    if (!count) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(12 * count);
        int rc = join(ctx, st, hipMemcpyAsync(rows.data(), pg->poses + 12 * first, rows.size() * sizeof(double), hipMemcpyDeviceToHost, st), what);
        if (rc != ELM_OK) return rc;
        for (size_t k = 0; k < count; ++k) rows12_to_pose16(&rows[12 * k], poses16 + 16 * k);
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_set_fixed(elm_ctx* ctx, elm_posegraph* pg, size_t first, size_t count, const uint8_t* fixed) {
    const char* what = "elm_posegraph_set_fixed";
    if (!ctx || !pg || (count && !fixed)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!range_ok(first, count, pg->N)) return ELM_ERR_INVALID;
    if (!count) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<uint8_t> fx(count);
        for (size_t k = 0; k < count; ++k) fx[k] = fixed[k] ? 1 : 0;
        int rc = join(ctx, st, hipMemcpyAsync(pg->d_fixed + first, fx.data(), count, hipMemcpyHostToDevice, st), what);
        if (rc != ELM_OK) return rc;
        std::copy(fx.begin(), fx.end(), pg->fixed.begin() + (long)first);
        pg->lin_valid = false;
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_add_edges(elm_ctx* ctx, elm_posegraph* pg, const int32_t* i, const int32_t* j, const double* Z16, const double* info36,
                                       size_t n) {
    const char* what = "elm_posegraph_add_edges";
    if (!ctx || !pg || (n && (!i || !j || !Z16 || !info36))) return ELM_ERR_INVALID;
    if (n > (size_t)ELM_POSEGRAPH_MAX_EDGES || !poses_finite(Z16, n)) return ELM_ERR_INVALID;
    for (size_t k = 0; k < n; ++k) {
        if (i[k] < 0 || j[k] < 0 || i[k] == j[k]) return ELM_ERR_INVALID;
        if (!finite36(info36 + 36 * k) || !symmetric36(info36 + 36 * k)) return ELM_ERR_INVALID;
    }
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    for (size_t k = 0; k < n; ++k)
        if ((uint32_t)i[k] >= pg->N || (uint32_t)j[k] >= pg->N) return ELM_ERR_INVALID;
    if (n > (size_t)(pg->e_cap - pg->E)) return refuse_full(ctx, what, "edges", pg->E, n, pg->e_cap);
    if (!n) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(12 * n);
        for (size_t k = 0; k < n; ++k) pose_rows12(Z16 + 16 * k, &rows[12 * k]);
        pg->ei.reserve((size_t)pg->E + n);
        pg->ej.reserve((size_t)pg->E + n);
        pg->wr.reserve((size_t)pg->E + n);
        pg->wt.reserve((size_t)pg->E + n);
        const size_t E0 = pg->E;
        hipError_t e = hipMemcpyAsync(pg->d_ei + E0, i, n * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_ej + E0, j, n * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_Z + 12 * E0, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_info + 36 * E0, info36, 36 * n * sizeof(double), hipMemcpyHostToDevice, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        pg->ei.insert(pg->ei.end(), i, i + n);
        pg->ej.insert(pg->ej.end(), j, j + n);
        for (size_t k = 0; k < n; ++k) { // the two traces as the kernels form them
            const double* om = info36 + 36 * k;
            pg->wt.push_back(((om[0] + om[7]) + om[14]) / 3.0);
            pg->wr.push_back(((om[21] + om[28]) + om[35]) / 3.0);
        }
        pg->E += (uint32_t)n;
        pg->csr_dirty = true;
        pg->lin_valid = false;
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_linearize(elm_ctx* ctx, elm_posegraph* pg, double huber_k, elm_posegraph_linearize_stats* stats) {
    const char* what = "elm_posegraph_linearize";
    if (!ctx || !pg || !fin_ge0(huber_k)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) {
        pg->lin_valid = false;
        hipError_t e = queue_linearize(pg, st, huber_k, 0.0, false);
        if (e != hipSuccess) return dev_error(ctx, what, e);
        PgOut o{};
        int rc = cost_at(ctx, pg, st, pg->poses, huber_k, 1, o, what);
        if (rc != ELM_OK) return rc;
        pg->lin_valid = true;
        if (stats) {
            stats->chi2 = o.chi2;
            stats->cost = o.cost;
            stats->grad_inf_norm = o.grad_inf;
            stats->n_outliers = (int64_t)o.n_outliers;
        }
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_download_linearization(elm_ctx* ctx, const elm_posegraph* pg, double* r, double* A, double* B, double* s, double* w,
                                                    double* grad, double* diag) {
    const char* what = "elm_posegraph_download_linearization";
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!pg->lin_valid) return ELM_ERR_INVALID;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const size_t E = pg->E, N = pg->N, S = pg->e_cap;
        const PgDev& d = pg->dev;
        // component-major on the device, [E][components] for the caller: each component row comes down, then the transpose
        struct Part { double* dst; const double* src; size_t comps; };
        const Part parts[3] = {{r, d.r, 6}, {A, d.A, 36}, {B, d.B, 36}};
        std::vector<double> tmp[3];
        hipError_t e = hipSuccess;
        for (int k = 0; k < 3 && E; ++k) {
            if (!parts[k].dst) continue;
            tmp[k].resize(parts[k].comps * E);
            for (size_t c = 0; c < parts[k].comps && e == hipSuccess; ++c)
                e = hipMemcpyAsync(&tmp[k][c * E], parts[k].src + c * S, E * sizeof(double), hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess && s && E) e = hipMemcpyAsync(s, d.s, E * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && w && E) e = hipMemcpyAsync(w, d.w, E * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && grad && N) e = hipMemcpyAsync(grad, d.g, 6 * N * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && diag && N) e = hipMemcpyAsync(diag, d.Hd, 36 * N * sizeof(double), hipMemcpyDeviceToHost, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        for (int k = 0; k < 3 && E; ++k)
            if (parts[k].dst)
                for (size_t c = 0; c < parts[k].comps; ++c)
                    for (size_t q = 0; q < E; ++q) parts[k].dst[q * parts[k].comps + c] = tmp[k][c * E + q];
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_solve(elm_ctx* ctx, elm_posegraph* pg, double lambda, double pcg_rel_tol, int pcg_max_iterations, double* delta,
                                   elm_posegraph_solve_stats* stats) {
    const char* what = "elm_posegraph_solve";
    if (!ctx || !pg || !fin_ge0(lambda) || !fin_ge0(pcg_rel_tol) || pcg_max_iterations < 1) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!pg->lin_valid) return ELM_ERR_INVALID;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const PgDev& d = dev_view(pg);
        hipError_t e = launched([&] { launch_damping(st, d, chain(pg), lambda, 0); });
        if (e != hipSuccess) return dev_error(ctx, what, e);
        PcgStats s;
        int rc = run_pcg(ctx, pg, st, lambda, pcg_rel_tol, pcg_max_iterations, kPgDefaultCheckEvery, s, what);
        if (rc != ELM_OK) return rc;
        if (delta && pg->N) {
            rc = join(ctx, st, hipMemcpyAsync(delta, d.x, 6 * (size_t)pg->N * sizeof(double), hipMemcpyDeviceToHost, st), what);
            if (rc != ELM_OK) return rc;
        }
        if (stats) {
            stats->iterations = s.iterations;
            stats->converged = s.converged;
            stats->rel_residual = s.rel_residual;
        }
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_optimize(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_config* cfg, elm_posegraph_result* result,
                                      elm_posegraph_trace* trace, int trace_cap) {
    const char* what = "elm_posegraph_optimize";
    if (!ctx || !pg || !config_ok(cfg) || trace_cap < 0 || (trace_cap > 0 && !trace)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (gauge_free(pg)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": no fixed node (the gauge is free)");
        return ELM_ERR_INVALID;
    }
    return on_stream(ctx, what, [&](hipStream_t st) { return optimize_impl(ctx, pg, st, *cfg, result, trace_cap > 0 ? trace : nullptr, trace_cap); });
}

extern "C" void elm_posegraph_init_config_default(elm_posegraph_init_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->pcg_rel_tol = 1e-8;
    c->pcg_max_iterations = 50000;
    c->pcg_check_every = kPgDefaultCheckEvery;
    c->stages = ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS;
}

extern "C" int elm_posegraph_initialize(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_init_config* cfg, elm_posegraph_init_result* result,
                                        double* rows_out, double* v_out) {
    const char* what = "elm_posegraph_initialize";
    if (!ctx || !pg || !result || !init_config_ok(cfg)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) -> int { // the check's vectors and texts are allocated inside the guard too
        const std::string refusal = init_refusal(pg, cfg->stages);
        if (!refusal.empty()) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + refusal);
            return ELM_ERR_INVALID;
        }
        return initialize_impl(ctx, pg, st, *cfg, result, rows_out, v_out, nullptr, what);
    });
}

extern "C" void elm_posegraph_init_prior_config_default(elm_posegraph_init_prior_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    elm_posegraph_init_config_default(&c->base);
    c->align_min_ratio = 1e-4;
}

extern "C" int elm_posegraph_initialize_priors(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_init_prior_config* cfg,
                                               elm_posegraph_init_prior_result* result, double* rows_out, double* v_pre_out, double* v_out,
                                               double* align_out, int align_capacity) {
    const char* what = "elm_posegraph_initialize_priors";
    if (!ctx || !pg || !result || !cfg || !init_config_ok(&cfg->base)) return ELM_ERR_INVALID;
    if (!(isfinite(cfg->align_min_ratio) && cfg->align_min_ratio > 0.0) || align_capacity < 0) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    return on_stream(ctx, what, [&](hipStream_t st) -> int { // the plan's vectors and texts are allocated inside the guard too
        std::string refusal = init_edge_refusal(pg, cfg->base.stages);
        elm_pginit::Plan plan;
        if (refusal.empty()) {
            const elm_pginit::Graph g{pg->N,           pg->E,           pg->P,          pg->ei.data(), pg->ej.data(),
                                      pg->fixed.data(), pg->pnode.data(), pg->pwr.data(), pg->pwt.data()};
            plan = elm_pginit::plan(g, cfg->base.stages);
            refusal = plan.refusal;
        }
        if (!refusal.empty()) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + refusal);
            return ELM_ERR_INVALID;
        }
        elm_posegraph_init_prior_result R{};
        const InitPriorRun run{&plan, cfg->align_min_ratio, &R, v_pre_out, align_out, align_capacity};
        const int rc = initialize_impl(ctx, pg, st, cfg->base, &R.base, rows_out, v_out, &run, what);
        if (rc == ELM_OK) *result = R;
        return rc;
    });
}
