// elm_pgcov.cpp -- the pose graph's marginal and relative covariances (include/elimaloc_hip_posegraph_cov.h): the
// argument checks, the scratch of one call (one DeviceBlob carved by cov_carve, as many column groups as fit under the cap), the passes
// -- each a run_batched of the column conjugate gradients, as run_pcg of elm_pgraph.cpp is -- the gather of the requested blocks, and
// the host's sums of the relative covariance.  The object is elm_pgraph_host.hpp's; the launches are those of elm_k_pgcov.hip.
// Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_pgraph_host.hpp"

using namespace elm;
using namespace elm_query;
using namespace elm_pgraph_host;

extern "C" void elm_posegraph_cov_config_default(elm_posegraph_cov_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->lambda = 0.0;
    c->pcg_rel_tol = 1e-10;
    c->pcg_max_iterations = 20000;
    c->pcg_check_every = kPgDefaultCheckEvery;
    c->scratch_bytes = 0;
}

namespace {

constexpr uint64_t kPgcovDefaultScratch = 2ull << 30;
constexpr size_t kPgcovMaxPairs = (size_t)1 << 25;

bool cov_config_ok(const elm_posegraph_cov_config* c) {
    return c && fin_ge0(c->lambda) && fin_ge0(c->pcg_rel_tol) && c->pcg_max_iterations >= 1 && c->pcg_check_every >= 1;
}

// The refusals that need the object, in the order of the header: ELM_OK when there is none.
int cov_refusal(elm_ctx* ctx, const elm_posegraph* pg, const elm_posegraph_cov_config& c, const char* what) {
    if (!pg->lin_valid) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": no valid linearization (linearize or optimize first)");
        return ELM_ERR_INVALID;
    }
    if (c.lambda == 0.0 && gauge_free(pg)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": no fixed node (the gauge is free)");
        return ELM_ERR_INVALID;
    }
    return ELM_OK;
}

bool nodes_in_range(const int32_t* v, size_t n, uint32_t N) {
    for (size_t k = 0; k < n; ++k)
        if (v[k] < 0 || (uint32_t)v[k] >= N) return false;
    return true;
}

// The scratch of one call, one allocation: the vectors and words of up to G groups (the words' bytes are [word_off, word_off +
// word_bytes) of it), the request's tables and the download buffer.
struct CovArrays {
    PgCovDev v{};
    int32_t *cols = nullptr, *row = nullptr;
    uint32_t* ci = nullptr;
    double* out = nullptr;
    size_t word_off = 0, word_bytes = 0;
};

CovArrays cov_carve(Carver& c, bool with_chain, size_t N, size_t G, size_t m, size_t P) {
    CovArrays a;
    PgCovDev& v = a.v;
    const size_t tile = G * N * 6 * kPgcovLanes, cols = G * kPgcovLanes, slots = (size_t)pgcov_blocks((uint32_t)N) * cols;
    v.x = c.take<double>(tile);
    v.r = c.take<double>(tile);
    v.z = c.take<double>(tile);
    v.p = c.take<double>(tile);
    v.q = c.take<double>(tile);
    if (with_chain) { // the apply's y and be: every level padded to whole segments, as the factor's arrays are
        PgcLevel lv[kPgcMaxLevels];
        const uint32_t nl = pgc_levels((uint32_t)N, lv);
        v.y_pad = lv[nl - 1].off + lv[nl - 1].nseg * kPgcSeg;
        v.y_segs = lv[nl - 1].soff + lv[nl - 1].nseg;
        v.y = c.take<double>(G * v.y_pad * 6 * kPgcovLanes);
        v.be = c.take<double>(G * v.y_segs * 6 * kPgcovLanes);
    }
    v.slot_pq = c.take<double>(slots);
    v.slot_rz = c.take<double>(slots);
    a.word_off = c.off;
    v.alpha = c.take<double>(cols);
    v.beta = c.take<double>(cols);
    v.rz0 = c.take<double>(cols);
    v.rzf = c.take<double>(cols);
    v.rz = c.take<double>(2 * cols);
    v.stop = c.take<uint32_t>(2 * cols);
    v.iters = c.take<uint32_t>(cols);
    v.converged = c.take<uint32_t>(cols);
    v.gstop = c.take<uint32_t>(2 * G);
    v.all_stop = c.take<uint32_t>(2);
    a.word_bytes = c.off - a.word_off;
    v.col_nodes = a.cols = c.take<int32_t>(m);
    a.ci = c.take<uint32_t>(P ? P : 1);
    a.row = c.take<int32_t>(P ? P : 1);
    a.out = c.take<double>(36 * (P ? P : 1));
    return a;
}

// The blocks Sigma(row[k], col_nodes[ci[k]]) of P pairs as solved into blocks [P][36], the per-column counts into iters and conv [6 m]
// (either may be null).  The caller has checked every index, the config, the linearization and the preconditioner; m >= 1, N >= 1.
int cov_core(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, const elm_posegraph_cov_config& cfg, const int32_t* col_nodes, size_t m,
             const std::vector<uint32_t>& ci, const std::vector<int32_t>& row, double* blocks, int32_t* iters, uint8_t* conv, elm_posegraph_cov_stats& S,
             const char* what) {
    const PgDev& d = dev_view(pg);
    const size_t N = pg->N, P = ci.size(), n_cols = 6 * m, G_all = (n_cols + kPgcovLanes - 1) / kPgcovLanes;
    hipError_t e = ensure_csr(pg, st);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    const PgcDev* const ch = chain(pg);
    const bool with_chain = ch != nullptr;
    // the groups of a pass: as many as fit under the cap, one at the least
    CovArrays a;
    auto bytes_for = [&](size_t G) { return carved_size([&](Carver& c) { a = cov_carve(c, with_chain, N, G, m, P); }); };
    const uint64_t cap = cfg.scratch_bytes ? cfg.scratch_bytes : kPgcovDefaultScratch;
    const size_t fixed_bytes = bytes_for(0), per_group = bytes_for(1) - fixed_bytes;
    size_t G = cap > fixed_bytes ? (size_t)((cap - fixed_bytes) / per_group) : 0;
    G = std::max<size_t>(1, std::min<size_t>({G, G_all, (size_t)kPgcovMaxGroups}));
    while (G > 1 && bytes_for(G) > cap) --G; // (the arrays' alignment padding)
    const size_t total = bytes_for(G);
    DeviceBlob scratch(st);
    e = scratch.alloc([&](Carver& c) { a = cov_carve(c, with_chain, N, G, m, P); });
    if (e != hipSuccess) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": " + std::to_string(total) + " bytes of scratch: " + hipGetErrorString(e));
        return ELM_ERR_DEVICE;
    }
    PgCovDev& v = a.v;
    StreamEvents<2> ev;
    e = hipMemcpyAsync(a.cols, col_nodes, m * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && P) e = hipMemcpyAsync(a.ci, ci.data(), P * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && P) e = hipMemcpyAsync(a.row, row.data(), P * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && P) e = hipMemsetAsync(a.out, 0, 36 * P * sizeof(double), st);
    if (e == hipSuccess) e = ev.mark(st);
    if (e == hipSuccess) e = launched([&] { launch_damping(st, d, ch, cfg.lambda, 0); });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    S = elm_posegraph_cov_stats{};
    S.n_columns = (int32_t)n_cols;
    S.scratch_bytes = total;
    v.n_cols = (uint32_t)n_cols;
    std::vector<uint32_t> h_it, h_cv;
    std::vector<double> h_rz0, h_rzf;
    for (size_t g0 = 0; g0 < G_all; g0 += G) {
        v.G = (uint32_t)std::min(G, G_all - g0);
        v.col0 = (uint32_t)(g0 * kPgcovLanes);
        const size_t cols = (size_t)v.G * kPgcovLanes;
        // the vectors of the pass's groups are the first v.G tiles of each array: zero them array by array
        const size_t tile_bytes = cols * N * 6 * sizeof(double);
        for (double* vec : {v.x, v.r, v.z, v.p, v.q})
            if (e == hipSuccess) e = hipMemsetAsync(vec, 0, tile_bytes, st);
        if (e == hipSuccess) e = hipMemsetAsync(scratch.p + a.word_off, 0, a.word_bytes, st);
        if (e == hipSuccess) e = launched([&] { launch_pgcov_begin(st, d, v, ch, cfg.pcg_rel_tol); });
        struct AllStop {
            uint32_t word[2];
        } all_stop{};
        if (e == hipSuccess)
            e = run_batched(
                st, cfg.pcg_check_every, cfg.pcg_max_iterations, [&](uint32_t it) { launch_pgcov_iteration(st, d, v, ch, cfg.lambda, cfg.pcg_rel_tol, it); },
                (const AllStop*)v.all_stop, &all_stop, [&](uint32_t it) { return all_stop.word[it & 1u] != 0; });
        if (e == hipSuccess) e = launched([&] { launch_pgcov_gather(st, d, v, a.ci, a.row, (uint32_t)P, a.out); });
        h_it.resize(cols);
        h_cv.resize(cols);
        h_rz0.resize(cols);
        h_rzf.resize(cols);
        if (e == hipSuccess) e = hipMemcpyAsync(h_it.data(), v.iters, cols * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_cv.data(), v.converged, cols * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_rz0.data(), v.rz0, cols * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_rzf.data(), v.rzf, cols * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return dev_error(ctx, what, e);
        for (size_t k = 0; k < cols && v.col0 + k < n_cols; ++k) {
            const size_t j = v.col0 + k;
            if (iters) iters[j] = (int32_t)h_it[k];
            if (conv) conv[j] = h_cv[k] ? 1 : 0;
            S.n_converged += h_cv[k] ? 1 : 0;
            S.iterations_max = std::max(S.iterations_max, (int32_t)h_it[k]);
            if (h_rz0[k] > 0.0) S.rel_residual_max = std::max(S.rel_residual_max, sqrt(h_rzf[k]) / sqrt(h_rz0[k]));
        }
        ++S.passes;
    }
    e = ev.mark(st);
    if (e == hipSuccess && P) e = hipMemcpyAsync(blocks, a.out, 36 * P * sizeof(double), hipMemcpyDeviceToHost, st);
    const int rc = join(ctx, st, e, what);
    S.ms_device = ev.ms(0);
    return rc;
}

} // namespace

extern "C" int elm_posegraph_covariance(elm_ctx* ctx, elm_posegraph* pg, const int32_t* col_nodes, size_t m, const int32_t* row_nodes, size_t n_rows,
                                        const elm_posegraph_cov_config* cfg, double* diag36, double* cross36, int32_t* iterations, uint8_t* converged,
                                        elm_posegraph_cov_stats* stats) {
    const char* what = "elm_posegraph_covariance";
    if (!ctx || !pg || !cov_config_ok(cfg) || (m && !col_nodes) || (n_rows && !row_nodes) || (cross36 && !n_rows)) return ELM_ERR_INVALID;
    if (m > (size_t)ELM_POSEGRAPH_MAX_NODES || n_rows > (size_t)ELM_POSEGRAPH_MAX_NODES) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!nodes_in_range(col_nodes, m, pg->N) || !nodes_in_range(row_nodes, n_rows, pg->N)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": a node index outside the graph's " + std::to_string(pg->N) + " nodes");
        return ELM_ERR_INVALID;
    }
    return on_stream(ctx, what, [&](hipStream_t st) -> int {
        int rc = cov_refusal(ctx, pg, *cfg, what);
        if (rc != ELM_OK) return rc;
        elm_posegraph_cov_stats S{};
        if (!m) {
            if (stats) *stats = S;
            return ELM_OK;
        }
        const size_t per_col = (diag36 ? 1 : 0) + (cross36 ? n_rows : 0), P = m * per_col;
        if (P > kPgcovMaxPairs) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + std::to_string(P) + " blocks requested, more than 2^25");
            return ELM_ERR_UNSUPPORTED;
        }
        // the pairs: per column node its own block (with diag36), then its row blocks
        std::vector<uint32_t> ci(P);
        std::vector<int32_t> row(P);
        for (size_t i = 0, k = 0; i < m; ++i) {
            if (diag36) ci[k] = (uint32_t)i, row[k++] = col_nodes[i];
            for (size_t q = 0; cross36 && q < n_rows; ++q) ci[k] = (uint32_t)i, row[k++] = row_nodes[q];
        }
        std::vector<double> blocks(36 * P);
        rc = cov_core(ctx, pg, st, *cfg, col_nodes, m, ci, row, blocks.data(), iterations, converged, S, what);
        if (rc != ELM_OK) return rc;
        for (size_t i = 0; i < m; ++i) {
            const double* B = &blocks[36 * i * per_col];
            if (diag36) {
                for (int a = 0; a < 6; ++a)
                    for (int b = 0; b < 6; ++b) diag36[36 * i + a * 6 + b] = 0.5 * (B[a * 6 + b] + B[b * 6 + a]);
                B += 36;
            }
            if (cross36) memcpy(cross36 + 36 * i * n_rows, B, 36 * n_rows * sizeof(double));
        }
        if (stats) *stats = S;
        return ELM_OK;
    });
}

extern "C" int elm_posegraph_relative_covariance(elm_ctx* ctx, elm_posegraph* pg, const int32_t* a, const int32_t* b, size_t L,
                                                 const elm_posegraph_cov_config* cfg, double* cov36, elm_posegraph_cov_stats* stats) {
    const char* what = "elm_posegraph_relative_covariance";
    if (!ctx || !pg || !cov_config_ok(cfg) || (L && (!a || !b || !cov36)) || L > kPgcovMaxPairs / 4) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!nodes_in_range(a, L, pg->N) || !nodes_in_range(b, L, pg->N)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": a node index outside the graph's " + std::to_string(pg->N) + " nodes");
        return ELM_ERR_INVALID;
    }
    for (size_t k = 0; k < L; ++k)
        if (a[k] == b[k]) return ELM_ERR_INVALID;
    return on_stream(ctx, what, [&](hipStream_t st) -> int {
        int rc = cov_refusal(ctx, pg, *cfg, what);
        if (rc != ELM_OK) return rc;
        elm_posegraph_cov_stats S{};
        if (!L) {
            if (stats) *stats = S;
            return ELM_OK;
        }
        // the columns: the unique nodes of a and b, ascending
        std::vector<int32_t> nodes(a, a + L);
        nodes.insert(nodes.end(), b, b + L);
        std::sort(nodes.begin(), nodes.end());
        nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
        auto at = [&](int32_t v) { return (uint32_t)(std::lower_bound(nodes.begin(), nodes.end(), v) - nodes.begin()); };
        // per pair the blocks Sigma_aa, Sigma_ba (columns of a), Sigma_ab, Sigma_bb (columns of b)
        std::vector<uint32_t> ci(4 * L);
        std::vector<int32_t> row(4 * L);
        for (size_t k = 0; k < L; ++k) {
            const uint32_t ia = at(a[k]), ib = at(b[k]);
            ci[4 * k] = ia, row[4 * k] = a[k];
            ci[4 * k + 1] = ia, row[4 * k + 1] = b[k];
            ci[4 * k + 2] = ib, row[4 * k + 2] = a[k];
            ci[4 * k + 3] = ib, row[4 * k + 3] = b[k];
        }
        std::vector<double> blocks(36 * 4 * L), rows(12 * nodes.size());
        hipError_t e = hipSuccess;
        for (size_t u = 0; u < nodes.size() && e == hipSuccess; ++u)
            e = hipMemcpyAsync(&rows[12 * u], pg->poses + 12 * (size_t)nodes[u], 12 * sizeof(double), hipMemcpyDeviceToHost, st);
        rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        rc = cov_core(ctx, pg, st, *cfg, nodes.data(), nodes.size(), ci, row, blocks.data(), nullptr, nullptr, S, what);
        if (rc != ELM_OK) return rc;
        for (size_t k = 0; k < L; ++k) {
            const double *Pa = &rows[12 * at(a[k])], *Pb = &rows[12 * at(b[k])];
            // Z = T_a^-1 T_b on pose rows
            double Ra[9], ta[3], Rb[9], tb[3], RZ[9], tZ[3], PZ[12], r[6], A[36], B[36];
            pg_split(Pa, Ra, ta);
            pg_split(Pb, Rb, tb);
            const double dt[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
            pg_mul3_at(Ra, Rb, RZ);
            pg_mul3_atv(Ra, dt, tZ);
            for (int q = 0; q < 3; ++q) {
                PZ[q * 4] = RZ[q * 3], PZ[q * 4 + 1] = RZ[q * 3 + 1], PZ[q * 4 + 2] = RZ[q * 3 + 2];
                PZ[q * 4 + 3] = tZ[q];
            }
            pg_edge_terms(Pa, Pb, PZ, r, A, B);
            const double *Saa = &blocks[36 * (4 * k)], *Sba = Saa + 36, *Sab = Saa + 72, *Sbb = Saa + 108;
            // X S Y^T for the four terms, added in the order of the header
            auto sandwich = [](const double* X, const double* Sg, const double* Y, double* out) {
                double XS[36];
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) XS[i * 6 + j] = pg_mm6(X, Sg, i, j);
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) out[i * 6 + j] = pg_mmt6(XS, Y, i, j);
            };
            double T1[36], T2[36], T3[36], T4[36], Csum[36];
            sandwich(A, Saa, A, T1);
            sandwich(A, Sab, B, T2);
            sandwich(B, Sba, A, T3);
            sandwich(B, Sbb, B, T4);
            for (int i = 0; i < 36; ++i) Csum[i] = ((T1[i] + T2[i]) + T3[i]) + T4[i];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) cov36[36 * k + i * 6 + j] = 0.5 * (Csum[i * 6 + j] + Csum[j * 6 + i]);
        }
        if (stats) *stats = S;
        return ELM_OK;
    });
}
