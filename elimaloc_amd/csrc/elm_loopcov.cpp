// elm_loopcov.cpp -- the loop consistency check with a propagated covariance (include/elimaloc_hip_loopcov.h): the
// argument checks, the one upload, the chain covariance, the pair kernels, and the greedy loop of elm_loops_host.hpp on the kernels of
// elm_k_loops.hip.  The launches are those of elm_k_loopcov.hip.  Each call owns one device allocation (elm_call.hpp's DeviceBlob) for its
// duration and keeps nothing afterwards.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "elm_dev_loopcov.hpp"
#include "elm_loops_host.hpp"

using namespace elm;
using namespace elm_query;
using namespace elm_loops_host;

namespace {

// the chain's preconditions that need no device: "" when they hold
std::string chain_refusal(const double* poses16, size_t n, const double* Q36, size_t q_count) {
    if (!poses16) return "a NULL poses";
    if (n < 1 || n > kLcMaxPoses) return "n outside 1 .. 2^20";
    if (q_count != 1 && q_count != n - 1) return "q_count must be 1 or n - 1";
    if (n > 1 && !Q36) return "a NULL Q";
    if (!poses_finite(poses16, n)) return "a non-finite pose";
    for (size_t v = 0; n > 1 && v < q_count; ++v) {
        if (!finite36(Q36 + 36 * v)) return "Q " + std::to_string(v) + ": non-finite";
        if (!symmetric36(Q36 + 36 * v)) return "Q " + std::to_string(v) + ": not symmetric";
    }
    return "";
}

std::string refusal(const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16, const double* Sigma36, size_t L,
                    const double* Q36, size_t q_count, const elm_loops_config* cfg, const void* result, const void* member_out,
                    const void* degree_out, const double* s_out) {
    if (!poses16 || !cfg || !result || !member_out || !degree_out) return "a NULL poses, config, result, member_out or degree_out";
    if (L && (!a || !b || !Z16 || !Sigma36)) return "a NULL a, b, Z or Sigma";
    if (n < 1 || n > kLcMaxPoses) return "n outside 1 .. 2^20";
    if (L > (size_t)ELM_LOOPS_MAX) return std::to_string(L) + " loops exceed ELM_LOOPS_MAX = " + std::to_string(ELM_LOOPS_MAX);
    if (s_out && L > (size_t)ELM_LOOPS_MAX_S) return "s_out with " + std::to_string(L) + " loops exceeds ELM_LOOPS_MAX_S = " + std::to_string(ELM_LOOPS_MAX_S);
    if (cfg->q_t != 0.0 || cfg->q_r != 0.0) return "q_t and q_r must be 0: the odometry is described by Q";
    if (!(isfinite(cfg->gamma) && cfg->gamma > 0.0)) return "gamma must be finite and > 0";
    if (cfg->steps_per_batch < 1) return "steps_per_batch must be >= 1";
    const std::string chain = chain_refusal(poses16, n, Q36, q_count);
    if (!chain.empty()) return chain;
    for (size_t k = 0; k < L; ++k) {
        const std::string loop = "loop " + std::to_string(k);
        if (a[k] < 0 || b[k] < 0 || (size_t)a[k] >= n || (size_t)b[k] >= n) return loop + ": an index outside 0 .. n - 1";
        if (a[k] == b[k]) return loop + ": a == b";
        if (!poses_finite(Z16 + 16 * k, 1)) return loop + ": a non-finite Z";
        if (!finite36(Sigma36 + 36 * k)) return loop + ": a non-finite Sigma";
        if (!symmetric36(Sigma36 + 36 * k)) return loop + ": Sigma is not symmetric";
        double S[kLcvSym];
        lcv_from36(Sigma36 + 36 * k, S);
        if (!lcv_ldl_ok(S)) return loop + ": Sigma is not positive definite (a pivot of its L D L^T is not > 0)";
    }
    return "";
}

struct ChainArrays {
    LcvChain c{};
    double *poses = nullptr, *Q = nullptr;
};

void carve_chain(ChainArrays& A, Carver& c, size_t n, size_t q_count) {
    const size_t nb = (n + kLcvScanBlock - 1) / kLcvScanBlock;
    A.poses = c.take<double>(12 * n);
    A.Q = c.take<double>(kLcvSym * q_count);
    A.c.Wc = c.take<double>(kLcvSym * n);
    A.c.tot = c.take<double>(kLcvSym * nb);
    A.c.n = (uint32_t)n;
    A.c.q_count = (uint32_t)q_count;
    A.c.nb = (uint32_t)nb;
    A.c.poses = A.poses;
    A.c.Q = A.Q;
}

// the host's copies of a chain's inputs as the kernels read them; they live until the stream is joined
struct ChainHost {
    std::vector<double> rows, q;
    ChainHost(const double* poses16, size_t n, const double* Q36, size_t q_count) : rows(12 * n), q(kLcvSym * q_count, 0.0) {
        for (size_t v = 0; v < n; ++v) pose_rows12(poses16 + 16 * v, &rows[12 * v]);
        for (size_t v = 0; n > 1 && v < q_count; ++v) lcv_from36(Q36 + 36 * v, &q[kLcvSym * v]);
    }
    hipError_t upload(hipStream_t st, const ChainArrays& A) const {
        hipError_t e = hipMemcpyAsync(A.poses, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(A.Q, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice, st);
        return e;
    }
};

int chain_impl(elm_ctx* ctx, hipStream_t st, const double* poses16, size_t n, const double* Q36, size_t q_count, double* W_out, double* S_out) {
    const char* what = "elm_loopcov_chain";
    const ChainHost host(poses16, n, Q36, q_count);
    ChainArrays A;
    double *d_W = nullptr, *d_S = nullptr;
    DeviceBlob blob(st);
    hipError_t e = blob.alloc([&](Carver& c) {
        carve_chain(A, c, n, q_count);
        d_W = c.take<double>(36 * n);
        d_S = S_out ? c.take<double>(36 * n) : nullptr;
    });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    e = host.upload(st, A);
    if (e == hipSuccess) e = launched([&] {
        launch_lcv_chain(st, A.c);
        launch_lcv_expand(st, A.c, d_W, d_S);
    });
    std::vector<double> W(36 * n), S(S_out ? 36 * n : 0); // the outputs stay untouched unless everything succeeds
    if (e == hipSuccess) e = hipMemcpyAsync(W.data(), d_W, W.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && S_out) e = hipMemcpyAsync(S.data(), d_S, S.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    const int rc = join(ctx, st, e, what);
    if (rc != ELM_OK) return rc;
    memcpy(W_out, W.data(), W.size() * sizeof(double));
    if (S_out) memcpy(S_out, S.data(), S.size() * sizeof(double));
    return ELM_OK;
}

struct LcvArrays {
    LcvDev d{};
    LcDev g{}; // the greedy kernels' view: adj and their own arrays
    int32_t *a = nullptr, *b = nullptr;
    double *Z = nullptr, *Sigma = nullptr;
};

void carve_loops(LcvArrays& A, Carver& c, size_t L, bool want_s) {
    const size_t W = lc_words((uint32_t)L), Lp = (L + 63) / 64 * 64;
    A.a = c.take<int32_t>(L);
    A.b = c.take<int32_t>(L);
    A.Z = c.take<double>(12 * L);
    A.Sigma = c.take<double>(kLcvSym * L);
    A.d.rec = c.take<double>(kLcvRecWords * Lp);
    A.d.adj = c.take<unsigned long long>(L * W);
    A.d.nanc = c.take<uint8_t>(L * W);
    A.d.nan_row = c.take<int32_t>(L);
    A.d.s = want_s ? c.take<double>(L * L) : nullptr;
    carve_greedy(A.g, c, L);
    A.g.adj = A.d.adj;
    A.d.L = (uint32_t)L;
    A.d.W = (uint32_t)W;
    A.d.Lp = (uint32_t)Lp;
    A.d.a = A.a;
    A.d.b = A.b;
    A.d.Z = A.Z;
    A.d.Sigma = A.Sigma;
}

int consistency_impl(elm_ctx* ctx, hipStream_t st, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16,
                     const double* Sigma36, size_t L, const double* Q36, size_t q_count, const elm_loops_config& c, elm_loopcov_result* result,
                     uint8_t* member_out, int32_t* degree_out, uint64_t* adj_out, double* s_out) {
    const char* what = "elm_loopcov_consistency";
    const size_t W = lc_words((uint32_t)L);
    const ChainHost host(poses16, n, Q36, q_count);
    std::vector<double> zrows(12 * L), sig(kLcvSym * L);
    for (size_t k = 0; k < L; ++k) {
        pose_rows12(Z16 + 16 * k, &zrows[12 * k]);
        lcv_from36(Sigma36 + 36 * k, &sig[kLcvSym * k]);
    }
    std::vector<unsigned long long> cand0;
    ChainArrays C;
    LcvArrays A;
    DeviceBlob blob(st);
    hipError_t e = blob.alloc([&](Carver& c) {
        carve_chain(C, c, n, q_count);
        carve_loops(A, c, L, s_out != nullptr);
    });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    StreamEvents<4> ev;
    e = host.upload(st, C);
    if (e == hipSuccess) e = hipMemcpyAsync(A.a, a, L * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.b, b, L * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.Z, zrows.data(), zrows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.Sigma, sig.data(), sig.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = greedy_reset(st, A.g, cand0);
    if (e == hipSuccess) e = ev.mark(st);
    if (e == hipSuccess) e = launched([&] { launch_lcv_chain(st, C.c); });
    if (e == hipSuccess) e = ev.mark(st);
    if (e == hipSuccess) e = launched([&] { launch_lcv_adjacency(st, C.c, A.d, c.gamma); });
    if (e == hipSuccess) e = ev.mark(st);
    LcState state{};
    if (e == hipSuccess) e = greedy_run(st, A.g, c.steps_per_batch, state);
    if (e == hipSuccess) e = ev.mark(st);
    std::vector<int32_t> deg(L), nan_row(L);
    std::vector<uint8_t> member(L);
    std::vector<unsigned long long> adj(adj_out ? L * W : 0);
    std::vector<double> s(s_out ? L * L : 0);
    if (e == hipSuccess) e = hipMemcpyAsync(deg.data(), A.g.deg0, L * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nan_row.data(), A.d.nan_row, L * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(member.data(), A.g.member, L, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && adj_out) e = hipMemcpyAsync(adj.data(), A.d.adj, adj.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && s_out) e = hipMemcpyAsync(s.data(), A.d.s, s.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    const int rc = join(ctx, st, e, what);
    if (rc != ELM_OK) return rc;
    int64_t sum = 0, nans = 0;
    for (size_t k = 0; k < L; ++k) {
        sum += deg[k]; // of step 0: every loop is a candidate, no -1
        nans += nan_row[k];
    }
    memcpy(degree_out, deg.data(), L * sizeof(int32_t));
    memcpy(member_out, member.data(), L);
    if (adj_out) memcpy(adj_out, adj.data(), adj.size() * sizeof(unsigned long long));
    if (s_out) memcpy(s_out, s.data(), s.size() * sizeof(double));
    result->size = (int32_t)state.size;
    result->steps = (int32_t)state.size; // every step before the stop makes one pick
    result->adjacent_pairs = sum / 2;
    result->non_finite_pairs = nans / 2;
    result->chain_ms = ev.ms(0);
    result->adjacency_ms = ev.ms(1);
    result->greedy_ms = ev.ms(2);
    return ELM_OK;
}

} // namespace

extern "C" int elm_loopcov_pair_terms(const double* T0, const double* Ta, const double* Tb, const double* Zk, const double* Sigma_k, const double* Tc,
                                      const double* Td, const double* Zl, const double* Sigma_l, const double* Ca, const double* Cb, double* e_out,
                                      double* cov_out, double* s_out) {
    const double* in[7] = {T0, Ta, Tb, Zk, Tc, Td, Zl};
    const double* mats[4] = {Sigma_k, Sigma_l, Ca, Cb};
    double P[7][12], Y[4][12], M[4][kLcvSym];
    for (int q = 0; q < 7; ++q) {
        if (!in[q] || !poses_finite(in[q], 1)) return ELM_ERR_INVALID;
        pose_rows12(in[q], P[q]);
    }
    for (int q = 0; q < 4; ++q) {
        if (!mats[q] || !finite36(mats[q])) return ELM_ERR_INVALID;
        lcv_from36(mats[q], M[q]);
    }
    if (!e_out || !cov_out || !s_out) return ELM_ERR_INVALID;
    const int ends[4] = {1, 2, 4, 5}; // a_k, b_k, a_l, b_l re-based on pose 0, as the per-loop kernel does
    for (int q = 0; q < 4; ++q) {
        double R[9], t[3];
        lc_between(P[0], P[ends[q]], R, t);
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) Y[q][r * 4 + j] = R[r * 3 + j];
            Y[q][r * 4 + 3] = t[r];
        }
    }
    double e[6], cov[kLcvSym];
    *s_out = lcv_pair(Y[0], Y[1], P[3], M[0], Y[2], Y[3], P[6], M[1], M[2], M[3], e, cov);
    memcpy(e_out, e, sizeof(e));
    lcv_to36(cov, cov_out);
    return ELM_OK;
}

extern "C" int elm_loopcov_chain(elm_ctx* ctx, const double* poses16, size_t n, const double* Q36, size_t q_count, double* W_out, double* S_out) {
    const char* what = "elm_loopcov_chain";
    if (!ctx) return ELM_ERR_INVALID;
    const int rc = check_call(ctx, what);
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, what, [&]() -> int {
        const std::string why = !W_out ? std::string("a NULL W_out") : chain_refusal(poses16, n, Q36, q_count);
        if (!why.empty()) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + why);
            return ELM_ERR_INVALID;
        }
        return on_stream(ctx, what, [&](hipStream_t st) { return chain_impl(ctx, st, poses16, n, Q36, q_count, W_out, S_out); });
    });
}

extern "C" int elm_loopcov_consistency(elm_ctx* ctx, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16,
                                       const double* Sigma36, size_t L, const double* Q36, size_t q_count, const elm_loops_config* cfg,
                                       elm_loopcov_result* result, uint8_t* member_out, int32_t* degree_out, uint64_t* adj_out, double* s_out) {
    const char* what = "elm_loopcov_consistency";
    if (!ctx) return ELM_ERR_INVALID;
    const int rc = check_call(ctx, what);
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, what, [&]() -> int {
        const std::string why = refusal(poses16, n, a, b, Z16, Sigma36, L, Q36, q_count, cfg, result, member_out, degree_out, s_out);
        if (!why.empty()) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + why);
            return ELM_ERR_INVALID;
        }
        if (!L) {
            memset(result, 0, sizeof(*result));
            return ELM_OK;
        }
        return on_stream(ctx, what, [&](hipStream_t st) {
            return consistency_impl(ctx, st, poses16, n, a, b, Z16, Sigma36, L, Q36, q_count, *cfg, result, member_out, degree_out, adj_out, s_out);
        });
    });
}
