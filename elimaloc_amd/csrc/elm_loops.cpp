// elm_loops.cpp -- the loop consistency check (include/elimaloc_hip_loops.h): the argument checks, the one upload
// of poses, loops and variances, the pair kernel, and the greedy loop (elm_loops_host.hpp) that queues steps_per_batch steps between two
// reads of the device's state (elm_call.hpp's run_batched, as the pose graph's conjugate gradients are).  The launches are those of
// elm_k_loops.hip.  The call owns one device allocation (DeviceBlob) for its duration and keeps nothing afterwards.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_loops_host.hpp"

using namespace elm;
using namespace elm_query;
using namespace elm_loops_host;

extern "C" void elm_loops_config_default(elm_loops_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->gamma = 16.81;
    c->steps_per_batch = 32;
}

extern "C" int elm_loops_pair_terms(const double* Ta, const double* Tb, const double* Zk, const double* Tc, const double* Td, const double* Zl,
                                    double* e_out) {
    const double* in[6] = {Ta, Tb, Zk, Tc, Td, Zl};
    double P[6][12];
    for (int q = 0; q < 6; ++q) {
        if (!in[q] || !poses_finite(in[q], 1)) return ELM_ERR_INVALID;
        pose_rows12(in[q], P[q]);
    }
    if (!e_out) return ELM_ERR_INVALID;
    double e[6];
    lc_pair_e(P[0], P[1], P[2], P[3], P[4], P[5], e);
    memcpy(e_out, e, sizeof(e));
    return ELM_OK;
}

namespace {

// the preconditions that need no device: "" when they hold, else the text for elm_last_error
std::string refusal(const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16, const double* var_t, const double* var_r,
                    size_t L, const elm_loops_config* cfg, const void* result, const void* member_out, const void* degree_out, const double* s_out) {
    if (!poses16 || !cfg || !result || !member_out || !degree_out) return "a NULL poses, config, result, member_out or degree_out";
    if (L && (!a || !b || !Z16 || !var_t || !var_r)) return "a NULL a, b, Z, var_t or var_r";
    if (n < 1 || n > kLcMaxPoses) return "n outside 1 .. 2^20";
    if (L > (size_t)ELM_LOOPS_MAX) return std::to_string(L) + " loops exceed ELM_LOOPS_MAX = " + std::to_string(ELM_LOOPS_MAX);
    if (s_out && L > (size_t)ELM_LOOPS_MAX_S) return "s_out with " + std::to_string(L) + " loops exceeds ELM_LOOPS_MAX_S = " + std::to_string(ELM_LOOPS_MAX_S);
    if (!fin_ge0(cfg->q_t) || !fin_ge0(cfg->q_r)) return "q_t and q_r must be finite and >= 0";
    if (!(isfinite(cfg->gamma) && cfg->gamma > 0.0)) return "gamma must be finite and > 0";
    if (cfg->steps_per_batch < 1) return "steps_per_batch must be >= 1";
    if (!poses_finite(poses16, n)) return "a non-finite pose";
    for (size_t k = 0; k < L; ++k) {
        const std::string loop = "loop " + std::to_string(k);
        if (a[k] < 0 || b[k] < 0 || (size_t)a[k] >= n || (size_t)b[k] >= n) return loop + ": an index outside 0 .. n - 1";
        if (a[k] == b[k]) return loop + ": a == b";
        if (!poses_finite(Z16 + 16 * k, 1)) return loop + ": a non-finite Z";
        if (!isfinite(var_t[k]) || !isfinite(var_r[k])) return loop + ": a non-finite variance";
        if (!(var_t[k] > 0.0) || !(var_r[k] > 0.0)) return loop + ": a variance <= 0";
    }
    return "";
}

struct LcArrays {
    LcDev d{};
    double* poses = nullptr;
    int32_t *a = nullptr, *b = nullptr;
    double *Z = nullptr, *var_t = nullptr, *var_r = nullptr;
};

void carve(LcArrays& A, Carver& c, size_t n, size_t L, bool want_s) {
    const size_t W = lc_words((uint32_t)L);
    A.poses = c.take<double>(12 * n);
    A.a = c.take<int32_t>(L);
    A.b = c.take<int32_t>(L);
    A.Z = c.take<double>(12 * L);
    A.var_t = c.take<double>(L);
    A.var_r = c.take<double>(L);
    A.d.adj = c.take<unsigned long long>(L * W);
    A.d.s = want_s ? c.take<double>(L * L) : nullptr;
    carve_greedy(A.d, c, L);
    A.d.n = (uint32_t)n;
    A.d.poses = A.poses;
    A.d.a = A.a;
    A.d.b = A.b;
    A.d.Z = A.Z;
    A.d.var_t = A.var_t;
    A.d.var_r = A.var_r;
}

int consistency_impl(elm_ctx* ctx, hipStream_t st, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16,
                     const double* var_t, const double* var_r, size_t L, const elm_loops_config& c, elm_loops_result* result, uint8_t* member_out,
                     int32_t* degree_out, uint64_t* adj_out, double* s_out) {
    const char* what = "elm_loops_consistency";
    const size_t W = lc_words((uint32_t)L);
    std::vector<double> rows(12 * n), zrows(12 * L);
    for (size_t v = 0; v < n; ++v) pose_rows12(poses16 + 16 * v, &rows[12 * v]);
    for (size_t k = 0; k < L; ++k) pose_rows12(Z16 + 16 * k, &zrows[12 * k]);
    std::vector<unsigned long long> cand0;
    LcArrays A;
    DeviceBlob blob(st);
    hipError_t e = blob.alloc([&](Carver& c) { carve(A, c, n, L, s_out != nullptr); });
    if (e != hipSuccess) return dev_error(ctx, what, e);
    const LcDev& d = A.d;
    StreamEvents<3> ev;
    e = hipMemcpyAsync(A.poses, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.a, a, L * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.b, b, L * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.Z, zrows.data(), zrows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.var_t, var_t, L * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(A.var_r, var_r, L * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = greedy_reset(st, d, cand0);
    if (e == hipSuccess) e = ev.mark(st);
    if (e == hipSuccess) e = launched([&] { launch_lc_adjacency(st, d, c.q_t, c.q_r, c.gamma); });
    if (e == hipSuccess) e = ev.mark(st);
    LcState state{};
    if (e == hipSuccess) e = greedy_run(st, d, c.steps_per_batch, state);
    if (e == hipSuccess) e = ev.mark(st);
    std::vector<int32_t> deg(L);
    std::vector<uint8_t> member(L);
    if (e == hipSuccess) e = hipMemcpyAsync(deg.data(), d.deg0, L * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(member.data(), d.member, L, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && adj_out) e = hipMemcpyAsync(adj_out, d.adj, L * W * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && s_out) e = hipMemcpyAsync(s_out, d.s, L * L * sizeof(double), hipMemcpyDeviceToHost, st);
    const int rc = join(ctx, st, e, what);
    if (rc != ELM_OK) return rc;
    int64_t sum = 0;
    for (size_t k = 0; k < L; ++k) sum += deg[k]; // of step 0: every loop is a candidate, no -1
    memcpy(degree_out, deg.data(), L * sizeof(int32_t));
    memcpy(member_out, member.data(), L);
    result->size = (int32_t)state.size;
    result->steps = (int32_t)state.size; // every step before the stop makes one pick
    result->adjacent_pairs = sum / 2;
    result->adjacency_ms = ev.ms(0);
    result->greedy_ms = ev.ms(1);
    return ELM_OK;
}

} // namespace

extern "C" int elm_loops_consistency(elm_ctx* ctx, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16,
                                     const double* var_t, const double* var_r, size_t L, const elm_loops_config* cfg, elm_loops_result* result,
                                     uint8_t* member_out, int32_t* degree_out, uint64_t* adj_out, double* s_out) {
    const char* what = "elm_loops_consistency";
    if (!ctx) return ELM_ERR_INVALID;
    const int rc = check_call(ctx, what);
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, what, [&]() -> int {
        const std::string why = refusal(poses16, n, a, b, Z16, var_t, var_r, L, cfg, result, member_out, degree_out, s_out);
        if (!why.empty()) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": " + why);
            return ELM_ERR_INVALID;
        }
        if (!L) {
            memset(result, 0, sizeof(*result));
            return ELM_OK;
        }
        return on_stream(ctx, what, [&](hipStream_t st) { // (the preconditions above need no device: they come first)
            return consistency_impl(ctx, st, poses16, n, a, b, Z16, var_t, var_r, L, *cfg, result, member_out, degree_out, adj_out, s_out);
        });
    });
}
