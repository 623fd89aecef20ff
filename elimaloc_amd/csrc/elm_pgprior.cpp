// elm_pgprior.cpp -- the pose graph's priors (include/elimaloc_hip_posegraph_prior.h): the second device
// allocation of the object (made by elm_posegraph_reserve_priors, so that a graph without priors costs nothing more), the argument
// checks, the rows of the nodes that have priors (a stable counting sort of the priors by node, redone when the prior set has changed)
// and the downloads.  The object is elm_pgraph_host.hpp's; elm_pgraph.cpp queues the priors' launches (elm_k_pgprior.hip) with the
// linearization and the cost.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "elm_pgraph_host.hpp"

using namespace elm;
using namespace elm_query;
using namespace elm_pgraph_host;

namespace {

// the device arrays of the priors from their one allocation
void carve_priors(elm_posegraph* pg, Carver& c) {
    const size_t Pc = pg->p_cap;
    PgPriorDev& p = pg->prior;
    pg->d_pnode = c.take<int32_t>(Pc);
    pg->d_pZ = c.take<double>(12 * Pc);
    pg->d_plever = c.take<double>(3 * Pc);
    pg->d_pinfo = c.take<double>(36 * Pc);
    pg->d_prow_node = c.take<uint32_t>(Pc);
    pg->d_prow_first = c.take<uint32_t>(Pc + 1);
    pg->d_porder = c.take<uint32_t>(Pc);
    p.r = c.take<double>(6 * Pc);
    p.J = c.take<double>(36 * Pc);
    p.s = c.take<double>(Pc);
    p.w = c.take<double>(Pc);
    p.g = c.take<double>(6 * Pc);
    p.H = c.take<double>(36 * Pc);
    p.part_cost = c.take<double>(3 * (size_t)pg_blocks((uint32_t)Pc));
    p.p_stride = (uint32_t)Pc;
    p.node = pg->d_pnode;
    p.Z = pg->d_pZ;
    p.lever = pg->d_plever;
    p.info = pg->d_pinfo;
    p.row_node = pg->d_prow_node;
    p.row_first = pg->d_prow_first;
    p.order = pg->d_porder;
}

int reserve_impl(elm_ctx* ctx, elm_posegraph* pg, hipStream_t st, uint32_t cap, const char* what) {
    pg->p_cap = cap;
    DeviceBlob blob(st);
    hipError_t e = blob.alloc([&](Carver& c) { carve_priors(pg, c); });
    if (e == hipSuccess) e = hipMemsetAsync(blob.p, 0, blob.bytes, st); // (on the context's stream and joined, as the object's own)
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        pg->p_cap = 0;
        pg->prior = PgPriorDev{};
        return dev_error(ctx, what, e);
    }
    pg->prior_blob = blob.release();
    return ELM_OK;
}

void invalidate(elm_posegraph* pg) {
    pg->prior_rows_dirty = true;
    pg->lin_valid = false;
}

} // namespace

// The rows of the current prior set: the nodes that have priors in ascending order, each with its priors in ascending prior index.
hipError_t elm_pgraph_host::ensure_prior_rows(elm_posegraph* pg, hipStream_t st) {
    if (!pg->P || !pg->prior_rows_dirty) return hipSuccess;
    const uint32_t P = pg->P, N = pg->N;
    std::vector<uint32_t> count((size_t)N + 1, 0u);
    for (uint32_t q = 0; q < P; ++q) ++count[(size_t)pg->pnode[q] + 1];
    std::vector<uint32_t> row_node, row_first;
    for (uint32_t v = 0; v < N; ++v) {
        if (count[v + 1]) {
            row_node.push_back(v);
            row_first.push_back(count[v]);
        }
        count[v + 1] += count[v];
    }
    row_first.push_back(P);
    std::vector<uint32_t> order(P);
    for (uint32_t q = 0; q < P; ++q) order[count[pg->pnode[q]]++] = q; // priors ascending: every row ends up ascending
    hipError_t e = hipMemcpyAsync(pg->d_prow_node, row_node.data(), row_node.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pg->d_prow_first, row_first.data(), row_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pg->d_porder, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st); // the host vectors are read until here
    if (e == hipSuccess) {
        pg->prior.n_rows = (uint32_t)row_node.size();
        pg->prior_rows_dirty = false;
    }
    return e;
}

extern "C" int elm_posegraph_prior_terms(const double* T16, const double* Z16, const double* lever3, double* r, double* J) {
    if (!T16 || !Z16 || !poses_finite(T16, 1) || !poses_finite(Z16, 1) || (lever3 && !finite3(lever3))) return ELM_ERR_INVALID;
    const double zero[3] = {0.0, 0.0, 0.0};
    double Pv[12], PZ[12], rr[6], JJ[36];
    pose_rows12(T16, Pv);
    pose_rows12(Z16, PZ);
    pg_prior_terms(Pv, PZ, lever3 ? lever3 : zero, rr, JJ);
    if (r) memcpy(r, rr, sizeof(rr));
    if (J) memcpy(J, JJ, sizeof(JJ));
    return ELM_OK;
}

extern "C" int elm_posegraph_reserve_priors(elm_ctx* ctx, elm_posegraph* pg, int capacity) {
    const char* what = "elm_posegraph_reserve_priors";
    if (!ctx || !pg || capacity < 1 || capacity > ELM_POSEGRAPH_MAX_PRIORS) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (pg->p_cap) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": the priors' capacity is already " + std::to_string(pg->p_cap) + " (once per object)");
        return ELM_ERR_INVALID;
    }
    return on_stream(ctx, what, [&](hipStream_t st) { return reserve_impl(ctx, pg, st, (uint32_t)capacity, what); });
}

extern "C" int elm_posegraph_add_priors(elm_ctx* ctx, elm_posegraph* pg, const int32_t* node, const double* Z16, const double* lever3,
                                        const double* info36, size_t n) {
    const char* what = "elm_posegraph_add_priors";
    if (!ctx || !pg || (n && (!node || !Z16 || !info36))) return ELM_ERR_INVALID;
    if (n > (size_t)ELM_POSEGRAPH_MAX_PRIORS || !poses_finite(Z16, n)) return ELM_ERR_INVALID;
    for (size_t k = 0; k < n; ++k) {
        if (node[k] < 0 || (lever3 && !finite3(lever3 + 3 * k))) return ELM_ERR_INVALID;
        if (!finite36(info36 + 36 * k) || !symmetric36(info36 + 36 * k)) return ELM_ERR_INVALID;
    }
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    for (size_t k = 0; k < n; ++k)
        if ((uint32_t)node[k] >= pg->N) return ELM_ERR_INVALID;
    if (!pg->p_cap) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": no room for priors (elm_posegraph_reserve_priors first)");
        return ELM_ERR_UNSUPPORTED;
    }
    if (n > (size_t)(pg->p_cap - pg->P)) return refuse_full(ctx, what, "priors", pg->P, n, pg->p_cap);
    if (!n) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(12 * n), lever(3 * n, 0.0);
        for (size_t k = 0; k < n; ++k) pose_rows12(Z16 + 16 * k, &rows[12 * k]);
        if (lever3) memcpy(lever.data(), lever3, 3 * n * sizeof(double));
        pg->pnode.reserve((size_t)pg->P + n);
        pg->pwr.reserve((size_t)pg->P + n);
        pg->pwt.reserve((size_t)pg->P + n);
        const size_t P0 = pg->P;
        hipError_t e = hipMemcpyAsync(pg->d_pnode + P0, node, n * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_pZ + 12 * P0, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_plever + 3 * P0, lever.data(), lever.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pg->d_pinfo + 36 * P0, info36, 36 * n * sizeof(double), hipMemcpyHostToDevice, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        pg->pnode.insert(pg->pnode.end(), node, node + n);
        for (size_t k = 0; k < n; ++k) { // the two traces, as elm_posegraph_add_edges keeps them per edge
            const double* om = info36 + 36 * k;
            pg->pwt.push_back(((om[0] + om[7]) + om[14]) / 3.0);
            pg->pwr.push_back(((om[21] + om[28]) + om[35]) / 3.0);
        }
        pg->P += (uint32_t)n;
        invalidate(pg);
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_prior_count(elm_ctx* ctx, const elm_posegraph* pg, size_t* n_priors) {
    if (!n_priors) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_prior_count");
    if (rc != ELM_OK) return rc;
    *n_priors = pg->P;
    return ELM_OK;
}

extern "C" int elm_posegraph_get_priors(elm_ctx* ctx, const elm_posegraph* pg, size_t first, size_t count, int32_t* node, double* Z16, double* lever3,
                                        double* info36) {
    const char* what = "elm_posegraph_get_priors";
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!range_ok(first, count, pg->P)) return ELM_ERR_INVALID;
    if (!count) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        std::vector<double> rows(Z16 ? 12 * count : 0);
        hipError_t e = hipSuccess;
        if (node) e = hipMemcpyAsync(node, pg->d_pnode + first, count * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && Z16) e = hipMemcpyAsync(rows.data(), pg->d_pZ + 12 * first, rows.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && lever3) e = hipMemcpyAsync(lever3, pg->d_plever + 3 * first, 3 * count * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && info36) e = hipMemcpyAsync(info36, pg->d_pinfo + 36 * first, 36 * count * sizeof(double), hipMemcpyDeviceToHost, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        for (size_t k = 0; k < count && Z16; ++k) {
            double* T = Z16 + 16 * k;
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 4; ++q) T[q * 4 + r] = rows[12 * k + r * 4 + q];
            T[3] = T[7] = T[11] = 0.0;
            T[15] = 1.0;
        }
        return (int)ELM_OK;
    });
}

extern "C" int elm_posegraph_clear_priors(elm_ctx* ctx, elm_posegraph* pg) {
    int rc = check_object(ctx, pg, "elm_posegraph_clear_priors");
    if (rc != ELM_OK) return rc;
    pg->P = 0;
    pg->pnode.clear();
    pg->pwr.clear();
    pg->pwt.clear();
    invalidate(pg);
    return ELM_OK;
}

extern "C" int elm_posegraph_set_prior_huber(elm_ctx* ctx, elm_posegraph* pg, double k) {
    if (!ctx || !pg || !fin_ge0(k)) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_set_prior_huber");
    if (rc != ELM_OK) return rc;
    pg->prior_huber = k;
    pg->lin_valid = false; // the weights of the linearization are those of the threshold it was made with
    return ELM_OK;
}

extern "C" int elm_posegraph_get_prior_huber(elm_ctx* ctx, const elm_posegraph* pg, double* k) {
    if (!k) return ELM_ERR_INVALID;
    int rc = check_object(ctx, pg, "elm_posegraph_get_prior_huber");
    if (rc != ELM_OK) return rc;
    *k = pg->prior_huber;
    return ELM_OK;
}

extern "C" int elm_posegraph_download_prior_linearization(elm_ctx* ctx, const elm_posegraph* pg, double* r, double* J, double* s, double* w) {
    const char* what = "elm_posegraph_download_prior_linearization";
    int rc = check_object(ctx, pg, what);
    if (rc != ELM_OK) return rc;
    if (!pg->lin_valid) return ELM_ERR_INVALID;
    if (!pg->P) return ELM_OK;
    return on_stream(ctx, what, [&](hipStream_t st) {
        const size_t P = pg->P, S = pg->p_cap;
        const PgPriorDev& p = pg->prior;
        // component-major on the device, [P][components] for the caller: each component row comes down, then the transpose
        struct Part { double* dst; const double* src; size_t comps; };
        const Part parts[2] = {{r, p.r, 6}, {J, p.J, 36}};
        std::vector<double> tmp[2];
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2; ++k) {
            if (!parts[k].dst) continue;
            tmp[k].resize(parts[k].comps * P);
            for (size_t c = 0; c < parts[k].comps && e == hipSuccess; ++c)
                e = hipMemcpyAsync(&tmp[k][c * P], parts[k].src + c * S, P * sizeof(double), hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess && s) e = hipMemcpyAsync(s, p.s, P * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && w) e = hipMemcpyAsync(w, p.w, P * sizeof(double), hipMemcpyDeviceToHost, st);
        int rc = join(ctx, st, e, what);
        if (rc != ELM_OK) return rc;
        for (int k = 0; k < 2; ++k)
            if (parts[k].dst)
                for (size_t c = 0; c < parts[k].comps; ++c)
                    for (size_t q = 0; q < P; ++q) parts[k].dst[q * parts[k].comps + c] = tmp[k][c * P + q];
        return (int)ELM_OK;
    });
}
