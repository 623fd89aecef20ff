// elm_pgraph_host.hpp -- what elm_pgraph.cpp (the object, the optimizer, the initialization) and elm_pgcov.cpp (the covariances) share
// and nobody else sees: the pose graph object, its device view and preconditioner seam, the damping launch, the record of a solve, and
// the incidence-list upload that elm_pgraph.cpp defines.  Host-side C++17.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "elm_dev_pgraph.hpp"
#include "elm_query.hpp"

struct elm_posegraph {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (as maps and scans keep it)
    uint32_t n_cap = 0, e_cap = 0, N = 0, E = 0;
    std::vector<uint8_t> fixed;     // [N]: the host's copy
    std::vector<int32_t> ei, ej;    // [E]: the host's copy
    std::vector<double> wr, wt;     // [E]: trace(Omega_ww) / 3 and trace(Omega_vv) / 3, the weights of elm_posegraph_initialize
    bool csr_dirty = true, lin_valid = false;
    double lin_huber = 0.0;         // the Huber k of the last linearization queued
    uint32_t n_hubs = 0;
    char* blob = nullptr;           // every device array below, one allocation
    double *poses = nullptr, *trial = nullptr;
    uint32_t *d_inc_start = nullptr, *d_inc = nullptr, *d_hubs = nullptr;
    int32_t *d_ei = nullptr, *d_ej = nullptr;
    double *d_Z = nullptr, *d_info = nullptr;
    uint8_t* d_fixed = nullptr;
    elm::PgDev dev{};
    int precond = ELM_PG_PRECOND_BLOCK_JACOBI; // kept across a reset
    uint32_t* d_ce = nullptr;                  // the chain-edge table, uploaded with the incidence lists
    elm::PgcDev chain{};
    // the priors (include/elimaloc_hip_posegraph_prior.h; elm_pgprior.cpp): nothing of it exists before elm_posegraph_reserve_priors
    uint32_t p_cap = 0, P = 0;
    std::vector<int32_t> pnode;     // [P]: the host's copy
    std::vector<double> pwr, pwt;   // [P]: trace(Omega_ww) / 3 and trace(Omega_vv) / 3, the weights of elm_posegraph_initialize_priors
    bool prior_rows_dirty = true;   // the rows of `prior` on the device are not those of pnode
    double prior_huber = 0.0;       // kept across a reset
    char* prior_blob = nullptr;     // every device array of `prior`, the second allocation
    int32_t* d_pnode = nullptr;
    double *d_pZ = nullptr, *d_plever = nullptr, *d_pinfo = nullptr;
    uint32_t *d_prow_node = nullptr, *d_prow_first = nullptr, *d_porder = nullptr;
    elm::PgPriorDev prior{};
};

namespace elm_pgraph_host {

constexpr int kPgDefaultCheckEvery = 32;

inline const elm::PgDev& dev_view(elm_posegraph* pg) {
    pg->dev.N = pg->N;
    pg->dev.E = pg->E;
    pg->dev.n_hubs = pg->n_hubs;
    return pg->dev;
}

// the preconditioner seam of the launchers: the chain's view, or null for block Jacobi
inline const elm::PgcDev* chain(const elm_posegraph* pg) { return pg->precond == ELM_PG_PRECOND_CHAIN ? &pg->chain : nullptr; }

// queues the damped diagonal blocks and their inverses at lambda and, for the conjugate gradients to follow with a chain, its factor
// (c: chain(pg) before a solve, null where none follows)
inline void launch_damping(hipStream_t st, const elm::PgDev& d, const elm::PgcDev* c, double lambda, int sum) {
    elm::launch_pg_nodes(st, d, lambda, sum);
    if (c) elm::launch_pgc_factor(st, d, *c, lambda);
}

// what a solve reports: the public stats records and the two stages of the initialization take their fields from it
struct PcgStats {
    int32_t iterations = 0, converged = 0;
    double rel_residual = 0.0;
};

// the incidence lists on the device are those of the current edge set (elm_pgraph.cpp)
hipError_t ensure_csr(elm_posegraph* pg, hipStream_t st);
// the rows of the priors on the device are those of the current prior set (elm_pgprior.cpp); nothing to do without priors
hipError_t ensure_prior_rows(elm_posegraph* pg, hipStream_t st);
// the priors' view for the launchers, or null when the object holds none: every added launch is then skipped
inline const elm::PgPriorDev* prior_view(elm_posegraph* pg) {
    pg->prior.P = pg->P;
    return pg->P ? &pg->prior : nullptr;
}
// no node of pg is fixed and no prior ties it to the world: the gauge is free
inline bool gauge_free(const elm_posegraph* pg) {
    return !pg->P && std::find(pg->fixed.begin(), pg->fixed.end(), (uint8_t)1) == pg->fixed.end();
}

} // namespace elm_pgraph_host
