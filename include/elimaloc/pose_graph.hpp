// pose_graph.hpp -- the pose graph (include/elimaloc_hip.h, "pose graph"): the C++ face of elm_posegraph in the shim's types.  Nodes and
// relative-pose edges resident on the device, their linearization, the damped normal equations solved by preconditioned conjugate
// gradients, and Levenberg-Marquardt: from odometry and loop constraints to corrected poses.  The residual, the Jacobians, the robust
// weight and the rules of the outer loop are those of the C header.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "registration.hpp"

struct PoseGraphConfig {
    int max_iterations = 20, pcg_max_iterations = 2000, pcg_check_every = 32;
    double lambda_init = 1e-4, lambda_up = 10.0, lambda_down = 0.1, lambda_min = 1e-12, lambda_max = 1e8;
    double cost_rel_tol = 1e-12, step_tol = 1e-10, pcg_rel_tol = 1e-8, huber_k = 0.0;
    elm_posegraph_config c_struct() const {
        elm_posegraph_config c;
        elm_posegraph_config_default(&c);
        c.max_iterations = max_iterations;
        c.pcg_max_iterations = pcg_max_iterations;
        c.pcg_check_every = pcg_check_every;
        c.lambda_init = lambda_init;
        c.lambda_up = lambda_up;
        c.lambda_down = lambda_down;
        c.lambda_min = lambda_min;
        c.lambda_max = lambda_max;
        c.cost_rel_tol = cost_rel_tol;
        c.step_tol = step_tol;
        c.pcg_rel_tol = pcg_rel_tol;
        c.huber_k = huber_k;
        return c;
    }
};

struct PoseGraphEdge {
    int i = 0, j = 1;
    elimaloc::Matrix4d Z = elimaloc::Matrix4d::Identity();           // ~ T_i^-1 T_j
    elimaloc::Matrix6d information = elimaloc::Matrix6d::Identity(); // symmetric, in the order [translation; rotation]
};

struct PoseGraphLinearization {
    std::vector<double> r, A, B, s, w, grad, diag; // [E][6], [E][36], [E][36], [E], [E], [N][6], [N][36], row-major
};

// an absolute factor on one node (elimaloc_hip_posegraph_prior.h): a measured pose, or with a singular information a measured position
struct PoseGraphPrior {
    int node = 0;
    elimaloc::Matrix4d Z = elimaloc::Matrix4d::Identity();           // ~ T_node: world <- measured frame
    elimaloc::Vector3d lever = elimaloc::Vector3d::Zero();           // the measured point in the node's frame
    elimaloc::Matrix6d information = elimaloc::Matrix6d::Identity(); // symmetric, in the order [translation; rotation]; may be singular
};

struct PoseGraphPriorLinearization {
    std::vector<double> r, J, s, w; // [P][6], [P][36], [P], [P], row-major
};

class PoseGraph {
public:
    using Poses = std::vector<elimaloc::Matrix4d>;
    PoseGraph(int node_capacity, int edge_capacity) {
        elimaloc::check(elm_posegraph_create(VoxelHashMap::ctx(), node_capacity, edge_capacity, &pg_), VoxelHashMap::ctx(), "elm_posegraph_create");
    }
    PoseGraph(const PoseGraph&) = delete; // owns device memory
    PoseGraph& operator=(const PoseGraph&) = delete;
    ~PoseGraph() { elm_posegraph_destroy(pg_); }

    inline size_t Nodes() const { return sizes().first; }
    inline size_t Edges() const { return sizes().second; }
    inline void Reset() { elimaloc::check(elm_posegraph_reset(VoxelHashMap::ctx(), pg_), VoxelHashMap::ctx(), "elm_posegraph_reset"); }
    // ELM_PG_PRECOND_BLOCK_JACOBI (the default) or ELM_PG_PRECOND_CHAIN, for Solve and Optimize alike; kept across Reset
    inline void SetPreconditioner(int kind) {
        elimaloc::check(elm_posegraph_set_preconditioner(VoxelHashMap::ctx(), pg_, kind), VoxelHashMap::ctx(), "elm_posegraph_set_preconditioner");
    }
    inline int Preconditioner() const {
        int kind = -1;
        elimaloc::check(elm_posegraph_get_preconditioner(VoxelHashMap::ctx(), pg_, &kind), VoxelHashMap::ctx(), "elm_posegraph_get_preconditioner");
        return kind;
    }

    inline void AddNodes(const Poses& poses, const std::vector<bool>* fixed = nullptr) {
        elimaloc::check(!fixed || fixed->size() == poses.size() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "PoseGraph::AddNodes: one flag per node");
        const std::vector<double> block = flat(poses);
        std::vector<uint8_t> fx(poses.size() + 1, 0);
        for (size_t k = 0; fixed && k < poses.size(); ++k) fx[k] = (*fixed)[k] ? 1 : 0;
        elimaloc::check(elm_posegraph_add_nodes(VoxelHashMap::ctx(), pg_, block.data(), fx.data(), poses.size()), VoxelHashMap::ctx(),
                        "elm_posegraph_add_nodes");
    }
    inline void SetPoses(const Poses& poses, size_t first = 0) {
        const std::vector<double> block = flat(poses);
        elimaloc::check(elm_posegraph_set_poses(VoxelHashMap::ctx(), pg_, first, poses.size(), block.data()), VoxelHashMap::ctx(),
                        "elm_posegraph_set_poses");
    }
    inline Poses GetPoses() const {
        const size_t n = Nodes();
        std::vector<double> block(16 * n + 1);
        elimaloc::check(elm_posegraph_get_poses(VoxelHashMap::ctx(), pg_, 0, n, block.data()), VoxelHashMap::ctx(), "elm_posegraph_get_poses");
        Poses out(n);
        for (size_t k = 0; k < n; ++k)
            for (int q = 0; q < 16; ++q) out[k].data()[q] = block[16 * k + (size_t)q];
        return out;
    }
    inline void SetFixed(const std::vector<bool>& fixed, size_t first = 0) {
        std::vector<uint8_t> fx(fixed.size() + 1, 0);
        for (size_t k = 0; k < fixed.size(); ++k) fx[k] = fixed[k] ? 1 : 0;
        elimaloc::check(elm_posegraph_set_fixed(VoxelHashMap::ctx(), pg_, first, fixed.size(), fx.data()), VoxelHashMap::ctx(),
                        "elm_posegraph_set_fixed");
    }
    inline void AddEdges(const std::vector<PoseGraphEdge>& edges) {
        const size_t n = edges.size();
        std::vector<int32_t> i(n + 1), j(n + 1);
        std::vector<double> Z(16 * n + 1), info(36 * n + 1);
        for (size_t k = 0; k < n; ++k) {
            i[k] = edges[k].i;
            j[k] = edges[k].j;
            for (int q = 0; q < 16; ++q) Z[16 * k + (size_t)q] = edges[k].Z.data()[q];
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) info[36 * k + (size_t)(r * 6 + c)] = edges[k].information(r, c);
        }
        elimaloc::check(elm_posegraph_add_edges(VoxelHashMap::ctx(), pg_, i.data(), j.data(), Z.data(), info.data(), n), VoxelHashMap::ctx(),
                        "elm_posegraph_add_edges");
    }
    inline elm_posegraph_linearize_stats Linearize(double huber_k = 0.0) {
        elm_posegraph_linearize_stats st;
        elimaloc::check(elm_posegraph_linearize(VoxelHashMap::ctx(), pg_, huber_k, &st), VoxelHashMap::ctx(), "elm_posegraph_linearize");
        return st;
    }
    inline PoseGraphLinearization Linearization() const {
        const size_t N = Nodes(), E = Edges();
        PoseGraphLinearization L;
        L.r.assign(6 * E + 1, 0.0);
        L.A.assign(36 * E + 1, 0.0);
        L.B.assign(36 * E + 1, 0.0);
        L.s.assign(E + 1, 0.0);
        L.w.assign(E + 1, 0.0);
        L.grad.assign(6 * N + 1, 0.0);
        L.diag.assign(36 * N + 1, 0.0);
        elimaloc::check(elm_posegraph_download_linearization(VoxelHashMap::ctx(), pg_, L.r.data(), L.A.data(), L.B.data(), L.s.data(), L.w.data(),
                                                             L.grad.data(), L.diag.data()),
                        VoxelHashMap::ctx(), "elm_posegraph_download_linearization");
        L.r.pop_back();
        L.A.pop_back();
        L.B.pop_back();
        L.s.pop_back();
        L.w.pop_back();
        L.grad.pop_back();
        L.diag.pop_back();
        return L;
    }
    // the step of the current linearization, [Nodes()][6]
    inline std::vector<double> Solve(double lambda, double pcg_rel_tol = 1e-8, int pcg_max_iterations = 2000, elm_posegraph_solve_stats* stats = nullptr) {
        std::vector<double> delta(6 * Nodes() + 1);
        elimaloc::check(elm_posegraph_solve(VoxelHashMap::ctx(), pg_, lambda, pcg_rel_tol, pcg_max_iterations, delta.data(), stats), VoxelHashMap::ctx(),
                        "elm_posegraph_solve");
        delta.pop_back();
        return delta;
    }
    inline elm_posegraph_result Optimize(const PoseGraphConfig& config = PoseGraphConfig(), std::vector<elm_posegraph_trace>* trace = nullptr) {
        const elm_posegraph_config c = config.c_struct();
        elm_posegraph_result res;
        std::vector<elm_posegraph_trace> tr((size_t)(c.max_iterations > 0 ? c.max_iterations : 0) + 1);
        elimaloc::check(elm_posegraph_optimize(VoxelHashMap::ctx(), pg_, &c, &res, tr.data(), (int)tr.size() - 1), VoxelHashMap::ctx(),
                        "elm_posegraph_optimize");
        if (trace) trace->assign(tr.begin(), tr.begin() + res.solves);
        return res;
    }
    // The linear initialization (elimaloc_hip_posegraph_init.h): rotations first, then translations, by this object's preconditioner;
    // the poses are replaced only if every requested stage converged (result.applied).  config: NULL for the defaults; rows [Nodes()][6]
    // (the solved rows before the projection) and v [Nodes()][3] when asked for.
    inline elm_posegraph_init_result Initialize(const elm_posegraph_init_config* config = nullptr, std::vector<double>* rows = nullptr,
                                                std::vector<double>* v = nullptr) {
        elm_posegraph_init_config c;
        elm_posegraph_init_config_default(&c);
        if (config) c = *config;
        const size_t n = (rows || v) ? Nodes() : 0;
        if (rows) rows->assign(6 * n + 1, 0.0);
        if (v) v->assign(3 * n + 1, 0.0);
        elm_posegraph_init_result res;
        elimaloc::check(elm_posegraph_initialize(VoxelHashMap::ctx(), pg_, &c, &res, rows ? rows->data() : nullptr, v ? v->data() : nullptr),
                        VoxelHashMap::ctx(), "elm_posegraph_initialize");
        if (rows) rows->pop_back();
        if (v) v->pop_back();
        return res;
    }
    // The linear initialization with the priors in it (elimaloc_hip_posegraph_init_prior.h): for a graph that priors hold and no fixed
    // node does.  The poses are replaced only if every solve converged and no alignment is rank-deficient (result.base.applied).
    // config: NULL for the defaults; rows [Nodes()][6], v_pre [Nodes()][3], v [Nodes()][3] and align [aligned_components][28] when
    // asked for.
    inline elm_posegraph_init_prior_result InitializeWithPriors(const elm_posegraph_init_prior_config* config = nullptr,
                                                                std::vector<double>* rows = nullptr, std::vector<double>* v_pre = nullptr,
                                                                std::vector<double>* v = nullptr, std::vector<double>* align = nullptr) {
        elm_posegraph_init_prior_config c;
        elm_posegraph_init_prior_config_default(&c);
        if (config) c = *config;
        const size_t n = (rows || v_pre || v || align) ? Nodes() : 0;
        if (rows) rows->assign(6 * n + 1, 0.0);
        if (v_pre) v_pre->assign(3 * n + 1, 0.0);
        if (v) v->assign(3 * n + 1, 0.0);
        // an aligned component has an edge, so two nodes, and a prior of its own: no more of them than N / 2 or than the priors
        const size_t cap = align ? std::min(n / 2, Priors()) : 0;
        if (align) align->assign(ELM_PG_INIT_ALIGN_ROW * cap + 1, 0.0);
        elm_posegraph_init_prior_result res;
        elimaloc::check(elm_posegraph_initialize_priors(VoxelHashMap::ctx(), pg_, &c, &res, rows ? rows->data() : nullptr,
                                                        v_pre ? v_pre->data() : nullptr, v ? v->data() : nullptr,
                                                        align ? align->data() : nullptr, (int)cap),
                        VoxelHashMap::ctx(), "elm_posegraph_initialize_priors");
        if (rows) rows->pop_back();
        if (v_pre) v_pre->pop_back();
        if (v) v->pop_back();
        if (align) align->resize((size_t)ELM_PG_INIT_ALIGN_ROW * (size_t)res.aligned_components);
        return res;
    }
    // Blocks of the inverse of the current linearization's normal equations (elimaloc_hip_posegraph_cov.h; this object's preconditioner), row-major
    // 6 x 6 in the tangent [v; w].  Covariance: diag [cols][36] = Sigma(col, col) symmetrised, cross [cols][rows][36] = Sigma(row, col) as
    // solved (either may be NULL; rows may be NULL for the diagonal blocks only).  config: NULL for the defaults.
    inline elm_posegraph_cov_stats Covariance(const std::vector<int32_t>& cols, const std::vector<int32_t>* rows, std::vector<double>* diag,
                                              std::vector<double>* cross, const elm_posegraph_cov_config* config = nullptr) {
        elm_posegraph_cov_config c;
        elm_posegraph_cov_config_default(&c);
        if (config) c = *config;
        const size_t m = cols.size(), n = rows ? rows->size() : 0;
        if (diag) diag->assign(36 * m + 1, 0.0);
        if (cross) cross->assign(36 * m * n + 1, 0.0);
        elm_posegraph_cov_stats st;
        elimaloc::check(elm_posegraph_covariance(VoxelHashMap::ctx(), pg_, m ? cols.data() : nullptr, m, n ? rows->data() : nullptr, n, &c,
                                                 diag ? diag->data() : nullptr, (cross && n) ? cross->data() : nullptr, nullptr, nullptr, &st),
                        VoxelHashMap::ctx(), "elm_posegraph_covariance");
        if (diag) diag->pop_back();
        if (cross) cross->pop_back();
        return st;
    }
    // the marginal covariances [nodes][36]
    inline std::vector<double> Marginals(const std::vector<int32_t>& nodes, const elm_posegraph_cov_config* config = nullptr,
                                         elm_posegraph_cov_stats* stats = nullptr) {
        std::vector<double> diag;
        const elm_posegraph_cov_stats st = Covariance(nodes, nullptr, &diag, nullptr, config);
        if (stats) *stats = st;
        return diag;
    }
    // the covariances [pairs][36] of the residual coordinates of T_a^-1 T_b at the current poses
    inline std::vector<double> RelativeCovariance(const std::vector<int32_t>& a, const std::vector<int32_t>& b,
                                                  const elm_posegraph_cov_config* config = nullptr, elm_posegraph_cov_stats* stats = nullptr) {
        elm_posegraph_cov_config c;
        elm_posegraph_cov_config_default(&c);
        if (config) c = *config;
        elimaloc::check(a.size() == b.size() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "PoseGraph::RelativeCovariance: one b per a");
        std::vector<double> cov(36 * a.size() + 1, 0.0);
        elimaloc::check(elm_posegraph_relative_covariance(VoxelHashMap::ctx(), pg_, a.empty() ? nullptr : a.data(), a.empty() ? nullptr : b.data(),
                                                          a.size(), &c, cov.data(), stats),
                        VoxelHashMap::ctx(), "elm_posegraph_relative_covariance");
        cov.pop_back();
        return cov;
    }
    // Priors (elimaloc_hip_posegraph_prior.h): room for them once per object, then absolute pose / position factors under a Huber
    // threshold of their own (0: off; kept across Reset, as the capacity is).  With at least one prior Optimize needs no fixed node.
    inline void ReservePriors(int capacity) {
        elimaloc::check(elm_posegraph_reserve_priors(VoxelHashMap::ctx(), pg_, capacity), VoxelHashMap::ctx(), "elm_posegraph_reserve_priors");
    }
    inline size_t Priors() const {
        size_t n = 0;
        elimaloc::check(elm_posegraph_prior_count(VoxelHashMap::ctx(), pg_, &n), VoxelHashMap::ctx(), "elm_posegraph_prior_count");
        return n;
    }
    inline void AddPriors(const std::vector<PoseGraphPrior>& priors) {
        const size_t n = priors.size();
        std::vector<int32_t> node(n + 1);
        std::vector<double> Z(16 * n + 1), lever(3 * n + 1), info(36 * n + 1);
        for (size_t k = 0; k < n; ++k) {
            node[k] = priors[k].node;
            for (int q = 0; q < 16; ++q) Z[16 * k + (size_t)q] = priors[k].Z.data()[q];
            for (int q = 0; q < 3; ++q) lever[3 * k + (size_t)q] = priors[k].lever(q);
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) info[36 * k + (size_t)(r * 6 + c)] = priors[k].information(r, c);
        }
        elimaloc::check(elm_posegraph_add_priors(VoxelHashMap::ctx(), pg_, node.data(), Z.data(), lever.data(), info.data(), n), VoxelHashMap::ctx(),
                        "elm_posegraph_add_priors");
    }
    // position measurements: Z = [I | position], the 3 x 3 information in the translation block, the rotation rows and columns zero
    inline void AddPositionPriors(const std::vector<int>& nodes, const std::vector<elimaloc::Vector3d>& positions,
                                  const elimaloc::Matrix3d& information = elimaloc::Matrix3d::Identity(),
                                  const elimaloc::Vector3d& lever = elimaloc::Vector3d::Zero()) {
        elimaloc::check(nodes.size() == positions.size() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "PoseGraph::AddPositionPriors: one position per node");
        std::vector<PoseGraphPrior> priors(nodes.size());
        for (size_t k = 0; k < nodes.size(); ++k) {
            priors[k].node = nodes[k];
            priors[k].lever = lever;
            priors[k].information = elimaloc::Matrix6d::Zero();
            for (int r = 0; r < 3; ++r) {
                priors[k].Z(r, 3) = positions[k](r);
                for (int c = 0; c < 3; ++c) priors[k].information(r, c) = information(r, c);
            }
        }
        AddPriors(priors);
    }
    inline void ClearPriors() { elimaloc::check(elm_posegraph_clear_priors(VoxelHashMap::ctx(), pg_), VoxelHashMap::ctx(), "elm_posegraph_clear_priors"); }
    inline void SetPriorHuber(double k) {
        elimaloc::check(elm_posegraph_set_prior_huber(VoxelHashMap::ctx(), pg_, k), VoxelHashMap::ctx(), "elm_posegraph_set_prior_huber");
    }
    inline PoseGraphPriorLinearization PriorLinearization() const {
        const size_t P = Priors();
        PoseGraphPriorLinearization L;
        L.r.assign(6 * P + 1, 0.0);
        L.J.assign(36 * P + 1, 0.0);
        L.s.assign(P + 1, 0.0);
        L.w.assign(P + 1, 0.0);
        elimaloc::check(elm_posegraph_download_prior_linearization(VoxelHashMap::ctx(), pg_, L.r.data(), L.J.data(), L.s.data(), L.w.data()),
                        VoxelHashMap::ctx(), "elm_posegraph_download_prior_linearization");
        L.r.pop_back();
        L.J.pop_back();
        L.s.pop_back();
        L.w.pop_back();
        return L;
    }
    // host only: the residual and Jacobians of one edge (row-major r[6], A[36], B[36])
    static inline void EdgeTerms(const elimaloc::Matrix4d& Ti, const elimaloc::Matrix4d& Tj, const elimaloc::Matrix4d& Z, double* r, double* A, double* B) {
        elimaloc::check(elm_posegraph_edge_terms(Ti.data(), Tj.data(), Z.data(), r, A, B), nullptr, "elm_posegraph_edge_terms");
    }

private:
    static std::vector<double> flat(const Poses& poses) {
        std::vector<double> block(16 * poses.size() + 1);
        for (size_t k = 0; k < poses.size(); ++k)
            for (int q = 0; q < 16; ++q) block[16 * k + (size_t)q] = poses[k].data()[q];
        return block;
    }
    std::pair<size_t, size_t> sizes() const {
        size_t n = 0, e = 0;
        elimaloc::check(elm_posegraph_size(VoxelHashMap::ctx(), pg_, &n, &e), VoxelHashMap::ctx(), "elm_posegraph_size");
        return std::make_pair(n, e);
    }
    elm_posegraph* pg_ = nullptr;
};
