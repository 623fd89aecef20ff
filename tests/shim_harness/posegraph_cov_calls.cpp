// Call lines of the pose graph's covariances in the C++ shim (include/elimaloc/pose_graph.hpp: PoseGraph::Marginals, Covariance,
// RelativeCovariance), compiled by tests/test_posegraph_cov_abi.py as tests/shim_harness/posegraph_init_calls.cpp is: C++14 and C++17,
// -Wall -Wextra -Werror.  Run without an argument it touches no device: it asks the C calls for their defaults and argument errors.
#include "pose_graph.hpp"

// a chain of four nodes closed by a loop edge: optimized, linearized, then the three covariance calls -> the columns they solved
int columns_after_an_optimization(const Eigen::Matrix4d& step) {
    PoseGraph graph(8, 8);
    PoseGraph::Poses poses(4, Eigen::Matrix4d::Identity());
    const std::vector<bool> fixed{true, false, false, false};
    graph.AddNodes(poses, &fixed);
    std::vector<PoseGraphEdge> edges(4);
    for (int k = 0; k < 3; ++k) {
        edges[(size_t)k].i = k;
        edges[(size_t)k].j = k + 1;
        edges[(size_t)k].Z = step;
    }
    edges[3].i = 3;
    edges[3].j = 0;
    graph.AddEdges(edges);
    graph.Optimize();
    graph.Linearize(0.0);
    const std::vector<int32_t> nodes{1, 3}, rows{0, 2}, a{1}, b{3};
    elm_posegraph_cov_stats st_m, st_r;
    const std::vector<double> marginals = graph.Marginals(nodes, nullptr, &st_m);
    std::vector<double> diag, cross;
    elm_posegraph_cov_config cfg;
    elm_posegraph_cov_config_default(&cfg);
    cfg.lambda = 1e-3;
    const elm_posegraph_cov_stats st_c = graph.Covariance(nodes, &rows, &diag, &cross, &cfg);
    const std::vector<double> rel = graph.RelativeCovariance(a, b, nullptr, &st_r);
    return st_m.n_columns + st_c.n_columns + st_r.n_columns + (int)marginals.size() + (int)diag.size() + (int)cross.size() + (int)rel.size();
}

int main(int argc, char**) {
    if (argc > 1) return columns_after_an_optimization(Eigen::Matrix4d::Identity());
    elm_posegraph_cov_config c;
    elm_posegraph_cov_config_default(&c);
    elm_posegraph_cov_stats s;
    double cov[36];
    const int32_t node = 0;
    const bool defaults = c.lambda == 0.0 && c.pcg_rel_tol == 1e-10 && c.pcg_max_iterations == 20000 && c.pcg_check_every == 32 && c.scratch_bytes == 0;
    const bool refused = elm_posegraph_covariance(nullptr, nullptr, &node, 1, nullptr, 0, &c, cov, nullptr, nullptr, nullptr, &s) == ELM_ERR_INVALID &&
                         elm_posegraph_relative_covariance(nullptr, nullptr, &node, &node, 1, &c, cov, &s) == ELM_ERR_INVALID;
    return (defaults && refused) ? 0 : 1;
}
