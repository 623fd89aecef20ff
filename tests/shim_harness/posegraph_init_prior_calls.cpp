// Call lines of the pose graph's initialization with priors in the C++ shim (include/elimaloc/pose_graph.hpp:
// PoseGraph::InitializeWithPriors), compiled by tests/test_posegraph_init_prior_abi.py as tests/shim_harness/posegraph_prior_calls.cpp is:
// C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device: it asks the C calls for their defaults and
// their argument errors.
#include "pose_graph.hpp"

// a chain of six nodes without a fixed node, held by four position priors -> initialized with the stages out, then optimized
int initialized_from_positions(const Eigen::Matrix4d& step) {
    PoseGraph graph(8, 8);
    graph.ReservePriors(8);
    PoseGraph::Poses poses(6, Eigen::Matrix4d::Identity());
    graph.AddNodes(poses);
    std::vector<PoseGraphEdge> edges(5);
    for (int k = 0; k < 5; ++k) {
        edges[(size_t)k].i = k;
        edges[(size_t)k].j = k + 1;
        edges[(size_t)k].Z = step;
    }
    graph.AddEdges(edges);
    const std::vector<int> nodes{0, 2, 3, 5};
    const std::vector<Eigen::Vector3d> positions{Eigen::Vector3d(0.0, 0.0, 0.0), Eigen::Vector3d(2.0, 1.0, 0.0), Eigen::Vector3d(3.0, 0.0, 1.0),
                                                 Eigen::Vector3d(5.0, 2.0, 0.0)};
    graph.AddPositionPriors(nodes, positions);
    elm_posegraph_init_prior_config config;
    elm_posegraph_init_prior_config_default(&config);
    config.base.pcg_rel_tol = 1e-10;
    config.align_min_ratio = 1e-6;
    std::vector<double> rows, v_pre, v, align;
    const elm_posegraph_init_prior_result res = graph.InitializeWithPriors(&config, &rows, &v_pre, &v, &align);
    const elm_posegraph_init_prior_result again = graph.InitializeWithPriors();
    graph.Optimize();
    return res.base.applied + again.base.applied + res.aligned_components + res.rank_deficient_components + res.pre_converged + (int)rows.size() +
           (int)v_pre.size() + (int)v.size() + (int)align.size() + (res.min_align_ratio > 0.0 ? 1 : 0);
}

int main(int argc, char**) {
    if (argc > 1) return initialized_from_positions(Eigen::Matrix4d::Identity());
    elm_posegraph_init_prior_config c;
    elm_posegraph_init_prior_config_default(&c);
    elm_posegraph_init_config base;
    elm_posegraph_init_config_default(&base);
    elm_posegraph_init_prior_result r;
    const bool defaults = c.align_min_ratio == 1e-4 && c.base.pcg_rel_tol == base.pcg_rel_tol && c.base.pcg_max_iterations == base.pcg_max_iterations &&
                          c.base.pcg_check_every == base.pcg_check_every && c.base.stages == (ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS);
    const bool refused = elm_posegraph_initialize_priors(nullptr, nullptr, &c, &r, nullptr, nullptr, nullptr, nullptr, 0) == ELM_ERR_INVALID;
    return (defaults && refused && ELM_PG_INIT_ALIGN_ROW == 28) ? 0 : 1;
}
