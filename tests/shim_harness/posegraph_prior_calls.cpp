// Call lines of the pose graph's priors in the C++ shim (include/elimaloc/pose_graph.hpp: PoseGraph::ReservePriors, AddPriors,
// AddPositionPriors, ClearPriors, SetPriorHuber, PriorLinearization), compiled by tests/test_posegraph_prior_abi.py as
// tests/shim_harness/posegraph_calls.cpp is: C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device: it
// asks the C calls for their argument errors and the host-only prior terms.
#include "pose_graph.hpp"

// a chain of four nodes without a fixed node, anchored by a pose prior and three position priors -> the priors linearized
int priors_after_an_optimization(const Eigen::Matrix4d& step) {
    PoseGraph graph(8, 8);
    graph.ReservePriors(8);
    PoseGraph::Poses poses(4, Eigen::Matrix4d::Identity());
    graph.AddNodes(poses);
    std::vector<PoseGraphEdge> edges(3);
    for (int k = 0; k < 3; ++k) {
        edges[(size_t)k].i = k;
        edges[(size_t)k].j = k + 1;
        edges[(size_t)k].Z = step;
    }
    graph.AddEdges(edges);
    std::vector<PoseGraphPrior> pose_prior(1);
    pose_prior[0].node = 0;
    pose_prior[0].lever = Eigen::Vector3d(0.5, -0.2, 1.2);
    graph.AddPriors(pose_prior);
    const std::vector<int> nodes{1, 2, 3};
    const std::vector<Eigen::Vector3d> positions(3, Eigen::Vector3d(1.0, 2.0, 3.0));
    graph.AddPositionPriors(nodes, positions);
    graph.SetPriorHuber(1.0);
    graph.Optimize();
    graph.Linearize(0.0);
    const PoseGraphPriorLinearization lin = graph.PriorLinearization();
    const int n = (int)graph.Priors();
    graph.ClearPriors();
    return n + (int)lin.r.size() + (int)lin.J.size() + (int)lin.s.size() + (int)lin.w.size() + (int)graph.Priors();
}

int main(int argc, char**) {
    if (argc > 1) return priors_after_an_optimization(Eigen::Matrix4d::Identity());
    const int32_t node = 0;
    size_t n = 7;
    double k = 3.0, r[6], J[36];
    const Eigen::Matrix4d I = Eigen::Matrix4d::Identity();
    const bool refused = elm_posegraph_reserve_priors(nullptr, nullptr, 4) == ELM_ERR_INVALID &&
                         elm_posegraph_add_priors(nullptr, nullptr, &node, I.data(), nullptr, J, 1) == ELM_ERR_INVALID &&
                         elm_posegraph_prior_count(nullptr, nullptr, &n) == ELM_ERR_INVALID && elm_posegraph_clear_priors(nullptr, nullptr) == ELM_ERR_INVALID &&
                         elm_posegraph_set_prior_huber(nullptr, nullptr, 1.0) == ELM_ERR_INVALID &&
                         elm_posegraph_get_prior_huber(nullptr, nullptr, &k) == ELM_ERR_INVALID &&
                         elm_posegraph_download_prior_linearization(nullptr, nullptr, r, J, nullptr, nullptr) == ELM_ERR_INVALID && n == 7 && k == 3.0;
    const bool terms = elm_posegraph_prior_terms(I.data(), I.data(), nullptr, r, J) == ELM_OK && r[0] == 0.0 && r[5] == 0.0 && J[0] == 1.0 && J[35] == 1.0 &&
                       J[1] == 0.0;
    return (refused && terms) ? 0 : 1;
}
