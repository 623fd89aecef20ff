// Call lines of the pose graph's preconditioner choice in the C++ shim (include/elimaloc/pose_graph.hpp: PoseGraph::SetPreconditioner,
// PoseGraph::Preconditioner), compiled by tests/test_posegraph_chain_abi.py as tests/shim_harness/posegraph_calls.cpp is: C++14 and
// C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device: it asks the C calls for their argument errors.
#include "pose_graph.hpp"

// a chain of four nodes closed by a loop edge, optimized with the chain preconditioner: the conjugate-gradient iterations it took
int iterations_of_a_small_loop(const Eigen::Matrix4d& step) {
    PoseGraph graph(8, 8);
    graph.SetPreconditioner(ELM_PG_PRECOND_CHAIN);
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
    const elm_posegraph_result result = graph.Optimize();
    graph.Reset();
    const int kept = graph.Preconditioner(); // the kind survives a reset
    graph.SetPreconditioner(ELM_PG_PRECOND_BLOCK_JACOBI);
    return (int)result.pcg_iterations_total + kept + graph.Preconditioner();
}

int main(int argc, char**) {
    if (argc > 1) return iterations_of_a_small_loop(Eigen::Matrix4d::Identity());
    int kind = 7;
    const bool refused = elm_posegraph_set_preconditioner(nullptr, nullptr, ELM_PG_PRECOND_CHAIN) == ELM_ERR_INVALID &&
                         elm_posegraph_get_preconditioner(nullptr, nullptr, &kind) == ELM_ERR_INVALID && kind == 7;
    return (refused && ELM_PG_PRECOND_BLOCK_JACOBI == 0 && ELM_PG_PRECOND_CHAIN == 1) ? 0 : 1;
}
