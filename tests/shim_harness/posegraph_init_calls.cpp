// Call lines of the pose graph's linear initialization in the C++ shim (include/elimaloc/pose_graph.hpp: PoseGraph::Initialize), compiled
// by tests/test_posegraph_init_abi.py as tests/shim_harness/posegraph_chain_calls.cpp is: C++14 and C++17, -Wall -Wextra -Werror.  Run
// without an argument it touches no device: it asks the C calls for their argument errors.
#include "pose_graph.hpp"

// a chain of four nodes closed by a loop edge, started at the identity: initialized, then optimized -> the solves Optimize still took
int solves_after_an_initialization(const Eigen::Matrix4d& step) {
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
    std::vector<double> rows, v;
    const elm_posegraph_init_result both = graph.Initialize(nullptr, &rows, &v);
    elm_posegraph_init_config only;
    elm_posegraph_init_config_default(&only);
    only.stages = ELM_PG_INIT_TRANS;
    const elm_posegraph_init_result again = graph.Initialize(&only);
    const elm_posegraph_result result = graph.Optimize();
    return result.solves + both.applied + again.applied + both.degenerate_nodes + (int)rows.size() + (int)v.size();
}

int main(int argc, char**) {
    if (argc > 1) return solves_after_an_initialization(Eigen::Matrix4d::Identity());
    elm_posegraph_init_config c;
    elm_posegraph_init_config_default(&c);
    elm_posegraph_init_result r;
    const bool defaults = c.pcg_rel_tol == 1e-8 && c.pcg_max_iterations == 50000 && c.pcg_check_every == 32 &&
                          c.stages == (ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS) && c.reserved == 0;
    const bool refused = elm_posegraph_initialize(nullptr, nullptr, &c, &r, nullptr, nullptr) == ELM_ERR_INVALID;
    return (defaults && refused && ELM_PG_INIT_ROT == 1 && ELM_PG_INIT_TRANS == 2) ? 0 : 1;
}
