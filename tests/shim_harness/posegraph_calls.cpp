// Call lines of the pose-graph part of the C++ shim (include/elimaloc/pose_graph.hpp: PoseGraphConfig, PoseGraphEdge, PoseGraph), compiled
// by tests/test_posegraph_abi.py as tests/shim_harness/places_calls.cpp is: the Eigen-typed form against tests/fake_eigen, C++14 and
// C++17, -Wall -Wextra -Werror.  Run without an argument it touches no device: it evaluates one edge on the host.
#include "pose_graph.hpp"

// a chain of three nodes closed by a loop edge, linearized, solved once by hand and then optimized: the solves it took
int solves_of_a_small_loop(const Eigen::Matrix4d& step) {
    PoseGraph graph(8, 8);
    PoseGraph::Poses poses(3, Eigen::Matrix4d::Identity());
    const std::vector<bool> fixed{true, false, false};
    graph.AddNodes(poses, &fixed);
    graph.SetPoses(PoseGraph::Poses(1, step), 1);
    graph.SetFixed(std::vector<bool>{false}, 2);
    std::vector<PoseGraphEdge> edges(3);
    edges[0].Z = step;
    edges[1].i = 1;
    edges[1].j = 2;
    edges[1].Z = step;
    edges[2].i = 2;
    edges[2].j = 0;
    edges[2].information(0, 0) = 4.0;
    graph.AddEdges(edges);
    const elm_posegraph_linearize_stats lin = graph.Linearize(1.5);
    const PoseGraphLinearization terms = graph.Linearization();
    elm_posegraph_solve_stats solve_stats;
    const std::vector<double> delta = graph.Solve(1e-3, 1e-8, 50, &solve_stats);
    PoseGraphConfig config;
    config.max_iterations = 5;
    config.huber_k = 1.5;
    std::vector<elm_posegraph_trace> trace;
    const elm_posegraph_result result = graph.Optimize(config, &trace);
    const PoseGraph::Poses corrected = graph.GetPoses();
    const size_t n = graph.Nodes() + graph.Edges() + terms.r.size() + delta.size() + trace.size() + corrected.size();
    graph.Reset();
    return result.solves + (int)n + (int)lin.n_outliers + solve_stats.iterations;
}

int main(int argc, char**) {
    if (argc > 1) return solves_of_a_small_loop(Eigen::Matrix4d::Identity());
    double r[6], A[36], B[36];
    PoseGraph::EdgeTerms(Eigen::Matrix4d::Identity(), Eigen::Matrix4d::Identity(), Eigen::Matrix4d::Identity(), r, A, B);
    return (r[0] == 0.0 && r[5] == 0.0 && A[0] == -1.0 && B[35] == 1.0) ? 0 : 1;
}
