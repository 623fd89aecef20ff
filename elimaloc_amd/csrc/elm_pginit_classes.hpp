// elm_pginit_classes.hpp -- the host's plan of elm_posegraph_initialize_priors (include/elimaloc_hip_posegraph_init_prior.h; DESIGN.md
// section 28): the connected components of the graph by a union-find over the edges (path halving, the smaller index the root, as
// elm_posegraph_initialize's refusal has it), their classes, the refusals, the gauge nodes, the weights of the priors in each of the
// three solves and the lists of the aligned components' priors; and the host half of the alignment, a component's rotation from the
// device's sums.  Nothing of HIP is included, and of the library only elm_la.hpp's fixed-size algebra: a CPU program tests it
// (tests/pginit_classes_check.cpp).  C++17.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_la.hpp"

namespace elm_pginit {

// One aligned component's row of align_out [28] from the device's sums [16] (c_a, c_b, S row-major, W): S = U Sigma V^T by svd3_jacobi,
// G = U diag(1, 1, det(U V^T)) V^T at row + 16 and sigma, descending, at row + 25.
inline void align_row(const double* sums, double* row) {
    memcpy(row, sums, 16 * sizeof(double));
    double U[9], V[9], sg[3], UV[9];
    elm::svd3_jacobi(sums + 6, U, sg, V);
    elm::mul3_bt(U, V, UV);
    const double det = UV[0] * (UV[4] * UV[8] - UV[5] * UV[7]) - UV[1] * (UV[3] * UV[8] - UV[5] * UV[6]) + UV[2] * (UV[3] * UV[7] - UV[4] * UV[6]);
    const double dd = det < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) U[r * 3 + 2] *= dd;
    elm::mul3_bt(U, V, row + 16);
    memcpy(row + 25, sg, sizeof(sg));
}

constexpr int kRot = 1, kTrans = 2; // ELM_PG_INIT_ROT, ELM_PG_INIT_TRANS

enum Class : uint8_t {
    kSingle = 0,     // no edge: never aligned, never refused
    kFixed = 1,      // has a fixed node
    kPriorAnchored,  // no fixed node, a prior with w_r > 0
    kAligned,        // no fixed node, no w_r > 0, a prior with w_t > 0
    kFree            // edges, no fixed node, no prior of positive weight: refused
};

struct Graph {
    uint32_t N, E, P;
    const int32_t *ei, *ej;  // [E]
    const uint8_t* fixed;    // [N]
    const int32_t* pnode;    // [P]
    const double *pwr, *pwt; // [P]: trace(Omega_ww) / 3, trace(Omega_vv) / 3
};

struct Plan {
    std::string refusal;              // "" when the call may run
    std::vector<uint32_t> root;       // [N]: the smallest node of v's component
    std::vector<uint8_t> cls;         // [N]: the class of the component whose root is v (kSingle elsewhere)
    // the aligned path (stages == ROT | TRANS only), components in ascending order of their smallest node
    std::vector<uint32_t> gauge;      // [A]: the smallest node of each aligned component
    std::vector<int32_t> node_comp;   // [N]: the aligned component of v, or -1
    std::vector<uint32_t> list_first; // [A + 1]
    std::vector<uint32_t> list;       // the priors with w_t > 0 of each aligned component, ascending
    // the weights of the priors in S1 (rotations), S2 (translations, aligned components masked) and S3 / the only translation solve
    std::vector<double> w_rot, w_pre, w_last; // [P]
    uint32_t aligned() const { return (uint32_t)gauge.size(); }
};

inline Plan plan(const Graph& g, int stages) {
    Plan p;
    const uint32_t N = g.N;
    p.root.resize(N);
    for (uint32_t v = 0; v < N; ++v) p.root[v] = v;
    auto find = [&](uint32_t v) {
        while (p.root[v] != v) v = p.root[v] = p.root[p.root[v]];
        return v;
    };
    for (uint32_t e = 0; e < g.E; ++e) {
        const uint32_t a = find((uint32_t)g.ei[e]), b = find((uint32_t)g.ej[e]);
        if (a != b) p.root[std::max(a, b)] = std::min(a, b);
    }
    for (uint32_t v = 0; v < N; ++v) p.root[v] = find(v);
    std::vector<uint8_t> has_edge(N, 0), has_fixed(N, 0), has_wr(N, 0), has_wt(N, 0);
    for (uint32_t e = 0; e < g.E; ++e) has_edge[p.root[(uint32_t)g.ei[e]]] = 1;
    for (uint32_t v = 0; v < N; ++v)
        if (g.fixed[v]) has_fixed[p.root[v]] = 1;
    for (uint32_t q = 0; q < g.P; ++q) {
        const uint32_t r = p.root[(uint32_t)g.pnode[q]];
        if (g.pwr[q] > 0.0) has_wr[r] = 1;
        if (g.pwt[q] > 0.0) has_wt[r] = 1;
    }
    const bool rot = (stages & kRot) != 0, trans = (stages & kTrans) != 0;
    p.cls.assign(N, kSingle);
    p.node_comp.assign(N, -1);
    for (uint32_t v = 0; v < N; ++v) {
        if (p.root[v] != v || !has_edge[v]) continue;
        const std::string who = "the connected component of node " + std::to_string(v);
        Class c = has_fixed[v] ? kFixed : has_wr[v] ? kPriorAnchored : has_wt[v] ? kAligned : kFree;
        p.cls[v] = c;
        if (!p.refusal.empty()) continue; // the first refusal is the text
        if (c == kFree) p.refusal = who + " has edges but no fixed node and no prior of positive weight (singular at lambda = 0)";
        else if (c == kPriorAnchored && trans && !has_wt[v])
            p.refusal = who + " has no fixed node and no prior with a positive translation weight trace(Omega_vv) / 3";
        else if (c == kAligned && !trans)
            p.refusal = who + " has no fixed node and only position priors: its rotations need ELM_PG_INIT_TRANS too";
        else if (c == kAligned && rot) p.gauge.push_back(v);
    }
    p.w_rot.assign(g.P, 0.0);
    p.w_pre.assign(g.P, 0.0);
    p.w_last.assign(g.P, 0.0);
    if (!p.refusal.empty()) {
        p.gauge.clear();
        return p;
    }
    std::vector<int32_t> comp_of_root(N, -1);
    for (uint32_t k = 0; k < p.gauge.size(); ++k) comp_of_root[p.gauge[k]] = (int32_t)k;
    for (uint32_t v = 0; v < N; ++v) p.node_comp[v] = comp_of_root[p.root[v]];
    std::vector<uint32_t> count(p.gauge.size() + 1, 0u);
    for (uint32_t q = 0; q < g.P; ++q) {
        const int32_t c = p.node_comp[(uint32_t)g.pnode[q]];
        p.w_rot[q] = g.pwr[q] > 0.0 ? g.pwr[q] : 0.0;
        p.w_last[q] = g.pwt[q] > 0.0 ? g.pwt[q] : 0.0;
        p.w_pre[q] = c >= 0 ? 0.0 : p.w_last[q];
        if (c >= 0 && p.w_last[q] > 0.0) ++count[(size_t)c + 1];
    }
    for (size_t k = 0; k < p.gauge.size(); ++k) count[k + 1] += count[k];
    p.list_first = count;
    p.list.resize(count.back());
    for (uint32_t q = 0; q < g.P; ++q) { // priors ascending: every list ends up ascending
        const int32_t c = p.node_comp[(uint32_t)g.pnode[q]];
        if (c >= 0 && p.w_last[q] > 0.0) p.list[count[(size_t)c]++] = q;
    }
    return p;
}

} // namespace elm_pginit
