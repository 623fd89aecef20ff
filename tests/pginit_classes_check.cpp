// pginit_classes_check.cpp -- the host's plan of elm_posegraph_initialize_priors (csrc/elm_pginit_classes.hpp) as a program of its own,
// compiled against that header alone (tests/test_posegraph_init_prior_abi.py builds it with the address and undefined-behaviour
// sanitizers and runs it): the components and their classes, every refusal, the gauge nodes, the weights of the three solves and the
// lists of the aligned components, on graphs small enough to be written down; and align_row, the host half of the alignment, on
// constructed S: a planted rotation, coplanar points, det(U V^T) = -1 and no spread at all.
#include <stdio.h>

#include <string>
#include <vector>

#include "elm_pginit_classes.hpp"

using namespace elm_pginit;

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                           \
        }                                                         \
    } while (0)

struct Case {
    std::vector<int32_t> ei, ej, pnode;
    std::vector<uint8_t> fixed;
    std::vector<double> pwr, pwt;
    Plan run(int stages) const {
        const Graph g{(uint32_t)fixed.size(), (uint32_t)ei.size(), (uint32_t)pnode.size(), ei.data(), ej.data(), fixed.data(), pnode.data(), pwr.data(),
                      pwt.data()};
        return plan(g, stages);
    }
};

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

int main() {
    // Nodes 0 .. 2 fixed component (edges stored out of order and reversed), 3 .. 5 prior-anchored, 6 .. 8 and 9 .. 11 aligned, 12 a single
    // node with a position prior, 13 a single node without anything.  The priors of the components are interleaved.
    Case c;
    c.fixed.assign(14, 0);
    c.fixed[1] = 1;
    c.ei = {2, 0, 4, 5, 7, 8, 11, 9};
    c.ej = {1, 1, 3, 4, 6, 7, 10, 10};
    //         q: 0    1    2    3    4    5    6    7    8    9
    c.pnode = {7, 3, 11, 1, 8, 12, 6, 9, 5, 7};
    c.pwr = {0.0, 2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    c.pwt = {1.0, 0.0, 3.0, 1.0, 0.5, 4.0, 0.0, 2.0, 5.0, 1.5};
    {
        const Plan p = c.run(kRot | kTrans);
        CHECK(p.refusal.empty());
        const uint32_t roots[14] = {0, 0, 0, 3, 3, 3, 6, 6, 6, 9, 9, 9, 12, 13};
        for (int v = 0; v < 14; ++v) CHECK(p.root[v] == roots[v]);
        CHECK(p.cls[0] == kFixed && p.cls[3] == kPriorAnchored && p.cls[6] == kAligned && p.cls[9] == kAligned);
        CHECK(p.cls[12] == kSingle && p.cls[13] == kSingle && p.cls[1] == kSingle); // (only roots of components with edges carry a class)
        CHECK(p.aligned() == 2 && p.gauge[0] == 6 && p.gauge[1] == 9);
        const int32_t comp[14] = {-1, -1, -1, -1, -1, -1, 0, 0, 0, 1, 1, 1, -1, -1};
        for (int v = 0; v < 14; ++v) CHECK(p.node_comp[v] == comp[v]);
        // prior 6 sits on the gauge node with weight 0: it is in no list; prior 0, 4, 9 are component 0's, ascending; 2, 7 component 1's
        CHECK(p.list_first == (std::vector<uint32_t>{0, 3, 5}));
        CHECK(p.list == (std::vector<uint32_t>{0, 4, 9, 2, 7}));
        CHECK(p.w_rot == c.pwr);
        CHECK(p.w_last == c.pwt);
        CHECK(p.w_pre == (std::vector<double>{0.0, 0.0, 0.0, 1.0, 0.0, 4.0, 0.0, 0.0, 5.0, 0.0})); // the aligned components masked
    }
    {   // TRANS alone: the position priors anchor directly, nothing is aligned or masked
        const Plan p = c.run(kTrans);
        CHECK(p.refusal.empty() && p.aligned() == 0 && p.list.empty() && p.w_pre == c.pwt && p.w_last == c.pwt);
        for (int v = 0; v < 14; ++v) CHECK(p.node_comp[v] == -1);
    }
    {   // ROT alone: the first aligned component is the refusal
        const Plan p = c.run(kRot);
        CHECK(has(p.refusal, "node 6") && has(p.refusal, "only position priors") && p.aligned() == 0);
    }
    {   // the prior-anchored component loses its translation weight: refused when TRANS is requested, legal for ROT alone
        Case d = c;
        d.pwt[8] = 0.0;
        CHECK(has(d.run(kRot | kTrans).refusal, "node 3") && has(d.run(kRot | kTrans).refusal, "translation weight"));
        CHECK(has(d.run(kTrans).refusal, "translation weight"));
        Case e = d;
        e.ei.resize(4);
        e.ej.resize(4); // (without the aligned components)
        CHECK(e.run(kRot).refusal.empty());
    }
    {   // a component with edges and nothing that holds it; a negative and a NaN weight hold nothing
        Case d = c;
        d.pwt[2] = -1.0;
        d.pwt[7] = 0.0 / 1.0;
        d.pwr[7] = __builtin_nan("");
        const Plan p = d.run(kRot | kTrans);
        CHECK(has(p.refusal, "node 9") && has(p.refusal, "no prior of positive weight") && p.gauge.empty());
        CHECK(p.w_rot.size() == 10 && p.w_pre.size() == 10 && p.w_last.size() == 10);
    }
    {   // a fixed node makes every class question moot: its component's priors keep their weights and nothing is aligned
        Case d = c;
        d.fixed[10] = 1;
        const Plan p = d.run(kRot | kTrans);
        CHECK(p.refusal.empty() && p.cls[9] == kFixed && p.aligned() == 1 && p.w_pre[2] == 3.0 && p.w_pre[7] == 2.0 && p.w_pre[0] == 0.0);
    }
    {   // no edge at all, no prior at all, and one node
        Case d;
        d.fixed.assign(3, 0);
        const Plan p = d.run(kRot | kTrans);
        CHECK(p.refusal.empty() && p.aligned() == 0 && p.list_first == (std::vector<uint32_t>{0}) && p.w_rot.empty());
        Case one;
        one.fixed.assign(1, 0);
        one.pnode = {0};
        one.pwr = {0.0};
        one.pwt = {1.0};
        CHECK(one.run(kRot).refusal.empty() && one.run(kRot | kTrans).aligned() == 0); // a single node is never aligned, never refused
    }
    {   // a long chain joined in the worst order for the union-find, and a self-contained check of path halving
        Case d;
        const int n = 1000;
        d.fixed.assign(n, 0);
        for (int v = n - 1; v > 0; --v) {
            d.ei.push_back(v);
            d.ej.push_back(v - 1);
        }
        d.pnode = {n - 1};
        d.pwr = {0.0};
        d.pwt = {1.0};
        const Plan p = d.run(kRot | kTrans);
        CHECK(p.refusal.empty() && p.aligned() == 1 && p.gauge[0] == 0 && p.list == (std::vector<uint32_t>{0}));
        for (int v = 0; v < n; ++v) CHECK(p.root[v] == 0 && p.node_comp[v] == 0);
    }
    // ---- the host half of the alignment: align_row on constructed sums (c_a, c_b, S, W)
    auto near = [](double a, double b) { return fabs(a - b) <= 1e-12; };
    auto det3 = [](const double* M) {
        return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    };
    {   // S = diag(3, 2, -1): U V^T is a reflection, and diag(1, 1, -1) makes G the identity, the nearest rotation
        double sums[16] = {1, 2, 3, 4, 5, 6, 3, 0, 0, 0, 2, 0, 0, 0, -1, 7}, row[28];
        align_row(sums, row);
        for (int k = 0; k < 16; ++k) CHECK(row[k] == sums[k]);
        CHECK(near(row[25], 3.0) && near(row[26], 2.0) && near(row[27], 1.0));
        for (int k = 0; k < 9; ++k) CHECK(near(row[16 + k], k % 4 == 0 ? 1.0 : 0.0));
        CHECK(near(det3(row + 16), 1.0));
    }
    {   // S = G0 D with a planted rotation G0 (about z by 0.7, then about x by -0.4) and D = diag(5, 2, 1) or the coplanar diag(5, 2, 0),
        // and with D's last entry negative (S = G0 times a reflection, det(U V^T) = -1): G is G0 in every case
        const double cz = cos(0.7), sz = sin(0.7), cx = cos(-0.4), sx = sin(-0.4);
        const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1}, Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
        double G0[9];
        elm::mul3(Rx, Rz, G0);
        const double last[3] = {1.0, 0.0, -1.0};
        for (int t = 0; t < 3; ++t) {
            const double D[3] = {5.0, 2.0, last[t]};
            double sums[16] = {0}, row[28];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) sums[6 + r * 3 + c] = G0[r * 3 + c] * D[c];
            sums[15] = 1.0;
            align_row(sums, row);
            CHECK(near(det3(row + 16), 1.0));
            CHECK(near(row[25], 5.0) && near(row[26], 2.0) && near(row[27], fabs(last[t])));
            for (int k = 0; k < 9; ++k) CHECK(near(row[16 + k], G0[k]));
        }
    }
    {   // no spread at all (one point): S = 0, sigma = 0, G still a rotation
        double sums[16] = {0}, row[28];
        sums[15] = 2.0;
        align_row(sums, row);
        CHECK(row[25] == 0.0 && row[26] == 0.0 && near(det3(row + 16), 1.0));
    }
    if (!failures) printf("all cases passed\n");
    return failures ? 1 : 0;
}
