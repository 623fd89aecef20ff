// Call lines of the loop consistency check in the C++ shim (include/elimaloc/loop_consistency.hpp), compiled by tests/test_loops_abi.py
// as tests/shim_harness/posegraph_init_calls.cpp is: C++14 and C++17, -Wall -Wextra -Werror.  Run without an argument it touches no
// device: it asks the C calls for their defaults and argument errors.  With a file (float64 throughout: n, L, q_t, q_r, gamma, poses
// [n][16], a [L], b [L], Z [L][16], var_t [L], var_r [L]) it runs the check on the device and prints "size adjacent_pairs steps" and the
// members, for tests/test_loops.py to hold against the Python call.
#include <cstdio>

#include "loop_consistency.hpp"

int run_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    std::vector<double> all;
    double buf[256];
    for (size_t got; (got = std::fread(buf, sizeof(double), 256, f)) > 0;) all.insert(all.end(), buf, buf + got);
    std::fclose(f);
    if (all.size() < 5) return 2;
    const size_t n = (size_t)all[0], L = (size_t)all[1];
    if (all.size() != 5 + 16 * n + 2 * L + 16 * L + 2 * L) return 2;
    elm_loops_config c;
    elm_loops_config_default(&c);
    c.q_t = all[2];
    c.q_r = all[3];
    c.gamma = all[4];
    const double *P = all.data() + 5, *a = P + 16 * n, *b = a + L, *Z = b + L, *vt = Z + 16 * L, *vr = vt + L;
    std::vector<elimaloc::Matrix4d> poses(n);
    for (size_t v = 0; v < n; ++v)
        for (int q = 0; q < 16; ++q) poses[v].data()[q] = P[16 * v + (size_t)q];
    std::vector<LoopMeasurement> loops(L);
    for (size_t k = 0; k < L; ++k) {
        loops[k].a = (int)a[k];
        loops[k].b = (int)b[k];
        loops[k].var_t = vt[k];
        loops[k].var_r = vr[k];
        for (int q = 0; q < 16; ++q) loops[k].Z.data()[q] = Z[16 * k + (size_t)q];
    }
    const LoopConsistencyResult r = LoopConsistency(poses, loops, &c);
    std::printf("%d %lld %d\n", r.result.size, (long long)r.result.adjacent_pairs, r.result.steps);
    for (int m : r.members()) std::printf("%d ", m);
    std::printf("\n");
    for (int32_t d : r.degree) std::printf("%d ", (int)d);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return run_file(argv[1]);
    elm_loops_config c;
    elm_loops_config_default(&c);
    elm_loops_result r;
    uint8_t member = 0;
    int32_t degree = 0;
    const bool defaults = c.q_t == 0.0 && c.q_r == 0.0 && c.gamma == 16.81 && c.steps_per_batch == 32 && c.reserved == 0;
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const bool refused = elm_loops_consistency(nullptr, I, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &c, &r, &member, &degree, nullptr, nullptr) ==
                         ELM_ERR_INVALID;
    double e[6] = {1, 1, 1, 1, 1, 1};
    const elimaloc::Matrix4d T = elimaloc::Matrix4d::Identity();
    LoopPairTerms(T, T, T, T, T, T, e);
    bool zero = true;
    for (double x : e) zero = zero && x == 0.0;
    const bool pair_refused = elm_loops_pair_terms(I, I, I, I, I, nullptr, e) == ELM_ERR_INVALID;
    return (defaults && refused && zero && pair_refused && ELM_LOOPS_MAX == 16384 && ELM_LOOPS_MAX_S == 2048) ? 0 : 1;
}
