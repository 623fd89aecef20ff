// Call lines of the covariance-model loop consistency check in the C++ shim (include/elimaloc/loop_covariance.hpp), compiled by
// tests/test_loopcov_abi.py as tests/shim_harness/loop_consistency_calls.cpp is: C++14 and C++17, -Wall -Wextra -Werror.  Run without an
// argument it touches no device: it asks the C calls for their argument errors and the host-only pair term for an exact cycle.  With a
// file (float64 throughout: n, L, q_count, gamma, poses [n][16], a [L], b [L], Z [L][16], cov [L][36], Q [q_count][36]) it runs the check
// on the device and prints "size adjacent_pairs steps non_finite_pairs", the members, the degrees and the trace of the last W, for
// tests/test_loopcov.py to hold against the Python calls.
#include <cstdio>

#include "loop_covariance.hpp"

int run_file(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    std::vector<double> all;
    double buf[256];
    for (size_t got; (got = std::fread(buf, sizeof(double), 256, f)) > 0;) all.insert(all.end(), buf, buf + got);
    std::fclose(f);
    if (all.size() < 4) return 2;
    const size_t n = (size_t)all[0], L = (size_t)all[1], qc = (size_t)all[2];
    if (all.size() != 4 + 16 * n + 2 * L + 16 * L + 36 * L + 36 * qc) return 2;
    elm_loops_config c;
    elm_loops_config_default(&c);
    c.gamma = all[3];
    const double *P = all.data() + 4, *a = P + 16 * n, *b = a + L, *Z = b + L, *S = Z + 16 * L, *Q = S + 36 * L;
    std::vector<elimaloc::Matrix4d> poses(n);
    for (size_t v = 0; v < n; ++v)
        for (int q = 0; q < 16; ++q) poses[v].data()[q] = P[16 * v + (size_t)q];
    std::vector<LoopMeasurementCov> loops(L);
    for (size_t k = 0; k < L; ++k) {
        loops[k].a = (int)a[k];
        loops[k].b = (int)b[k];
        for (int q = 0; q < 16; ++q) loops[k].Z.data()[q] = Z[16 * k + (size_t)q];
        for (int q = 0; q < 36; ++q) loops[k].cov.data()[q] = S[36 * k + (size_t)q];
    }
    std::vector<elimaloc::Matrix6d> Qs(qc);
    for (size_t v = 0; v < qc; ++v)
        for (int q = 0; q < 36; ++q) Qs[v].data()[q] = Q[36 * v + (size_t)q];
    const LoopConsistencyCovResult r = LoopConsistencyCov(poses, loops, Qs, &c);
    std::printf("%d %lld %d %lld\n", r.result.size, (long long)r.result.adjacent_pairs, r.result.steps, (long long)r.result.non_finite_pairs);
    for (int m : r.members()) std::printf("%d ", m);
    std::printf("\n");
    for (int32_t d : r.degree) std::printf("%d ", (int)d);
    std::printf("\n");
    std::vector<elimaloc::Matrix6d> local;
    const std::vector<elimaloc::Matrix6d> W = ChainCovariance(poses, Qs, &local);
    double tr = 0.0, trl = 0.0;
    for (int q = 0; q < 6; ++q) {
        tr += W[n - 1].data()[q * 7];
        trl += local[n - 1].data()[q * 7];
    }
    std::printf("%.17g %.17g\n", tr, trl);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return run_file(argv[1]);
    elm_loops_config c;
    elm_loops_config_default(&c);
    elm_loopcov_result r;
    uint8_t member = 0;
    int32_t degree = 0;
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double Q[36] = {0}, W[36];
    for (int q = 0; q < 6; ++q) Q[q * 7] = 1.0;
    const bool refused = elm_loopcov_consistency(nullptr, I, 1, nullptr, nullptr, nullptr, nullptr, 0, Q, 1, &c, &r, &member, &degree, nullptr, nullptr) ==
                             ELM_ERR_INVALID &&
                         elm_loopcov_chain(nullptr, I, 1, Q, 1, W, nullptr) == ELM_ERR_INVALID;
    double e[6] = {1, 1, 1, 1, 1, 1}, cov[36], s = 1.0;
    const bool pair = elm_loopcov_pair_terms(I, I, I, I, Q, I, I, I, Q, Q, Q, e, cov, &s) == ELM_OK;
    bool zero = s == 0.0;
    for (double x : e) zero = zero && x == 0.0;
    bool four = true; // Sigma_e = I + (I + I) + I on identity poses
    for (int q = 0; q < 36; ++q) four = four && cov[q] == (q % 7 == 0 ? 4.0 : 0.0);
    const bool pair_refused = elm_loopcov_pair_terms(I, I, I, I, Q, I, I, I, Q, Q, nullptr, e, cov, &s) == ELM_ERR_INVALID;
    LoopMeasurementCov m;
    return (refused && pair && zero && four && pair_refused && m.cov.data()[7] == 1.0 && sizeof(elm_loopcov_result) == 48) ? 0 : 1;
}
