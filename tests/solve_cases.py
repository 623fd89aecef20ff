"""6x6 systems that sit ON the discrete decisions of the LM-damped solve ("as Eigen's LDLT does"), for
tests/test_solve_cases.py (CPU: the oracle, the numpy statement and csrc/elm_la.hpp compiled for the host) and tests/test_solve_step.py
(the device: wave_ldlt6 inside k_solve, fed through the exchange hook).  Plain numpy and mpmath, no GPU, no oracle.

The decisions, as the published routine takes them (Eigen/src/Cholesky/LDLT.h, ldlt_inplace<Lower>::unblocked and LDLT::_solve_impl):

* pivot order    the largest |entry| of the NOT-YET-UPDATED diagonal of the rows k.. (the routine is left-looking), the first of equal
                 maxima; a search on the updated (Schur complement) diagonal is a different rule and `ldlt(..., search="schur")` states it.
* zero pivot     an exactly zero pivot leaves its column of L undivided; the column takes part in both substitutions.
* cut-off        the component of a pivot is y / d only when |d| > 1 / DBL_MAX, otherwise it is exactly 0.

A case is `Case(name, A, b, lam, x, rule)`: A symmetric 6x6, the right-hand side, the LM factor, the expectation
`np_ref.eigen_ldlt_solve(damped(A, lam), b)` and the family it belongs to.  Every expectation comes from that numpy statement, never from
the code under test.  The damped matrix is A with every diagonal entry h replaced by `h + lam * h` (two roundings, what reg.cpp:55 does).
"""
import collections

import numpy as np

import np_ref

Case = collections.namedtuple("Case", "name A b lam x rule")

TOL = 1.0 / np.finfo(np.float64).max          # 5.562684646268003e-309, Eigen's cut-off (a subnormal)
assert TOL == 5.562684646268003e-309

PIVOT_ORDER, ZERO_PIVOT, CUTOFF, SIGNED, DAMPING, RANDOM_PD, RANDOM_INDEF = "pivot-order", "zero-pivot", "cut-off", "signed", "damping", "random-pd", "random-indef"
# zero-pivot cases whose undivided column is NOT zero (indefinite): the only ones on which the two pivot searches can return another x
NONZERO_COLUMN = set()
# cases whose zero pivots are zero only in exact arithmetic (see cases()): checked between implementations of ONE operation order only
ROUNDING_DECIDED = set()

_CACHE = {}


def default_lambda():
    """lm_lambda as elm_reg_config_default ships it."""
    if "lam" not in _CACHE:
        from elimaloc_amd.registration import RegistrationConfig
        _CACHE["lam"] = float(RegistrationConfig().lm_lambda)
    return _CACHE["lam"]


def damped(A, lam):
    D = np.array(A, dtype=np.float64)
    for i in range(6):
        D[i, i] = D[i, i] + lam * D[i, i]
    return D


def factor(A, search="original"):
    """P A P^T = L D L^T as the routine leaves it, with an explicit permutation and a switch for the pivot search: "original" is Eigen's
    rule, "schur" searches the updated diagonal.  Returns (pivot sequence as original indices, d in pivot order, L with the undivided
    columns of zero pivots)."""
    M = np.array(A, dtype=np.float64)
    M = np.tril(M) + np.tril(M, -1).T
    perm = list(range(6))
    L = np.zeros((6, 6))
    d = np.zeros(6)
    for k in range(6):
        if search == "original":
            diag = [abs(M[i, i]) for i in range(k, 6)]
        else:
            diag = [abs(M[i, i] - sum(L[i, c] * L[i, c] * d[c] for c in range(k))) for i in range(k, 6)]
        p = k + int(np.argmax(diag))  # the first maximum
        if p != k:
            M[[k, p], :] = M[[p, k], :]
            M[:, [k, p]] = M[:, [p, k]]
            L[[k, p], :] = L[[p, k], :]
            perm[k], perm[p] = perm[p], perm[k]
        d[k] = M[k, k] - sum(L[k, c] * (d[c] * L[k, c]) for c in range(k))
        for i in range(k + 1, 6):
            s = M[i, k] - sum(L[i, c] * (d[c] * L[k, c]) for c in range(k))
            L[i, k] = s / d[k] if d[k] != 0.0 else s
    return perm, d, L


def ldlt(A, b, search="original"):
    """The solve on factor(): (pivot sequence, d, x).  tests/test_solve_cases.py checks that its "original" x is
    np_ref.eigen_ldlt_solve's on every case, so the sequences and zeroed components reported here are the rule's."""
    perm, d, L = factor(A, search)
    y = np.array([b[perm[i]] for i in range(6)], dtype=np.float64)
    for i in range(6):
        for j in range(i):
            y[i] -= L[i, j] * y[j]
    for i in range(6):
        y[i] = y[i] / d[i] if abs(d[i]) > TOL else 0.0
    for i in range(5, -1, -1):
        for j in range(i + 1, 6):
            y[i] -= L[j, i] * y[j]
    x = np.zeros(6)
    for i in range(6):
        x[perm[i]] = y[i]
    return perm, d, x


def isolated_zero_pivots(D):
    """original indices of the pivots at or below the cut-off whose column of L is zero: the rows and columns of L^-T D^+ L^-1 that stay
    exactly zero (a zero pivot with a non-zero undivided column is reached by the back substitution)"""
    perm, d, L = factor(D)
    return [perm[k] for k in range(6) if not abs(d[k]) > TOL and not np.any(L[k + 1:, k])]


def zero_pivots(case):
    """original indices whose pivot is at or below the cut-off under Eigen's rule (in pivot order)"""
    perm, d, _ = ldlt(damped(case.A, case.lam), case.b)
    return [perm[k] for k in range(6) if not abs(d[k]) > TOL]


def zeroed(case):
    """components of x that the rule sets to exactly 0: a zero pivot's component stays 0 through the back substitution when no LATER
    pivot's undivided column reaches it, i.e. wherever the expectation itself is an exact zero at a zero pivot."""
    return [i for i in zero_pivots(case) if case.x[i] == 0.0]


def nonsingular(case):
    return not zero_pivots(case)


def mp_solve_matrix(Dn, b, dps=50):
    """(x, inverse) of a nonsingular 6x6 at `dps` digits, as float64 arrays"""
    import mpmath
    Dn = np.array(Dn, dtype=np.float64)
    with mpmath.workdps(dps):
        if np.array_equal(Dn, np.diag(np.diag(Dn))):  # (mpmath's LU calls a subnormal pivot singular)
            inv = mpmath.diag([1 / mpmath.mpf(float(v)) for v in np.diag(Dn)])
        else:
            inv = mpmath.matrix(Dn.tolist()) ** -1
        x = inv * mpmath.matrix([float(v) for v in b])
        return (np.array([float(v) for v in x]), np.array([[float(inv[i, j]) for j in range(6)] for i in range(6)]))


def mp_solve(case, dps=50):
    """(x, inverse) of the case's damped matrix at `dps` digits (nonsingular cases only)"""
    return mp_solve_matrix(damped(case.A, case.lam), case.b, dps)


def cond_inf(A):
    return np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf)


def _sym(diag, off=()):
    A = np.diag(np.array(diag, dtype=np.float64))
    for i, j, v in off:
        A[i, j] = A[j, i] = v
    return A


def _case(name, A, b, lam, rule):
    A = np.array(A, dtype=np.float64)
    b = np.array(b, dtype=np.float64)
    assert np.array_equal(A, A.T), name
    return Case(name, A, b, float(lam), np_ref.eigen_ldlt_solve(damped(A, lam), b), rule)


def _scaled(A, b, lam, bound=2.0):
    """b scaled by a power of two so that |x| <= bound (the pose tolerance of the device test is stated for |t| <= 10)"""
    x = np_ref.eigen_ldlt_solve(damped(A, lam), b)
    m = float(np.abs(x).max())
    return b if m <= bound else b * 2.0 ** -int(np.ceil(np.log2(m / bound)))


def zero_at_step_one(i, j, k):
    """diag 16, 4, 3 on (i, j, k), 2, 1, 0.5 on the rest in index order, A[i][j] = 8, A[j][k] = 1: after the pivot 16 Eigen takes the 4,
    whose updated value is 4 - 8 * 8 / 16 = 0 exactly -- a zero pivot with the undivided column entry 1 at row k; a Schur-diagonal search
    takes the 3 instead and never meets a zero.  Symmetric, indefinite (det of the i, j, k block = -16), nonsingular."""
    rest = [r for r in range(6) if r not in (i, j, k)]
    diag = np.zeros(6)
    diag[[i, j, k]] = (16.0, 4.0, 3.0)
    diag[rest] = (2.0, 1.0, 0.5)
    return _sym(diag, [(i, j, 8.0), (j, k, 1.0)])


def cases():
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = []
    b16 = np.arange(1.0, 7.0)
    # ---- pivot order ---------------------------------------------------------------------------------------------------------------
    for tri in ((0, 1, 2), (3, 4, 5), (5, 2, 0), (2, 4, 1)):
        name = "order-zero-step1-%d%d%d" % tri
        out.append(_case(name, zero_at_step_one(*tri), b16, 0.0, PIVOT_ORDER))
        NONZERO_COLUMN.add(name)
    H = np.full((6, 6), 0.25) + np.diag([2.0, 2.0, 2.0, 1.0, 2.0, 1.0])  # equal diagonal entries: the first maximum wins
    out.append(_case("order-equal-diagonal", H, b16, 0.0, PIVOT_ORDER))
    # the two searches take another order, no pivot is zero: positive definite (6 - 64 / 16 = 2 < 3) and indefinite (2.5 - 4 = -1.5)
    out.append(_case("order-differs-pd", _sym([16, 6, 3, 2, 1, 0.5], [(0, 1, 8.0), (1, 2, 1.0), (3, 5, 0.25)]), b16 / 4, 0.0, PIVOT_ORDER))
    out.append(_case("order-differs-indef", _sym([16, 2.5, 3, 2, 1, 0.5], [(0, 1, 8.0), (1, 4, 0.5)]), b16 / 4, 0.0, PIVOT_ORDER))
    # ---- exactly zero pivots, small integers -----------------------------------------------------------------------------------------
    J = np.array([[1, 0, 0, 0, 2, -1], [0, 1, 0, -2, 0, 3], [0, 0, 1, 1, -3, 0]], dtype=np.float64)
    # (tests/test_oracle.py calls this one "integers: no rounding", but its first pivot is 13: the columns of L are thirteenths, the
    # three pivots that are zero in exact arithmetic come out as -8.9e-16, -2.2e-16 and 0, and x is what the division by those residues
    # leaves.  Two left-looking implementations with the same operation order agree on it; an elimination in any other order cannot.)
    out.append(_case("zero-rank3-JtJ", J.T @ J, J.T @ np.array([1.0, -2.0, 0.5]), 0.0, ZERO_PIVOT))
    ROUNDING_DECIDED.add("zero-rank3-JtJ")
    # the same shape [I | -[p]x] for p = (2, 0, 0) and (2, 2, 0): every pivot is a power of two, every quotient dyadic, nothing rounds
    for tag, p in (("x-axis", (2.0, 0.0, 0.0)), ("xy", (2.0, 2.0, 0.0))):
        K = -np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        Jp = np.hstack([np.eye(3), K])
        out.append(_case("zero-rank3-exact-" + tag, Jp.T @ Jp, Jp.T @ np.array([1.0, -2.0, 0.5]), 0.0, ZERO_PIVOT))
    Z = np.zeros((6, 6)); Z[0, 0] = 4.0; Z[2, 2] = 1.0; Z[0, 2] = Z[2, 0] = 1.0
    out.append(_case("zero-Z", Z, [1.0, 5.0, 2.0, 7.0, 0.0, 3.0], 0.0, ZERO_PIVOT))
    out.append(_case("zero-all", np.zeros((6, 6)), np.ones(6), 0.0, ZERO_PIVOT))
    # met first: a zero diagonal, so the very first pivot is 0 and its undivided column (0, 2, 0, ...) is not; every later pivot is 0 too
    out.append(_case("zero-first-indef", _sym([0, 0, 0, 0, 0, 0], [(0, 1, 2.0), (2, 5, 1.0)]), b16, 0.0, ZERO_PIVOT))
    NONZERO_COLUMN.add("zero-step1-indef")
    out.append(_case("zero-step1-indef", zero_at_step_one(1, 3, 4), [2.0, -1.0, 0.5, 1.0, 3.0, -2.0], 0.0, ZERO_PIVOT))
    # in the middle, semidefinite: the [[4, 2], [2, 1]] block gives 1 - 2 * 2 / 4 = 0 at step 1 and the rest of its column is zero
    out.append(_case("zero-middle-psd", _sym([4, 1, 0.5, 0.5, 0.25, 0.25], [(0, 1, 2.0)]), b16 / 4, 0.0, ZERO_PIVOT))
    # last: [[1, 1], [1, 1]] at the end of the order, 1 - 1 * 1 / 1 = 0 at step 5
    out.append(_case("zero-last-psd", _sym([16, 8, 4, 2, 1, 1], [(4, 5, 1.0)]), b16, 0.0, ZERO_PIVOT))
    out.append(_case("zero-last-diagonal", _sym([4, 0, 2, 1, 1, 1], [(0, 2, 1.0)]), b16, 0.0, ZERO_PIVOT))
    # ---- the cut-off -------------------------------------------------------------------------------------------------------------------
    for label, dv in (("0", 0.0), ("tol", TOL), ("tol-next", np.nextafter(TOL, 1.0)), ("5.58e-309", 5.58e-309), ("5.6e-309", 5.6e-309),
                      ("5.6e-309-next", np.nextafter(5.6e-309, 1.0)), ("1e-300", 1e-300)):
        out.append(_case("cutoff-" + label, _sym([dv, 1, 1, 1, 1, 1]), [2.0 * dv, 1.0, -1.0, 0.5, 2.0, -0.25], 0.0, CUTOFF))
    # ---- negative and mixed-sign pivots: the orthogonal-similarity matrices of tests/test_oracle.py, same generator and seed ------------
    rng = np.random.default_rng(7)
    for n in range(20):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        A = Q @ np.diag([5.0, -3.0, 2.0, -1.5, 1.0, 0.7]) @ Q.T
        A = np.tril(A) + np.tril(A, -1).T
        out.append(_case("signed-%02d" % n, A, _scaled(A, rng.normal(size=6), 0.0), 0.0, SIGNED))
    # ---- damping: diagonal entries for which h + lam * h rounds (thirds, tenths, 1 + ulp), all three factors ----------------------------
    Dm = _sym([1.0 / 3.0, 0.7, 1.0 + 2.0 ** -52, 2.1, 5.0 / 7.0, 1.9], [(0, 1, 0.125), (1, 2, -0.25), (2, 3, 0.125), (3, 4, 0.0625), (4, 5, -0.125), (0, 5, 0.03125)])
    for lam in sorted({0.0, 1e-6, default_lambda(), 1.0}):
        out.append(_case("damping-lam-%g" % lam, Dm, b16 / 8, lam, DAMPING))
    # ---- well-conditioned random systems, at the default damping -----------------------------------------------------------------------
    rng = np.random.default_rng(4242)
    lam = default_lambda()
    n = 0
    while n < 20:
        G = rng.normal(size=(6, 12))
        A = G @ G.T / 12.0 + 0.5 * np.eye(6)
        A = np.tril(A) + np.tril(A, -1).T
        if cond_inf(damped(A, lam)) <= 1e3:
            out.append(_case("random-pd-%02d" % n, A, _scaled(A, rng.normal(size=6), lam), lam, RANDOM_PD))
            n += 1
    n = 0
    while n < 20:
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        ev = rng.uniform(0.5, 4.0, size=6) * np.where(np.arange(6) % 2 == 0, 1.0, -1.0)
        A = Q @ np.diag(ev) @ Q.T
        A = np.tril(A) + np.tril(A, -1).T
        if cond_inf(damped(A, lam)) <= 1e3:
            out.append(_case("random-indef-%02d" % n, A, _scaled(A, rng.normal(size=6), lam), lam, RANDOM_INDEF))
            n += 1
    for c in out:
        if c.rule in (RANDOM_PD, RANDOM_INDEF):
            assert cond_inf(damped(c.A, c.lam)) <= 1e3, c.name
    assert len({c.name for c in out}) == len(out)
    _CACHE["cases"] = out
    return out


# ---- 6x6 inverses (elm::inv6, Gauss-Jordan with partial pivoting; the reference's Matrix<double, 6, 6>::inverse() is PartialPivLU) -------
def inverse_edges():
    """(name, A) on the discrete decisions of partial pivoting: the first largest |entry| of the column is the pivot row.  Nonsingular,
    not symmetric, small dyadic entries."""
    rng = np.random.default_rng(99)
    out = []
    A = np.eye(6) * 2.0
    A[3, 0] = -2.0; A[5, 0] = 2.0; A[0, 4] = 1.0; A[3, 5] = 0.5   # column 0: |2|, |-2|, |2| -- row 0 stays
    out.append(("equal-column-maxima", A))
    A = np.eye(6)
    A[0, 0] = 0.0; A[0, 3] = 1.0; A[3, 0] = 2.0; A[3, 3] = 0.0; A[1, 0] = 2.0; A[1, 2] = 0.5  # a zero leading entry; rows 1 and 3 tie
    out.append(("zero-leading-entry", A))
    A = np.zeros((6, 6))                                              # a row exchange at every step: the big entries sit one row below
    for k in range(6):
        A[(k + 1) % 6, k] = 4.0 + k
        A[k, k] = 1.0
    A[0, 5] = 0.5
    out.append(("exchange-every-step", A))
    A = np.eye(6)                                                     # a tie met at step 2: rows 2, 3 and 5 of column 2 hold |3|, row 2 stays
    A[2, 2] = 3.0; A[3, 2] = -3.0; A[5, 2] = 3.0; A[2, 4] = 0.5; A[3, 5] = 0.25; A[0, 1] = 0.5
    out.append(("tie-at-step-two", A))
    A = np.round(rng.normal(size=(6, 6)) * 4.0) / 4.0 + 3.0 * np.eye(6)[:, [1, 0, 3, 2, 5, 4]]  # general, dyadic entries
    out.append(("general-dyadic", A))
    for name, M in out:
        assert abs(np.linalg.det(M)) > 1e-3 and cond_inf(M) < 1e4, name
    return out


# ---- csrc/elm_la.hpp compiled for the host (as tests/test_sincosf.py does) ----------------------------------------------------------------
HOST_SRC = r"""
#include <cstdio>
#include "elm_la.hpp"
// stdin: n_solve, n_inv, then n_solve records of 36 + 6 doubles (row-major A, b), then n_inv records of 36 doubles; raw float64.
// stdout: n_solve x 6 doubles (x) then n_inv x 36 doubles (row-major inverse), raw.
int main() {
    double head[2];
    if (std::fread(head, 8, 2, stdin) != 2) return 2;
    const int ns = (int)head[0], ni = (int)head[1];
    for (int c = 0; c < ns; ++c) {
        double rec[42], x[6];
        if (std::fread(rec, 8, 42, stdin) != 42) return 3;
        elm::ldlt_solve6(rec, rec + 36, x);
        std::fwrite(x, 8, 6, stdout);
    }
    for (int c = 0; c < ni; ++c) {
        double A[36], R[36];
        if (std::fread(A, 8, 36, stdin) != 36) return 4;
        elm::inv6(A, R);
        std::fwrite(R, 8, 36, stdout);
    }
    return 0;
}
"""


def build_host_la(directory):
    """Compile elm::ldlt_solve6 / elm::inv6 for the host into `directory`; returns run(solves [(A, b)], inverses [A]) -> (x [n, 6],
    inverse [m, 6, 6])."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(str(directory), "la.cpp")
    exe = os.path.join(str(directory), "la")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "elimaloc_amd", "csrc"), src, "-o", exe, "-lm"])

    def run(solves, inverses):
        buf = struct.pack("2d", len(solves), len(inverses))
        for A, b in solves:
            buf += np.ascontiguousarray(A, dtype=np.float64).tobytes() + np.ascontiguousarray(b, dtype=np.float64).tobytes()
        for A in inverses:
            buf += np.ascontiguousarray(A, dtype=np.float64).tobytes()
        out = np.frombuffer(subprocess.run([exe], input=buf, stdout=subprocess.PIPE, check=True, timeout=60).stdout, dtype=np.float64)
        assert out.size == 6 * len(solves) + 36 * len(inverses)
        return out[:6 * len(solves)].reshape(-1, 6), out[6 * len(solves):].reshape(-1, 6, 6)
    return run
