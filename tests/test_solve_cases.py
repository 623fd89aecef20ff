"""The 6x6 solve at Eigen's discrete decisions, on the CPU (cases: tests/solve_cases.py).

Two halves.  The first pins the cases: the oracle and the numpy statement of the published routine agree on every one, the zeroed
components are exact zeros, the nonsingular ones agree with a 50-digit solve, and the cases can tell the two pivot searches apart.  The
second compiles csrc/elm_la.hpp for the host (as tests/test_sincosf.py does) and holds elm::ldlt_solve6 -- the function k_align_solve
runs on the device -- and elm::inv6 to the same expectations.  No GPU needed."""
import numpy as np
import pytest

import np_ref
import solve_cases as SC

RTOL, ATOL = 1e-11, 1e-13   # the bound tests/test_oracle.py uses between the oracle and the numpy statement


@pytest.fixture(scope="module")
def cases():
    return SC.cases()


# ------------------------------------------------------------------------------------------------ the cases are what they claim
def test_default_lambda_is_the_shipped_one():
    from elimaloc_amd.registration import RegistrationConfig
    assert SC.default_lambda() == RegistrationConfig().lm_lambda and SC.default_lambda() > 0.0
    assert SC.TOL == 1.0 / 1.7976931348623157e308 and np.nextafter(SC.TOL, 1.0) > SC.TOL


def test_families_are_complete(cases):
    count = lambda rule: sum(c.rule == rule for c in cases)
    assert count(SC.PIVOT_ORDER) == 7 and count(SC.ZERO_PIVOT) >= 9 and count(SC.CUTOFF) == 7 and count(SC.SIGNED) == 20
    assert count(SC.RANDOM_PD) == 20 and count(SC.RANDOM_INDEF) == 20
    assert sorted(c.lam for c in cases if c.rule == SC.DAMPING) == sorted({0.0, 1e-6, SC.default_lambda(), 1.0})
    for c in cases:
        assert np.array_equal(c.A, c.A.T) and c.A.shape == (6, 6) and c.b.shape == (6,)
        # the pose bound of the device test is stated for |t| <= 10: T0 there has |t0| <= 1, so |R x_t| <= |x_t|_2 must stay below 9
        assert np.linalg.norm(c.x[:3]) <= 9.0, c.name
        if c.rule in (SC.RANDOM_PD, SC.RANDOM_INDEF):
            assert SC.cond_inf(SC.damped(c.A, c.lam)) <= 1e3
        if c.rule == SC.RANDOM_PD:
            assert np.linalg.eigvalsh(c.A).min() > 0
        if c.rule in (SC.RANDOM_INDEF, SC.SIGNED):
            ev = np.linalg.eigvalsh(c.A)
            assert ev.min() < 0 < ev.max()
    # the damping matrix: h + lam * h is inexact for the shipped factor on at least four of its diagonal entries
    import fractions
    d = next(c for c in cases if c.rule == SC.DAMPING and c.lam == 1e-6)
    inexact = [fractions.Fraction(h) + fractions.Fraction(1e-6) * fractions.Fraction(h) != fractions.Fraction(h + 1e-6 * h) for h in np.diag(d.A)]
    assert sum(inexact) >= 4


def test_oracle_and_numpy_statement_agree_on_every_case(oracle, cases):
    for c in cases:
        D = SC.damped(c.A, c.lam)
        assert np.array_equal(c.x, np_ref.eigen_ldlt_solve(D, c.b))
        np.testing.assert_allclose(oracle.ldlt_solve6(D, c.b), c.x, rtol=RTOL, atol=ATOL, err_msg=c.name)
        # the instrumented restatement that names pivots and zeroed components is the same rule
        np.testing.assert_allclose(SC.ldlt(D, c.b)[2], c.x, rtol=RTOL, atol=ATOL, err_msg=c.name)
        for i in SC.zeroed(c):
            assert c.x[i] == 0.0 and oracle.ldlt_solve6(D, c.b)[i] == 0.0, (c.name, i)


def test_zeroed_components_and_cutoff_rule(cases):
    by = {c.name: c for c in cases}
    assert SC.zeroed(by["zero-all"]) == [0, 1, 2, 3, 4, 5] and SC.zeroed(by["zero-first-indef"]) == [0, 1, 2, 3, 4, 5]
    assert sorted(SC.zeroed(by["zero-Z"])) == [1, 3, 4, 5]
    assert SC.zeroed(by["zero-middle-psd"]) == [1] and SC.zeroed(by["zero-last-psd"]) == [5] and SC.zeroed(by["zero-last-diagonal"]) == [1]
    for tag in ("x-axis", "xy"):
        assert len(SC.zero_pivots(by["zero-rank3-exact-" + tag])) == 3   # rank 3, exactly
    # where the zero pivot is met: first, in the middle (step 1), last
    step = lambda c: [k for k, d in enumerate(SC.ldlt(SC.damped(c.A, c.lam), c.b)[1]) if d == 0.0]
    assert step(by["zero-first-indef"])[0] == 0 and step(by["zero-step1-indef"]) == [1] and step(by["zero-middle-psd"]) == [1]
    assert step(by["zero-last-psd"]) == [5] and step(by["order-zero-step1-012"]) == [1]
    # the issue's worked example
    assert np.array_equal(by["order-zero-step1-012"].x, [0.3125, -0.5, 0.5, 2.0, 5.0, 12.0])
    # the cut-off: divided only when |d| > 1 / DBL_MAX, else exactly 0 -- 2 d / d = 2 exactly, also for subnormal d
    want = {"0": 0.0, "tol": 0.0, "tol-next": 2.0, "5.58e-309": 2.0, "5.6e-309": 2.0, "5.6e-309-next": 2.0, "1e-300": 2.0}
    for label, x0 in want.items():
        c = by["cutoff-" + label]
        assert c.x[0] == x0 and np.array_equal(c.x[1:], c.b[1:]), label
        assert (SC.zeroed(c) == [0]) == (x0 == 0.0)


def test_nonsingular_cases_agree_with_50_digits(cases):
    n = 0
    for c in cases:
        if not SC.nonsingular(c):
            continue
        x, _ = SC.mp_solve(c)
        # cond_inf <= 1e3 asserted for the random families (the fixed ones are milder): a backward-stable solve is within
        # cond * 6 * eps ~ 1.3e-12 relative to |x|_inf; diagonal pivoting on an indefinite matrix may grow, hence 1e-9 as tests/test_oracle.py
        np.testing.assert_allclose(c.x, x, rtol=0, atol=1e-9 * max(1.0, np.abs(x).max()), err_msg=c.name)
        n += 1
    assert n == 72  # 3 + 5 + 20 + 4 + 20 + 20


def test_cases_tell_the_two_pivot_searches_apart(cases):
    by = {c.name: c for c in cases}
    for c in cases:
        D = SC.damped(c.A, c.lam)
        p0, _, x0 = SC.ldlt(D, c.b, "original")
        p1, _, x1 = SC.ldlt(D, c.b, "schur")
        if c.rule == SC.PIVOT_ORDER and c.name != "order-equal-diagonal":
            assert p0 != p1, c.name           # a Schur-diagonal search takes another pivot sequence
        if c.name in SC.NONZERO_COLUMN:
            assert not np.allclose(x0, x1, rtol=1e-6, atol=1e-6), c.name   # ... and, at a zero pivot with a non-zero column, another x
        elif c.name.startswith("order-differs"):
            np.testing.assert_allclose(x0, x1, rtol=RTOL, atol=ATOL)       # no zero pivot: both orders agree to rounding
    # (a zero pivot of a semidefinite matrix has a zero column -- |a_ij|^2 <= a_ii a_jj on the Schur complement -- and a matrix with a zero
    # diagonal is all zero pivots under either search: those cases return one x whatever the search, and say so here)
    for name in ("zero-middle-psd", "zero-last-psd", "zero-Z", "zero-all", "zero-first-indef"):
        D = SC.damped(by[name].A, 0.0)
        assert np.array_equal(SC.ldlt(D, by[name].b, "original")[2], SC.ldlt(D, by[name].b, "schur")[2])
    assert len(SC.NONZERO_COLUMN) == 5 and all(n in by for n in SC.NONZERO_COLUMN)
    # equal diagonal entries: the first maximum wins, in both searches' first step
    assert SC.ldlt(by["order-equal-diagonal"].A, by["order-equal-diagonal"].b)[0][:3] == [0, 1, 2]


# ------------------------------------------------------------------------------------------------ csrc/elm_la.hpp compiled for the host
@pytest.fixture(scope="module")
def host_la(tmp_path_factory):
    return SC.build_host_la(tmp_path_factory.mktemp("elm_la_host"))


def test_host_compiled_ldlt_solve6_follows_the_rule(host_la, cases):
    """elm::ldlt_solve6 (the scalar solve of k_align_solve) on every case: x within the oracle / numpy bound of the expectation, exact
    zeros where the rule zeroes.  Only the lower triangle is read: the upper one is filled with NaN.  (The one case of
    solve_cases.ROUNDING_DECIDED is fed too, for a finite answer only: its x is the quotient of rounding residues.)"""
    feed = []
    for c in cases:
        D = SC.damped(c.A, c.lam)
        D[np.triu_indices(6, 1)] = np.nan
        feed.append((D, c.b))
    x, _ = host_la(feed, [])
    bad = []
    for c, got in zip(cases, x):
        ok = np.allclose(got, c.x, rtol=RTOL, atol=ATOL) and all(got[i] == 0.0 for i in SC.zeroed(c))
        if c.name in SC.ROUNDING_DECIDED:
            ok = bool(np.all(np.isfinite(got)))
        if not ok:
            bad.append(f"{c.name} [{c.rule}]: got {got.tolist()} want {c.x.tolist()}")
    assert not bad, "\n".join(bad)


def test_host_compiled_inv6(host_la, oracle, cases):
    """elm::inv6 (GICP's local_cov in k_align_solve): against the 50-digit inverse on the nonsingular cases (rtol 1e-7, atol 1e-12, the
    bound tests/test_correspondences.py holds this quantity to) and against the oracle's PartialPivLU inverse on the edges of partial
    pivoting -- equal column maxima (the first wins), a zero leading entry, an exchange at every step -- within rtol 1e-11 / atol 1e-13:
    the same pivots, a Gauss-Jordan sweep instead of LU plus substitutions.
    Observed (x86-64, g++ -O2): worst error against 50 digits = 2.3e-6 of the bound."""
    ns = [c for c in cases if SC.nonsingular(c) and c.rule != SC.CUTOFF]
    edges = SC.inverse_edges()
    _, inv = host_la([], [SC.damped(c.A, c.lam) for c in ns] + [A for _, A in edges])
    worst = 0.0
    for c, got in zip(ns, inv):
        want = SC.mp_solve(c)[1]
        worst = max(worst, float(np.max(np.abs(got - want) / (1e-12 + 1e-7 * np.abs(want)))))
        np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-12, err_msg=c.name)
    print(f"inv6 against 50 digits: worst error / bound = {worst:.3e}")
    for (name, A), got in zip(edges, inv[len(ns):]):
        np.testing.assert_allclose(got, oracle.inverse6(A), rtol=RTOL, atol=ATOL, err_msg=name)
        np.testing.assert_allclose(got @ A, np.eye(6), rtol=0, atol=1e-12, err_msg=name)
