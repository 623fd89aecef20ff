"""The pose graph's priors (include/elimaloc_hip_posegraph_prior.h) on the CPU: the mirror of the contract
(tests/posegraph_prior_ref.py) against central differences of its own residual; the library's elm_posegraph_prior_terms (the code the
kernel runs, compiled for the host) against the mirror, against elm_posegraph_edge_terms at a zero lever arm, and on a case worked out by
hand; the priors' Huber threshold; the mirror's completed dense system against its block-sparse product and conjugate gradients; the two
anchored-ring fixtures and their committed recording; the symbols, the argument errors without a device and the C++ shim's call lines."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_prior_cases as pcases
import posegraph_prior_ref as pref
import posegraph_ref as ref
import test_binding
from test_posegraph_abi import LIB_VS_MIRROR, MIRROR_VS_DIFFERENCES  # the same bounds, measured there

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_posegraph_prior.h"
NAMES = {"elm_posegraph_reserve_priors", "elm_posegraph_add_priors", "elm_posegraph_prior_count", "elm_posegraph_get_priors",
         "elm_posegraph_clear_priors", "elm_posegraph_set_prior_huber", "elm_posegraph_get_prior_huber",
         "elm_posegraph_download_prior_linearization", "elm_posegraph_prior_terms"}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the Jacobian
def _central_differences(T, Z, lever, h=1e-6):
    J = np.zeros((6, 6))
    one = np.ones(1, bool)
    for k in range(6):
        d = np.zeros((1, 6))
        d[0, k] = h
        J[:, k] = (pref.prior_residual(ref.retract(T[None], d, one)[0], Z, lever) - pref.prior_residual(ref.retract(T[None], -d, one)[0], Z, lever)) / (2.0 * h)
    return J


def _random_priors():
    """the pose generator of test_posegraph_abi.test_jacobians_against_central_differences, lever arms up to 2 m; relative rotations up
    to 3 rad (below 3.1: a step of 1e-6 across pi meets Log's jump) and the rotation family's angles below 3.1"""
    rng = np.random.default_rng(1)
    out = []
    for t in range(400):
        T = cases.rand_pose(rng, 3.0, 10.0)
        out.append((T, T @ cases.rand_pose(rng, 3.0 if t % 2 else 0.5, 1.0), rng.uniform(-2.0, 2.0, 3)))
    g, P = pcases.rotation_family()
    out += [(g.poses[P.node[q]], P.Z[q], P.lever[q]) for q in range(P.P) if cases.ROT_FAMILY[q] < 3.1]
    return out


def test_mirror_jacobian_against_central_differences():
    worst = 0.0
    for T, Z, lever in _random_priors():
        _, J = pref.prior_terms(T, Z, lever)
        worst = max(worst, np.abs(J - _central_differences(T, Z, lever)).max() / max(1.0, np.abs(J).max()))
    print(f"mirror against central differences {worst:.3e}")
    assert worst <= MIRROR_VS_DIFFERENCES


def test_library_prior_terms_against_the_mirror(L):
    from elimaloc_amd.posegraph import PriorTerms
    worst = 0.0
    for T, Z, lever in _random_priors():
        r, J = pref.prior_terms(T, Z, lever)
        rl, Jl = PriorTerms(T, Z, lever)
        worst = max(worst, np.abs(r - rl).max(), np.abs(J - Jl).max())
    print(f"library against mirror {worst:.3e}")
    assert worst <= LIB_VS_MIRROR


def test_zero_lever_is_the_edge_from_the_identity(L):
    """with l = 0, r and J equal as numbers the r and B of EdgeTerms(I, T, Z), across the branches of Log and of c(theta)"""
    from elimaloc_amd.posegraph import EdgeTerms, PriorTerms
    rng = np.random.default_rng(3)
    for th in cases.ROT_FAMILY:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        T = cases.rand_pose(rng, 3.0, 10.0)
        Z = np.eye(4)
        Z[:3, :3] = T[:3, :3] @ ref.exp_so3(-th * ax)
        Z[:3, 3] = T[:3, 3] + rng.uniform(-1.0, 1.0, 3)
        re_, _, B = EdgeTerms(np.eye(4), T, Z)
        for lever in (None, np.zeros(3)):
            r, J = PriorTerms(T, Z, lever)
            assert (r == re_).all() and (J == B).all(), th


def test_hand_case_is_exact(L):
    from elimaloc_amd.posegraph import PriorTerms
    g, P, want_r, want_s = pcases.hand_integers()
    lin = pref.linearize(g, P)
    assert lin["pr"].tobytes() == want_r.tobytes() and not np.signbit(lin["pr"][:, 3:]).any()  # Log(I) is +0
    assert lin["ps"].tobytes() == want_s.tobytes() and (lin["pw"] == 1.0).all() and lin["chi2"] == 23.0
    for q in range(P.P):
        want_J = np.eye(6)
        want_J[:3, 3:] = -ref.hat(P.lever[q])
        r, J = PriorTerms(g.poses[q], P.Z[q], P.lever[q])
        assert r.tobytes() == want_r[q].tobytes() and (J == want_J).all() and (lin["pJ"][q] == want_J).all()
        assert float(r @ P.info[q] @ r) == want_s[q]
    # H_q = J^T Omega J and g_q = J^T Omega r of a diagonal Omega, in integers
    assert (lin["diag"][1] == np.diag([4.0, 4.0, 1.0, 0.0, 0.0, 0.0])).all() and not lin["grad"][1].any()
    J0 = lin["pJ"][0]
    assert (lin["diag"][0] == J0.T @ P.info[0] @ J0).all() and (lin["grad"][0] == J0.T @ P.info[0] @ want_r[0]).all()
    assert lin["active"].all()  # free nodes that have only priors are active


def test_prior_huber_threshold_is_closed():
    g, P, _, want_s = pcases.hand_integers()  # s = 13, 0, 10
    P = P.take([0, 2])
    k = float(np.sqrt(np.float64(16.0)))
    P.info[0] = np.diag([4.0, 2.0, 3.0, 1.0, 1.0, 1.0])  # s = 4 + 12 = 16 = k^2
    lin = pref.linearize(g, P, prior_huber_k=k)
    assert lin["ps"].tolist() == [16.0, 10.0] and lin["pw"].tolist() == [1.0, 1.0] and lin["n_outliers"] == 0  # s == k^2 is an inlier
    below = float(np.nextafter(4.0, 0.0))
    lin = pref.linearize(g, P, prior_huber_k=below)
    assert lin["pw"][0] == below / 4.0 and lin["pw"][0] < 1.0 and lin["pw"][1] == 1.0 and lin["n_outliers"] == 1
    assert lin["cost"] == ((2.0 * below) * 4.0 - below * below) + 10.0
    assert pref.cost(g, P, g.poses, 0.0, below) == lin["cost"]
    lin = pref.linearize(g, P, huber_k=0.5, prior_huber_k=0.0)  # the edges' threshold does not reach the priors
    assert (lin["pw"] == 1.0).all() and lin["cost"] == 26.0


# ---------------------------------------------------------------- the mirror's own consistency
SYSTEMS = {"fixed_and_priors": pcases.fixed_and_priors, "priors_only": pcases.priors_only}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_mirror_dense_and_block_sparse_agree_with_priors(name):
    g, P = SYSTEMS[name]()
    lin = pref.linearize(g, P, huber_k=1.5, prior_huber_k=1.0)
    assert lin["active"].sum() == g.N - int(g.fixed.sum())
    rng = np.random.default_rng(7)
    for lam in (0.0, 1.0):
        H, b = pref.dense_system(g, lin, lam)
        p = rng.normal(size=(g.N, 6))
        p[~lin["active"]] = 0.0
        q = ref.spmv(g, lin, lam, p)
        want = (H @ p.reshape(-1)).reshape(g.N, 6)
        want[~lin["active"]] = 0.0
        assert np.abs(q - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
        delta, its, rel, conv = ref.pcg(g, lin, lam, 1e-10, 500)
        x = np.linalg.solve(H, b).reshape(g.N, 6)
        rho = pref.true_rel_residual(g, lin, lam, delta)
        print(f"{name} lambda {lam}: {its} iterations, recurrence residual {rel:.2e}, true relative residual {rho:.2e}")
        assert conv and rho <= 1e-8 and np.abs(delta - x).max() <= 1e-7 * max(1.0, np.abs(x).max())
        assert (delta[~lin["active"]] == 0.0).all()
    # without priors the completed system is posegraph_ref's
    none = pref.Priors()
    l0, lr = pref.linearize(g, none, huber_k=1.5), ref.linearize(g, huber_k=1.5)
    assert all(np.asarray(l0[k]).tobytes() == np.asarray(lr[k]).tobytes() for k in lr)
    if g.fixed.any():
        assert np.array_equal(pref.dense_system(g, l0, 1.0)[0], ref.dense_system(g, lr, 1.0)[0])


def test_mirror_sums_priors_after_edges_in_ascending_prior_order():
    g, P = pcases.node_counts()
    lin = pref.linearize(g, P)
    edges = ref.linearize(g)
    v = 9
    acc = edges["diag"][v].copy()
    for q in np.flatnonzero(P.node == v):
        acc = acc + lin["pH"][q]
    assert acc.tobytes() == lin["diag"][v].tobytes() and (P.node == v).sum() == 70


# ---------------------------------------------------------------- the fixtures
def test_the_anchored_ring_fixtures_and_their_recording():
    g, P, truth = pcases.anchored_ring()
    assert g.N == 64 and g.E == 63 and not g.fixed.any() and P.P == 8 and P.node.tolist() == list(range(0, 64, 8))
    assert (P.info[:, 3:, :] == 0.0).all() and (P.info[:, :, 3:] == 0.0).all() and (P.info[:, :3, :3] == np.diag([4.0, 4.0, 1.0])).all()
    assert pref.cost(g, P, truth) <= 1e-24  # the edges and the positions are the truth's own
    run = pcases.mirror_rings()
    accepted, clear, dt, dr, dt0 = pcases.anchor_conditions(run)
    assert accepted, "a rejected step: reseed the drift, not the rule"
    assert clear, "a step with F_new / F within 1e-3 of 1: reseed the drift"
    assert dt <= 1e-4 and dr <= 1e-5  # the project's pose tolerance, against the truth
    assert dt0 > 1.0  # the start is well off
    assert str(run["anchor_stop"]) == "step_tol" and len(run["anchor_cost"]) >= 3
    # the outlier: every step accepted, the planted prior ends as the only one with a weight below 0.1, and the end is nearer the
    # truth than the same run with the threshold off (Huber bounds the pull, it does not remove it)
    oacc, only, d_on, d_off = pcases.outlier_conditions(run)
    print(f"outlier: {d_on:.2f} m from the truth with the threshold, {d_off:.2f} m without; accepted without: {run['plain_accepted'].tolist()}")
    assert oacc and only and d_on < d_off and len(run["outlier_cost"]) == pcases.OUTLIER_SOLVES
    gold = np.load(pcases.GOLDEN)
    assert set(gold.files) == set(run)
    for k in ("anchor_accepted", "outlier_accepted", "plain_accepted", "anchor_stop", "outlier_stop", "truth", "anchor_start", "outlier_start"):
        assert np.asarray(run[k]).tobytes() == gold[k].tobytes(), k
    for name in ("anchor", "outlier"):  # (libm may differ between hosts by an ulp: the recording is compared as numbers)
        assert max(ref.pose_error(run[name + "_poses"], gold[name + "_poses"])) <= 1e-9
        assert np.allclose(run[name + "_cost"], gold[name + "_cost"], rtol=1e-6, atol=1e-20)


# ---------------------------------------------------------------- the ABI
def test_the_new_header_against_its_signature_table(L):
    from elimaloc_amd import _lib
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_PGPRIOR
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_PGPRIOR == list(table)
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params and restype is C.c_int and ret == "int", name
        fn = getattr(L, name)  # exported, and carrying what the table says
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # elimaloc_hip.h's own list of pose-graph calls is unchanged: one include line and nothing else
    import test_posegraph_abi
    top = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", top, flags=re.S)
    assert test_posegraph_abi.NAMES == set(re.findall(r"\b(elm_posegraph_[a-z0-9_]+)\s*\(", src))
    assert top.count('#include "elimaloc_hip_posegraph_prior.h"') == 1 and '#include "elimaloc_hip_posegraph_cov.h"\n#include "elimaloc_hip_posegraph_prior.h"\n' in top
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT) | set(_lib.EXPORTS_LOOPS) | set(_lib.EXPORTS_LOOPCOV) | set(_lib.EXPORTS_PGCOV)
    assert not NAMES & others
    import __graft_entry__ as g
    assert "EXPORTS_PGPRIOR" in open(g.__file__).read()  # build()'s missing-symbol check reads the new table
    assert "ELM_POSEGRAPH_MAX_PRIORS (1 << 22)" in open(os.path.join(ROOT, "include", HEADER)).read() and _lib.POSEGRAPH_MAX_PRIORS == 1 << 22


def test_the_header_compiles_as_c():
    probe = ('#include "elimaloc_hip.h"\nint main(void) { double r[6], J[36], k = 0.0; size_t n = 0;\n'
             '  return elm_posegraph_reserve_priors(0, 0, 1) == ELM_ERR_INVALID && elm_posegraph_prior_count(0, 0, &n) == ELM_ERR_INVALID &&\n'
             '         elm_posegraph_get_prior_huber(0, 0, &k) == ELM_ERR_INVALID && elm_posegraph_prior_terms(0, 0, 0, r, J) == ELM_ERR_INVALID ? 0 : 1; }\n')
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=probe.encode(), check=True)


def test_invalid_arguments_without_device(L):
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    nan, inf = float("nan"), float("inf")
    ptr = lambda a: a.ctypes.data_as(dp)
    # reserve: the capacity is 1 .. 2^22
    assert L.elm_posegraph_reserve_priors(None, one, 4) == INVALID and L.elm_posegraph_reserve_priors(one, None, 4) == INVALID
    for cap in (0, -1, (1 << 22) + 1):
        assert L.elm_posegraph_reserve_priors(one, one, cap) == INVALID, cap
    # add: NULLs, a negative node, a non-finite Z / lever / Omega, an Omega that is not exactly symmetric -- all before the object is read
    node = np.array([0, 1], np.int32)
    Z = np.tile(np.eye(4).ravel(), 2)
    lever = np.zeros(6)
    info = np.tile(np.eye(6).ravel(), 2)
    npn = node.ctypes.data_as(i32p)
    assert L.elm_posegraph_add_priors(None, one, npn, ptr(Z), ptr(lever), ptr(info), 2) == INVALID
    assert L.elm_posegraph_add_priors(one, None, npn, ptr(Z), ptr(lever), ptr(info), 2) == INVALID
    for args in ((None, ptr(Z), ptr(lever), ptr(info)), (npn, None, ptr(lever), ptr(info)), (npn, ptr(Z), ptr(lever), None)):
        assert L.elm_posegraph_add_priors(one, one, *args, 2) == INVALID
    neg = np.array([0, -1], np.int32)
    assert L.elm_posegraph_add_priors(one, one, neg.ctypes.data_as(i32p), ptr(Z), ptr(lever), ptr(info), 2) == INVALID
    assert L.elm_posegraph_add_priors(one, one, npn, ptr(Z), ptr(lever), ptr(info), (1 << 22) + 1) == INVALID
    for v in (nan, inf, -inf):
        for base, at, slot in ((Z, 16 + 13, 1), (lever, 3 + 1, 2), (info, 36 + 7, 3)):
            bad = base.copy()
            bad[at] = v
            args = [npn, ptr(Z), ptr(lever), ptr(info)]
            args[slot] = ptr(bad)
            assert L.elm_posegraph_add_priors(one, one, *args, 2) == INVALID, (v, slot)
    bad = info.copy()
    bad[36 + 1 * 6 + 2] = 0.5
    bad[36 + 2 * 6 + 1] = float(np.nextafter(0.5, 1.0))  # symmetric to the last bit but one
    assert L.elm_posegraph_add_priors(one, one, npn, ptr(Z), None, ptr(bad), 2) == INVALID
    # count, get, clear, the threshold, the download
    n, k = C.c_size_t(7), C.c_double(3.0)
    assert L.elm_posegraph_prior_count(one, one, None) == INVALID and L.elm_posegraph_prior_count(None, one, C.byref(n)) == INVALID
    assert L.elm_posegraph_prior_count(one, None, C.byref(n)) == INVALID and n.value == 7
    assert L.elm_posegraph_get_priors(None, one, 0, 1, None, None, None, None) == INVALID
    assert L.elm_posegraph_get_priors(one, None, 0, 1, None, None, None, None) == INVALID
    assert L.elm_posegraph_clear_priors(None, one) == INVALID and L.elm_posegraph_clear_priors(one, None) == INVALID
    assert L.elm_posegraph_set_prior_huber(None, one, 1.0) == INVALID and L.elm_posegraph_set_prior_huber(one, None, 1.0) == INVALID
    for bad_k in (-1.0, nan, inf, -inf):
        assert L.elm_posegraph_set_prior_huber(one, one, bad_k) == INVALID, bad_k
    assert L.elm_posegraph_get_prior_huber(one, one, None) == INVALID and L.elm_posegraph_get_prior_huber(None, one, C.byref(k)) == INVALID
    assert L.elm_posegraph_get_prior_huber(one, None, C.byref(k)) == INVALID and k.value == 3.0
    assert L.elm_posegraph_download_prior_linearization(None, one, None, None, None, None) == INVALID
    assert L.elm_posegraph_download_prior_linearization(one, None, None, None, None, None) == INVALID
    # prior terms: host only
    r = np.full(6, 5.0)
    I4 = np.eye(4).ravel()
    assert L.elm_posegraph_prior_terms(None, ptr(I4), None, ptr(r), None) == INVALID and L.elm_posegraph_prior_terms(ptr(I4), None, None, ptr(r), None) == INVALID
    bad = I4.copy()
    bad[12] = nan
    assert L.elm_posegraph_prior_terms(ptr(bad), ptr(I4), None, ptr(r), None) == INVALID and L.elm_posegraph_prior_terms(ptr(I4), ptr(bad), None, ptr(r), None) == INVALID
    assert L.elm_posegraph_prior_terms(ptr(I4), ptr(I4), ptr(np.array([0.0, inf, 0.0])), ptr(r), None) == INVALID and (r == 5.0).all()
    assert L.elm_posegraph_prior_terms(ptr(I4), ptr(I4), None, None, None) == 0
    from elimaloc_amd._lib import ElmError
    from elimaloc_amd.posegraph import PoseGraph
    pg = PoseGraph.__new__(PoseGraph)  # no device: the lengths are checked before the library is asked
    with pytest.raises(ElmError, match="one Z, information and lever per prior"):
        pg.AddPriors([0, 1], np.eye(4)[None])
    with pytest.raises(ElmError, match="one position, information and lever per prior"):
        pg.AddPositionPriors([0, 1], np.zeros((3, 3)))


def test_shim_prior_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/posegraph_prior_calls.cpp, built as tests/test_posegraph_abi.py builds posegraph_calls.cpp"""
    exe = tmp_path / "posegraph_prior_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "posegraph_prior_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
