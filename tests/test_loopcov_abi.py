"""The loop consistency check with a propagated covariance (include/elimaloc_hip_loopcov.h) on the CPU: the three
calls' symbols, signatures and struct layout against the fifth signature table, the argument errors that need no device, the C++ shim's
call lines, the host-only pair term against the mirror (tests/loopcov_ref.py), and the mirror's own properties: W against a direct
propagation, s under a rigid shift, the two forms of the pair term, and the conditions of the fixtures (tests/loopcov_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loopcov_cases as ccases
import loopcov_ref as cref
import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import test_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_loopcov.h"
NAMES = {"elm_loopcov_chain", "elm_loopcov_pair_terms", "elm_loopcov_consistency"}
OTHERS = ("elimaloc_hip.h", "elimaloc_hip_posegraph_precond.h", "elimaloc_hip_posegraph_init.h", "elimaloc_hip_loops.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the ABI
def test_the_new_header_against_its_signature_table(L):
    from elimaloc_amd import _lib
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_LOOPCOV
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_LOOPCOV == list(table) and len(table) == 3
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params, name
        assert restype is C.c_int and ret == "int", name
        fn = getattr(L, name)  # exported, and carrying what the table says
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert [len(table[n][1]) for n in ("elm_loopcov_chain", "elm_loopcov_pair_terms", "elm_loopcov_consistency")] == [7, 14, 16]
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for other in OTHERS:  # no new name in the text of the other headers, comments aside; one include line and nothing else
        assert not re.search(r"elm_loopcov|ELM_LOOPCOV", strip(other)), other
    assert not NAMES & (set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT) | set(_lib.EXPORTS_LOOPS))
    top = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    assert top.count("elimaloc_hip_loopcov") == 1 and '#include "elimaloc_hip_loops.h"\n#include "elimaloc_hip_loopcov.h"\n' in top
    import __graft_entry__ as g
    assert "EXPORTS_LOOPCOV" in open(g.__file__).read()  # build()'s missing-symbol check reads the fifth table


def test_struct_layout(L, tmp_path):
    from elimaloc_amd import _lib
    name, cls = "elm_loopcov_result", _lib.LoopCovResultC
    offs = ", ".join("offsetof(%s, %s)" % (name, f) for f, _ in cls._fields_)
    line = '  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs)
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + line + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    row = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_] and row[0] == 48
    assert [f for f, _ in cls._fields_] == ["size", "steps", "adjacent_pairs", "non_finite_pairs", "chain_ms", "adjacency_ms", "greedy_ms"]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.loops import LoopConsistencyConfig
    cfg, res = LoopConsistencyConfig(), _lib.LoopCovResultC()
    res.size = 7
    I, Q = np.eye(4).ravel(), np.eye(6).ravel()
    member, degree, W = np.full(1, 9, np.uint8), np.full(1, 9, np.int32), np.full(36, 5.0)
    dp, ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double)), lambda x, t: x.ctypes.data_as(C.POINTER(t))
    # a NULL context is refused before anything is read
    assert L.elm_loopcov_consistency(None, dp(I), 1, None, None, None, None, 0, dp(Q), 1, C.byref(cfg), C.byref(res), ptr(member, C.c_uint8),
                                     ptr(degree, C.c_int32), None, None) == INVALID
    assert L.elm_loopcov_chain(None, dp(I), 1, dp(Q), 1, dp(W), None) == INVALID
    assert res.size == 7 and member[0] == 9 and degree[0] == 9 and (W == 5.0).all()
    # the host-only pair term: a NULL or non-finite argument
    e, cov, s = np.full(6, 5.0), np.full(36, 5.0), np.full(1, 5.0)
    bad, inf = I.copy(), Q.copy()
    bad[13] = np.nan
    inf[7] = np.inf
    good = [I, I, I, I, Q, I, I, I, Q, Q, Q]
    for at, value in ((0, None), (3, None), (4, None), (10, None), (0, bad), (6, bad), (4, inf), (9, inf), (10, inf)):
        args = [value if k == at else x for k, x in enumerate(good)]
        assert L.elm_loopcov_pair_terms(*[None if x is None else dp(np.ascontiguousarray(x)) for x in args], dp(e), dp(cov), dp(s)) == INVALID, at
    for out in ((None, dp(cov), dp(s)), (dp(e), None, dp(s)), (dp(e), dp(cov), None)):
        assert L.elm_loopcov_pair_terms(*[dp(x) for x in good], *out) == INVALID
    assert (e == 5.0).all() and (cov == 5.0).all() and s[0] == 5.0
    # the preconditions by name, as the mirror states them (the library's texts are held against them on a live context)
    ok = dict(n=4, a=[0, 1], b=[2, 3], Z=np.tile(np.eye(4), (2, 1, 1)), Sigma=np.eye(6), Q=np.eye(6))
    assert cref.refusal(**ok) is None and cref.refusal(**{**ok, "Q": np.tile(np.eye(6), (3, 1, 1))}) is None
    asym = np.eye(6)
    asym[0, 1] = 1e-300
    indef = np.eye(6)
    indef[2, 2] = -1.0
    semi = np.eye(6)
    semi[5, 5] = 0.0
    nanq = np.eye(6)
    nanq[3, 3] = np.nan
    for change, why in ((dict(Q=asym), "Q not symmetric"), (dict(Q=nanq), "Q non-finite"), (dict(Q=np.tile(np.eye(6), (2, 1, 1))), "q_count"),
                        (dict(Q=np.tile(np.eye(6), (4, 1, 1))), "q_count"), (dict(Sigma=indef), "Sigma not positive definite"),
                        (dict(Sigma=semi), "Sigma not positive definite"), (dict(Sigma=asym), "Sigma not symmetric"),
                        (dict(Sigma=nanq), "Sigma non-finite"), (dict(q_t=1e-12), "q"), (dict(q_r=1.0), "q"), (dict(a=[0, 4]), "index"),
                        (dict(a=[2, 1]), "a == b"), (dict(gamma=0.0), "gamma"), (dict(steps_per_batch=0), "steps_per_batch"), (dict(n=0), "n"),
                        (dict(Z=np.full((2, 4, 4), np.inf)), "non-finite Z"), (dict(Q=-np.eye(6)), None)):  # Q need not be definite
        assert cref.refusal(**{**ok, **change}) == why, change
    assert cref.refusal(1, [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), asym) is None  # n = 1: q_count = 1 is accepted, nothing is read
    big = dict(n=4, a=np.zeros(2049, int), b=np.ones(2049, int), Z=np.tile(np.eye(4), (2049, 1, 1)), Sigma=np.eye(6), Q=np.eye(6))
    assert cref.refusal(**big) is None and cref.refusal(**big, want_s=True) == "ELM_LOOPS_MAX_S"


def test_shim_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/loop_covariance_calls.cpp, built as tests/test_loops_abi.py builds loop_consistency_calls.cpp"""
    exe = tmp_path / "loop_covariance_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "loop_covariance_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the pair term
def _close(got, want, what):
    err = float(np.abs(got - want).max())
    bound = 1e-12 * max(1.0, float(np.abs(want).max()))
    print(f"  {what}: |lib - mirror| {err:.3e} (bound {bound:.1e}), largest {float(np.abs(want).max()):.3e}")
    assert err <= bound, what


def _lib_pair(poses, a, b, Z, Sigma, W, k, l):
    from elimaloc_amd.loops import PairTermsCov
    return PairTermsCov(poses[0], poses[a[k]], poses[b[k]], Z[k], Sigma[k], poses[a[l]], poses[b[l]], Z[l], Sigma[l], cref.range_cov(W, a[k], a[l]),
                        cref.range_cov(W, b[k], b[l]))


def _mirror_pair(poses, a, b, Z, Sigma, W, k, l):
    e = lref.pair_e(poses[a[k]], poses[b[k]], Z[k], poses[a[l]], poses[b[l]], Z[l])
    cov = cref.pair_cov(poses, a[k], b[k], Z[k], Sigma[k], a[l], b[l], Z[l], Sigma[l], W)
    return e, cov, float(cref.ldl_form(cov, e))


def test_pair_terms_against_the_mirror():
    """random pairs over the random chain (half the loops reversed), and every pair of the planted fixture"""
    for name, c in (("random 65", ccases.random_case(65)), ("planted", ccases.planted_honest())):
        W = cref.chain_W(c["poses"], c["Q"])
        L = len(c["a"])
        k, l = np.triu_indices(L, 1)
        pick = np.random.default_rng(31).choice(k.size, min(k.size, 200), replace=False)
        worst = [0.0, 0.0, 0.0]
        for u, v in zip(k[pick], l[pick]):
            got, want = _lib_pair(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], W, u, v), _mirror_pair(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], W, u, v)
            assert np.array_equal(got[1], got[1].T)  # Sigma_e is exactly symmetric
            for q in range(3):
                err = float(np.abs(np.asarray(got[q]) - want[q]).max()) / max(1.0, float(np.abs(want[q]).max()))
                worst[q] = max(worst[q], err)
            worst[2] = max(worst[2], abs(got[2] - c["s"][u, v]) / max(1.0, abs(c["s"][u, v])))  # and against the case's own s
        print(f"  {name}: worst |lib - mirror| / max(1, |mirror|): e {worst[0]:.3e}, Sigma_e {worst[1]:.3e}, s {worst[2]:.3e} (bound 1e-12)")
        assert max(worst) <= 1e-12, name


def test_pair_terms_with_a_failed_pivot_give_nan():
    c = ccases.random_case(2)
    W = cref.chain_W(c["poses"], -10.0 * np.eye(6))
    e, cov, s = _lib_pair(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], W, 0, 1)
    want = _mirror_pair(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], W, 0, 1)
    assert np.isnan(s) and np.isnan(want[2]) and np.isfinite(e).all() and np.isfinite(cov).all()


def test_s_is_exactly_zero_on_an_exact_cycle():
    """integer translations and quarter turns: every product is exact, the cycle composes to the identity, e and so s are exactly 0"""
    from elimaloc_amd.loops import PairTermsCov

    def pose(quarter_z, quarter_x, t):
        Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
        Rx = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
        T = np.eye(4)
        T[:3, :3] = np.linalg.matrix_power(Rz, quarter_z) @ np.linalg.matrix_power(Rx, quarter_x)
        T[:3, 3] = t
        return np.round(T)

    T = [pose(0, 1, [1, 2, 3]), pose(1, 0, [3, -2, 5]), pose(2, 1, [7, 7, -1]), pose(3, 3, [-4, 0, 2]), pose(0, 2, [10, -6, 1])]
    Zk = np.round(cases.inv_pose(T[1]) @ T[2])
    Zl = np.round(cases.inv_pose(T[3]) @ T[4])
    S = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    e, cov, s = PairTermsCov(T[0], T[1], T[2], Zk, S, T[3], T[4], Zl, S, 2.0 * S, 3.0 * S)
    assert (e == 0.0).all() and s == 0.0 and np.array_equal(cov, cov.T) and np.isfinite(cov).all()
    assert (lref.pair_e(T[1], T[2], Zk, T[3], T[4], Zl) == 0.0).all()


# ---------------------------------------------------------------- the mirror's properties
def test_w_differences_against_a_direct_propagation():
    """C(u, v) = W_v - W_u against the pose-by-pose propagation of the range in np.longdouble, one step at the far end included"""
    for name in ("1025-one", "1025-each", "257-shifted"):
        c = ccases.chain_case(name)
        n = c["n"]
        W = cref.chain_W(c["poses"], c["Q"], "sequential")
        for u, v in ((0, 1), (0, n - 1), (n - 2, n - 1), (n // 2, n // 2 + 37), (3, n - 5)):
            want = cref.direct_range(c["poses"], c["Q"], u, v)
            rel = float(np.abs(cref.range_cov(W, u, v) - want).max() / np.abs(want).max())
            print(f"  {name} range {u} .. {v}: |C - direct| / max |direct| {rel:.3e}")
            assert rel <= 1e-9, (name, u, v)


def test_s_is_invariant_under_a_rigid_shift():
    c = ccases.planted_honest()
    shift = cases.rand_pose(np.random.default_rng(32), 2.0, 1e3)
    moved = shift @ c["poses"]
    s = cref.pair_s(moved, c["a"], c["b"], c["Z"], c["Sigma"], cref.chain_W(moved, c["Q"]))
    rel = float((np.abs(s - c["s"]) / np.maximum(1.0, np.abs(c["s"]))).max())
    print(f"  planted, shifted by 1e3 m: worst |s - s0| / max(1, |s0|) {rel:.3e} (bound {max(ccases.S_FLOOR, c['bound']):.1e})")
    assert rel <= c["bound"]


def test_the_plain_and_the_one_sandwich_form_agree():
    for c in (ccases.planted_honest(), ccases.random_case(65)):
        W = cref.chain_W(c["poses"], c["Q"])
        k, l = np.triu_indices(len(c["a"]), 1)
        a, b = c["a"], c["b"]
        one = cref.pair_s_one_sandwich(c["poses"], a[k], b[k], c["Z"][k], c["Sigma"][k], a[l], b[l], c["Z"][l], c["Sigma"][l], W)
        rel = float((np.abs(one - c["s"][k, l]) / np.maximum(1.0, np.abs(c["s"][k, l]))).max())
        print(f"  plain against one-sandwich: worst relative {rel:.3e}")
        assert rel <= 1e-9


def test_the_planted_fixture_meets_its_five_conditions():
    p = ccases.planted_honest()  # asserts them
    raw = lcases.planted()
    assert ccases.HONEST_SEED == 2 and len(p["a"]) == 13 and int(p["is_true"].sum()) == 8
    # the chain and loops are loops_cases' own for the same seed
    seed0 = ccases._planted_raw(lcases.PLANTED_SEED)
    assert np.array_equal(seed0[1], raw["poses"]) and np.array_equal(seed0[2], raw["a"]) and np.array_equal(seed0[4], raw["Z"])
    print(f"  planted_honest: true-true s <= {p['true_true_max']:.2f}, with a false loop s >= {p['with_false_min']:.1f}, closest to gamma "
          f"{p['margin']:.2f}; the scalar model at the honest q keeps {p['scalar_true_pairs']} of {p['true_pairs']} true pairs")
    assert p["scalar_true_pairs"] < p["true_pairs"] == 28
    assert ccases.in_band(p["s"], p["gamma"], p["bound"]) == 0
    assert cref.refusal(lcases.PLANTED_N, p["a"], p["b"], p["Z"], p["Sigma"], p["Q"]) is None


def test_the_random_cases_have_no_pair_in_the_band():
    for L in ccases.SIZES:
        c = ccases.random_case(L)
        assert ccases.in_band(c["s"], c["gamma"], c["bound"]) == 0 and np.isfinite(c["s"]).all()
        assert cref.refusal(lcases.CHAIN_N, c["a"], c["b"], c["Z"], c["Sigma"], c["Q"]) is None
        if L >= 63:
            density = c["adj"].sum() / (L * (L - 1))
            assert 0.45 <= density <= 0.55, (L, density)


def test_the_mirror_orders_agree_on_the_chains():
    for name in ("3-one", "1025-each", "3073-one"):
        c = ccases.chain_case(name)
        print(f"  chain {name}: delta_W {c['delta_W']:.3e}, delta_S {c['delta_S']:.3e}")
        assert c["delta_W"] <= 1e-12 and c["delta_S"] <= 1e-10
        W = cref.chain_W(c["poses"], c["Q"], "pairwise")
        assert np.array_equal(W, np.swapaxes(W, 1, 2)) and not W[0].any()
