"""The pose graph (include/elimaloc_hip.h, "pose graph") on the CPU: the numpy mirror of the contract
(tests/posegraph_ref.py) on cases worked out by hand; its Jacobians and the library's (elm_posegraph_edge_terms, the code the kernel
runs, compiled for the host) against central differences of the mirror's residual; the mirror's own consistency (dense against
block-sparse, conjugate gradients against the dense solve); the loop fixture and its committed recording; the symbols, the struct
layouts, the argument errors without a device and the C++ shim's call lines."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

# Measured on the development host, each bound 10 x the worst value seen, to cover libm differences between hosts:
#   library against mirror, r / A / B of 400 random edges with relative rotations up to 3 rad: 1.8e-15 absolute on entries up to 30
#   mirror against central differences (step 1e-6), relative to max(1, max |J|): 1.8e-9
#   c(theta) of either branch against the np.longdouble closed form, theta in 5e-3 .. 2e-2: closed form 1.5e-11, series 3.6e-14 relative
LIB_VS_MIRROR = 1.8e-14
MIRROR_VS_DIFFERENCES = 1.8e-8
C_CLOSED_REL, C_SERIES_REL = 1.5e-10, 3.6e-13


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _exp_pose(phi, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = ref.exp_so3(np.asarray(phi, dtype=np.float64))
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------- by hand, exact
def test_integer_translations_are_exact(L):
    from elimaloc_amd.posegraph import EdgeTerms
    g, want_rt = cases.hand_integers()
    lin = ref.linearize(g)
    assert lin["r"][:, :3].tobytes() == want_rt.tobytes() and (lin["r"][:, 3:] == 0.0).all() and not np.signbit(lin["r"][:, 3:]).any()
    assert lin["s"].tolist() == [4.0, 9.0, 1.0, 18.0] and (lin["w"] == 1.0).all()
    for e in range(g.E):
        r, A, B = EdgeTerms(g.poses[g.i[e]], g.poses[g.j[e]], g.Z[e])
        assert r.tolist() == want_rt[e].tolist() + [0.0, 0.0, 0.0]
        assert (A[:3, :3] == -np.eye(3)).all() and (B == np.eye(6)).all() and (A[3:, 3:] == -np.eye(3)).all() and (A[3:, :3] == 0.0).all()
        assert (A[:3, 3:] == ref.hat(g.poses[g.j[e], :3, 3] - g.poses[g.i[e], :3, 3])).all()  # [d]x of the integer difference


def test_huber_threshold_is_closed():
    s = np.array([4.0])
    below = float(np.nextafter(2.0, 0.0))
    assert ref.huber_weight(s, 2.0)[0] == 1.0 and ref.huber_cost(s, 2.0)[0] == 4.0  # s == k^2 is an inlier
    assert ref.huber_weight(s, below)[0] < 1.0 and ref.huber_weight(s, below)[0] == below / 2.0
    assert ref.huber_cost(s, below)[0] == (2.0 * below) * 2.0 - below * below
    assert ref.huber_weight(s, 0.0)[0] == 1.0 and ref.huber_cost(np.array([1e9]), 0.0)[0] == 1e9  # off
    g, _ = cases.hand_integers()
    assert ref.linearize(g, huber_k=2.0)["w"].tolist() == [1.0, 2.0 / 3.0, 1.0, 2.0 / math.sqrt(18.0)]
    assert ref.linearize(g, huber_k=below)["n_outliers"] == 3


def test_log_of_the_identity_and_of_exp(L):
    from elimaloc_amd.posegraph import EdgeTerms
    assert (ref.log_so3(np.eye(3)) == 0.0).all() and not np.signbit(ref.log_so3(np.eye(3))).any()
    r, _, _ = EdgeTerms(np.eye(4), np.eye(4), np.eye(4))
    assert (r == 0.0).all() and not np.signbit(r).any()
    ax = np.array([2.0, -1.0, 2.0]) / 3.0
    for ang in (1e-12, 1.9e-8, 2.1e-8, 1.0, math.pi - 1e-6):  # 2e-8 is |phi| at the small-n branch (n = |phi| / 2 = 1e-8)
        phi = ang * ax
        got = ref.log_so3(ref.exp_so3(phi))
        lib = EdgeTerms(np.eye(4), _exp_pose(phi), np.eye(4))[0][3:]
        # Exp rounds its entries to 1e-16 absolute, which is all a rotation matrix holds of a small angle; near pi the quaternion's w is
        # 5e-7 and carries that rounding as 2e-10 relative
        tol = 4e-16 + (1e-9 if ang > 3.0 else 1e-15) * ang
        assert np.abs(got - phi).max() <= tol and np.abs(lib - phi).max() <= tol, ang


# ---------------------------------------------------------------- the Jacobians
def _central_differences(Ti, Tj, Z, h=1e-6):
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    one = np.ones(1, bool)
    for k in range(6):
        d = np.zeros((1, 6))
        d[0, k] = h
        A[:, k] = (ref.residual(ref.retract(Ti[None], d, one)[0], Tj, Z) - ref.residual(ref.retract(Ti[None], -d, one)[0], Tj, Z)) / (2.0 * h)
        B[:, k] = (ref.residual(Ti, ref.retract(Tj[None], d, one)[0], Z) - ref.residual(Ti, ref.retract(Tj[None], -d, one)[0], Z)) / (2.0 * h)
    return A, B


def test_jacobians_against_central_differences(L):
    from elimaloc_amd.posegraph import EdgeTerms
    rng = np.random.default_rng(1)
    worst_lib = worst_nd = 0.0
    edges = []
    for t in range(400):
        Ti = cases.rand_pose(rng, 3.0, 10.0)
        Tj = Ti @ cases.rand_pose(rng, 3.0, 5.0)
        edges.append((Ti, Tj, cases.inv_pose(Ti) @ Tj @ cases.rand_pose(rng, 3.0 if t % 2 else 0.5, 1.0)))
    fam = cases.rotation_family()
    # (below 3.1: a step of 1e-6 across pi meets Log's jump.  The angles above it, up to pi itself, are held against a 100-digit
    # derivative of the exact residual in tests/test_rotation_edges_abi.py)
    edges += [(fam.poses[fam.i[e]], fam.poses[fam.j[e]], fam.Z[e]) for e in range(fam.E) if cases.ROT_FAMILY[e] < 3.1]
    for Ti, Tj, Z in edges:
        r, A, B = ref.edge_terms(Ti, Tj, Z)
        rl, Al, Bl = EdgeTerms(Ti, Tj, Z)
        worst_lib = max(worst_lib, np.abs(r - rl).max(), np.abs(A - Al).max(), np.abs(B - Bl).max())
        An, Bn = _central_differences(Ti, Tj, Z)
        worst_nd = max(worst_nd, np.abs(A - An).max() / max(1.0, np.abs(A).max()), np.abs(B - Bn).max() / max(1.0, np.abs(B).max()))
    print(f"library against mirror {worst_lib:.3e}; mirror against central differences {worst_nd:.3e}")
    assert worst_lib <= LIB_VS_MIRROR and worst_nd <= MIRROR_VS_DIFFERENCES


def test_c_of_theta_on_both_sides_of_the_series_switch(monkeypatch):
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18
    worst = {"closed": 0.0, "series": 0.0}
    for theta in (5e-3, 9e-3, 9.9e-3, 1e-2, 1.01e-2, 1.5e-2, 2e-2):
        t = ld(theta)
        want = ld(1) / (t * t) - (ld(1) + np.cos(t)) / (ld(2) * t * np.sin(t))
        w, n = math.cos(theta / 2.0), math.sin(theta / 2.0)
        for name, switch in (("closed", 0.0), ("series", 1.0)):
            monkeypatch.setattr(ref, "SERIES_THETA", switch)
            got = float(ref.jinv_c(theta, w, n))
            worst[name] = max(worst[name], abs(float((ld(got) - want) / want)))
    monkeypatch.undo()
    print(f"c(theta): closed form {worst['closed']:.3e}, series {worst['series']:.3e} relative")
    assert worst["closed"] <= C_CLOSED_REL and worst["series"] <= C_SERIES_REL
    assert ref.SERIES_THETA == 1e-2 and float(ref.jinv_c(1e-9, 1.0, 5e-10)) == 1.0 / 12.0


def test_library_jinv_across_the_switch_and_near_pi(L):
    """B's lower right block is J^-1(phi): against I + [phi]x / 2 + c [phi]x^2 with c from the longdouble closed form"""
    from elimaloc_amd.posegraph import EdgeTerms
    ld = np.longdouble
    ax = np.array([1.0, 2.0, -2.0]) / 3.0
    for theta in (1e-5, 9.9e-3, 1e-2, 1.01e-2, 0.5, 3.0, math.pi - 1e-3):
        phi = theta * ax
        _, _, B = EdgeTerms(np.eye(4), _exp_pose(phi), np.eye(4))
        t = ld(theta)
        c = float(ld(1) / (t * t) - (ld(1) + np.cos(t)) / (ld(2) * t * np.sin(t)))
        K = ref.hat(phi)
        want = np.eye(3) + 0.5 * K + c * (K @ K)
        assert np.abs(B[3:, 3:] - want).max() <= 1e-12, theta  # (phi itself comes back from Log to 1e-15; J^-1 has entries of order 1)


# ---------------------------------------------------------------- the mirror's own consistency
SMALL = {"two": lambda: cases.chain(2, 1, loops=0), "chain12": lambda: cases.chain(12, 2), "star5": lambda: cases.star(5, 3),
         "random9": lambda: cases.random_graph(9, 20, 4, fixed=(0, 4), ang=0.3)}
RHO_REF = {}  # the mirror's true relative residual at pcg_rel_tol 1e-10, per fixture and lambda (tests/test_posegraph.py measures the same)


@pytest.mark.parametrize("name", list(SMALL))
def test_mirror_dense_and_block_sparse_agree(name):
    g = SMALL[name]()
    lin = ref.linearize(g, huber_k=1.5)
    rng = np.random.default_rng(7)
    for lam in (0.0, 1.0):
        H, b = ref.dense_system(g, lin, lam)
        p = rng.normal(size=(g.N, 6))
        p[~lin["active"]] = 0.0
        q = ref.spmv(g, lin, lam, p)
        want = (H @ p.reshape(-1)).reshape(g.N, 6)
        want[~lin["active"]] = 0.0
        assert np.abs(q - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
        delta, its, rel, conv = ref.pcg(g, lin, lam, 1e-10, 500)
        x = np.linalg.solve(H, b).reshape(g.N, 6)
        rho = ref.true_rel_residual(g, lin, lam, delta)
        RHO_REF[(name, lam)] = rho
        print(f"{name} lambda {lam}: {its} iterations, recurrence residual {rel:.2e}, true relative residual {rho:.2e}")
        assert conv and rho <= 1e-8 and np.abs(delta - x).max() <= 1e-7 * max(1.0, np.abs(x).max())
        assert (delta[~lin["active"]] == 0.0).all()


def test_mirror_sums_run_in_ascending_edge_order():
    g = cases.star(5, 3)
    lin = ref.linearize(g)
    acc = np.zeros((6, 6))
    for e in range(g.E):
        acc = acc + (lin["Hii"][e] if g.i[e] == 0 else lin["Hjj"][e])
    assert acc.tobytes() == lin["diag"][0].tobytes()


# ---------------------------------------------------------------- the loop fixture
def test_the_ring_fixture_and_its_recording():
    g, truth = cases.ring()
    assert g.N == 64 and g.E == 66 and g.fixed.tolist() == [True] + [False] * 63
    assert ref.cost(g, truth) <= 1e-24  # the edges are the truth's own
    run = cases.mirror_ring()
    accepted, clear, dt, dr = cases.ring_conditions(run)
    assert accepted, "a rejected step: reseed the drift (posegraph_cases.DRIFT_SEED), not the rule"
    assert clear, "a step with F_new / F within 1e-3 of 1: reseed the drift"
    assert dt <= 1e-4 and dr <= 1e-5  # the project's pose tolerance, against the truth
    assert str(run["ring_stop"]) == "step_tol" and len(run["ring_cost"]) >= 3
    dt0, dr0 = ref.pose_error(run["ring_start"], truth)
    assert dt0 > 1.0 and dr0 > 0.05  # the start is well off
    gold = np.load(cases.GOLDEN)
    assert set(gold.files) == set(run)
    for k in ("ring_accepted", "false_accepted", "ring_stop", "false_stop", "truth", "ring_start", "false_start"):
        assert np.asarray(run[k]).tobytes() == gold[k].tobytes(), k
    for name in ("ring", "false"):  # (libm may differ between hosts by an ulp: the recording is compared as numbers)
        assert max(ref.pose_error(run[name + "_poses"], gold[name + "_poses"])) <= 1e-9
        assert np.allclose(run[name + "_cost"], gold[name + "_cost"], rtol=1e-6, atol=1e-20)
    # the false loop under Huber: every step accepted, the cost falls, the false edge ends as the one outlier
    assert gold["false_accepted"].all() and float(gold["false_cost_final"]) < float(gold["false_cost_initial"])
    gf, _ = cases.ring(false_loop=True)
    lin = ref.linearize(gf, gold["false_poses"], cases.FALSE_CFG["huber_k"])
    assert lin["n_outliers"] == 1 and lin["w"][-1] < 0.1 and (lin["w"][:-1] == 1.0).all()


# ---------------------------------------------------------------- the ABI
NAMES = {"elm_posegraph_config_default", "elm_posegraph_create", "elm_posegraph_destroy", "elm_posegraph_reset", "elm_posegraph_size",
         "elm_posegraph_add_nodes", "elm_posegraph_set_poses", "elm_posegraph_get_poses", "elm_posegraph_set_fixed", "elm_posegraph_add_edges",
         "elm_posegraph_linearize", "elm_posegraph_download_linearization", "elm_posegraph_solve", "elm_posegraph_optimize",
         "elm_posegraph_edge_terms"}


def test_symbols_are_declared_and_exported(L):
    from elimaloc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read(), flags=re.S)
    assert NAMES == set(re.findall(r"\b(elm_posegraph_[a-z0-9_]+)\s*\(", src)) and NAMES <= set(_lib.EXPORTS)
    for n in NAMES:
        assert hasattr(L, n)
    for k, v in _lib.PG_STOP.items():
        assert re.search(r"#define ELM_PG_STOP_%s %d\b" % (v.upper(), k), src), v
    assert _lib.PG_STOP == ref.STOP and "ELM_POSEGRAPH_MAX_NODES (1 << 20)" in src and "ELM_POSEGRAPH_MAX_EDGES (1 << 22)" in src


def test_config_defaults(L):
    from elimaloc_amd.posegraph import PoseGraphConfig
    c = PoseGraphConfig()
    for k, v in ref.DEFAULTS.items():
        assert getattr(c, k) == v, k
    assert PoseGraphConfig(huber_k=2, max_iterations=3).huber_k == 2.0
    with pytest.raises(AttributeError):
        PoseGraphConfig(no_such_field=1)
    L.elm_posegraph_config_default(None)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    structs = {"elm_posegraph_config": (_lib.PoseGraphConfigC, {}), "elm_posegraph_linearize_stats": (_lib.PoseGraphLinearizeStatsC, {}),
               "elm_posegraph_solve_stats": (_lib.PoseGraphSolveStatsC, {}), "elm_posegraph_result": (_lib.PoseGraphResultC, {}),
               "elm_posegraph_trace": (_lib.PoseGraphTraceC, {"lambda_": "lambda"})}
    lines = []
    for name, (cls, rename) in structs.items():
        offs = ", ".join("offsetof(%s, %s)" % (name, rename.get(f, f)) for f, _ in cls._fields_)
        lines.append('  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs))
    lines.append('  printf("%zu %zu %zu\\n", sizeof(elm_places_config), sizeof(elm_place_candidate), sizeof(elm_odometry_config));')
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for row, (name, (cls, _)) in zip(rows, structs.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name
    assert [r[0] for r in rows[:5]] == [88, 32, 16, 48, 24]
    assert rows[5] == [C.sizeof(_lib.PlacesConfigC), C.sizeof(_lib.PlaceCandidateC), C.sizeof(_lib.OdometryConfigC)]  # no existing struct moved


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.posegraph import PoseGraphConfig
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    out = C.c_void_p()
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    nan, inf = float("nan"), float("inf")
    assert L.elm_posegraph_create(None, 4, 4, C.byref(out)) == INVALID and L.elm_posegraph_create(one, 4, 4, None) == INVALID
    for nc, ec in ((0, 4), (-1, 4), ((1 << 20) + 1, 4), (4, 0), (4, -1), (4, (1 << 22) + 1)):
        assert L.elm_posegraph_create(one, nc, ec, C.byref(out)) == INVALID, (nc, ec)
    L.elm_posegraph_destroy(None)
    assert L.elm_posegraph_reset(None, one) == INVALID and L.elm_posegraph_reset(one, None) == INVALID
    n, e = C.c_size_t(0), C.c_size_t(0)
    assert L.elm_posegraph_size(one, one, None, C.byref(e)) == INVALID and L.elm_posegraph_size(one, one, C.byref(n), None) == INVALID
    assert L.elm_posegraph_size(None, one, C.byref(n), C.byref(e)) == INVALID and L.elm_posegraph_size(one, None, C.byref(n), C.byref(e)) == INVALID
    # nodes and poses
    eye = np.tile(np.eye(4).ravel(), 2)
    fx = np.zeros(2, np.uint8)
    ep, fp = eye.ctypes.data_as(dp), fx.ctypes.data_as(u8p)
    assert L.elm_posegraph_add_nodes(None, one, ep, fp, 2) == INVALID and L.elm_posegraph_add_nodes(one, None, ep, fp, 2) == INVALID
    assert L.elm_posegraph_add_nodes(one, one, None, fp, 2) == INVALID
    assert L.elm_posegraph_set_poses(None, one, 0, 2, ep) == INVALID and L.elm_posegraph_set_poses(one, one, 0, 2, None) == INVALID
    assert L.elm_posegraph_get_poses(one, None, 0, 2, ep) == INVALID and L.elm_posegraph_get_poses(one, one, 0, 2, None) == INVALID
    assert L.elm_posegraph_set_fixed(one, None, 0, 2, fp) == INVALID and L.elm_posegraph_set_fixed(one, one, 0, 2, None) == INVALID
    for v in (nan, inf, -inf):
        bad = eye.copy()
        bad[16 + 13] = v
        assert L.elm_posegraph_add_nodes(one, one, bad.ctypes.data_as(dp), fp, 2) == INVALID
        assert L.elm_posegraph_set_poses(one, one, 0, 2, bad.ctypes.data_as(dp)) == INVALID
    # edges: i == j, a negative index, a non-finite entry, an information that is not exactly symmetric -- all before the object is read
    ii, jj = np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    info = np.tile(np.eye(6).ravel(), 2)
    ip, jp, op = ii.ctypes.data_as(i32p), jj.ctypes.data_as(i32p), info.ctypes.data_as(dp)
    assert L.elm_posegraph_add_edges(None, one, ip, jp, ep, op, 2) == INVALID and L.elm_posegraph_add_edges(one, None, ip, jp, ep, op, 2) == INVALID
    for args in ((None, jp, ep, op), (ip, None, ep, op), (ip, jp, None, op), (ip, jp, ep, None)):
        assert L.elm_posegraph_add_edges(one, one, *args, 2) == INVALID
    same = np.array([1, 1], np.int32)
    assert L.elm_posegraph_add_edges(one, one, ip, same.ctypes.data_as(i32p), ep, op, 2) == INVALID
    neg = np.array([0, -1], np.int32)
    assert L.elm_posegraph_add_edges(one, one, neg.ctypes.data_as(i32p), jp, ep, op, 2) == INVALID
    for v in (nan, inf):
        bad = eye.copy()
        bad[16 + 2] = v
        assert L.elm_posegraph_add_edges(one, one, ip, jp, bad.ctypes.data_as(dp), op, 2) == INVALID
        bad = info.copy()
        bad[36 + 7] = v
        assert L.elm_posegraph_add_edges(one, one, ip, jp, ep, bad.ctypes.data_as(dp), 2) == INVALID
    bad = info.copy()
    bad[36 + 1 * 6 + 2] = 0.5
    bad[36 + 2 * 6 + 1] = float(np.nextafter(0.5, 1.0))  # symmetric to the last bit but one
    assert L.elm_posegraph_add_edges(one, one, ip, jp, ep, bad.ctypes.data_as(dp), 2) == INVALID
    # linearize, download, solve, optimize
    assert L.elm_posegraph_linearize(None, one, 0.0, None) == INVALID and L.elm_posegraph_linearize(one, None, 0.0, None) == INVALID
    for k in (-1.0, nan, inf):
        assert L.elm_posegraph_linearize(one, one, k, None) == INVALID
    assert L.elm_posegraph_download_linearization(None, one, *([None] * 7)) == INVALID
    assert L.elm_posegraph_download_linearization(one, None, *([None] * 7)) == INVALID
    assert L.elm_posegraph_solve(None, one, 0.0, 0.0, 5, None, None) == INVALID and L.elm_posegraph_solve(one, None, 0.0, 0.0, 5, None, None) == INVALID
    for lam, tol, it in ((-1.0, 0.0, 5), (nan, 0.0, 5), (0.0, -1e-3, 5), (0.0, nan, 5), (0.0, 0.0, 0), (0.0, 0.0, -3), (inf, 0.0, 5)):
        assert L.elm_posegraph_solve(one, one, lam, tol, it, None, None) == INVALID, (lam, tol, it)
    cfg = PoseGraphConfig()
    res = _lib.PoseGraphResultC()
    tr = (_lib.PoseGraphTraceC * 4)()
    assert L.elm_posegraph_optimize(None, one, C.byref(cfg), C.byref(res), tr, 4) == INVALID
    assert L.elm_posegraph_optimize(one, None, C.byref(cfg), C.byref(res), tr, 4) == INVALID
    assert L.elm_posegraph_optimize(one, one, None, C.byref(res), tr, 4) == INVALID
    assert L.elm_posegraph_optimize(one, one, C.byref(cfg), C.byref(res), None, 4) == INVALID
    assert L.elm_posegraph_optimize(one, one, C.byref(cfg), C.byref(res), tr, -1) == INVALID
    for kw in (dict(max_iterations=0), dict(pcg_max_iterations=0), dict(pcg_check_every=0), dict(lambda_init=-1.0), dict(lambda_init=nan),
               dict(lambda_up=0.5), dict(lambda_up=inf), dict(lambda_down=0.0), dict(lambda_down=2.0), dict(lambda_min=1.0, lambda_max=0.5),
               dict(lambda_max=inf), dict(cost_rel_tol=-1.0), dict(step_tol=nan), dict(pcg_rel_tol=-1.0), dict(huber_k=-0.1), dict(huber_k=nan)):
        assert L.elm_posegraph_optimize(one, one, C.byref(PoseGraphConfig(**kw)), C.byref(res), tr, 4) == INVALID, kw
    # edge terms: host only
    r = np.zeros(6)
    I4 = np.eye(4).ravel()
    ok = I4.ctypes.data_as(dp)
    assert L.elm_posegraph_edge_terms(None, ok, ok, r.ctypes.data_as(dp), None, None) == INVALID
    assert L.elm_posegraph_edge_terms(ok, None, ok, None, None, None) == INVALID and L.elm_posegraph_edge_terms(ok, ok, None, None, None, None) == INVALID
    bad = I4.copy()
    bad[12] = nan
    assert L.elm_posegraph_edge_terms(ok, bad.ctypes.data_as(dp), ok, None, None, None) == INVALID
    assert L.elm_posegraph_edge_terms(ok, ok, ok, None, None, None) == 0


def test_shim_posegraph_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/posegraph_calls.cpp, built as tests/test_places_abi.py builds places_calls.cpp"""
    exe = tmp_path / "posegraph_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "posegraph_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
