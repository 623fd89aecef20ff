"""The pose graph's linear initialization with priors (include/elimaloc_hip_posegraph_init_prior.h) on the CPU:
the two calls' symbols, struct layouts and argument errors without a device, the C++ shim's call lines, the host's plan as a program of
its own (tests/pginit_classes_check.cpp), and the algebra of the mirror (tests/posegraph_init_prior_ref.py): the priors' terms against
posegraph_prior_ref.prior_terms in the isotropic form, every stage's H symmetric positive definite, the padding solution, the Kabsch
alignment, the three prototype results, the noisy chain that only priors correct, the independence of the start, and the fitness of
every GPU shape to judge five iterations."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_ref as cref
import posegraph_init_prior_cases as ipcases
import posegraph_init_prior_ref as ipref
import posegraph_init_ref as iref
import posegraph_prior_cases as pcases
import posegraph_prior_ref as pref
import posegraph_ref as ref
import test_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_posegraph_init_prior.h"
NAMES = {"elm_posegraph_init_prior_config_default", "elm_posegraph_initialize_priors"}

# The mirror's direct solve against the truth, measured here ("Measured accuracy"); the bounds are 10 x these.
MEASURED_RING8_M, MEASURED_RING8_RAD, MEASURED_RING8_COST = 3.8e-14, 4.5e-15, 1.6e-27
MEASURED_RING16_M = 1.0e-13
MEASURED_GNSS_M, MEASURED_GNSS_RAD = 0.59, 0.089
MEASURED_PRIORS_ONLY_COST = 1.2345


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
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_PGINITP
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_PGINITP == list(table)
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params and (restype is None) == (ret == "void") and (ret == "void" or (restype is C.c_int and ret == "int")), name
        fn = getattr(L, name)  # exported, and carrying what the table says
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    top = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    assert '#include "elimaloc_hip_posegraph_prior.h"\n#include "elimaloc_hip_posegraph_init_prior.h"\n' in top
    # elm_posegraph_initialize's own header is as it was: its two calls and nothing of this one
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    assert set(re.findall(r"\b(elm_[a-z0-9_]+)\s*\(", strip("elimaloc_hip_posegraph_init.h"))) == set(_lib.EXPORTS_INIT)
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT) | set(_lib.EXPORTS_LOOPS) | set(_lib.EXPORTS_LOOPCOV)
              | set(_lib.EXPORTS_PGCOV) | set(_lib.EXPORTS_PGPRIOR))
    assert not NAMES & others
    import __graft_entry__ as g
    assert "EXPORTS_PGINITP" in open(g.__file__).read()  # build()'s missing-symbol check reads the new table
    assert re.search(r"#define ELM_PG_INIT_ALIGN_ROW %d\b" % _lib.PG_INIT_ALIGN_ROW, strip(HEADER)) and _lib.PG_INIT_ALIGN_ROW == ipref.ALIGN_ROW == 28


def test_the_header_compiles_as_c():
    probe = ('#include "elimaloc_hip.h"\nint main(void) { elm_posegraph_init_prior_config c; elm_posegraph_init_prior_result r; double a[ELM_PG_INIT_ALIGN_ROW];\n'
             '  elm_posegraph_init_prior_config_default(&c); r.base.applied = 0; r.aligned_components = 0;\n'
             '  return elm_posegraph_initialize_priors(0, 0, &c, &r, 0, 0, 0, a, 1) == ELM_ERR_INVALID && c.base.stages == (ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS)\n'
             '         ? r.base.applied + r.aligned_components : 1; }\n')
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=probe.encode(), check=True)


def test_struct_layouts_and_defaults(L, tmp_path):
    from elimaloc_amd import _lib
    from elimaloc_amd.posegraph import PoseGraphInitConfig, PoseGraphInitPriorConfig
    structs = {"elm_posegraph_init_prior_config": _lib.PoseGraphInitPriorConfigC, "elm_posegraph_init_prior_result": _lib.PoseGraphInitPriorResultC}
    lines = []
    for name, cls in structs.items():
        offs = ", ".join("offsetof(%s, %s)" % (name, f) for f, _ in cls._fields_)
        lines.append('  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs))
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for row, (name, cls) in zip(rows, structs.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name
    assert [r[0] for r in rows] == [32, 88]
    c = PoseGraphInitPriorConfig()
    assert bytes(c.base) == bytes(PoseGraphInitConfig()) and c.align_min_ratio == ipref.ALIGN_MIN_RATIO == 1e-4
    c = PoseGraphInitPriorConfig(stages=iref.ROT, pcg_rel_tol=1e-3, align_min_ratio=0.5)
    assert (c.base.stages, c.base.pcg_rel_tol, c.align_min_ratio) == (1, 1e-3, 0.5)
    with pytest.raises(AttributeError, match="PoseGraphInitPriorConfig has no field lambda_init"):
        PoseGraphInitPriorConfig(lambda_init=1.0)
    L.elm_posegraph_init_prior_config_default(None)


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.posegraph import PoseGraphInitPriorConfig
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    res = _lib.PoseGraphInitPriorResultC()
    res.base.applied, res.aligned_components = 7, 9
    good = PoseGraphInitPriorConfig()
    call = lambda ctx, pg, cfg, r, cap=0: L.elm_posegraph_initialize_priors(ctx, pg, C.byref(cfg) if cfg is not None else None,
                                                                            C.byref(r) if r is not None else None, None, None, None, None, cap)
    assert call(None, one, good, res) == INVALID and call(one, None, good, res) == INVALID
    assert call(one, one, None, res) == INVALID and call(one, one, good, None) == INVALID
    for bad in (dict(stages=0), dict(stages=4), dict(stages=-1), dict(pcg_rel_tol=0.0), dict(pcg_rel_tol=-1e-8), dict(pcg_rel_tol=float("nan")),
                dict(pcg_rel_tol=float("inf")), dict(pcg_max_iterations=0), dict(pcg_max_iterations=-3), dict(pcg_check_every=0),
                dict(align_min_ratio=0.0), dict(align_min_ratio=-1e-4), dict(align_min_ratio=float("nan")), dict(align_min_ratio=float("inf"))):
        assert call(one, one, PoseGraphInitPriorConfig(**bad), res) == INVALID, bad
    assert call(one, one, good, res, -1) == INVALID
    assert res.base.applied == 7 and res.aligned_components == 9


def test_shim_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/posegraph_init_prior_calls.cpp, built as tests/test_posegraph_prior_abi.py builds posegraph_prior_calls.cpp"""
    exe = tmp_path / "posegraph_init_prior_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "posegraph_init_prior_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


def test_the_classes_program(tmp_path):
    """tests/pginit_classes_check.cpp against csrc/elm_pginit_classes.hpp alone, under the address and undefined-behaviour sanitizers, run
    as a program of its own (nothing is loaded into this process)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/pginit_classes_check.cpp")
    exe = str(tmp_path / "pginit_classes_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-static-libubsan", "-I", os.path.join(ROOT, "elimaloc_amd", "csrc"), os.path.join(ROOT, "tests", "pginit_classes_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases passed" in run.stdout


def test_the_mirrors_plan_is_the_programs():
    """the graph of tests/pginit_classes_check.cpp, through the mirror's classes"""
    fixed = np.zeros(14, bool)
    fixed[1] = True
    T = np.tile(np.eye(4), (14, 1, 1))
    g = ref.Graph(T, fixed, [2, 0, 4, 5, 7, 8, 11, 9], [1, 1, 3, 4, 6, 7, 10, 10], np.tile(np.eye(4), (8, 1, 1)))
    wr = [0.0, 2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    wt = [1.0, 0.0, 3.0, 1.0, 0.5, 4.0, 0.0, 2.0, 5.0, 1.5]
    info = np.zeros((10, 6, 6))
    for q in range(10):
        info[q, :3, :3], info[q, 3:, 3:] = wt[q] * np.eye(3), wr[q] * np.eye(3)
    P = pref.Priors([7, 3, 11, 1, 8, 12, 6, 9, 5, 7], None, None, info)
    plan = ipref.classes(g, P)
    assert plan["refusal"] is None and plan["cls"] == {0: "fixed", 3: "prior-anchored", 6: "aligned", 9: "aligned"} and plan["gauge"] == [6, 9]
    assert plan["node_comp"].tolist() == [-1] * 6 + [0] * 3 + [1] * 3 + [-1, -1]
    assert [l.tolist() for l in plan["lists"]] == [[0, 4, 9], [2, 7]]
    assert plan["w_rot"].tolist() == wr and plan["w_last"].tolist() == wt and plan["w_pre"].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 4.0, 0.0, 0.0, 5.0, 0.0]
    assert ipref.classes(g, P, ipref.TRANS)["gauge"] == [] and ipref.classes(g, P, ipref.ROT)["refusal"] is not None
    assert ipref.classes(g, pref.Priors())["refusal"] is not None


# ---------------------------------------------------------------- the terms and the systems
def test_prior_terms_against_the_full_prior_in_the_isotropic_form():
    """With Omega = diag(w_t I, w_r I) and l = 0 the translation block of prior_terms' g and H is this stage's (J_tt = R_E, and R_E^T
    R_Z^T u = R_v^T u); with a lever arm the translation columns still are.  The rotation stage's residual is zero exactly where
    prior_terms' rotation residual is."""
    rng = np.random.default_rng(11)
    for _ in range(50):
        T, Z = cases.rand_pose(rng, 3.0, 10.0), cases.rand_pose(rng, 3.0, 10.0)
        lever = rng.uniform(-2.0, 2.0, 3)
        wt, wr = rng.uniform(0.5, 4.0, 2)
        P = pref.Priors([0], Z[None], lever, np.diag([wt] * 3 + [wr] * 3))
        assert np.allclose(ipref.prior_weights(P), ([wr], [wt]), rtol=1e-15)
        r, J = pref.prior_terms(T, Z, lever)
        g_t, H_t = ipref.trans_terms(P, np.array([wt]), T[None])
        full_g, full_H = J.T @ P.info[0] @ r, J.T @ P.info[0] @ J
        assert np.abs(H_t[0][:3, :3] - full_H[:3, :3]).max() <= 1e-13 * wt and np.abs(g_t[0][:3] - (J[:3, :3].T * wt) @ r[:3]).max() <= 1e-12 * wt * 30.0
        assert not g_t[0][3:].any() and np.array_equal(H_t[0], wt * np.eye(6))
        P0 = pref.Priors([0], Z[None], None, P.info)
        r0, J0 = pref.prior_terms(T, Z)
        g0, _ = ipref.trans_terms(P0, np.array([wt]), T[None])
        assert np.abs(g0[0][:3] - (J0.T @ P.info[0] @ r0)[:3]).max() <= 1e-12 * wt * 30.0  # l = 0: the whole upper gradient of the full prior
        g_r, H_r = ipref.rot_terms(P, np.array([wr]), T[None])
        assert np.array_equal(H_r[0], wr * np.eye(6)) and np.abs(g_r[0] - wr * (iref.rows_of(T[None]) - iref.rows_of(Z[None]))[0]).max() <= 1e-15 * wr
        same = T.copy()
        same[:3, :3] = Z[:3, :3]
        assert not ipref.rot_terms(P, np.array([wr]), same[None])[0].any() and not pref.prior_terms(same, Z, lever)[0][3:].any()


SMALL = ("aligned3", "aligned4_lever0", "node_counts", "far_1e5", "every_class", "anchored_ring", "gnss_chain")


@pytest.mark.parametrize("name", SMALL + ("N257_P257_aligned", "N255_P255_anchored"))
def test_every_stage_is_symmetric_positive_definite_and_the_padding_is_zero(name):
    g, P = ipcases.SHAPES[name]()
    out = ipref.initialize(g, P)
    for stage in ("rot_lin", "pre_lin", "trans_lin"):
        lin = out[stage]
        if lin is None:
            assert stage == "pre_lin" and out["aligned_components"] == 0
            continue
        H, b = pref.dense_system(g, lin, 0.0)
        assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
        low = float(np.linalg.eigvalsh((H + H.T) / 2.0).min())
        print(f"{name} {stage}: smallest eigenvalue of H {low:.3e}, {int(lin['active'].sum())} active nodes of {g.N}")
        assert low > 0.0
    assert out["padding"] == 0.0  # the lower three unknowns of every translation solve, exactly
    if out["aligned_components"]:  # the gauge nodes are held in S1 and S2 and free in S3
        gauge = ipref.classes(g, P)["gauge"]
        assert not out["rot_lin"]["active"][gauge].any() and not out["pre_lin"]["active"][gauge].any() and out["trans_lin"]["active"][gauge].all()
        assert not out["v_pre"][gauge].any()


# ---------------------------------------------------------------- the alignment
def _cloud(rng, n, flat=False):
    a = rng.uniform(-5.0, 5.0, (n, 3))
    if flat:
        a[:, 2] = 0.0
    return a


def test_kabsch_finds_a_planted_motion():
    rng = np.random.default_rng(21)
    for n, flat in ((3, False), (4, False), (40, False), (40, True), (3, True)):
        a, w = _cloud(rng, n, flat), rng.uniform(0.5, 2.0, n)
        G, s = ref.exp_so3(rng.uniform(-1.5, 1.5, 3)), rng.uniform(-20.0, 20.0, 3)
        b = a @ G.T + s
        K = ipref.kabsch(a, b, w)
        assert not K["deficient"] and np.abs(K["G"] - G).max() <= 1e-12 and np.abs(K["cb"] - (G @ K["ca"] + s)).max() <= 1e-12
        assert abs(np.linalg.det(K["G"]) - 1.0) <= 1e-12 and np.abs((K["cb"] + (a - K["ca"]) @ K["G"].T) - b).max() <= 1e-11
        assert K["row"].shape == (28,) and K["row"][15] == K["W"] == float(w.sum())
        if flat:  # coplanar points: sigma_3 = 0 and the rotation is still determined
            assert K["sigma"][2] <= 1e-12 * K["sigma"][0] and K["sigma"][1] > ipref.ALIGN_MIN_RATIO * K["sigma"][0]


def test_kabsch_takes_the_rotation_when_u_vt_is_a_reflection():
    """coplanar points mirrored in their plane's normal: U V^T of S has determinant -1, and diag(1, 1, -1) turns it into the rotation"""
    rng = np.random.default_rng(22)
    a = _cloud(rng, 12, flat=True)
    G = ref.exp_so3(np.array([0.3, -0.2, 0.9]))
    b = a @ G.T
    # coplanar points: the SVD's sign of the null vector decides whether U V^T is a reflection; G is the planted rotation either way
    K = ipref.kabsch(a, b, np.ones(12))
    assert abs(abs(K["det_uvt"]) - 1.0) <= 1e-12 and abs(np.linalg.det(K["G"]) - 1.0) <= 1e-12 and np.abs(K["G"] - G).max() <= 1e-12
    S = np.diag([3.0, 2.0, 1.0]) @ np.diag([1.0, 1.0, -1.0])  # S itself a reflection: sigma = (3, 2, 1), U V^T = diag(1, 1, -1)
    U, sg, Vt = np.linalg.svd(S)
    assert np.linalg.det(U @ Vt) < 0.0
    # a constructed point set with that S: a = e_k, b = S e_k about zero centroids (the points and their negatives)
    a = np.concatenate([np.eye(3), -np.eye(3)])
    K = ipref.kabsch(a, a @ S.T, np.full(6, 0.5))
    assert K["det_uvt"] < 0.0 and np.allclose(K["S"], S, atol=1e-15) and abs(np.linalg.det(K["G"]) - 1.0) <= 1e-12
    assert np.allclose(K["G"], np.eye(3), atol=1e-12)  # the nearest rotation to diag(3, 2, -1) flips the smallest axis back


def test_kabsch_rank_deficiency_on_either_side_of_the_ratio():
    rng = np.random.default_rng(23)
    line = np.outer(np.linspace(-3.0, 3.0, 9), [1.0, 2.0, -0.5])
    for pts in (line[:1], line[:2], line):  # one point, two points, collinear points
        K = ipref.kabsch(pts, pts + 1.0, np.ones(len(pts)))
        assert K["deficient"] and K["ratio"] <= 1e-12
    # a lateral spread e of a line of length 1: sigma_2 / sigma_1 ~ e^2, so 1e-4 is a spread of 1 %
    for e, deficient in ((0.003, True), (0.03, False)):
        pts = np.stack([np.linspace(-0.5, 0.5, 21), e * np.cos(np.arange(21.0)), e * 0.1 * np.sin(np.arange(21.0))], 1)
        K = ipref.kabsch(pts, pts @ ref.exp_so3(rng.uniform(-1.0, 1.0, 3)).T, np.ones(21))
        print(f"spread {e}: sigma_2 / sigma_1 = {K['ratio']:.3e}")
        assert K["deficient"] == deficient
    K = ipref.kabsch(pts, pts, np.ones(21))
    assert ipref.kabsch(pts, pts, np.ones(21), min_ratio=K["ratio"])["deficient"]  # sigma_2 == ratio sigma_1 is deficient
    assert not ipref.kabsch(pts, pts, np.ones(21), min_ratio=K["ratio"] * (1.0 - 1e-9))["deficient"]


# ---------------------------------------------------------------- the prototype's results
def test_the_anchored_ring_is_reproduced_from_its_moved_start():
    g, P, truth = pcases.anchored_ring()
    out = ipref.initialize(g, P)
    dt0, dr0 = ref.pose_error(g.poses, truth)
    dt, dr = ref.pose_error(out["poses"], truth)
    print(f"every 8: start {dt0:.3e} m {dr0:.3e} rad off, after the call {dt:.3e} m {dr:.3e} rad, cost {out['cost_before']:.4e} -> {out['cost_after']:.3e}")
    assert dt0 > 5.9 and abs(dr0 - 0.2) < 1e-12 and abs(out["cost_before"] - 599.09) < 0.01
    assert out["applied"] and out["aligned_components"] == 1 and out["rank_deficient_components"] == 0
    assert dt <= 10.0 * MEASURED_RING8_M and dr <= 10.0 * MEASURED_RING8_RAD and out["cost_after"] <= 10.0 * MEASURED_RING8_COST
    g, P, truth = pcases.anchored_ring(every=16)
    out = ipref.initialize(g, P)
    dt, _ = ref.pose_error(out["poses"], truth)
    print(f"every 16: {dt:.3e} m, sigma {out['align'][0, 25:]}")
    assert out["applied"] and P.P == 4 and dt <= 10.0 * MEASURED_RING16_M
    g, P, truth = pcases.anchored_ring(every=32)  # two priors: collinear
    out = ipref.initialize(g, P)
    sigma = out["align"][0, 25:]
    print(f"every 32: sigma {sigma}, {ref.pose_error(out['poses'], truth)[0]:.3f} m off")
    assert P.P == 2 and not out["applied"] and out["rank_deficient_components"] == 1 and all(out[k][2] for k in ("rot", "pre", "trans"))
    assert sigma[0] > 2e3 and sigma[1] <= 1e-12 * sigma[0] and ref.pose_error(out["poses"], truth)[0] > 1e-3


def test_priors_only_costs():
    g, P = pcases.priors_only()
    out = ipref.initialize(g, P)
    print(f"priors_only: cost {out['cost_before']:.5f} -> {out['cost_after']:.5f}, classes {ipref.classes(g, P)['cls']}")
    assert out["applied"] and out["aligned_components"] == 0 and abs(out["cost_before"] - 9.348) < 1e-3
    assert abs(out["cost_after"] - MEASURED_PRIORS_ONLY_COST) <= 1e-3
    start = ref.Graph(out["poses"], g.fixed, g.i, g.j, g.Z, g.info)
    _, alone = pref.optimize(g, P)
    _, then = pref.optimize(start, P)
    assert (alone["solves"], then["solves"]) == (7, 6) and abs(then["cost_final"] - 0.46653) < 1e-5 and abs(alone["cost_final"] - then["cost_final"]) < 1e-9


def test_gnss_chain_needs_the_initialization():
    g, P, truth = ipcases.gnss_chain()
    dt0, dr0 = ref.pose_error(g.poses, truth)
    assert g.N == 200 and g.E == 199 and not g.fixed.any() and P.P == 20 and abs(dt0 - 73.9) < 0.05 and abs(dr0 - 1.09) < 0.005
    poses_alone, alone = pref.optimize(g, P, **cases.RING_CFG)
    out = ipref.initialize(g, P)
    dt, dr = ref.pose_error(out["poses"], truth)
    poses_then, then = pref.optimize(ref.Graph(out["poses"], g.fixed, g.i, g.j, g.Z, g.info), P, **cases.RING_CFG)
    far, near = ref.pose_error(poses_alone, truth), ref.pose_error(poses_then, truth)
    print(f"Optimize alone: {alone['solves']} solves, {alone['accepted']} accepted, {alone['stop_reason']}, {far[0]:.2f} m {far[1]:.2f} rad off; "
          f"after the initialization alone {dt:.3f} m {dr:.4f} rad; then Optimize: {then['solves']} solves, {then['accepted']} accepted, "
          f"{then['stop_reason']}, {near[0]:.3f} m {near[1]:.4f} rad, cost {then['cost_final']:.5f}; last translation solve moves by {np.abs(out['v']).max():.2f} m")
    assert out["applied"] and dt <= 10.0 * MEASURED_GNSS_M and dr <= 10.0 * MEASURED_GNSS_RAD and dt < 1.0
    assert alone["stop_reason"] == "max_iterations" and alone["solves"] == 20
    assert then["stop_reason"] == "cost_tol" and then["rejected"] == 0 and then["accepted"] == then["solves"]
    assert far[0] >= 10.0 * near[0] and far[1] >= 10.0 * near[1]
    assert np.abs(out["v"]).max() > 1.0  # the priors bend the trajectory, they do not just place it


@pytest.mark.parametrize("name", ["anchored_ring", "every_class", "aligned3"])
def test_the_result_does_not_depend_on_the_start_of_the_free_nodes(name):
    """Every solve is the minimum of a quadratic, so the start of a free node does not enter -- but for the gauge nodes, which S1 and S2
    hold where they start.  The two-row rotation problem is not invariant under a rotation of the world when the edges carry noise (the
    third row is not in it), so on a noisy graph the gauge node's start rotation reaches the result at the level of that noise; on the
    noise-free ring it does not.  Hence: the noise-free ring from a start that moves every node, the noisy graphs from a start that moves
    every free node but the gauge nodes.  With the gauge nodes moved too the two results stay within the noise of ONE edge of the graph
    (posegraph_cases' 0.05 rad, and that angle times the graph's extent in metres: the error of the two-row problem is that of its
    data), and Optimize brings both to the same minimum: the same cost to 1e-9, the poses as close as its cost_rel_tol of 1e-12 leaves
    them (1e-6).  A node without edges keeps its rotation in every case: no stage solves it."""
    g, P = ipcases.SHAPES[name]()
    lone = sorted(set(range(g.N)) - set(g.i.tolist()) - set(g.j.tolist()))
    gauge = ipref.classes(g, P)["gauge"]
    a = ipref.initialize(g, P)
    b = ipref.initialize(ipcases.scramble(g, 31, hold=lone if name == "anchored_ring" else gauge + lone), P)
    dt, dr = ref.pose_error(a["poses"], b["poses"])
    print(f"{name}: two starts end {dt:.3e} m {dr:.3e} rad apart")
    assert a["applied"] and b["applied"] and dt <= 1e-8 and dr <= 1e-9
    edge_noise_rad = 0.0 if name == "anchored_ring" else 0.05  # posegraph_cases._measure's rot_noise; the ring's edges are the truth's own
    extent = float(np.linalg.norm(g.poses[:, None, :3, 3] - g.poses[None, :, :3, 3], axis=-1).max())
    graph_at = lambda poses: ref.Graph(poses, g.fixed, g.i, g.j, g.Z, g.info)
    pa, ra = pref.optimize(graph_at(a["poses"]), P, **cases.RING_CFG)
    for seed in (31, 32, 33):
        c = ipref.initialize(ipcases.scramble(g, seed, hold=lone), P)
        dt, dr = ref.pose_error(a["poses"], c["poses"])
        pc, rc = pref.optimize(graph_at(c["poses"]), P, **cases.RING_CFG)
        ot, orr = ref.pose_error(pa, pc)
        print(f"{name} seed {seed}: with the gauge nodes moved too {dt:.3e} m {dr:.3e} rad apart (bounds {max(edge_noise_rad * extent, 1e-8):.2e}, "
              f"{max(edge_noise_rad, 1e-9):.2e}); after Optimize {ot:.3e} m {orr:.3e} rad, cost {ra['cost_final']:.12e} / {rc['cost_final']:.12e}")
        assert c["applied"] and dr <= max(edge_noise_rad, 1e-9) and dt <= max(edge_noise_rad * extent, 1e-8)
        assert ra["stop_reason"] == rc["stop_reason"] and ot <= 1e-6 and orr <= 1e-6
        assert abs(ra["cost_final"] - rc["cost_final"]) <= 1e-9 * max(ra["cost_final"], 1e-18)


@pytest.mark.parametrize("name", ["anchored_ring", "every_class"])
def test_mirror_pcg_reaches_the_direct_solve(name):
    g, P = ipcases.SHAPES[name]()
    want = ipref.initialize(g, P)
    for kind, pcg in (("block_jacobi", lambda g, lin: ref.pcg(g, lin, 0.0, 1e-12, 2000)), ("chain", lambda g, lin: cref.pcg_chain(g, lin, 0.0, 1e-12, 2000))):
        got = ipref.initialize(g, P, solver=pcg)
        dt, dr = ref.pose_error(got["poses"], want["poses"])
        print(f"{name} {kind}: iterations {got['rot'][0]} + {got['pre'][0]} + {got['trans'][0]}, against the direct solve {dt:.3e} m {dr:.3e} rad")
        assert got["applied"] and dt <= 1e-8 and dr <= 1e-9


def test_without_priors_the_mirror_is_the_initialization_mirror():
    for make in (lambda: cases.ring()[0], lambda: cases.chain(12, 2)):
        g = make()
        a, b = iref.initialize(g), ipref.initialize(g, pref.Priors())
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("poses", "rows", "v", "cost_before", "cost_after"))
        assert b["aligned_components"] == 0 and not b["v_pre"].any()


def test_the_recording_is_the_mirrors():
    gold, run = np.load(ipcases.GOLDEN), ipcases.mirror_recording()
    assert set(gold.files) == set(run)
    for k in run:  # (libm may differ between hosts by an ulp: the recording is compared as numbers)
        assert np.allclose(run[k], gold[k], rtol=1e-6, atol=1e-9), k


# ---------------------------------------------------------------- the GPU test's shapes
@pytest.mark.parametrize("name", list(ipcases.SHAPES))
def test_every_gpu_shape_is_fit_to_judge_five_iterations(name):
    """tests/test_posegraph_init_abi.py's check of the same name, for every stage of this call: the mirror's five iterations with the
    chain preconditioner on two equally valid direct solves of the same M (LU, banded Cholesky) agree within 1e-3 of the contract
    1e-9 max(1, max |ref|) in rows, v_pre, v and the alignment rows."""
    g, P = ipcases.SHAPES[name]()
    lu = ipref.initialize(g, P, solver=lambda g, lin: cref.pcg_chain(g, lin, 0.0, 1e-300, 5))
    ch = ipref.initialize(g, P, solver=lambda g, lin: cref.pcg_chain(g, lin, 0.0, 1e-300, 5, solve=cref.chain_solver_cholesky(g, lin, 0.0)))
    for key in ("rows", "v_pre", "v", "align"):
        own = float(np.abs(lu[key] - ch[key]).max()) if lu[key].size else 0.0
        contract = 1e-9 * max(1.0, float(np.abs(lu[key]).max()) if lu[key].size else 0.0)
        print(f"{name} {key}: the mirror's two direct solves after 5 iterations differ by {own:.3e} (contract {contract:.1e})")
        assert own <= 1e-3 * contract
