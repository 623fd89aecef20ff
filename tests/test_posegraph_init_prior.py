"""The pose graph's linear initialization with priors on the GPU (include/elimaloc_hip_posegraph_init_prior.h)
against its mirror (tests/posegraph_init_prior_ref.py), with both preconditioners, on the shapes of posegraph_init_prior_cases.SHAPES:
five conjugate-gradient iterations of every stage under the project's 1e-9 contract, the iteration counts and final poses at 1e-10, the
call without priors against Initialize in bytes, the rank-deficient alignment, non-convergence, single stages, the refusals on a live
object, the run-to-run bytes, the recording, and LoopCloser.Close(initialize="priors")."""
import ctypes as C
import functools

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_ref as cref
import posegraph_init_cases as icases
import posegraph_init_prior_cases as ipcases
import posegraph_init_prior_ref as ipref
import posegraph_prior_cases as pcases
import posegraph_prior_ref as pref
import posegraph_ref as ref
from elimaloc_amd import _lib
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig, PoseGraphInitConfig, PoseGraphInitPriorConfig

pytestmark = pytest.mark.gpu

KINDS = ("block_jacobi", "chain")
TOL = 1e-10
NEVER = 1e-300  # a tolerance no solve meets: the iteration count is then pcg_max_iterations
STAGE_KEYS = ("rows", "v_pre", "v", "align")


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


def _mirror_pcg(kind, tol, max_it):
    if kind == "chain":
        return lambda g, lin: cref.pcg_chain(g, lin, 0.0, tol, max_it)
    return lambda g, lin: ref.pcg(g, lin, 0.0, tol, max_it)


@functools.lru_cache(maxsize=None)
def _case(name):
    return ipcases.SHAPES[name]()


@functools.lru_cache(maxsize=None)
def _direct(name):
    """the mirror's whole call with direct solves, computed once per shape and left unchanged"""
    return ipref.initialize(*_case(name))


@functools.lru_cache(maxsize=None)
def _mirror(name, kind, tol, max_it):
    return ipref.initialize(*_case(name), solver=_mirror_pcg(kind, tol, max_it))


def _upload(ctx, g, P, kind="block_jacobi", room=0):
    pg = PoseGraph(max(g.N, 1), g.E + 1, ctx, prior_capacity=P.P + room)
    pg.SetPreconditioner(kind)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    if P.P:
        pg.AddPriors(P.node, P.Z, P.info, P.lever)
    return pg


def _close(got, want, what, own=0.0):
    """The sums contract of DESIGN.md section 22, 1e-9 max(1, max |ref|); where the reference itself lacks those digits (`own`: the
    mirror's conjugate gradients against its direct solve on that shape) the bound is 10 x that difference."""
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(np.asarray(got) - want).max()) if want.size else 0.0
    contract = 1e-9 * max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    bound = max(contract, 10.0 * own)
    print(f"  {what}: |gpu - ref| {err:.3e} (bound {bound:.1e}: contract {contract:.1e}, the mirror against itself {own:.1e})")
    assert np.asarray(got).shape == want.shape and err <= bound, what


def _state(pg):
    """what a call that is not applied must leave: the poses, the priors, their threshold, and how the graph behaves under its flags"""
    pri = pg.Priors()
    return pg.Poses().tobytes() + b"".join(pri[k].tobytes() for k in ("node", "Z", "lever", "information")) + np.float64(pg.PriorHuber()).tobytes()


# ---------------------------------------------------------------- five iterations of every stage
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ipcases.SHAPES))
def test_five_iterations_against_the_mirror(ctx, name, kind):
    g, P = _case(name)
    want = _mirror(name, kind, NEVER, 5)
    pg = _upload(ctx, g, P, kind)
    try:
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(pcg_rel_tol=NEVER, pcg_max_iterations=5), return_stages=True)
        print(f"  {name} {kind}: iterations {res['rot_iterations']} + {res['pre_iterations']} + {res['trans_iterations']} "
              f"(mirror {want['rot'][0]} + {want['pre'][0]} + {want['trans'][0]}), aligned {res['aligned_components']}")
        assert res["aligned_components"] == want["aligned_components"] and res["align"].shape == want["align"].shape
        for stage in ("rot", "pre", "trans"):
            got, ref_its = res[f"{stage}_iterations"], want[stage][0]
            ended_exactly = (got < 5 and res[f"{stage}_rel_residual"] == 0.0) or (ref_its < 5 and want[stage][1] == 0.0)
            assert got == ref_its or (ended_exactly and 0 <= got <= 5), stage
        for key in STAGE_KEYS:
            _close(res[key], want[key], f"{name} {kind} {key} after 5 iterations")
        assert not res["applied"] or all(res[f"{s}_rel_residual"] == 0.0 for s in ("rot", "trans"))
        if not res["applied"]:
            assert pg.Poses().tobytes() == g.poses.tobytes()
    finally:
        pg.close()


# ---------------------------------------------------------------- to the tolerance
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(ipcases.SHAPES))
def test_converged_iterations_and_final_poses(ctx, name, kind):
    g, P = _case(name)
    direct, want = _direct(name), _mirror(name, kind, TOL, 5000)
    pg = _upload(ctx, g, P, kind)
    try:
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(pcg_rel_tol=TOL, pcg_max_iterations=5000), return_stages=True)
        poses = pg.Poses()
        print(f"  {name} {kind}: iterations {res['rot_iterations']} + {res['pre_iterations']} + {res['trans_iterations']} "
              f"(mirror {want['rot'][0]} + {want['pre'][0]} + {want['trans'][0]}); cost {res['cost_before']:.4e} -> {res['cost_after']:.4e}; "
              f"aligned {res['aligned_components']}, smallest ratio {res['min_align_ratio']:.3e}")
        assert want["applied"] and direct["applied"] and res["applied"] and res["rot_converged"] and res["trans_converged"]
        assert res["degenerate_nodes"] == direct["degenerate_nodes"] == 0 and res["rank_deficient_components"] == 0
        assert res["aligned_components"] == direct["aligned_components"] and bool(res["pre_converged"]) == (direct["aligned_components"] > 0)
        for stage in ("rot", "pre", "trans"):
            assert res[f"{stage}_iterations"] == want[stage][0], stage
            assert res[f"{stage}_rel_residual"] <= TOL
        own = float(np.abs(want["poses"] - direct["poses"]).max())
        _close(poses, direct["poses"], f"{name} {kind} poses against the direct solve", own)
        _close(res["rows"], direct["rows"], f"{name} {kind} rows against the direct solve", float(np.abs(want["rows"] - direct["rows"]).max()))
        _close(res["align"][:, 16:25], direct["align"][:, 16:25], f"{name} {kind} G against the direct solve",
               float(np.abs(want["align"][:, 16:25] - direct["align"][:, 16:25]).max()) if direct["aligned_components"] else 0.0)
        assert np.isclose(res["min_align_ratio"], direct["min_align_ratio"], rtol=1e-6, atol=1e-12)
        assert np.isclose(res["cost_before"], direct["cost_before"], rtol=1e-9) and poses[g.fixed].tobytes() == g.poses[g.fixed].tobytes()
        assert abs(res["cost_after"] - direct["cost_after"]) <= 1e-6 * max(1.0, direct["cost_after"])
        with pytest.raises(ElmError):  # an applied call invalidates the linearization, as SetPoses does
            pg.Linearization()
    finally:
        pg.close()


# ---------------------------------------------------------------- no prior is the parent
@pytest.mark.parametrize("name", ("ring", "N257", "two_components", "isolated_free_node"))
def test_without_priors_the_call_is_initialize_in_bytes(ctx, name):
    g = icases.SHAPES[name]()
    for kind, reserve in (("block_jacobi", 0), ("chain", 4)):  # with and without room for priors: none is in the object
        outs = []
        for call in ("Initialize", "InitializeWithPriors"):
            pg = PoseGraph(g.N, max(g.E, 1), ctx, prior_capacity=reserve)
            try:
                pg.SetPreconditioner(kind)
                pg.AddNodes(g.poses, g.fixed)
                pg.AddEdges(g.i, g.j, g.Z, g.info)
                res = getattr(pg, call)(return_stages=True)
                outs.append((res, pg.Poses()))
            finally:
                pg.close()
        (a, pa), (b, pb) = outs
        assert a["applied"] and pa.tobytes() == pb.tobytes() and pa.tobytes() != g.poses.tobytes()
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
        assert b["aligned_components"] == 0 and b["pre_iterations"] == 0 and not b["v_pre"].any() and b["align"].shape == (0, 28)


# ---------------------------------------------------------------- not applied: rank-deficient, not converged
def _assert_untouched(pg, g, before, lin_before, step):
    assert _state(pg) == before and pg.Poses().tobytes() == g.poses.tobytes()
    lin = pg.Linearization()  # a valid linearization is still valid, and the same, the priors' part included
    assert all(lin_before[k].tobytes() == lin[k].tobytes() for k in lin_before)
    # the fixed flags on the device are the object's own: the same solve gives the same bytes, and no gauge node is still held
    assert pg.Solve(1e-3, 1e-10, 500)[0].tobytes() == step.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_the_collinear_ring_is_reported_and_not_applied(ctx, kind):
    g, P, _ = pcases.anchored_ring(every=32)  # two position priors: collinear
    pg = _upload(ctx, g, P, kind, room=2)
    try:
        pg.SetPriorHuber(0.75)
        pg.Linearize(1.5)
        before, lin_before, step = _state(pg), pg.Linearization(), pg.Solve(1e-3, 1e-10, 500)[0]
        assert step[0].any()  # node 0, the gauge node, is free
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(pcg_rel_tol=TOL), return_stages=True)
        assert res["aligned_components"] == 1 and res["rank_deficient_components"] == 1 and not res["applied"]
        assert res["rot_converged"] and res["pre_converged"] and res["trans_converged"] and res["min_align_ratio"] <= 1e-10
        _assert_untouched(pg, g, before, lin_before, step)
        # either side of align_min_ratio on the four-prior ring, whose ratio the call reports
        pg.ClearPriors()
        _, P4, _ = pcases.anchored_ring(every=16)
        pg.AddPriors(P4.node, P4.Z, P4.info, P4.lever)
        ratio = pg.InitializeWithPriors(PoseGraphInitPriorConfig(align_min_ratio=1e-12))["min_align_ratio"]
        assert 0.0 < ratio < 1.0
        pg.SetPoses(g.poses)
        # (the same start gives the same sigma; 1e-12 either way is far above the rounding of the quotient and its product)
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(align_min_ratio=ratio * (1.0 + 1e-12)))
        assert not res["applied"] and res["rank_deficient_components"] == 1 and res["min_align_ratio"] == ratio
        assert pg.Poses().tobytes() == g.poses.tobytes()
        assert pg.InitializeWithPriors(PoseGraphInitPriorConfig(align_min_ratio=ratio * (1.0 - 1e-12)))["applied"]
    finally:
        pg.close()


@pytest.mark.parametrize("kind", KINDS)
def test_non_convergence_leaves_the_graph_as_it_was(ctx, kind):
    g, P = _case("every_class")
    pg = _upload(ctx, g, P, kind)
    try:
        pg.SetPriorHuber(0.5)
        cfg = PoseGraphInitPriorConfig(pcg_max_iterations=2)
        res = pg.InitializeWithPriors(cfg, return_stages=True)
        assert not res["applied"] and not res["rot_converged"] and res["rot_iterations"] == 2 and res["aligned_components"] == 2
        assert pg.Poses().tobytes() == g.poses.tobytes() and np.isfinite(res["cost_after"])
        with pytest.raises(ElmError):  # no linearization before, none after
            pg.Linearization()
        pg.Linearize(1.5)
        before, lin_before, step = _state(pg), pg.Linearization(), pg.Solve(1e-3, 1e-10, 500)[0]
        pri_before = pg.PriorLinearization()
        assert not pg.InitializeWithPriors(cfg)["applied"]
        _assert_untouched(pg, g, before, lin_before, step)
        pri = pg.PriorLinearization()
        assert all(pri_before[k].tobytes() == pri[k].tobytes() for k in pri)
    finally:
        pg.close()


# ---------------------------------------------------------------- single stages, legal and refused
def test_single_stages(ctx):
    g, P = _case("N255_P255_anchored")  # pose and position priors: both single stages are legal
    for stages in (ipref.ROT, ipref.TRANS):
        want = ipref.initialize(g, P, stages=stages)
        pg = _upload(ctx, g, P, "chain")
        try:
            res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(stages=stages, pcg_rel_tol=TOL), return_stages=True)
            poses = pg.Poses()
            assert res["applied"] and bool(res["rot_converged"]) == (stages == ipref.ROT) and bool(res["trans_converged"]) == (stages == ipref.TRANS)
            assert res["aligned_components"] == 0 and res["pre_iterations"] == 0
            for key in ("rows", "v", "v_pre"):
                _close(res[key], want[key], f"stages {stages} {key}")
            _close(poses, want["poses"], f"stages {stages} poses")
            if stages == ipref.ROT:
                assert poses[:, :3, 3].tobytes() == g.poses[:, :3, 3].tobytes() and res["trans_iterations"] == 0
            else:
                assert poses[:, :3, :3].tobytes() == g.poses[:, :3, :3].tobytes() and res["rot_iterations"] == 0
        finally:
            pg.close()
    # position priors alone: TRANS alone anchors the translations directly and aligns nothing, ROT alone is refused
    g, P = _case("aligned4_lever0")
    want = ipref.initialize(g, P, stages=ipref.TRANS)
    pg = _upload(ctx, g, P)
    try:
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(stages=ipref.TRANS, pcg_rel_tol=TOL), return_stages=True)
        assert res["applied"] and res["aligned_components"] == 0 and want["aligned_components"] == 0
        _close(pg.Poses(), want["poses"], "position priors, TRANS alone")
        before = pg.Poses().tobytes()
        with pytest.raises(ElmError, match="only position priors"):
            pg.InitializeWithPriors(PoseGraphInitPriorConfig(stages=ipref.ROT))
        assert pg.Poses().tobytes() == before
    finally:
        pg.close()


def test_refusals_on_a_live_object(ctx):
    res = _lib.PoseGraphInitPriorResultC()
    L = _lib.lib()
    g, P = _case("aligned3")
    none = pref.Priors()
    rot_only = pcases.rand_priors(g, 2, 9, kind="pose", nodes=[1, 5])
    rot_only.info[:, :3, :] = 0.0
    rot_only.info[:, :, :3] = 0.0
    for priors, stages, text in ((none, 3, "no prior of positive weight"), (rot_only, 3, "positive translation weight"), (rot_only, 2, "positive translation weight"),
                                 (P, 1, "only position priors")):
        assert ipref.classes(g, priors, stages)["refusal"] is not None
        pg = _upload(ctx, g, priors if priors.P else P)
        try:
            if not priors.P:
                pg.ClearPriors()
            pg.Linearize()
            before = _state(pg)
            with pytest.raises(ElmError, match=text):
                pg.InitializeWithPriors(PoseGraphInitPriorConfig(stages=stages))
            assert _state(pg) == before
            pg.Linearization()  # raised before any launch: the linearization is still valid
        finally:
            pg.close()
    assert ipref.classes(g, rot_only, 1)["refusal"] is None  # rotation priors alone carry the rotation stage
    pg = _upload(ctx, g, P)
    try:
        before = _state(pg)
        cfg = PoseGraphInitPriorConfig()
        for bad in (dict(align_min_ratio=0.0), dict(align_min_ratio=-1.0), dict(align_min_ratio=float("nan")), dict(align_min_ratio=float("inf")),
                    dict(stages=0), dict(stages=4), dict(pcg_rel_tol=0.0), dict(pcg_max_iterations=0), dict(pcg_check_every=0)):
            with pytest.raises(ElmError):
                pg.InitializeWithPriors(PoseGraphInitPriorConfig(**bad))
        assert L.elm_posegraph_initialize_priors(ctx._h, pg._h, C.byref(cfg), C.byref(res), None, None, None, None, -1) == -1
        assert L.elm_posegraph_initialize_priors(ctx._h, pg._h, None, C.byref(res), None, None, None, None, 0) == -1
        assert L.elm_posegraph_initialize_priors(ctx._h, pg._h, C.byref(cfg), None, None, None, None, None, 0) == -1
        assert _state(pg) == before
        # Initialize still refuses the graph that this call takes
        with pytest.raises(ElmError, match="no fixed node"):
            pg.Initialize()
        # an edge without a rotation weight is refused here as there
        info = np.eye(6)
        info[3:, 3:] = 0.0
        pg.AddEdges([0], [2], (np.linalg.inv(g.poses[0]) @ g.poses[2])[None], info)
        with pytest.raises(ElmError, match="rotation weight"):
            pg.InitializeWithPriors()
    finally:
        pg.close()


# ---------------------------------------------------------------- bytes
@pytest.mark.parametrize("kind", KINDS)
def test_three_runs_give_the_same_bytes(ctx, kind):
    g, P = _case("every_class")
    outs = []
    for _ in range(3):
        pg = _upload(ctx, g, P, kind)
        try:
            res = pg.InitializeWithPriors(return_stages=True)
            outs.append(b"".join(np.asarray(res[k]).tobytes() for k in sorted(res)) + pg.Poses().tobytes())
            assert res["applied"] and res["aligned_components"] == 2
        finally:
            pg.close()
    assert outs[0] == outs[1] == outs[2]


# ---------------------------------------------------------------- the recording, and what the call is for
@pytest.mark.parametrize("name", list(ipcases.RECORDED))
def test_the_recorded_fixtures(ctx, name):
    gold = np.load(ipcases.GOLDEN)
    g, P = ipcases.RECORDED[name]()
    pg = _upload(ctx, g, P, "chain")
    try:
        res = pg.InitializeWithPriors(PoseGraphInitPriorConfig(pcg_rel_tol=TOL), return_stages=True)
        assert res["applied"] and res["aligned_components"] == 1
        dt, dr = ref.pose_error(pg.Poses(), gold[name + "_poses"])
        print(f"  {name}: against the recording {dt:.3e} m {dr:.3e} rad; cost {res['cost_before']:.4e} -> {res['cost_after']:.4e}")
        assert dt <= 1e-7 and dr <= 1e-8
        assert np.isclose(res["cost_before"], gold[name + "_cost"][0], rtol=1e-9)
        _close(res["align"][:, :16], gold[name + "_align"][:, :16], f"{name} sums against the recording", 1e-9)
        if name == "gnss_chain":  # the start that Optimize needs: every step accepted, and it stops on its tolerance
            out = pg.Optimize(PoseGraphConfig(**cases.RING_CFG))
            assert out["stop_reason"] == "cost_tol" and out["rejected"] == 0 and out["solves"] <= 8
    finally:
        pg.close()


def _closer(ctx, g, P):
    lc = LoopCloser.__new__(LoopCloser)  # the graph alone: no scan is described
    lc.ctx, lc.scans, lc.poses, lc.loops = ctx, [None] * g.N, [T.copy() for T in g.poses], []
    lc.priors = [(int(P.node[q]), P.Z[q], P.info[q], P.lever[q]) for q in range(P.P)]
    return lc


def test_close_with_priors_is_the_hand_composition(ctx):
    g, P, _ = ipcases.gnss_chain()
    lc = _closer(ctx, g, P)
    cfg = PoseGraphConfig(**cases.RING_CFG)
    poses, res = lc.Close(cfg, fixed=(), preconditioner="chain", initialize="priors")
    Z = np.linalg.inv(g.poses[:-1]) @ g.poses[1:]
    pg = PoseGraph(g.N, g.N, ctx, prior_capacity=P.P)
    try:
        pg.SetPreconditioner("chain")
        pg.AddNodes(g.poses, np.zeros(g.N, bool))
        pg.AddEdges(np.arange(g.N - 1), np.arange(1, g.N), Z)
        pg.SetPriorHuber(0.0)
        pg.AddPriors(P.node, P.Z, P.info, P.lever)
        init = pg.InitializeWithPriors()
        out = pg.Optimize(cfg)
        assert poses.tobytes() == pg.Poses().tobytes() and res["initialize"] == init and init["applied"] and init["aligned_components"] == 1
        assert {k: v for k, v in res.items() if k != "initialize"} == out
    finally:
        pg.close()
    with pytest.raises(ElmError):  # initialize=True ignores the priors and refuses the graph without a fixed node, as before
        lc.Close(cfg, fixed=(), preconditioner="chain", initialize=True)
    with pytest.raises(ElmError, match="False, True or"):
        lc.Close(cfg, initialize="prior")
    # initialize=True with a fixed node: Initialize, in bytes
    a, ra = lc.Close(cfg, preconditioner="chain", initialize=True)
    pg = PoseGraph(g.N, g.N, ctx, prior_capacity=P.P)
    try:
        fx = np.zeros(g.N, bool)
        fx[0] = True
        pg.SetPreconditioner("chain")
        pg.AddNodes(g.poses, fx)
        pg.AddEdges(np.arange(g.N - 1), np.arange(1, g.N), Z)
        pg.AddPriors(P.node, P.Z, P.info, P.lever)
        init = pg.Initialize()
        out = pg.Optimize(cfg)
        assert a.tobytes() == pg.Poses().tobytes() and ra["initialize"] == init and {k: v for k, v in ra.items() if k != "initialize"} == out
    finally:
        pg.close()
