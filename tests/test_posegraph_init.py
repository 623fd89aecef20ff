"""The pose graph's linear initialization on the GPU (include/elimaloc_hip_posegraph_init.h) against its mirror
(tests/posegraph_init_ref.py), with both preconditioners, on the smallest shapes at which each path can go wrong: five conjugate-gradient
iterations of both stages under the project's 1e-9 contract, the iteration counts and residuals at 1e-10, the final poses against the
mirror's direct solve, the constructed degenerate node, non-convergence, the preconditions on a live object, the run-to-run bytes, and
Initialize before Optimize on the loop fixture and through LoopCloser.Close."""
import ctypes as C
import functools

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_ref as cref
import posegraph_init_cases as icases
import posegraph_init_ref as iref
import posegraph_ref as ref
from elimaloc_amd import _lib
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig, PoseGraphInitConfig

pytestmark = pytest.mark.gpu

KINDS = ("block_jacobi", "chain")
TOL = 1e-10
NEVER = 1e-300  # a tolerance no solve meets: the call needs one above 0, the iteration count is then pcg_max_iterations


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
def _graph(name):
    return icases.SHAPES[name]() if name in icases.SHAPES else getattr(icases, name)()


@functools.lru_cache(maxsize=None)
def _direct(name):
    """the mirror's whole call with direct solves, computed once per shape and left unchanged"""
    return iref.initialize(_graph(name))


@functools.lru_cache(maxsize=None)
def _mirror(name, kind, tol, max_it):
    return iref.initialize(_graph(name), solver=_mirror_pcg(kind, tol, max_it))


def _upload(ctx, g, kind="block_jacobi"):
    pg = PoseGraph(max(g.N, 1), max(g.E, 1), ctx)
    pg.SetPreconditioner(kind)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
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


def _true_rel_residual(g, lin, delta):
    """|b - H delta| / |b| in the 2-norm, from the mirror's system"""
    H, b = iref.system(g, lin)
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(b - H @ np.where(lin["active"][:, None], delta, 0.0).reshape(-1))) / nb if nb > 0.0 else 0.0


# ---------------------------------------------------------------- five iterations of both stages
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(icases.SHAPES))
def test_five_iterations_against_the_mirror(ctx, name, kind):
    g = _graph(name)
    want = _mirror(name, kind, NEVER, 5)
    pg = _upload(ctx, g, kind)
    try:
        res = pg.Initialize(PoseGraphInitConfig(pcg_rel_tol=NEVER, pcg_max_iterations=5), return_stages=True)
        print(f"  {name} {kind}: iterations {res['rot_iterations']} + {res['trans_iterations']} (mirror {want['rot'][0]} + {want['trans'][0]})")
        for stage in ("rot", "trans"):
            # Exactly five, as the mirror.  The one way out of five iterations at this tolerance is r'z == 0, a solve that ended exactly:
            # with one free node the first step is the solution, and the last bit decides on which side the residual is exactly 0 (the
            # GPU's translations and the mirror's rotations on the two-node graph).  Any other early stop fails here.
            got, got_res, ref_its, ref_res = res[f"{stage}_iterations"], res[f"{stage}_rel_residual"], want[stage][0], want[stage][1]
            ended_exactly = (got < 5 and got_res == 0.0) or (ref_its < 5 and ref_res == 0.0)
            assert got == ref_its == 5 or (ended_exactly and 1 <= got <= 5), stage
        # both against the mirror's own five iterations of both stages, under the contract alone (posegraph_init_cases.py says what makes
        # a shape fit for that)
        _close(res["rows"], want["rows"], f"{name} {kind} rows after 5 iterations")
        _close(res["v"], want["v"], f"{name} {kind} v after 5 iterations")
        # in addition, the second stage alone: the mirror's five iterations at the rotations projected from the GPU's rows, which is the
        # system the GPU solved (a difference in the rows otherwise reaches v times the lever arm)
        inactive = ~want["rot_lin"]["active"]
        R, deg = iref.project(res["rows"])
        trial = g.poses.copy()
        move = ~inactive & ~deg
        trial[move, :3, :3] = R[move]
        lin = iref.trans_system(g, trial)
        v_ref = np.where(lin["active"][:, None], _mirror_pcg(kind, NEVER, 5)(g, lin)[0][:, :3], 0.0)
        _close(res["v"], v_ref, f"{name} {kind} v after 5 iterations at the same rotations")
        assert np.array_equal(res["rows"][inactive], iref.rows_of(g.poses)[inactive]) and not res["v"][inactive].any()
        if not res["applied"]:  # (a solve that ends exactly, on the smallest graphs, may meet even this tolerance)
            assert pg.Poses().tobytes() == g.poses.tobytes()
    finally:
        pg.close()


# ---------------------------------------------------------------- to the tolerance
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(icases.SHAPES))
def test_converged_iterations_residuals_and_final_poses(ctx, name, kind):
    g = _graph(name)
    direct, want = _direct(name), _mirror(name, kind, TOL, 5000)
    pg = _upload(ctx, g, kind)
    try:
        res = pg.Initialize(PoseGraphInitConfig(pcg_rel_tol=TOL, pcg_max_iterations=5000), return_stages=True)
        poses = pg.Poses()
        d_rot = res["rows"] - iref.rows_of(g.poses)
        d_trans = np.concatenate([res["v"], np.zeros((g.N, 3))], axis=1)
        rho_r, rho_t = _true_rel_residual(g, direct["rot_lin"], d_rot), _true_rel_residual(g, want["trans_lin"], d_trans)
        print(f"  {name} {kind}: iterations {res['rot_iterations']} + {res['trans_iterations']} (mirror {want['rot'][0]} + {want['trans'][0]}); "
              f"recurrence residuals {res['rot_rel_residual']:.2e}, {res['trans_rel_residual']:.2e}; true relative residuals {rho_r:.2e}, {rho_t:.2e}; "
              f"cost {res['cost_before']:.4e} -> {res['cost_after']:.4e}")
        assert want["applied"] and res["applied"] and res["rot_converged"] and res["trans_converged"] and res["degenerate_nodes"] == 0
        assert res["rot_rel_residual"] <= TOL and res["trans_rel_residual"] <= TOL
        assert abs(res["rot_iterations"] - want["rot"][0]) <= 1 and abs(res["trans_iterations"] - want["trans"][0]) <= 1
        own_rows = float(np.abs(want["rows"] - direct["rows"]).max())
        own_pose = float(np.abs(want["poses"] - direct["poses"]).max())
        _close(res["rows"], direct["rows"], f"{name} {kind} rows against the direct solve", own_rows)
        _close(poses, direct["poses"], f"{name} {kind} poses against the direct solve", own_pose)
        assert np.isclose(res["cost_before"], direct["cost_before"], rtol=1e-9) and poses[g.fixed].tobytes() == g.poses[g.fixed].tobytes()
        assert abs(res["cost_after"] - direct["cost_after"]) <= 1e-6 * max(1.0, direct["cost_after"])
        with pytest.raises(ElmError):  # an applied call invalidates the linearization, as SetPoses does
            pg.Linearization()
    finally:
        pg.close()


def test_a_node_without_edges_and_the_fixed_nodes_keep_their_bytes(ctx):
    g = _graph("isolated_free_node")
    pg = _upload(ctx, g)
    try:
        assert pg.Initialize()["applied"]
        poses = pg.Poses()
        assert poses[-1].tobytes() == g.poses[-1].tobytes() and poses[g.fixed].tobytes() == g.poses[g.fixed].tobytes()
    finally:
        pg.close()
    g = _graph("fixed_interior")
    pg = _upload(ctx, g, "chain")
    try:
        assert g.fixed[5] and pg.Initialize()["applied"]
        assert pg.Poses()[g.fixed].tobytes() == g.poses[g.fixed].tobytes()
    finally:
        pg.close()


# ---------------------------------------------------------------- single stages
@pytest.mark.parametrize("stages", (iref.ROT, iref.TRANS))
def test_single_stages(ctx, stages):
    g = _graph("ring")
    want = iref.initialize(g, stages=stages)
    pg = _upload(ctx, g, "chain")
    try:
        res = pg.Initialize(PoseGraphInitConfig(stages=stages, pcg_rel_tol=TOL), return_stages=True)
        poses = pg.Poses()
        assert res["applied"] and bool(res["rot_converged"]) == (stages == iref.ROT) and bool(res["trans_converged"]) == (stages == iref.TRANS)
        _close(res["rows"], want["rows"], f"stages {stages} rows")
        _close(res["v"], want["v"], f"stages {stages} v")
        _close(poses, want["poses"], f"stages {stages} poses")
        if stages == iref.ROT:
            assert poses[:, :3, 3].tobytes() == g.poses[:, :3, 3].tobytes() and res["trans_iterations"] == 0
        else:
            assert poses[:, :3, :3].tobytes() == g.poses[:, :3, :3].tobytes() and res["rot_iterations"] == 0
    finally:
        pg.close()


# ---------------------------------------------------------------- the degenerate node
@pytest.mark.parametrize("kind", KINDS)
def test_the_constructed_degenerate_node_keeps_its_rotation(ctx, kind):
    g = icases.degenerate_node()
    want = iref.initialize(g)
    pg = _upload(ctx, g, kind)
    try:
        res = pg.Initialize(PoseGraphInitConfig(pcg_rel_tol=TOL), return_stages=True)
        poses = pg.Poses()
        assert want["degenerate_nodes"] == 1 and res["degenerate_nodes"] == 1 and res["applied"]
        assert np.abs(res["rows"][1]).max() <= 1e-12 and poses[1, :3, :3].tobytes() == g.poses[1, :3, :3].tobytes()
        _close(res["rows"], want["rows"], f"{kind} rows with a degenerate node")
        _close(poses, want["poses"], f"{kind} poses with a degenerate node")
    finally:
        pg.close()


# ---------------------------------------------------------------- non-convergence, preconditions, bytes
def test_non_convergence_leaves_the_graph_as_it_was(ctx):
    g = _graph("ring")
    for kind in KINDS:
        pg = _upload(ctx, g, kind)
        try:
            cfg = PoseGraphInitConfig(pcg_max_iterations=2)
            res = pg.Initialize(cfg, return_stages=True)
            assert not res["applied"] and not res["rot_converged"] and res["rot_iterations"] == 2 and res["trans_iterations"] <= 2
            assert pg.Poses().tobytes() == g.poses.tobytes() and np.isfinite(res["cost_after"]) and np.abs(res["rows"]).max() > 0.0
            with pytest.raises(ElmError):  # no linearization before, none after
                pg.Linearization()
            pg.Linearize(1.5)
            before = pg.Linearization()
            step = pg.Solve(1e-3, 1e-10, 500)[0]
            assert not pg.Initialize(cfg)["applied"]
            after = pg.Linearization()  # a valid linearization is still valid, and the same
            assert all(before[k].tobytes() == after[k].tobytes() for k in before)
            assert pg.Solve(1e-3, 1e-10, 500)[0].tobytes() == step.tobytes() and pg.Poses().tobytes() == g.poses.tobytes()
        finally:
            pg.close()


def test_preconditions_on_a_live_object(ctx):
    res = _lib.PoseGraphInitResultC()
    for g, stages, ok_stages in ((icases.zero_trace("r"), iref.ROT, iref.TRANS), (icases.zero_trace("t"), iref.TRANS, iref.ROT),
                                 (icases.zero_trace("r"), iref.ROT | iref.TRANS, None), (icases.unanchored(), iref.ROT | iref.TRANS, None),
                                 (icases.unanchored(), iref.TRANS, None)):
        assert iref.refusal(g, stages) is not None
        pg = _upload(ctx, g)
        try:
            lin = pg.Linearize()
            before = pg.Linearization()
            cfg = PoseGraphInitConfig(stages=stages)
            assert _lib.lib().elm_posegraph_initialize(ctx._h, pg._h, C.byref(cfg), C.byref(res), None, None) == -1
            with pytest.raises(ElmError, match=r"\(-1\).*(weight|fixed node)"):
                pg.Initialize(cfg)
            assert pg.Poses().tobytes() == g.poses.tobytes() and pg.Size() == (g.N, g.E)
            assert all(before[k].tobytes() == pg.Linearization()[k].tobytes() for k in before) and pg.Linearize() == lin
            if ok_stages is not None:  # the other stage alone is served
                assert iref.refusal(g, ok_stages) is None and pg.Initialize(PoseGraphInitConfig(stages=ok_stages))["applied"]
        finally:
            pg.close()
    pg = PoseGraph(4, 4, ctx)
    try:
        with pytest.raises(ElmError, match=r"\(-1\).*no node"):
            pg.Initialize()
        cfg = PoseGraphInitConfig()
        for bad in (dict(stages=0), dict(stages=4), dict(pcg_rel_tol=0.0), dict(pcg_max_iterations=0), dict(pcg_check_every=0)):
            with pytest.raises(ElmError, match=r"\(-1\)"):
                pg.Initialize(PoseGraphInitConfig(**bad))
        assert _lib.lib().elm_posegraph_initialize(ctx._h, pg._h, C.byref(cfg), None, None, None) == -1
    finally:
        pg.close()


def test_two_calls_from_the_same_start_give_the_same_bytes(ctx):
    for name, kind in (("N513", "chain"), ("star70", "block_jacobi"), ("ring", "chain")):
        g = _graph(name)
        pg = _upload(ctx, g, kind)
        try:
            runs = []
            for _ in range(3):
                pg.SetPoses(g.poses)
                res = pg.Initialize(return_stages=True)
                runs.append((pg.Poses().tobytes(), res["rows"].tobytes(), res["v"].tobytes(), repr({k: v for k, v in res.items() if k not in ("rows", "v")})))
            assert all(r == runs[0] for r in runs[1:]), name
        finally:
            pg.close()


# ---------------------------------------------------------------- end to end
def test_initialize_then_optimize_the_ring(ctx):
    gold = np.load(cases.GOLDEN)
    g, truth = cases.ring()
    for kind in KINDS:
        pg = _upload(ctx, g, kind)
        try:
            plain = pg.Optimize(PoseGraphConfig(**cases.RING_CFG))
            pg.SetPoses(g.poses)
            init = pg.Initialize()
            dt0, dr0 = ref.pose_error(pg.Poses(), truth)
            res = pg.Optimize(PoseGraphConfig(**cases.RING_CFG))
            poses = pg.Poses()
            print(f"  ring {kind}: after the initialization alone {dt0:.3e} m, {dr0:.3e} rad of the truth, cost {init['cost_before']:.3e} -> "
                  f"{init['cost_after']:.3e}; then {res['solves']} solves (without: {plain['solves']})")
            assert init["applied"] and init["cost_after"] < 1e-6 * init["cost_before"]
            for want in (gold["ring_poses"], truth):
                dt, dr = ref.pose_error(poses, want)
                assert dt <= 1e-4 and dr <= 1e-5  # the bounds of tests/test_posegraph.py::test_optimize_the_ring
            assert res["solves"] <= plain["solves"] and res["rejected"] == 0 and poses[0].tobytes() == g.poses[0].tobytes()
        finally:
            pg.close()


def _scan_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32))


def test_loop_closer_close_with_and_without_the_initialization(ctx):
    """the loop fixture of tests/test_posegraph.py::test_loop_closer_close_and_map: the drifted ring inserted, its three loops added"""
    g, truth = cases.ring()
    db = PlaceDatabase(PlaceConfig(), cases.RING_N, ctx)
    try:
        lc = LoopCloser(db)
        for k in range(cases.RING_N):
            lc.Insert(_scan_points(64, 500 + k), g.poses[k])
        for a, b in cases.RING_LOOPS:
            lc.AddLoop(a, b, cases.inv_pose(truth[a]) @ truth[b])
        cfg = PoseGraphConfig(**cases.RING_CFG)
        poses, res = lc.Close(cfg)
        named, res_named = lc.Close(cfg, initialize=False)
        assert poses.tobytes() == named.tobytes() and repr(res) == repr(res_named) and "initialize" not in res  # the default path: the same bytes
        with_init, res_init = lc.Close(cfg, initialize=True)
        dt, dr = ref.pose_error(with_init, poses)
        print(f"  Close with the initialization against without: {dt:.3e} m, {dr:.3e} rad; solves {res_init['solves']} against {res['solves']}; "
              f"init {res_init['initialize']}")
        assert res_init["initialize"]["applied"] and dt <= 1e-4 and dr <= 1e-5
        assert np.stack(lc.poses).tobytes() == g.poses.tobytes()
    finally:
        db.close()
