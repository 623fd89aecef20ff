"""The pose graph on the GPU (elm_posegraph_*): the linearization, the conjugate-gradient step and
Levenberg-Marquardt against the numpy mirror of the contract (tests/posegraph_ref.py) under the project's 1e-9 sums contract; the loop
fixture against its committed recording and the truth; the run-to-run bytes; misuse; and LoopCloser.Close / Map against the hand
composition of the public calls they are made of."""
import math

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_ref as ref
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig
from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig, Scan, VoxelHashMap

pytestmark = pytest.mark.gpu

# elm_internal.hpp: k_pg_spmv serves kPgNodesPerBlock = 32 nodes per workgroup and writes one partial of p^T q each; the lanes that
# reduce the slots are kPgBlock = 256, so from 256 * 32 + 1 nodes on a lane adds more than one slot before the tree
NODES_PER_BLOCK, REDUCE_LANES, HUB_DEGREE = 32, 256, 64
SECOND_TRIP_NODES = REDUCE_LANES * NODES_PER_BLOCK + 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _upload(ctx, g, node_capacity=None, edge_capacity=None):
    pg = PoseGraph(node_capacity or max(g.N, 1), edge_capacity or max(g.E, 1), ctx)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    return pg


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(np.asarray(got) - want).max()) if want.size else 0.0
    bound = 1e-9 * max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    print(f"  {what}: |gpu - ref| {err:.3e} (bound {bound:.1e})")
    assert np.asarray(got).shape == want.shape and err <= bound, what


# ---------------------------------------------------------------- linearize
def _duplicates():
    g = cases.random_graph(6, 10, 31)
    i, j = np.concatenate([g.i, g.i[:4], g.j[:3]]), np.concatenate([g.j, g.j[:4], g.i[:3]])  # each of four edges twice, three reversed
    return ref.Graph(g.poses, g.fixed, i, j, np.concatenate([g.Z, g.Z[:4], np.stack([cases.inv_pose(Z) for Z in g.Z[:3]])]),
                     np.concatenate([g.info, g.info[:4], g.info[:3]]))


def _isolated():
    g = cases.random_graph(9, 12, 32)
    poses = np.concatenate([g.poses, g.poses[:1] @ cases.rand_pose(np.random.default_rng(1), 1.0, 5.0)[None]])
    return ref.Graph(poses, np.append(g.fixed, False), g.i, g.j, g.Z, g.info)  # node 9: free, no edge


LIN_CASES = {
    "N1_fixed_E0": lambda: ref.Graph(np.eye(4)[None], [True], [], [], np.zeros((0, 4, 4))),
    "N2_E0": lambda: cases.random_graph(2, 0, 10),
    "N2_E1": lambda: cases.random_graph(2, 1, 11),
    "E63": lambda: cases.random_graph(40, 63, 12),
    "E64": lambda: cases.random_graph(40, 64, 13),
    "E65": lambda: cases.random_graph(40, 65, 14),
    "N255_E255": lambda: cases.random_graph(255, 255, 15),
    "N256_E256": lambda: cases.random_graph(256, 256, 16),
    "N257_E257": lambda: cases.random_graph(257, 257, 17),
    "N1025_E1100": lambda: cases.random_graph(1025, 1100, 18),
    "degree1": lambda: cases.star(1, 21),
    "degree2": lambda: cases.star(2, 22),
    "degree64": lambda: cases.star(64, 23),
    "degree65": lambda: cases.star(65, 24),
    "hub300": lambda: cases.star(300, 25),
    "duplicates": _duplicates,
    "isolated_free_node": _isolated,
    "all_fixed": lambda: cases.random_graph(6, 8, 33, fixed=range(6)),
    "poses_at_1e5_m": lambda: cases.random_graph(30, 60, 34, offset=1e5),
    "rotation_family": cases.rotation_family,
}


@pytest.mark.parametrize("name", list(LIN_CASES))
def test_linearize_against_the_mirror(ctx, name):
    g = LIN_CASES[name]()
    pg = _upload(ctx, g)
    try:
        assert pg.Size() == (g.N, g.E)
        for k in (0.0, 0.3):  # (0.3: inliers and outliers in every random case)
            want = ref.linearize(g, huber_k=k)
            st = pg.Linearize(k)
            got = pg.Linearization()
            for a in ("r", "A", "B", "s", "w", "grad", "diag"):
                _close(got[a], want[a], f"{name} huber {k} {a}")
            _close([st["chi2"], st["cost"], st["grad_inf_norm"]], [want["chi2"], want["cost"], want["grad_inf_norm"]], "stats")
            assert st["n_outliers"] == want["n_outliers"]
        _close(pg.Poses(), g.poses, "poses")
    finally:
        pg.close()


def test_linearize_hand_cases_in_bytes(ctx):
    g, want_rt = cases.hand_integers()
    pg = _upload(ctx, g)
    try:
        pg.Linearize(0.0)
        L = pg.Linearization()
        assert L["r"][:, :3].tobytes() == want_rt.tobytes() and L["r"][:, 3:].tobytes() == np.zeros((4, 3)).tobytes()  # Log(I) == +0
        assert L["s"].tolist() == [4.0, 9.0, 1.0, 18.0] and L["w"].tolist() == [1.0] * 4
        assert (L["B"] == np.eye(6)).all() and (L["A"][:, 3:, 3:] == -np.eye(3)).all() and (L["A"][:, :3, :3] == -np.eye(3)).all()
        assert pg.Poses().tobytes() == g.poses.tobytes()
        st = pg.Linearize(2.0)  # s = 4 == k^2: an inlier
        w = pg.Linearization()["w"]
        assert w[0] == 1.0 and w[2] == 1.0 and w[1] == 2.0 / 3.0 and st["n_outliers"] == 2
        below = float(np.nextafter(2.0, 0.0))
        st = pg.Linearize(below)
        w = pg.Linearization()["w"]
        assert w[0] == below / 2.0 and w[0] < 1.0 and w[2] == 1.0 and st["n_outliers"] == 3
    finally:
        pg.close()


# ---------------------------------------------------------------- solve
SMALL = {"two": lambda: cases.chain(2, 1, loops=0), "chain12": lambda: cases.chain(12, 2), "star5": lambda: cases.star(5, 3),
         "random9": lambda: cases.random_graph(9, 20, 4, fixed=(0, 4), ang=0.3)}
FIVE = dict(SMALL)
FIVE.update({"degree64": lambda: cases.star(HUB_DEGREE, 23), "degree65": lambda: cases.star(HUB_DEGREE + 1, 24), "hub300": lambda: cases.star(300, 25),
             "isolated_free_node": _isolated, "second_trip_of_the_slots": lambda: cases.chain(SECOND_TRIP_NODES, 40, loops=20)})


@pytest.mark.parametrize("name", list(FIVE))
def test_five_iterations_against_the_mirror(ctx, name):
    g = FIVE[name]()
    pg = _upload(ctx, g)
    try:
        lin = ref.linearize(g, huber_k=1.5)
        pg.Linearize(1.5)
        for lam in (0.0, 1.0):
            want, its, _, conv = ref.pcg(g, lin, lam, 0.0, 5)
            delta, st = pg.Solve(lam, 0.0, 5)
            assert (its, conv) == (5, False) and st["iterations"] == 5 and not st["converged"]
            _close(delta, want, f"{name} lambda {lam} delta after 5 iterations")
            assert (delta[~lin["active"]] == 0.0).all() and (delta[g.fixed] == 0.0).all()
    finally:
        pg.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_solve_to_tolerance_true_residual(ctx, name):
    tol = 1e-10
    g = SMALL[name]()
    pg = _upload(ctx, g)
    try:
        lin = ref.linearize(g, huber_k=1.5)
        pg.Linearize(1.5)
        for lam in (0.0, 1.0):
            d_ref, its_ref, _, conv_ref = ref.pcg(g, lin, lam, tol, 500)
            rho_ref = ref.true_rel_residual(g, lin, lam, d_ref)  # measured on the CPU first
            delta, st = pg.Solve(lam, tol, 500)
            rho = ref.true_rel_residual(g, lin, lam, delta)
            print(f"  {name} lambda {lam}: gpu {st['iterations']} iterations (mirror {its_ref}), true relative residual {rho:.2e} (mirror {rho_ref:.2e})")
            assert conv_ref and st["converged"] and st["rel_residual"] <= tol
            assert rho <= 10.0 * max(tol, rho_ref)
            assert (delta[g.fixed] == 0.0).all()
    finally:
        pg.close()


# ---------------------------------------------------------------- optimize
def _cfg(d):
    return PoseGraphConfig(**d)


def test_optimize_the_ring(ctx):
    gold = np.load(cases.GOLDEN)
    g, truth = cases.ring()
    pg = _upload(ctx, g)
    try:
        res = pg.Optimize(_cfg(cases.RING_CFG))
        poses = pg.Poses()
        assert [t["accepted"] for t in res["trace"]] == gold["ring_accepted"].astype(bool).tolist()
        assert res["stop_reason"] == str(gold["ring_stop"]) and res["solves"] == len(gold["ring_cost"]) == res["accepted"] and res["rejected"] == 0
        for name, want in (("the fixture", gold["ring_poses"]), ("the truth", truth)):
            dt, dr = ref.pose_error(poses, want)
            print(f"  ring against {name}: {dt:.3e} m, {dr:.3e} rad")
            assert dt <= 1e-4 and dr <= 1e-5
        assert res["cost_final"] <= res["cost_initial"] and math.isclose(res["cost_initial"], float(gold["ring_cost_initial"]), rel_tol=1e-9)
        assert res["pcg_iterations_total"] == sum(t["pcg_iterations"] for t in res["trace"]) > 0
        assert poses[0].tobytes() == g.poses[0].tobytes()  # the fixed node
    finally:
        pg.close()


def test_optimize_the_false_loop_with_huber(ctx):
    gold = np.load(cases.GOLDEN)
    g, _ = cases.ring(false_loop=True)
    pg = _upload(ctx, g)
    try:
        res = pg.Optimize(_cfg(cases.FALSE_CFG))
        assert [t["accepted"] for t in res["trace"]] == gold["false_accepted"].astype(bool).tolist() and res["stop_reason"] == str(gold["false_stop"])
        dt, dr = ref.pose_error(pg.Poses(), gold["false_poses"])
        print(f"  false loop against the recording: {dt:.3e} m, {dr:.3e} rad")
        assert dt <= 1e-4 and dr <= 1e-5
        assert np.allclose([t["cost"] for t in res["trace"]], gold["false_cost"], rtol=1e-6)
        assert pg.Linearize(cases.FALSE_CFG["huber_k"])["n_outliers"] == 1
    finally:
        pg.close()


def test_optimize_one_iteration_and_the_optimum(ctx):
    g, truth = cases.ring()
    pg = _upload(ctx, g)
    try:
        cfg = dict(cases.RING_CFG)
        cfg["max_iterations"] = 1
        res = pg.Optimize(_cfg(cfg))
        want, wres = ref.optimize(g, **cfg)
        assert (res["solves"], res["accepted"], res["stop_reason"]) == (1, 1, "max_iterations") == (wres["solves"], wres["accepted"], wres["stop_reason"])
        assert max(ref.pose_error(pg.Poses(), want)) <= 1e-7 and math.isclose(res["cost_final"], wres["cost_final"], rel_tol=1e-6)
    finally:
        pg.close()
    # at its optimum: translations that are integers and rotations that are the identity make every residual exactly 0
    poses = np.tile(np.eye(4), (5, 1, 1))
    poses[:, :3, 3] = [[0, 0, 0], [2, 1, 0], [4, -3, 1], [5, 5, 5], [-1, 0, 2]]
    i, j = [0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 0, 2]
    g0 = ref.Graph(poses, [True, False, False, False, False], i, j, np.stack([cases.inv_pose(poses[a]) @ poses[b] for a, b in zip(i, j)]))
    pg = _upload(ctx, g0)
    try:
        res = pg.Optimize()
        assert (res["solves"], res["stop_reason"], res["cost_initial"], res["cost_final"]) == (0, "cost_zero", 0.0, 0.0) and res["trace"] == []
        assert pg.Poses().tobytes() == poses.tobytes()
    finally:
        pg.close()


def test_optimize_forced_rejection(ctx):
    """The mirror rejects the plain Gauss-Newton step of cases.wild_chain(): with lambda_init = 0 the damping stays 0, every solve is
    rejected and the poses are unchanged in bytes; from lambda 1e-9 with lambda_up 1e4 two rejections are followed by accepted steps."""
    g = cases.wild_chain()
    pg = _upload(ctx, g)
    try:
        kw = dict(lambda_init=0.0, max_iterations=2, pcg_rel_tol=1e-10, pcg_max_iterations=500)
        _, want = ref.optimize(g, **kw)
        res = pg.Optimize(_cfg(kw))
        assert [t["accepted"] for t in want["trace"]] == [False, False] == [t["accepted"] for t in res["trace"]]
        assert (res["rejected"], res["accepted"], res["lambda_final"], res["stop_reason"]) == (2, 0, 0.0, "max_iterations")
        assert res["cost_final"] == res["cost_initial"] and pg.Poses().tobytes() == g.poses.tobytes()
        assert np.allclose([t["cost"] for t in res["trace"]], [t["cost"] for t in want["trace"]], rtol=1e-6)
        kw = dict(lambda_init=1e-9, lambda_up=1e4, max_iterations=4, pcg_rel_tol=1e-10, pcg_max_iterations=500)
        want_poses, want = ref.optimize(g, **kw)
        res = pg.Optimize(_cfg(kw))
        assert [t["accepted"] for t in want["trace"]] == [False, False, True, True] == [t["accepted"] for t in res["trace"]]
        assert all(abs(t["ratio"] - 1.0) > 0.04 for t in want["trace"])  # no decision hangs on a last digit
        assert np.allclose([t["lambda_"] for t in res["trace"]], [t["lambda_"] for t in want["trace"]], rtol=1e-12)
        assert max(ref.pose_error(pg.Poses(), want_poses)) <= 1e-6 and res["cost_final"] < res["cost_initial"]
        # a rejection at lambda_max ends the run
        kw = dict(lambda_init=0.0, lambda_max=0.0, lambda_min=0.0, max_iterations=5, pcg_rel_tol=1e-10, pcg_max_iterations=500)
        pg.SetPoses(g.poses)
        res = pg.Optimize(_cfg(kw))
        assert (res["solves"], res["rejected"], res["stop_reason"]) == (1, 1, "lambda_max") and pg.Poses().tobytes() == g.poses.tobytes()
    finally:
        pg.close()


def test_optimize_is_byte_identical_from_run_to_run(ctx):
    g, _ = cases.ring(false_loop=True)
    pg = _upload(ctx, g)
    try:
        runs = []
        for _ in range(5):
            pg.SetPoses(g.poses)
            res = pg.Optimize(_cfg(dict(cases.FALSE_CFG, max_iterations=3)))
            runs.append((pg.Poses().tobytes(), repr(res)))
        assert all(r == runs[0] for r in runs[1:])
    finally:
        pg.close()


# ---------------------------------------------------------------- misuse
def test_capacity_reset_and_misuse(ctx):
    g = cases.chain(6, 9)
    pg = _upload(ctx, g, node_capacity=8, edge_capacity=g.E + 1)
    with pytest.raises(ElmError, match=r"\(-5\).*capacity"):  # three more nodes would overfill: refused, nothing changes
        pg.AddNodes(g.poses[:3])
    with pytest.raises(ElmError, match=r"\(-5\).*capacity"):
        pg.AddEdges(g.i[:2], g.j[:2], g.Z[:2])
    assert pg.Size() == (6, g.E) and pg.Poses().tobytes() == g.poses.tobytes()
    first = pg.Optimize(_cfg(dict(max_iterations=2)))
    for bad in (lambda: pg.AddEdges([0], [0], g.Z[:1]), lambda: pg.AddEdges([0], [6], g.Z[:1]), lambda: pg.AddEdges([-1], [2], g.Z[:1]),
                lambda: pg.AddEdges([0], [1], g.Z[:1], np.triu(np.ones((6, 6)))), lambda: pg.AddEdges([0], [1], np.full((1, 4, 4), np.nan)),
                lambda: pg.SetPoses(g.poses, first=1), lambda: pg.Poses(5, 2), lambda: pg.SetFixed([1, 1], first=5),
                lambda: pg.Linearize(-1.0), lambda: pg.Solve(-1.0), lambda: pg.Optimize(_cfg(dict(lambda_up=0.5)))):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
        assert pg.Size() == (6, g.E)
    pg.AddEdges([5], [0], g.Z[:1])  # a correct call after them; the linearization is gone with the change
    with pytest.raises(ElmError, match=r"\(-1\)"):
        pg.Solve(0.0)
    with pytest.raises(ElmError, match=r"\(-1\)"):
        pg.Linearization()
    pg.Linearize()
    assert pg.Solve(1.0)[1]["converged"]
    pg.SetFixed([0] * 6)
    with pytest.raises(ElmError, match=r"\(-1\).*fixed"):  # no fixed node at all
        pg.Optimize()
    pg.Reset()
    assert pg.Size() == (0, 0)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    again = pg.Optimize(_cfg(dict(max_iterations=2)))
    assert repr(again) == repr(first)  # the same graph after a Reset: the same run
    other = Context(0)
    try:
        opg = PoseGraph(4, 4, other)
        with pytest.raises(ElmError, match=r"\(-1\)"):
            _size_through(other, pg)  # an object of another context
        assert opg.Size() == (0, 0) and pg.Size() == (6, g.E)
        opg.close()
    finally:
        other.close()
    # a batch in flight: every call that takes ctx is refused, and works again once the batch is finished
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(_scan_points(2000, 77))
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    sc = Scan(ctx, _scan_points(300, 78))
    reg.EnqueueBatch([sc], vm, [np.eye(4)])
    for bad in (lambda: pg.Size(), lambda: pg.Reset(), lambda: pg.AddNodes(g.poses[:1]), lambda: pg.SetPoses(g.poses[:1]), lambda: pg.Poses(),
                lambda: pg.SetFixed([1]), lambda: pg.AddEdges([0], [1], g.Z[:1]), lambda: pg.Linearize(), lambda: pg.Linearization(),
                lambda: pg.Solve(0.0), lambda: pg.Optimize(), lambda: PoseGraph(4, 4, ctx)):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
    reg.FinishBatch()
    assert pg.Size() == (6, g.E) and pg.Linearize()["cost"] == again["cost_final"]
    with pytest.raises(ElmError, match=r"\(-1\)"):
        PoseGraph(0, 4, ctx)
    with pytest.raises(ElmError, match=r"\(-1\)"):
        PoseGraph(4, (1 << 22) + 1, ctx)
    pg.close()
    with pytest.raises(ElmError, match="closed"):
        pg.Size()


def test_a_device_group_is_refused(ctx):
    grp = Context.multi([0, 0])
    try:
        with pytest.raises(ElmError, match=r"\(-5\).*one rank only"):
            PoseGraph(4, 4, grp)
    finally:
        grp.close()
    pg = PoseGraph(4, 4, ctx)  # a plain context next to it is served
    assert pg.Size() == (0, 0)
    pg.close()


def _size_through(ctx, pg):
    import ctypes as C
    from elimaloc_amd import _lib
    n, e = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().elm_posegraph_size(ctx._h, pg._h, C.byref(n), C.byref(e)), ctx._h, "elm_posegraph_size")


def _scan_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32))


# ---------------------------------------------------------------- LoopCloser
def test_loop_closer_close_and_map(ctx):
    g, truth = cases.ring()
    db = PlaceDatabase(PlaceConfig(), cases.RING_N, ctx)
    lc = LoopCloser(db)
    scans = [_scan_points(256, 500 + k) for k in range(cases.RING_N)]
    for k in range(cases.RING_N):
        lc.Insert(scans[k], g.poses[k])
    for a, b in cases.RING_LOOPS:
        lc.AddLoop(a, b, cases.inv_pose(truth[a]) @ truth[b])
    with pytest.raises(ElmError):
        lc.AddLoop(3, 3, np.eye(4))
    cfg = _cfg(cases.RING_CFG)
    poses, res = lc.Close(cfg)
    # by hand: the odometry edges of the inserted poses, then the loops
    P = g.poses
    pg = PoseGraph(cases.RING_N, cases.RING_N - 1 + len(cases.RING_LOOPS), ctx)
    pg.AddNodes(P, g.fixed)
    pg.AddEdges(np.arange(cases.RING_N - 1), np.arange(1, cases.RING_N), np.linalg.inv(P[:-1]) @ P[1:])
    pg.AddEdges([a for a, _ in cases.RING_LOOPS], [b for _, b in cases.RING_LOOPS],
                np.stack([cases.inv_pose(truth[a]) @ truth[b] for a, b in cases.RING_LOOPS]))
    want_res = pg.Optimize(cfg)
    want = pg.Poses()
    pg.close()
    assert poses.tobytes() == want.tobytes() and repr(res) == repr(want_res)
    assert np.stack(lc.poses).tobytes() == P.tobytes()  # apply=False leaves the closer's poses
    # the odometry edges are the drifted poses' own, so only the three loops pull and the chain shares their error out: the mirror's run
    # of the same graph
    i = list(range(cases.RING_N - 1)) + [a for a, _ in cases.RING_LOOPS]
    j = list(range(1, cases.RING_N)) + [b for _, b in cases.RING_LOOPS]
    Z = np.concatenate([np.linalg.inv(P[:-1]) @ P[1:], np.stack([cases.inv_pose(truth[a]) @ truth[b] for a, b in cases.RING_LOOPS])])
    m_poses, m_res = ref.optimize(ref.Graph(P, g.fixed, i, j, Z), **cases.RING_CFG)
    dt, dr = ref.pose_error(poses, m_poses)
    print(f"  Close against the mirror: {dt:.3e} m, {dr:.3e} rad; cost {res['cost_final']:.6e} (mirror {m_res['cost_final']:.6e})")
    assert dt <= 1e-4 and dr <= 1e-5 and math.isclose(res["cost_final"], m_res["cost_final"], rel_tol=1e-4)
    assert res["cost_final"] < 0.1 * res["cost_initial"]
    poses2, _ = lc.Close(cfg, apply=True)
    assert poses2.tobytes() == want.tobytes() and np.stack(lc.poses).tobytes() == want.tobytes()
    m = lc.Map()
    by_hand = VoxelHashMap(lc.voxel_size, lc.max_points_per_voxel, ctx, device_build=True).UpdatedFromScans(lc.scans, want)
    assert m.Pointcloud().tobytes() == by_hand.Pointcloud().tobytes() and len(m.Pointcloud()) > 0
    m0 = lc.Map(P)
    by_hand0 = VoxelHashMap(lc.voxel_size, lc.max_points_per_voxel, ctx, device_build=True).UpdatedFromScans(lc.scans, P)
    assert m0.Pointcloud().tobytes() == by_hand0.Pointcloud().tobytes() and m0.Pointcloud().tobytes() != m.Pointcloud().tobytes()
    db.close()
