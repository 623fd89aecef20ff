"""The pose graph's priors on the GPU (elm_posegraph_*prior*; include/elimaloc_hip_posegraph_prior.h): the
linearization with priors, the conjugate-gradient step and Levenberg-Marquardt against the numpy mirror (tests/posegraph_prior_ref.py on
top of tests/posegraph_ref.py) under the project's 1e-9 sums contract; the two anchored-ring fixtures against their committed recording
and the truth; a graph without priors against an object that never had any, in bytes; the covariances; misuse; and LoopCloser.Close with
priors against the hand composition of the public calls.  Every device call whose bytes are promised is made twice and compared."""
import math

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_ref as cref
import posegraph_cov_ref as cov
import posegraph_prior_cases as pcases
import posegraph_prior_ref as pref
import posegraph_ref as ref
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig, PoseGraphCovConfig
from elimaloc_amd.registration import Context

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _upload(ctx, g, P=None, prior_capacity=None):
    """the graph, and the priors when given (prior_capacity: room for more than them)"""
    cap = prior_capacity if prior_capacity is not None else (P.P if P is not None else 0)
    pg = PoseGraph(max(g.N, 1), max(g.E, 1), ctx, prior_capacity=cap)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    if P is not None and P.P:
        pg.AddPriors(P.node, P.Z, P.info, P.lever)
    return pg


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(np.asarray(got) - want).max()) if want.size else 0.0
    bound = 1e-9 * max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    print(f"  {what}: |gpu - ref| {err:.3e} (bound {bound:.1e})")
    assert np.asarray(got).shape == want.shape and err <= bound, what


def _bytes(d):
    return {k: np.asarray(v).tobytes() for k, v in d.items()}


def _cfg(d):
    return PoseGraphConfig(**d)


# ---------------------------------------------------------------- linearize
# P = 31, 32, 33: the workgroup edge of the lane groups (32 priors per workgroup); 255, 256, 257, 513: the cost kernel's (256 lanes)
LIN_CASES = {
    "P1_N1_E0": pcases.one_node,
    "P31": lambda: pcases.counted(31, 101),
    "P32": lambda: pcases.counted(32, 102),
    "P33": lambda: pcases.counted(33, 103),
    "P255": lambda: pcases.counted(255, 104),
    "P256": lambda: pcases.counted(256, 105),
    "P257": lambda: pcases.counted(257, 106),
    "P513": lambda: pcases.counted(513, 107),
    "node_counts_1_2_64_65_70": pcases.node_counts,
    "node_without_edges": pcases.node_without_edges,
    "fixed_node": pcases.fixed_node,
    "duplicates": pcases.duplicates,
    "star65_hub": pcases.star_hub,
    "poses_at_1e5_m": pcases.far_away,
    "rotation_family": pcases.rotation_family,
    "position_only": lambda: (lambda g: (g, pcases.rand_priors(g, 40, 109, kind="position")))(cases.random_graph(40, 65, 108)),
    "full_information": lambda: (lambda g: (g, pcases.rand_priors(g, 40, 111, kind="pose")))(cases.random_graph(40, 65, 110)),
}


@pytest.mark.parametrize("name", list(LIN_CASES))
def test_linearize_with_priors_against_the_mirror(ctx, name):
    g, P = LIN_CASES[name]()
    pg = _upload(ctx, g, P)
    try:
        assert pg.Size() == (g.N, g.E) and pg.PriorCount() == P.P
        back = pg.Priors()
        assert np.array_equal(back["node"], P.node) and back["Z"].tobytes() == P.Z.tobytes() and back["lever"].tobytes() == P.lever.tobytes()
        assert back["information"].tobytes() == P.info.tobytes()
        for k, pk in ((0.0, 0.0), (0.3, 0.5)):  # (thresholds that leave inliers and outliers in every random case)
            want = pref.linearize(g, P, huber_k=k, prior_huber_k=pk)
            pg.SetPriorHuber(pk)
            st = pg.Linearize(k)
            got, gotp = pg.Linearization(), pg.PriorLinearization()
            for a, b in (("r", "pr"), ("J", "pJ"), ("s", "ps"), ("w", "pw")):
                _close(gotp[a], want[b], f"{name} huber {k}/{pk} prior {a}")
            for a in ("r", "A", "B", "s", "w", "grad", "diag"):
                _close(got[a], want[a], f"{name} huber {k}/{pk} {a}")
            _close([st["chi2"], st["cost"], st["grad_inf_norm"]], [want["chi2"], want["cost"], want["grad_inf_norm"]], "stats")
            assert st["n_outliers"] == want["n_outliers"]
            st2 = pg.Linearize(k)  # the same call again: the same bytes
            assert st2 == st and _bytes(pg.Linearization()) == _bytes(got) and _bytes(pg.PriorLinearization()) == _bytes(gotp)
        if name == "rotation_family":
            assert np.abs(np.linalg.norm(want["pr"][:, 3:], axis=1) - np.array(cases.ROT_FAMILY)).max() <= 1e-8  # up to pi - 1e-6
    finally:
        pg.close()


def test_linearize_hand_case_in_bytes(ctx):
    g, P, want_r, want_s = pcases.hand_integers()
    pg = _upload(ctx, g, P)
    try:
        st = pg.Linearize(0.0)
        L, D = pg.PriorLinearization(), pg.Linearization()
        assert L["r"].tobytes() == want_r.tobytes()  # Log(I) == +0
        assert L["s"].tobytes() == want_s.tobytes() and L["w"].tolist() == [1.0] * 3
        for q in range(3):
            want_J = np.eye(6)
            want_J[:3, 3:] = -ref.hat(P.lever[q])
            assert (L["J"][q] == want_J).all()
            assert (D["diag"][q] == want_J.T @ P.info[q] @ want_J).all() and (D["grad"][q] == want_J.T @ P.info[q] @ want_r[q]).all()
        assert (st["chi2"], st["cost"], st["n_outliers"]) == (23.0, 23.0, 0)
        pg.SetPriorHuber(3.0)  # s = 13 and 10 are above k^2 = 9
        st = pg.Linearize(0.0)
        w = pg.PriorLinearization()["w"]
        assert w.tolist() == [3.0 / math.sqrt(13.0), 1.0, 3.0 / math.sqrt(10.0)] and st["n_outliers"] == 2
        # the threshold is closed: s == k^2 is an inlier (the case of test_posegraph_prior_abi.test_prior_huber_threshold_is_closed)
        P2 = P.take([0, 2])
        P2.info[0] = np.diag([4.0, 2.0, 3.0, 1.0, 1.0, 1.0])  # s = 4 + 12 = 16
        pg.ClearPriors()
        pg.AddPriors(P2.node, P2.Z, P2.info, P2.lever)
        pg.SetPriorHuber(4.0)
        st = pg.Linearize(0.0)
        L = pg.PriorLinearization()
        assert L["s"].tolist() == [16.0, 10.0] and L["w"].tolist() == [1.0, 1.0] and (st["n_outliers"], st["cost"]) == (0, 26.0)
        below = float(np.nextafter(4.0, 0.0))
        pg.SetPriorHuber(below)
        st = pg.Linearize(0.0)
        w = pg.PriorLinearization()["w"]
        assert w[0] == below / 4.0 and w[0] < 1.0 and w[1] == 1.0 and st["n_outliers"] == 1
        assert st["cost"] == ((2.0 * below) * 4.0 - below * below) + 10.0
    finally:
        pg.close()


# ---------------------------------------------------------------- no prior is the parent
def _ring_graph():
    return cases.ring()[0]


PARENT_CASES = {"N2_E1": lambda: cases.random_graph(2, 1, 11), "E65": lambda: cases.random_graph(40, 65, 14), "hub300": lambda: cases.star(300, 25),
                "ring": _ring_graph}


@pytest.mark.parametrize("name", list(PARENT_CASES))
def test_without_priors_every_result_is_the_parents(ctx, name):
    """an object on which ReservePriors was never called against one with a reserve, priors added and then cleared"""
    g = PARENT_CASES[name]()
    P = pcases.rand_priors(g, 5, 120)
    cfg = _cfg(dict(cases.RING_CFG, max_iterations=3, huber_k=0.5))
    runs = []
    for with_reserve in (False, True):
        pg = _upload(ctx, g, P if with_reserve else None, prior_capacity=8 if with_reserve else 0)
        try:
            if with_reserve:
                pg.SetPriorHuber(0.7)
                pg.Linearize(0.5)  # the priors have been through every kernel before they go
                pg.ClearPriors()
                assert pg.PriorCount() == 0
            st = pg.Linearize(0.5)
            lin = _bytes(pg.Linearization())
            delta, sst = pg.Solve(1e-3, 1e-10, 300)
            res = pg.Optimize(cfg)
            runs.append((repr(st), lin, delta.tobytes(), repr(sst), repr(res), pg.Poses().tobytes()))
        finally:
            pg.close()
    assert runs[0] == runs[1]


# ---------------------------------------------------------------- solve
SOLVE_CASES = {  # name: (graph and priors, preconditioner, the dampings)
    "priors_only": (pcases.priors_only, "block_jacobi", (1.0,)),
    "fixed_and_priors": (pcases.fixed_and_priors, "block_jacobi", (0.0,)),
    "chain12_with_priors_chain": (pcases.fixed_and_priors, "chain", (0.0, 1.0)),
}


def _mirror_pcg(g, lin, lam, tol, max_it, precond):
    if precond == "chain":
        return cref.pcg_chain(g, lin, lam, tol, max_it)
    return ref.pcg(g, lin, lam, tol, max_it)


def _true_residual(g, lin, lam, delta, precond):
    return pref.true_rel_residual(g, lin, lam, delta, solve=cref.chain_solver(g, lin, lam, sparse=False) if precond == "chain" else None)


@pytest.mark.parametrize("name", list(SOLVE_CASES))
def test_five_iterations_with_priors_against_the_mirror(ctx, name):
    make, precond, lams = SOLVE_CASES[name]
    g, P = make()
    pg = _upload(ctx, g, P)
    try:
        pg.SetPreconditioner(precond)
        pg.SetPriorHuber(1.0)
        lin = pref.linearize(g, P, huber_k=1.5, prior_huber_k=1.0)
        pg.Linearize(1.5)
        for lam in lams:
            want, its, _, conv = _mirror_pcg(g, lin, lam, 0.0, 5, precond)
            delta, st = pg.Solve(lam, 0.0, 5)
            assert (its, conv) == (5, False) and st["iterations"] == 5 and not st["converged"]
            _close(delta, want, f"{name} lambda {lam} delta after 5 iterations")
            assert (delta[~lin["active"]] == 0.0).all() and (delta[g.fixed] == 0.0).all()
            again, st2 = pg.Solve(lam, 0.0, 5)
            assert again.tobytes() == delta.tobytes() and st2 == st
    finally:
        pg.close()


@pytest.mark.parametrize("name", list(SOLVE_CASES))
def test_solve_to_tolerance_with_priors_true_residual(ctx, name):
    tol = 1e-10
    make, precond, lams = SOLVE_CASES[name]
    g, P = make()
    pg = _upload(ctx, g, P)
    try:
        pg.SetPreconditioner(precond)
        pg.SetPriorHuber(1.0)
        lin = pref.linearize(g, P, huber_k=1.5, prior_huber_k=1.0)
        pg.Linearize(1.5)
        for lam in lams:
            d_ref, its_ref, _, conv_ref = _mirror_pcg(g, lin, lam, tol, 500, precond)
            rho_ref = _true_residual(g, lin, lam, d_ref, precond)  # measured on the CPU first
            delta, st = pg.Solve(lam, tol, 500)
            rho = _true_residual(g, lin, lam, delta, precond)
            print(f"  {name} lambda {lam}: gpu {st['iterations']} iterations (mirror {its_ref}), true relative residual {rho:.2e} (mirror {rho_ref:.2e})")
            assert conv_ref and st["converged"] and st["rel_residual"] <= tol
            assert rho <= 10.0 * max(tol, rho_ref)
            assert (delta[g.fixed] == 0.0).all()
    finally:
        pg.close()


# ---------------------------------------------------------------- optimize
def test_optimize_the_anchored_ring(ctx):
    gold = np.load(pcases.GOLDEN)
    g, P, truth = pcases.anchored_ring()
    pg = _upload(ctx, g, P)
    try:
        assert not g.fixed.any()  # no node is fixed: the priors alone tie the graph to the world
        res = pg.Optimize(_cfg(pcases.ANCHOR_CFG))
        poses = pg.Poses()
        assert [t["accepted"] for t in res["trace"]] == gold["anchor_accepted"].astype(bool).tolist()
        assert res["stop_reason"] == str(gold["anchor_stop"]) and res["solves"] == len(gold["anchor_cost"]) == res["accepted"] and res["rejected"] == 0
        for name, want in (("the fixture", gold["anchor_poses"]), ("the truth", truth)):
            dt, dr = ref.pose_error(poses, want)
            print(f"  anchored ring against {name}: {dt:.3e} m, {dr:.3e} rad")
            assert dt <= 1e-4 and dr <= 1e-5
        assert res["cost_final"] <= res["cost_initial"] and math.isclose(res["cost_initial"], float(gold["anchor_cost_initial"]), rel_tol=1e-9)
        pg.ClearPriors()
        with pytest.raises(ElmError, match=r"\(-1\).*no fixed node"):  # the same graph without its priors: the gauge is free
            pg.Optimize(_cfg(pcases.ANCHOR_CFG))
        assert pg.Poses().tobytes() == poses.tobytes()
    finally:
        pg.close()


def test_optimize_the_outlier_with_the_priors_huber(ctx):
    gold = np.load(pcases.GOLDEN)
    g, P, _ = pcases.anchored_ring(outlier=True)
    pg = _upload(ctx, g, P)
    try:
        pg.SetPriorHuber(pcases.OUTLIER_PRIOR_HUBER)
        res = pg.Optimize(_cfg(pcases.OUTLIER_CFG))
        assert [t["accepted"] for t in res["trace"]] == gold["outlier_accepted"].astype(bool).tolist() and res["stop_reason"] == str(gold["outlier_stop"])
        dt, dr = ref.pose_error(pg.Poses(), gold["outlier_poses"])
        print(f"  outlier against the recording: {dt:.3e} m, {dr:.3e} rad")
        assert dt <= 1e-4 and dr <= 1e-5
        assert np.allclose([t["cost"] for t in res["trace"]], gold["outlier_cost"], rtol=1e-6)
        assert pg.Linearize(pcases.OUTLIER_CFG["huber_k"])["n_outliers"] == 1
        w = pg.PriorLinearization()["w"]
        assert int(np.argmin(w)) == pcases.OUTLIER_AT and w[pcases.OUTLIER_AT] < 0.1 and (np.delete(w, pcases.OUTLIER_AT) == 1.0).all()
    finally:
        pg.close()


def _wild_with_priors():
    """posegraph_cases.wild_chain() (a start so far off that the mirror rejects the plain Gauss-Newton step) with position priors on
    nodes 6 and 11 where the chain lay before it was disturbed: F_new / F = 2.30 at lambda 1e-9, 2.27 at 1e-5, then accepted steps at
    0.17 and 0.53"""
    g = cases.wild_chain()
    calm = cases.chain(12, 4, info_random=False)
    return g, pcases.rand_priors(ref.Graph(calm.poses, g.fixed, g.i, g.j, g.Z, g.info), 2, 130, kind="position", nodes=[6, 11])


def test_optimize_forced_rejection_with_priors(ctx):
    """lambda_init tiny and a start that overshoots: rejections first, so the completed H_vv has to survive the read-back entry of the
    node kernel (launch_damping with sum = 0) for the later solves to be the mirror's"""
    g, P = _wild_with_priors()
    pg = _upload(ctx, g, P)
    try:
        kw = dict(lambda_init=1e-9, lambda_up=1e4, max_iterations=4, pcg_rel_tol=1e-10, pcg_max_iterations=500)
        want_poses, want = pref.optimize(g, P, **kw)
        res = pg.Optimize(_cfg(kw))
        print("  mirror:", [(t["accepted"], round(t["ratio"], 4)) for t in want["trace"]])
        assert [t["accepted"] for t in want["trace"]] == [False, False, True, True]
        assert all(abs(t["ratio"] - 1.0) > 0.01 for t in want["trace"])  # no decision hangs on a last digit
        assert [t["accepted"] for t in want["trace"]] == [t["accepted"] for t in res["trace"]]
        assert np.allclose([t["lambda_"] for t in res["trace"]], [t["lambda_"] for t in want["trace"]], rtol=1e-12)
        assert np.allclose([t["cost"] for t in res["trace"]], [t["cost"] for t in want["trace"]], rtol=1e-6)
        assert max(ref.pose_error(pg.Poses(), want_poses)) <= 1e-6 and res["cost_final"] < res["cost_initial"]
    finally:
        pg.close()


def test_optimize_with_priors_is_byte_identical_from_run_to_run(ctx):
    g, P, _ = pcases.anchored_ring(outlier=True)
    pg = _upload(ctx, g, P)
    try:
        pg.SetPriorHuber(pcases.OUTLIER_PRIOR_HUBER)
        runs = []
        for _ in range(3):
            pg.SetPoses(g.poses)
            res = pg.Optimize(_cfg(dict(pcases.OUTLIER_CFG, max_iterations=3)))
            runs.append((pg.Poses().tobytes(), repr(res)))
        assert all(r == runs[0] for r in runs[1:])
    finally:
        pg.close()


# ---------------------------------------------------------------- covariances
def test_marginal_of_one_node_under_one_prior(ctx):
    g, P = pcases.one_node()
    pg = _upload(ctx, g, P)
    try:
        pg.Linearize(0.0)
        J = pg.PriorLinearization()["J"][0]
        want = np.linalg.inv(J.T @ P.info[0] @ J)
        got = pg.Marginals([0])  # lambda = 0 without a fixed node: the prior fixes the gauge
        _close(got[0], 0.5 * (want + want.T), "Sigma of one node against (J^T Omega J)^-1")
        assert pg.Marginals([0]).tobytes() == got.tobytes()
    finally:
        pg.close()


def test_marginals_of_the_anchored_ring_at_its_optimum(ctx):
    gold = np.load(pcases.GOLDEN)
    g, P, _ = pcases.anchored_ring()
    g.poses = gold["anchor_poses"]
    nodes = np.array([0, 5, 32, 63])
    lin = pref.linearize(g, P)
    dense = pref.cov_dense(g, lin, 0.0)
    want = cov.dense_blocks(dense, nodes, nodes)[np.arange(4), np.arange(4)]
    b = cov.bound(dense, nodes).reshape(4, 6)
    pg = _upload(ctx, g, P)
    try:
        pg.Linearize(0.0)
        got, info = pg.Marginals(nodes, PoseGraphCovConfig(lambda_=0.0), return_stats=True)
        both = 0.5 * (b[:, :, None] + b[:, None, :])  # the diagonal block is symmetrised: entry (a, b) mixes the columns a and b
        ratio = float((np.abs(got - 0.5 * (want + np.swapaxes(want, 1, 2))) / both).max())
        print(f"  anchored ring marginals: |gpu - dense| / bound {ratio:.3e} (bound {b.min():.2e} .. {b.max():.2e}), iterations up to {info['iterations_max']}")
        assert info["converged"].all() and ratio <= 2.0
        pg.ClearPriors()
        pg.Linearize(0.0)
        with pytest.raises(ElmError, match=r"\(-1\).*no fixed node"):
            pg.Marginals(nodes)
    finally:
        pg.close()


# ---------------------------------------------------------------- misuse
def test_prior_capacity_reset_and_misuse(ctx):
    g, P = pcases.fixed_and_priors()
    pg = _upload(ctx, g)
    with pytest.raises(ElmError, match=r"\(-5\).*reserve"):  # no reserve: refused, nothing changes
        pg.AddPriors(P.node, P.Z, P.info, P.lever)
    assert pg.PriorCount() == 0 and pg.PriorHuber() == 0.0
    pg.Linearize()
    assert pg.PriorLinearization()["r"].shape == (0, 6)
    pg.ReservePriors(P.P + 1)
    with pytest.raises(ElmError, match=r"\(-1\).*once per object"):
        pg.ReservePriors(4)
    pg.AddPriors(P.node, P.Z, P.info, P.lever)
    with pytest.raises(ElmError, match=r"\(-1\)"):  # the priors invalidate the linearization
        pg.Solve(0.0)
    with pytest.raises(ElmError, match=r"\(-1\)"):
        pg.PriorLinearization()
    with pytest.raises(ElmError, match=r"\(-5\).*capacity"):  # two more would overfill
        pg.AddPriors(P.node[:2], P.Z[:2], P.info[:2], P.lever[:2])
    for bad in (lambda: pg.AddPriors([g.N], P.Z[:1]), lambda: pg.AddPriors([-1], P.Z[:1]), lambda: pg.AddPriors([0], P.Z[:1], np.triu(np.ones((6, 6)))),
                lambda: pg.AddPriors([0], np.full((1, 4, 4), np.nan)), lambda: pg.AddPriors([0], P.Z[:1], None, [0.0, np.inf, 0.0]),
                lambda: pg.SetPriorHuber(-1.0), lambda: pg.SetPriorHuber(float("nan"))):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
        assert pg.PriorCount() == P.P
    first = pg.Linearize()
    pg.SetPriorHuber(0.5)
    with pytest.raises(ElmError, match=r"\(-1\)"):  # so does the threshold
        pg.Solve(0.0)
    assert pg.Linearize()["cost"] == first["cost"]  # (every s_q of this case is below 0.06)
    pg.SetPriorHuber(0.125)
    assert pg.Linearize()["cost"] < first["cost"] and pg.PriorHuber() == 0.125
    pg.SetPriorHuber(0.5)
    pg.ClearPriors()
    with pytest.raises(ElmError, match=r"\(-1\)"):  # and clearing them
        pg.Linearization()
    pg.AddPriors(P.node, P.Z, P.info, P.lever)
    pg.SetPreconditioner("chain")
    pg.Reset()  # clears the priors with the nodes; the capacity and the threshold stay, as the preconditioner kind does
    assert pg.Size() == (0, 0) and pg.PriorCount() == 0 and pg.PriorHuber() == 0.5 and pg.Preconditioner() == "chain"
    with pytest.raises(ElmError, match=r"\(-1\).*once per object"):
        pg.ReservePriors(4)
    with pytest.raises(ElmError, match=r"\(-1\)"):  # no node yet
        pg.AddPriors(P.node[:1], P.Z[:1])
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    pg.AddPriors(P.node, P.Z, P.info, P.lever)
    pg.AddPriors(P.node[:1], P.Z[:1], P.info[:1], P.lever[:1])  # the capacity is still P + 1
    assert pg.PriorCount() == P.P + 1
    pg.close()
    with pytest.raises(ElmError, match="closed"):
        pg.PriorCount()


def test_a_device_group_is_refused_priors(ctx):
    grp = Context.multi([0, 0])
    try:
        with pytest.raises(ElmError, match=r"\(-5\).*one rank only"):
            PoseGraph(4, 4, grp, prior_capacity=4)
        pg = PoseGraph(4, 4, ctx)  # an object of a plain context through the group's lead
        try:
            import ctypes as C
            from elimaloc_amd import _lib
            with pytest.raises(ElmError, match=r"\(-5\).*one rank only"):
                _lib.check(_lib.lib().elm_posegraph_reserve_priors(grp._h, pg._h, 4), grp._h, "elm_posegraph_reserve_priors")
            n = C.c_size_t(0)
            with pytest.raises(ElmError, match=r"\(-5\).*one rank only"):
                _lib.check(_lib.lib().elm_posegraph_prior_count(grp._h, pg._h, C.byref(n)), grp._h, "elm_posegraph_prior_count")
            pg.ReservePriors(4)  # the plain context next to it is served
            assert pg.PriorCount() == 0
        finally:
            pg.close()
    finally:
        grp.close()


# ---------------------------------------------------------------- LoopCloser
def _scan_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32))


def test_loop_closer_close_with_priors(ctx):
    g, P, truth = pcases.anchored_ring()
    n = cases.RING_N
    db = PlaceDatabase(PlaceConfig(), n, ctx)
    lc = LoopCloser(db)
    for k in range(n):
        lc.Insert(_scan_points(64, 700 + k), g.poses[k])
    cfg = _cfg(pcases.ANCHOR_CFG)
    with pytest.raises(ElmError, match=r"\(-1\).*no fixed node"):  # no prior yet: fixed=() is refused as ever
        lc.Close(cfg, fixed=())
    base, base_res = lc.Close(cfg)  # the default call, before any prior
    lever = np.array(pcases.ANCHOR_LEVER)
    for q in range(1, P.P):
        lc.AddPositionPrior(int(P.node[q]), P.Z[q, :3, 3], pcases.ANCHOR_INFO, lever)
    pose_info = np.diag([4.0, 4.0, 1.0, 25.0, 25.0, 25.0])
    lc.AddPosePrior(0, truth[0], pose_info)
    with pytest.raises(ElmError, match="no such entry"):
        lc.AddPositionPrior(n, np.zeros(3))
    poses, res = lc.Close(cfg, fixed=(), prior_huber_k=2.0)
    # by hand: the odometry edges of the inserted poses, then the priors in the order they were given
    Pz = g.poses
    pg = PoseGraph(n, n - 1 + 1, ctx, prior_capacity=P.P)
    try:
        pg.AddNodes(Pz, np.zeros(n, bool))
        pg.AddEdges(np.arange(n - 1), np.arange(1, n), np.linalg.inv(Pz[:-1]) @ Pz[1:])
        pg.SetPriorHuber(2.0)
        pg.AddPositionPriors(P.node[1:], P.Z[1:, :3, 3], pcases.ANCHOR_INFO, lever)
        pg.AddPriors([0], truth[:1], pose_info)
        want_res = pg.Optimize(cfg)
        want = pg.Poses()
    finally:
        pg.close()
    assert poses.tobytes() == want.tobytes() and repr(res) == repr(want_res)
    # the odometry edges are the drifted poses' own, so only the priors pull: the end lies nearer the truth than the start, not on it
    assert res["cost_final"] < 0.1 * res["cost_initial"] and ref.pose_error(poses, truth)[0] < 0.5 * ref.pose_error(Pz, truth)[0]
    # without priors the default call is the parent's: the hand composition of test_posegraph.test_loop_closer_close_and_map
    fx = np.zeros(n, bool)
    fx[0] = True
    pg = PoseGraph(n, n - 1 + 1, ctx)
    try:
        pg.AddNodes(Pz, fx)
        pg.AddEdges(np.arange(n - 1), np.arange(1, n), np.linalg.inv(Pz[:-1]) @ Pz[1:])
        want_res = pg.Optimize(cfg)
        want = pg.Poses()
    finally:
        pg.close()
    assert base.tobytes() == want.tobytes() and repr(base_res) == repr(want_res)
    db.close()
