"""Rotation residuals beyond 120 degrees on the GPU (the family, its 50-digit truth and its census are
tests/rotation_cases.py, the conditions on them tests/test_rotation_edges_abi.py): k_pg_linearize and k_pg_cost on graphs whose edges
take every branch of Log and both signs of the raw quaternion w, with the kinds mixed in every wavefront and with a wavefront of each
kind alone; k_lc_adjacency and k_lcv_adjacency on loop sets whose pairs do; the optimizer on false loops that claim a half turn about x
and about y.  Against the mirrors under the project's 1e-9 contract, and on the planted sets against the truth under the bounds of the
CPU test: rotation_cases.BOUNDS, 10 x the host library's measured error, not derived from the device.  Every device call runs twice and
gives the same bytes."""
import numpy as np
import pytest

import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref
import rotation_cases as rc
from elimaloc_amd.loops import LoopConsistency, LoopConsistencyConfig, LoopConsistencyCov
from elimaloc_amd.posegraph import PoseGraphConfig
from test_posegraph import _close, _upload

pytestmark = pytest.mark.gpu

PER_EDGE = ("r", "A", "B", "s", "w")
_LIN, _LOOPS = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the graphs
def _device(ctx, layout, order):
    """the device's linearization of one graph at huber 0 and at its k1, its stats, and the cost the optimizer reports at the start
    poses, each once per graph; every call is made twice and has to give the same bytes"""
    key = (layout, order)
    if key not in _LIN:
        g, _, _ = rc.graph(layout, order)
        pg = _upload(ctx, g)
        try:
            out = {}
            for k in (0.0, rc.huber_of(layout)):
                runs = []
                for _ in range(2):
                    st = pg.Linearize(k)
                    lin = pg.Linearization()
                    # one solve, so that Optimize evaluates the start poses with k_pg_cost; the poses are put back
                    res = pg.Optimize(PoseGraphConfig(huber_k=k, max_iterations=1, pcg_max_iterations=4))
                    pg.SetPoses(g.poses)
                    runs.append((lin, st, res["cost_initial"]))
                (lin, st, f0), (lin2, st2, f02) = runs
                assert all(lin[q].tobytes() == lin2[q].tobytes() for q in lin) and repr(st) == repr(st2) and f0 == f02, (key, k)
                out[k] = dict(lin=lin, stats=st, cost_initial=f0)
            assert pg.Poses().tobytes() == g.poses.tobytes()
            _LIN[key] = out
        finally:
            pg.close()
    return _LIN[key]


@pytest.mark.parametrize("layout,order", rc.GRAPH_SETS)
def test_linearize_against_the_mirror(ctx, layout, order):
    g, _, _ = rc.graph(layout, order)
    dev = _device(ctx, layout, order)
    for k in (0.0, rc.huber_of(layout)):
        want = ref.linearize(g, huber_k=k)
        got, st = dev[k]["lin"], dev[k]["stats"]
        assert all(np.isfinite(got[a]).all() for a in got)
        for a in PER_EDGE + ("grad", "diag"):
            _close(got[a], want[a], f"{layout} {order} huber {k:.4g} {a}")
        assert st["n_outliers"] == want["n_outliers"] and (k == 0.0 or 0 < want["n_outliers"] < g.E)


@pytest.mark.parametrize("order", rc.ORDERS)
def test_linearize_against_the_truth_on_the_planted_graph(ctx, order):
    """r, A, B, s and w of k_pg_linearize against 50 digits under the host library's bounds.  A near-pi ladder edge may come back as phi
    or as -phi, r and B alike; which ones do must be what the mirror does (on the development host: none)."""
    g, perm, _ = rc.graph("planted", order)
    c, truth = rc.canonical("planted"), rc.planted_truth()
    dev = _device(ctx, "planted", order)
    _, mirror_negated = rc.graph_errors(ref.linearize(g), truth, perm, c["either_sign"], k1=False)
    for k in (0.0, truth["huber_k1"]):
        errs, negated = rc.graph_errors(dev[k]["lin"], truth, perm, c["either_sign"], k1=k > 0.0)
        print(f"  planted {order} huber {k:.4g}: " + ", ".join(f"{q} {v:.2e} (bound {rc.BOUNDS[q]:.1e})" for q, v in errs.items()))
        assert np.array_equal(negated, mirror_negated)
        for q, v in errs.items():
            assert v <= rc.BOUNDS[q], (order, k, q, v)


@pytest.mark.parametrize("layout,order", rc.GRAPH_SETS)
def test_the_cost_kernel_against_the_truth_and_the_mirror(ctx, layout, order):
    """k_pg_cost, one lane per edge: the cost the optimizer reports at the start poses and Linearize's chi2 and cost, at both Huber
    settings, under the summation bound of the stats (1e-9 max(1, |sum|)); on the planted graphs the sums are the 50-digit ones"""
    g, _, _ = rc.graph(layout, order)
    dev = _device(ctx, layout, order)
    k1 = rc.huber_of(layout)
    if layout == "planted":
        sums = rc.truth_sums(rc.planted_truth())
        want = {0.0: (sums["s"], sums["s"]), k1: (sums["s"], sums["rho1"])}
    else:
        s = ref.edge_s(g, g.poses)
        want = {k: (float(s.sum()), float(ref.huber_cost(s, k).sum())) for k in (0.0, k1)}
    for k in (0.0, k1):
        st = dev[k]["stats"]
        _close([st["chi2"], st["cost"], dev[k]["cost_initial"]], [want[k][0], want[k][1], want[k][1]], f"{layout} {order} huber {k:.4g} chi2, cost, cost_initial")
    assert want[k1][1] < 0.9 * want[k1][0]  # Huber takes a tenth off the cost at least: the outliers carry weight in the sum


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_the_order_of_the_edges_does_not_change_an_edges_bytes(ctx, layout):
    """the same lane arithmetic in a wavefront that diverges over the kinds and in one that holds one kind: per edge the same bytes"""
    mixed, uniform = _device(ctx, layout, "round_robin"), _device(ctx, layout, "runs")
    _, perm, _ = rc.graph(layout, "round_robin")
    assert sorted(perm.tolist()) == list(range(len(perm))) and (perm[:rc.NK] == rc.RUN * np.arange(rc.NK)).all()
    for k in (0.0, rc.huber_of(layout)):
        for a in PER_EDGE:
            assert mixed[k]["lin"][a].tobytes() == np.ascontiguousarray(uniform[k]["lin"][a][perm]).tobytes(), (layout, k, a)
        for a in ("grad", "diag"):  # every node has one edge, and keeps it in both orders
            assert mixed[k]["lin"][a].tobytes() == uniform[k]["lin"][a].tobytes(), (layout, k, a)


# ---------------------------------------------------------------- the loop sets
LOOP_CASES = [(layout, size, order, cov) for cov in (False, True) for layout, size, order in rc.LOOP_SETS]
LOOP_IDS = [f"{layout}-{size}-{order}-{'covariance' if cov else 'scalar'}" for layout, size, order, cov in LOOP_CASES]


def _call(ctx, c, cov):
    if cov:
        return LoopConsistencyCov(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], c["Q"], LoopConsistencyConfig(gamma=c["gamma"]), ctx, adjacency=True, s=True)
    cfg = LoopConsistencyConfig(q_t=c["q_t"], q_r=c["q_r"], gamma=c["gamma"])
    return LoopConsistency(c["poses"], c["a"], c["b"], c["Z"], c["var_t"], c["var_r"], cfg, ctx, adjacency=True, s=True)


def _bytes(out):
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("members", "mask", "degree", "adjacency", "s")) + (
        out["size"], out["steps"], out["adjacent_pairs"], out.get("non_finite_pairs", 0))


def _loops(ctx, case):
    if case not in _LOOPS:
        layout, size, order, cov = case
        c = rc.loop_set(layout, size, order, cov)
        first, again = _call(ctx, c, cov), _call(ctx, c, cov)
        assert _bytes(first) == _bytes(again), case
        _LOOPS[case] = first
    return _LOOPS[case]


@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_pair_s_against_the_mirror(ctx, case):
    layout, size, order, cov = case
    c, out = rc.loop_set(layout, size, order, cov), _loops(ctx, case)
    s, want = out["s"], c["s"]
    assert s.shape == (size, size) and np.array_equal(s, s.T) and not np.diag(s).any()
    rel = np.abs(s - want) / np.maximum(1.0, np.abs(want))
    print(f"  {LOOP_IDS[LOOP_CASES.index(case)]}: worst |s - ref| / max(1, |ref|) {float(rel.max()):.3e} (bound 1e-9), largest s {float(want.max()):.3e}")
    assert np.isfinite(s).all() and (rel <= 1e-9).all() and out.get("non_finite_pairs", 0) == 0


@pytest.mark.parametrize("case", [c for c in LOOP_CASES if c[0] == "planted"], ids=[i for c, i in zip(LOOP_CASES, LOOP_IDS) if c[0] == "planted"])
def test_pair_s_against_the_truth_on_the_planted_loops(ctx, case):
    _, size, order, cov = case
    truth, out = rc.planted_loops_truth(size, order, cov), _loops(ctx, case)
    got = out["s"][truth["k"], truth["l"]]
    err = truth["s"].err(got) / np.maximum(1.0, truth["s"].hi)
    key = "pair_s_cov" if cov else "pair_s"
    kinds = rc.planted_loops(size, order, cov)["pair_kind"][truth["k"], truth["l"]]
    print(f"  planted {size} {order} {'covariance' if cov else 'scalar'}: worst |s - truth| / max(1, s) {float(err.max()):.2e} (bound {rc.BOUNDS[key]:.1e}); "
          f"per kind {[float(f'{err[kinds == q].max():.1e}') for q in range(rc.NK)]}")
    assert (err <= rc.BOUNDS[key]).all() and np.array_equal(out["s"][truth["l"], truth["k"]], got)


@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_adjacency_bit_for_bit_and_the_greedy_clique(ctx, case):
    layout, size, order, cov = case
    c, out = rc.loop_set(layout, size, order, cov), _loops(ctx, case)
    assert lcases.in_band(c["s"], c["gamma"]) == 0  # no pair is excused: the builder draws until the band is empty
    words = out["adjacency"]
    assert words.dtype == np.uint64 and words.shape == (size, (size + 63) // 64)
    bits = lref.unpack(words, size)
    assert not bits[:, size:].any()
    adj = bits[:, :size]
    assert np.array_equal(adj, adj.T) and not np.diag(adj).any()
    assert np.array_equal(adj, c["adj"]) and np.array_equal(words, lref.pack(c["adj"]))
    members, degree0 = lref.greedy(adj)
    assert out["members"].tolist() == sorted(members) and out["mask"].tolist() == [k in members for k in range(size)]
    assert out["size"] == out["steps"] == len(members) and out["adjacent_pairs"] == int(adj.sum()) // 2
    assert np.array_equal(out["degree"], degree0) and lref.is_clique(adj, out["members"]) and lref.is_maximal(adj, out["members"])


# ---------------------------------------------------------------- the optimizer
@pytest.mark.parametrize("axis", list(rc.HALF_TURNS))
def test_optimize_a_false_loop_that_claims_a_half_turn(ctx, axis):
    """as test_optimize_the_false_loop_with_huber of tests/test_posegraph.py, whose false edge is z-leads, against the mirror's run"""
    want = rc.half_turn_conditions(axis)
    g = want["g"]
    pg = _upload(ctx, g)
    try:
        runs = []
        for _ in range(2):
            pg.SetPoses(g.poses)
            res = pg.Optimize(PoseGraphConfig(**cases.FALSE_CFG))
            runs.append((pg.Poses(), res))
        (poses, res), (poses2, res2) = runs
        assert poses.tobytes() == poses2.tobytes() and repr(res) == repr(res2)
        assert [t["accepted"] for t in res["trace"]] == want["accepted"] and res["stop_reason"] == want["res"]["stop_reason"]
        dt, dr = ref.pose_error(poses, want["poses"])
        print(f"  half turn about {axis} against the mirror: {dt:.3e} m, {dr:.3e} rad")
        assert dt <= 1e-4 and dr <= 1e-5
        assert np.allclose([t["cost"] for t in res["trace"]], [t["cost"] for t in want["res"]["trace"]], rtol=1e-6)
        assert np.isclose(res["cost_initial"], want["res"]["cost_initial"], rtol=1e-9, atol=0.0)
        lin = pg.Linearize(cases.FALSE_CFG["huber_k"])
        assert lin["n_outliers"] == 1 and pg.Linearization()["w"][-1] < 0.1
    finally:
        pg.close()
