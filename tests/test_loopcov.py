"""The loop consistency check with a propagated covariance on the GPU (include/elimaloc_hip_loopcov.h) against its
mirror (tests/loopcov_ref.py): W and S at the prefix sum's edges under ten times the float64 mirrors' own error, s under
max(1e-9, 10 delta_s), adj bit for bit outside an (empty) band around gamma, the greedy clique exactly the mirror's on the device's own
adjacency; the planted fixture with the honest noise, which the scalar call at the same noise does not solve; an indefinite and a zero Q;
the batch size, the run-to-run bytes, the preconditions, LoopCloser with and without odom_covariance, and the C++ harness."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loopcov_cases as ccases
import loopcov_ref as cref
import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
from elimaloc_amd import _lib
from elimaloc_amd._lib import ElmError
from elimaloc_amd.loops import ChainCovariance, LoopConsistency, LoopConsistencyConfig, LoopConsistencyCov
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [str(L) for L in ccases.SIZES] + ["planted"]
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


def _case(name):
    """the inputs and the mirror's s and adjacency, computed once per case and left unchanged"""
    return ccases.planted_honest() if name == "planted" else ccases.random_case(int(name))


def _call(ctx, c, gamma=None, adjacency=True, s=False, Q=None, **kw):
    cfg = LoopConsistencyConfig(gamma=c["gamma"] if gamma is None else gamma, **kw)
    return LoopConsistencyCov(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], c["Q"] if Q is None else Q, cfg, ctx, adjacency=adjacency, s=s)


def _run(ctx, name):
    """the device's answer with both optional outputs, once per case"""
    if name not in _RUNS:
        _RUNS[name] = _call(ctx, _case(name), s=True)
    return _RUNS[name]


def _bytes(out):
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("members", "mask", "degree", "adjacency", "s") if k in out) + (
        out["size"], out["steps"], out["adjacent_pairs"], out["non_finite_pairs"])


# ---------------------------------------------------------------- the chain covariance
@pytest.mark.parametrize("name", ccases.CHAIN_NAMES)
def test_w_and_s_of_the_chain_against_the_mirror(ctx, name):
    c = ccases.chain_case(name)
    n = c["n"]
    W, S = ChainCovariance(c["poses"], c["Q"], ctx, local=True)  # (one pose with a Q per step: q_count = 0 and no Q at all)
    only = ChainCovariance(c["poses"], c["Q"], ctx)
    assert W.shape == S.shape == (n, 6, 6) and W.tobytes() == only.tobytes()
    assert np.array_equal(W, W.transpose(0, 2, 1)) and np.array_equal(S, S.transpose(0, 2, 1)) and not W[0].any() and not S[0].any()
    err_W, err_S = float(ccases.node_error(W, c["W"]).max()), float(ccases.node_error(S, c["S"]).max())
    print(f"  chain {name}: |W - W_ld| / max(1, |W_ld|) {err_W:.3e} (bound {10 * c['delta_W']:.3e}), S {err_S:.3e} (bound {10 * c['delta_S']:.3e}), "
          f"largest |W| {float(np.abs(c['W']).max()):.3e}")
    assert np.isfinite(W).all() and np.isfinite(S).all()
    assert err_W <= 10.0 * c["delta_W"] and err_S <= 10.0 * c["delta_S"]


def test_the_chain_twice_gives_the_same_bytes_and_its_preconditions(ctx):
    c = ccases.chain_case("3073-each")
    first, again = ChainCovariance(c["poses"], c["Q"], ctx, local=True), ChainCovariance(c["poses"], c["Q"], ctx, local=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    asym = c["Q"].copy()
    asym[1000, 2, 4] += 1e-12
    bad_pose = c["poses"].copy()
    bad_pose[17, 0, 3] = np.nan
    for poses, Q, text in ((c["poses"], asym, "Q 1000: not symmetric"), (c["poses"], c["Q"][:-1], "q_count"), (bad_pose, c["Q"], "non-finite pose"),
                           (c["poses"], np.where(np.arange(3072)[:, None, None] == 5, np.inf, c["Q"]), "Q 5: non-finite")):
        with pytest.raises(ElmError, match=r"\(-1\).*elm_loopcov_chain: .*" + text):
            ChainCovariance(poses, Q, ctx)
        assert ChainCovariance(c["poses"], c["Q"], ctx).tobytes() == first[0].tobytes(), text


# ---------------------------------------------------------------- the pair terms
@pytest.mark.parametrize("name", CASES)
def test_s_against_the_mirror(ctx, name):
    c, out = _case(name), _run(ctx, name)
    s, want = out["s"], c["s"]
    L = len(c["a"])
    assert s.shape == (L, L) and np.array_equal(s, s.T) and not np.diag(s).any()
    rel = np.abs(s - want) / np.maximum(1.0, np.abs(want))
    print(f"  {name}: worst |s - ref| / max(1, |ref|) {float(rel.max()) if L else 0.0:.3e} (bound {c['bound']:.1e}, delta_s {c['delta']:.2e}), "
          f"largest s {float(want.max()) if L else 0.0:.3e}")
    assert np.isfinite(s).all() and (rel <= c["bound"]).all() and out["non_finite_pairs"] == 0


@pytest.mark.parametrize("name", CASES)
def test_adjacency_bit_for_bit(ctx, name):
    c, out = _case(name), _run(ctx, name)
    L = len(c["a"])
    assert ccases.in_band(c["s"], c["gamma"], c["bound"]) == 0  # no pair is excused: the cap on excluded pairs is zero
    words = out["adjacency"]
    assert words.dtype == np.uint64 and words.shape == (L, (L + 63) // 64)
    bits = lref.unpack(words, L)
    assert not bits[:, L:].any()  # the padding bits
    adj = bits[:, :L]
    assert np.array_equal(adj, adj.T) and not np.diag(adj).any()
    assert np.array_equal(adj, c["adj"]) and np.array_equal(words, lref.pack(c["adj"]))


@pytest.mark.parametrize("name", CASES)
def test_greedy_is_the_mirrors_on_the_devices_adjacency(ctx, name):
    c, out = _case(name), _run(ctx, name)
    L = len(c["a"])
    adj = lref.unpack(out["adjacency"], L)[:, :L]
    members, degree0 = lref.greedy(adj)
    print(f"  {name}: clique of {out['size']} among {L} loops, {out['adjacent_pairs']} adjacent pairs; chain {out['chain_ms']:.3f} ms, "
          f"pairs {out['adjacency_ms']:.3f} ms, greedy {out['greedy_ms']:.3f} ms")
    assert out["members"].tolist() == sorted(members) and out["mask"].tolist() == [k in members for k in range(L)]
    assert out["size"] == out["steps"] == len(members) and out["adjacent_pairs"] == int(adj.sum()) // 2
    assert out["degree"].dtype == np.int32 and np.array_equal(out["degree"], degree0)
    assert lref.is_clique(adj, out["members"]) and lref.is_maximal(adj, out["members"])


# ---------------------------------------------------------------- the planted fixture with the honest noise
def test_the_planted_members_are_the_true_loops_and_the_scalar_call_misses_them(ctx):
    p, out = ccases.planted_honest(), _run(ctx, "planted")
    want = np.flatnonzero(p["is_true"]).tolist()
    assert out["members"].tolist() == want and out["size"] == 8
    scalar = LoopConsistency(p["poses"], p["a"], p["b"], p["Z"], lcases.PLANTED_VAR_T, lcases.PLANTED_VAR_R,
                             LoopConsistencyConfig(gamma=p["gamma"], **ccases.HONEST_SCALAR), ctx)
    print(f"  planted, honest noise: the covariance model keeps {out['members'].tolist()}, the scalar model at q_t = 0.02^2, q_r = 0.002^2 keeps "
          f"{scalar['members'].tolist()}")
    assert scalar["members"].tolist() != want and scalar["size"] < 8


# ---------------------------------------------------------------- an indefinite and a zero Q
def test_an_indefinite_q_makes_every_pair_non_finite(ctx):
    c = _case("65")
    L = len(c["a"])
    k, l = np.triu_indices(L, 1)
    assert ((c["a"][k] != c["a"][l]) | (c["b"][k] != c["b"][l])).all()  # every pair runs over some odometry
    out = _call(ctx, c, s=True, Q=-10.0 * np.eye(6))
    want = cref.pair_s(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], cref.chain_W(c["poses"], -10.0 * np.eye(6)))
    assert np.isnan(want[k, l]).all()
    assert np.isnan(out["s"][k, l]).all() and np.isnan(out["s"][l, k]).all() and not np.diag(out["s"]).any()
    assert out["non_finite_pairs"] == L * (L - 1) // 2 == cref.non_finite_pairs(want)
    assert not out["adjacency"].any() and not out["degree"].any()
    assert (out["size"], out["steps"], out["adjacent_pairs"]) == (1, 1, 0) and out["members"].tolist() == [0]


def test_a_zero_q_leaves_the_loops_own_covariances(ctx):
    """s = e^T (Sigma_k + G_l Sigma_l G_l^T)^-1 e: the mirror's pair term with W = 0"""
    for name in ("65", "planted"):
        c = _case(name)
        L = len(c["a"])
        out = _call(ctx, c, s=True, Q=np.zeros((6, 6)))
        want = cref.pair_s(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], np.zeros((len(c["poses"]), 6, 6)))
        rel = np.abs(out["s"] - want) / np.maximum(1.0, np.abs(want))
        print(f"  {name}, Q = 0: worst |s - ref| / max(1, |ref|) {float(rel.max()):.3e} (bound {ccases.S_FLOOR:.1e})")
        assert np.isfinite(out["s"]).all() and (rel <= ccases.S_FLOOR).all() and out["non_finite_pairs"] == 0
        assert np.array_equal(lref.unpack(out["adjacency"], L)[:, :L], cref.adjacency(out["s"], c["gamma"]))


# ---------------------------------------------------------------- the bytes
@pytest.mark.parametrize("name", ["129", "planted"])
def test_steps_per_batch_does_not_change_the_bytes(ctx, name):
    c = _case(name)
    want = _bytes(_run(ctx, name))
    for spb in (1, 32, 100000):  # one step a batch, the default, more than any clique
        assert _bytes(_call(ctx, c, s=True, steps_per_batch=spb)) == want, spb


def test_two_calls_give_the_same_bytes(ctx):
    for name in ("257", "planted"):
        c = _case(name)
        first = _call(ctx, c, s=True)
        again = _call(ctx, c, s=True)
        assert _bytes(first) == _bytes(again) == _bytes(_run(ctx, name))


def test_one_loop_no_loops_and_the_limit_of_s_out(ctx):
    out = _run(ctx, "1")
    assert (out["size"], out["steps"], out["adjacent_pairs"], out["non_finite_pairs"]) == (1, 1, 0, 0)
    assert out["members"].tolist() == [0] and out["degree"].tolist() == [0] and out["adjacency"].tolist() == [[0]] and out["s"].tolist() == [[0.0]]
    poses = _case("2")["poses"]
    Q = ccases.HONEST_Q
    none = LoopConsistencyCov(poses, [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), Q, None, ctx, adjacency=True, s=True)
    assert (none["size"], none["steps"], none["adjacent_pairs"], none["non_finite_pairs"]) == (0, 0, 0, 0) and none["members"].size == 0
    assert none["adjacency"].shape == (0, 0) and none["s"].shape == (0, 0) and none["degree"].size == 0 and none["chain_ms"] == 0.0
    L = _lib.LOOPS_MAX_S + 1
    rng = np.random.default_rng(5)
    a = rng.integers(0, lcases.CHAIN_N, L)
    b = (a + rng.integers(1, lcases.CHAIN_N, L)) % lcases.CHAIN_N
    Z = np.tile(np.eye(4), (L, 1, 1))
    with pytest.raises(ElmError, match=r"\(-1\).*ELM_LOOPS_MAX_S"):
        LoopConsistencyCov(poses, a, b, Z, np.eye(6), Q, None, ctx, s=True)
    big = LoopConsistencyCov(poses, a, b, Z, np.eye(6), Q, LoopConsistencyConfig(gamma=1e-300), ctx)  # without s_out the same loops are served
    assert big["size"] >= 1 and big["mask"].shape == (L,)
    with pytest.raises(ElmError, match=r"\(-1\).*ELM_LOOPS_MAX\b"):
        n = _lib.LOOPS_MAX + 1
        LoopConsistencyCov(poses, np.zeros(n, np.int32), np.ones(n, np.int32), np.tile(np.eye(4), (n, 1, 1)), np.eye(6), Q, None, ctx)
    # one pose: q_count = 1 is accepted and nothing is read
    assert not ChainCovariance(poses[:1], np.full((6, 6), np.nan), ctx).any()


# ---------------------------------------------------------------- the preconditions
def test_preconditions_on_a_live_context(ctx):
    c = _case("65")
    want = _bytes(_run(ctx, "65"))
    L = len(c["a"])
    base = dict(poses=c["poses"], a=c["a"], b=c["b"], Z=c["Z"], Sigma=c["Sigma"], Q=c["Q"])
    good = dict(gamma=c["gamma"])

    def changed(key, index, value):
        arr = np.array(base[key], copy=True)
        arr[index] = value
        return {**base, key: arr}

    indefinite = np.array(c["Sigma"], copy=True)
    indefinite[9] -= 1.0 * np.eye(6)
    bad_inputs = [
        (changed("a", 3, lcases.CHAIN_N), {}, "index outside"), (changed("b", 0, -1), {}, "index outside"),
        (changed("a", 5, int(c["b"][5])), {}, "a == b"), (changed("poses", (7, 1, 3), np.nan), {}, "non-finite pose"),
        (changed("Z", (2, 0, 0), np.inf), {}, "non-finite Z"), (changed("Sigma", (4, 1, 1), np.nan), {}, "loop 4: a non-finite Sigma"),
        (changed("Sigma", (64, 0, 5), 7.0), {}, "loop 64: Sigma is not symmetric"), ({**base, "Sigma": indefinite}, {}, "loop 9: Sigma is not positive definite"),
        (changed("Q", (11, 2, 3), 1.0), {}, "Q 11: not symmetric"), (changed("Q", (0, 0, 0), np.inf), {}, "Q 0: non-finite"),
        ({**base, "Q": c["Q"][:5]}, {}, "q_count"), ({**base, "Q": np.concatenate([c["Q"], c["Q"][:1]])}, {}, "q_count"),
        (base, dict(q_t=1e-12), "q_t and q_r must be 0"), (base, dict(q_r=0.5), "q_t and q_r must be 0"), (base, dict(gamma=0.0), "gamma"),
        (base, dict(gamma=np.inf), "gamma"), (base, dict(steps_per_batch=0), "steps_per_batch"),
    ]
    for inputs, cfg_change, text in bad_inputs:
        assert cref.refusal(lcases.CHAIN_N, inputs["a"], inputs["b"], inputs["Z"], inputs["Sigma"], inputs["Q"],
                            **{**good, **cfg_change}) is not None or "pose" in text, text  # the mirror refuses the same ones
        with pytest.raises(ElmError, match=r"\(-1\).*elm_loopcov_consistency: .*" + text):
            LoopConsistencyCov(inputs["poses"], inputs["a"], inputs["b"], inputs["Z"], inputs["Sigma"], inputs["Q"],
                               LoopConsistencyConfig(**{**good, **cfg_change}), ctx)
        # the call after it succeeds, with the bytes it always gives
        assert _bytes(_call(ctx, c, s=True)) == want, text
    # NULL arguments, by the raw call: refused with a text, the outputs untouched
    lib, cfg, res = _lib.lib(), LoopConsistencyConfig(**good), _lib.LoopCovResultC()
    res.size = 7
    P, Z = np.ascontiguousarray(c["poses"].transpose(0, 2, 1)).ravel(), np.ascontiguousarray(c["Z"].transpose(0, 2, 1)).ravel()
    Sg, Q = np.ascontiguousarray(c["Sigma"]).ravel(), np.ascontiguousarray(c["Q"]).ravel()
    member, degree = np.full(L, 9, np.uint8), np.full(L, 9, np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(x.dtype)))
    args = [P, lcases.CHAIN_N, c["a"], c["b"], Z, Sg, L, Q, lcases.CHAIN_N - 1, cfg, res, member, degree]
    for drop in (0, 2, 3, 4, 5, 7, 9, 10, 11, 12):
        a = [None if k == drop else (C.byref(x) if isinstance(x, C.Structure) else (x if isinstance(x, int) else ptr(x))) for k, x in enumerate(args)]
        assert lib.elm_loopcov_consistency(ctx._h, *a, None, None) == -1, drop
        assert b"NULL" in lib.elm_last_error(ctx._h)
    assert res.size == 7 and (member == 9).all() and (degree == 9).all()
    assert _bytes(_call(ctx, c, s=True)) == want


def test_a_device_group_and_a_batch_in_flight_are_refused(ctx):
    """refused as every pose-graph call that takes ctx is, and served again once the batch is finished"""
    from elimaloc_amd.context import Scan
    from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig
    from elimaloc_amd.voxel_map import VoxelHashMap
    c = _case("2")
    want = _bytes(_run(ctx, "2"))
    grp = Context.multi([0, 0])
    try:
        with pytest.raises(ElmError, match="one rank only"):
            _call(grp, c)
        with pytest.raises(ElmError, match="one rank only"):
            ChainCovariance(c["poses"], c["Q"], grp)
    finally:
        grp.close()
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(_scan_points(2000, 77))
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    reg.EnqueueBatch([Scan(ctx, _scan_points(300, 78))], vm, [np.eye(4)])
    try:
        with pytest.raises(ElmError, match=r"\(-1\)"):
            _call(ctx, c)
        with pytest.raises(ElmError, match=r"\(-1\)"):
            ChainCovariance(c["poses"], c["Q"], ctx)
    finally:
        reg.FinishBatch()
    assert _bytes(_call(ctx, c, s=True)) == want


# ---------------------------------------------------------------- LoopCloser
def _scan_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32))


def _closer(ctx, db, poses, loops):
    lc = LoopCloser(db)
    for k in range(len(poses)):
        lc.Insert(_scan_points(64, 700 + k), poses[k])
    for a, b, Z, info in loops:
        lc.AddLoop(a, b, Z, info)
    return lc


def _scalar_bytes(out):
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("members", "mask", "degree")) + (out["size"], out["steps"], out["adjacent_pairs"])


def test_close_with_the_covariance_model_equals_close_on_the_true_loops_alone(ctx):
    p = ccases.planted_honest()
    loops = [(int(p["a"][k]), int(p["b"][k]), p["Z"][k], p["info"][k]) for k in range(len(p["a"]))]
    odom_info = np.linalg.inv(p["Q"])
    cfg = PoseGraphConfig(**cases.RING_CFG)
    consistency = LoopConsistencyConfig(gamma=p["gamma"])
    db_all, db_true = PlaceDatabase(PlaceConfig(), lcases.PLANTED_N, ctx), PlaceDatabase(PlaceConfig(), lcases.PLANTED_N, ctx)
    try:
        lc_all = _closer(ctx, db_all, p["poses"], loops)
        lc_true = _closer(ctx, db_true, p["poses"], [l for l, t in zip(loops, p["is_true"]) if t])
        auto = lc_all.ConsistentLoops(consistency, odom_covariance=p["Q"])
        assert auto["members"].tolist() == np.flatnonzero(p["is_true"]).tolist() and auto["non_finite_pairs"] == 0
        per_step = lc_all.ConsistentLoops(consistency, odom_covariance=np.tile(p["Q"], (lcases.PLANTED_N - 1, 1, 1)))
        assert _scalar_bytes(per_step) == _scalar_bytes(auto)
        kept, res_kept = lc_all.Close(cfg, odom_info, consistency=consistency, odom_covariance=p["Q"])
        only, res_only = lc_true.Close(cfg, odom_info)
        assert res_kept["consistency"]["members"].tolist() == auto["members"].tolist() and "consistency" not in res_only
        assert np.array_equal(kept, only) and repr({k: v for k, v in res_kept.items() if k != "consistency"}) == repr(res_only)
        # the scalar model through the same door, at the same noise, keeps another set
        scalar = lc_all.ConsistentLoops(LoopConsistencyConfig(gamma=p["gamma"], **ccases.HONEST_SCALAR))
        assert scalar["members"].tolist() != auto["members"].tolist()
    finally:
        db_all.close()
        db_true.close()


def test_closer_without_odom_covariance_is_what_it_was(ctx):
    """ConsistentLoops() and Close() by default and with odom_covariance=None named, against the direct calls they have always made: on
    the ring and on loops_cases.planted"""
    p = lcases.planted()
    loops = [(int(p["a"][k]), int(p["b"][k]), p["Z"][k], p["info"][k]) for k in range(len(p["a"]))]
    odom_info = np.diag([1.0 / lcases.ODOM_SIGMA_T ** 2] * 3 + [1.0 / lcases.ODOM_SIGMA_R ** 2] * 3)
    cfg = PoseGraphConfig(**cases.RING_CFG)
    consistency = LoopConsistencyConfig(**p["cfg"])
    db = PlaceDatabase(PlaceConfig(), lcases.PLANTED_N, ctx)
    try:
        lc = _closer(ctx, db, p["poses"], loops)
        direct = LoopConsistency(p["poses"], p["a"], p["b"], p["Z"], p["var_t"], p["var_r"], consistency, ctx)
        plain, named = lc.ConsistentLoops(consistency), lc.ConsistentLoops(consistency, odom_covariance=None)
        assert _scalar_bytes(plain) == _scalar_bytes(named) == _scalar_bytes(direct) and "non_finite_pairs" not in plain
        assert plain["members"].tolist() == np.flatnonzero(p["is_true"]).tolist()
        poses, res = lc.Close(cfg, odom_info, consistency=consistency)
        poses_named, res_named = lc.Close(cfg, odom_info, consistency=consistency, odom_covariance=None)
        strip = lambda r: repr({k: v for k, v in r.items() if k != "consistency"})
        assert np.array_equal(poses, poses_named) and strip(res) == strip(res_named)
        assert _scalar_bytes(res["consistency"]) == _scalar_bytes(res_named["consistency"]) == _scalar_bytes(direct)
        blind, res_blind = lc.Close(cfg, odom_info)
        blind_named, res_blind_named = lc.Close(cfg, odom_info, odom_covariance=p["cfg"]["q_t"] * np.eye(6))  # unused without consistency
        assert np.array_equal(blind, blind_named) and repr(res_blind) == repr(res_blind_named) and "consistency" not in res_blind
    finally:
        db.close()
    g, truth = cases.ring()
    db = PlaceDatabase(PlaceConfig(), cases.RING_N, ctx)
    try:
        lc = _closer(ctx, db, g.poses, [(a, b, cases.inv_pose(truth[a]) @ truth[b], None) for a, b in cases.RING_LOOPS])
        poses, res = lc.Close(cfg)
        named, res_named = lc.Close(cfg, consistency=None, odom_covariance=None)
        assert np.array_equal(poses, named) and repr(res) == repr(res_named) and "consistency" not in res
        n = cases.RING_N
        pg = PoseGraph(n, n - 1 + len(cases.RING_LOOPS), ctx)
        try:
            fx = np.zeros(n, bool)
            fx[0] = True
            pg.AddNodes(g.poses, fx)
            pg.AddEdges(np.arange(n - 1), np.arange(1, n), np.linalg.inv(g.poses[:-1]) @ g.poses[1:])
            pg.AddEdges([a for a, _ in cases.RING_LOOPS], [b for _, b in cases.RING_LOOPS],
                        np.stack([cases.inv_pose(truth[a]) @ truth[b] for a, b in cases.RING_LOOPS]), np.tile(np.eye(6), (3, 1, 1)))
            res_hand = pg.Optimize(cfg)
            assert np.array_equal(pg.Poses(), poses) and repr(res_hand) == repr(res)
        finally:
            pg.close()
    finally:
        db.close()


# ---------------------------------------------------------------- the C++ face
def test_the_cpp_harness_agrees_on_the_planted_fixture(ctx, tmp_path):
    p, out = ccases.planted_honest(), _run(ctx, "planted")
    L = len(p["a"])
    exe, data = tmp_path / "loop_covariance_calls", tmp_path / "planted.f64"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                           "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_harness", "loop_covariance_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    np.concatenate([[lcases.PLANTED_N, L, 1, p["gamma"]], p["poses"].transpose(0, 2, 1).ravel(), p["a"].astype(np.float64), p["b"].astype(np.float64),
                    p["Z"].transpose(0, 2, 1).ravel(), p["Sigma"].ravel(), p["Q"].ravel()]).astype(np.float64).tofile(str(data))
    lines = subprocess.run([str(exe), str(data)], check=True, capture_output=True, timeout=120).stdout.decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [out["size"], out["adjacent_pairs"], out["steps"], out["non_finite_pairs"]]
    assert [int(x) for x in lines[1].split()] == out["members"].tolist() and [int(x) for x in lines[2].split()] == out["degree"].tolist()
    W, S = ChainCovariance(p["poses"], p["Q"], ctx, local=True)
    assert [float(x) for x in lines[3].split()] == [sum(float(M[-1][q, q]) for q in range(6)) for M in (W, S)]
