"""The loop consistency check on the GPU (include/elimaloc_hip_loops.h) against its mirror (tests/loops_ref.py):
s_out under the project's 1e-9 sums contract, adj_out bit for bit outside an (empty) band around gamma, the greedy clique exactly the
mirror's on the device's own adjacency, at the sizes where the word, wavefront and pick-tree edges lie; the batch size, the empty and the
complete graph, the run-to-run bytes, the planted fixture through LoopCloser.Close, the preconditions, and the C++ harness."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref
from elimaloc_amd import _lib
from elimaloc_amd._lib import ElmError
from elimaloc_amd.loops import LoopConsistency, LoopConsistencyConfig
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [str(L) for L in lcases.SIZES] + ["planted"]
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


def _case(name):
    """the inputs and the mirror's s and adjacency, computed once per case and left unchanged"""
    if name != "planted":
        return lcases.random_case(int(name))
    p = lcases.planted()
    return dict(poses=p["poses"], a=p["a"], b=p["b"], Z=p["Z"], var_t=p["var_t"], var_r=p["var_r"], q_t=p["cfg"]["q_t"], q_r=p["cfg"]["q_r"],
                gamma=p["cfg"]["gamma"], s=p["s"], adj=p["adj"])


def _call(ctx, c, gamma=None, adjacency=True, s=False, **kw):
    cfg = LoopConsistencyConfig(q_t=c["q_t"], q_r=c["q_r"], gamma=c["gamma"] if gamma is None else gamma, **kw)
    return LoopConsistency(c["poses"], c["a"], c["b"], c["Z"], c["var_t"], c["var_r"], cfg, ctx, adjacency=adjacency, s=s)


def _run(ctx, name):
    """the device's answer with both optional outputs, once per case"""
    if name not in _RUNS:
        _RUNS[name] = _call(ctx, _case(name), s=True)
    return _RUNS[name]


def _bytes(out):
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("members", "mask", "degree", "adjacency") if k in out) + (
        out["size"], out["steps"], out["adjacent_pairs"])


# ---------------------------------------------------------------- the pair terms
@pytest.mark.parametrize("name", CASES)
def test_s_against_the_mirror(ctx, name):
    c, out = _case(name), _run(ctx, name)
    s, want = out["s"], c["s"]
    L = len(c["a"])
    assert s.shape == (L, L) and np.array_equal(s, s.T) and not np.diag(s).any()
    rel = np.abs(s - want) / np.maximum(1.0, np.abs(want))
    print(f"  {name}: worst |s - ref| / max(1, |ref|) {float(rel.max()) if L else 0.0:.3e} (bound 1e-9), largest s {float(want.max()) if L else 0.0:.3e}")
    assert np.isfinite(s).all() and (rel <= 1e-9).all()


@pytest.mark.parametrize("name", CASES)
def test_adjacency_bit_for_bit(ctx, name):
    c, out = _case(name), _run(ctx, name)
    L = len(c["a"])
    assert lcases.in_band(c["s"], c["gamma"]) == 0  # no pair is excused: the cap on excluded pairs is zero
    words = out["adjacency"]
    assert words.dtype == np.uint64 and words.shape == (L, (L + 63) // 64)
    bits = lref.unpack(words, L)
    assert not bits[:, L:].any()  # the padding bits
    adj = bits[:, :L]
    assert np.array_equal(adj, adj.T) and not np.diag(adj).any()
    assert np.array_equal(adj, c["adj"]) and np.array_equal(words, lref.pack(c["adj"]))


# ---------------------------------------------------------------- the greedy clique
@pytest.mark.parametrize("name", CASES)
def test_greedy_is_the_mirrors_on_the_devices_adjacency(ctx, name):
    c, out = _case(name), _run(ctx, name)
    L = len(c["a"])
    adj = lref.unpack(out["adjacency"], L)[:, :L]
    members, degree0 = lref.greedy(adj)
    print(f"  {name}: clique of {out['size']} among {L} loops, {out['adjacent_pairs']} adjacent pairs")
    assert out["members"].tolist() == sorted(members) and out["mask"].tolist() == [k in members for k in range(L)]
    assert out["size"] == out["steps"] == len(members) and out["adjacent_pairs"] == int(adj.sum()) // 2
    assert out["degree"].dtype == np.int32 and np.array_equal(out["degree"], degree0)
    assert lref.is_clique(adj, out["members"]) and lref.is_maximal(adj, out["members"])


@pytest.mark.parametrize("name", ["129", "planted"])
def test_steps_per_batch_does_not_change_the_bytes(ctx, name):
    c = _case(name)
    want = _bytes(_run(ctx, name))
    for spb in (1, 32, 100000):  # one step a batch, the default, more than any clique
        assert _bytes(_call(ctx, c, steps_per_batch=spb)) == want, spb


def test_an_empty_and_a_complete_graph(ctx):
    for name in ("2", "65", "129"):
        c = _case(name)
        L = len(c["a"])
        none = _call(ctx, c, gamma=1e-300)
        assert (none["size"], none["steps"], none["adjacent_pairs"]) == (1, 1, 0) and none["members"].tolist() == [0]
        assert not none["adjacency"].any() and not none["degree"].any()
        every = _call(ctx, c, gamma=1e300, steps_per_batch=7)
        assert (every["size"], every["steps"], every["adjacent_pairs"]) == (L, L, L * (L - 1) // 2) and every["mask"].all()
        assert np.array_equal(every["adjacency"], lref.pack(~np.eye(L, dtype=bool))) and (every["degree"] == L - 1).all()


def test_two_calls_give_the_same_bytes(ctx):
    for name in ("257", "planted"):
        c = _case(name)
        first = _call(ctx, c, s=True)
        again = _call(ctx, c, s=True)
        assert _bytes(first) == _bytes(again) == _bytes(_run(ctx, name)) and first["s"].tobytes() == again["s"].tobytes()


def test_one_loop(ctx):
    out = _run(ctx, "1")
    assert (out["size"], out["steps"], out["adjacent_pairs"]) == (1, 1, 0) and out["members"].tolist() == [0] and out["degree"].tolist() == [0]
    assert out["adjacency"].tolist() == [[0]] and out["s"].tolist() == [[0.0]]


# ---------------------------------------------------------------- the planted fixture
def test_the_planted_members_are_the_true_loops(ctx):
    p, out = lcases.planted(), _run(ctx, "planted")
    assert out["members"].tolist() == np.flatnonzero(p["is_true"]).tolist() and out["size"] == 8


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


def test_close_with_consistency_equals_close_on_the_true_loops_alone(ctx):
    p = lcases.planted()
    loops = [(int(p["a"][k]), int(p["b"][k]), p["Z"][k], p["info"][k]) for k in range(len(p["a"]))]
    odom_info = np.diag([1.0 / lcases.ODOM_SIGMA_T ** 2] * 3 + [1.0 / lcases.ODOM_SIGMA_R ** 2] * 3)
    cfg = PoseGraphConfig(**cases.RING_CFG)
    consistency = LoopConsistencyConfig(**p["cfg"])
    db_all, db_true = PlaceDatabase(PlaceConfig(), lcases.PLANTED_N, ctx), PlaceDatabase(PlaceConfig(), lcases.PLANTED_N, ctx)
    try:
        lc_all = _closer(ctx, db_all, p["poses"], loops)
        lc_true = _closer(ctx, db_true, p["poses"], [l for l, t in zip(loops, p["is_true"]) if t])
        # the default variances are the informations' traces inverted: those of the fixture
        auto = lc_all.ConsistentLoops(consistency)
        assert auto["members"].tolist() == np.flatnonzero(p["is_true"]).tolist()
        assert _bytes(auto) == _bytes(lc_all.ConsistentLoops(consistency, var_t=p["var_t"], var_r=p["var_r"]))
        kept, res_kept = lc_all.Close(cfg, odom_info, consistency=consistency)
        only, res_only = lc_true.Close(cfg, odom_info)
        blind, res_blind = lc_all.Close(cfg, odom_info)
        assert res_kept["consistency"]["members"].tolist() == auto["members"].tolist() and "consistency" not in res_only
        assert np.array_equal(kept, only) and repr({k: v for k, v in res_kept.items() if k != "consistency"}) == repr(res_only)
        start = ref.pose_error(p["poses"], p["truth"])
        err_kept, err_blind = ref.pose_error(kept, p["truth"]), ref.pose_error(blind, p["truth"])
        print(f"  planted: odometry {start[0]:.3f} m {start[1]:.4f} rad off the truth; Close with consistency {err_kept[0]:.3f} m {err_kept[1]:.4f} rad "
              f"({res_kept['solves']} solves); Close with all 13 loops {err_blind[0]:.3f} m {err_blind[1]:.4f} rad ({res_blind['solves']} solves)")
        assert err_blind[0] > err_kept[0] and err_blind[1] > err_kept[1]
        assert np.stack(lc_all.poses).tobytes() == p["poses"].tobytes() and len(lc_all.loops) == 13
    finally:
        db_all.close()
        db_true.close()


def test_close_without_consistency_is_what_it_was_on_the_ring(ctx):
    """Close() by default, with consistency=None named, and the hand composition of the PoseGraph calls it has always made"""
    g, truth = cases.ring()
    db = PlaceDatabase(PlaceConfig(), cases.RING_N, ctx)
    try:
        lc = _closer(ctx, db, g.poses, [(a, b, cases.inv_pose(truth[a]) @ truth[b], None) for a, b in cases.RING_LOOPS])
        cfg = PoseGraphConfig(**cases.RING_CFG)
        poses, res = lc.Close(cfg)
        named, res_named = lc.Close(cfg, consistency=None)
        assert poses.tobytes() == named.tobytes() and repr(res) == repr(res_named) and "consistency" not in res
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
            assert pg.Poses().tobytes() == poses.tobytes() and repr(res_hand) == repr(res)
        finally:
            pg.close()
    finally:
        db.close()


# ---------------------------------------------------------------- the preconditions
def test_preconditions_on_a_live_context(ctx):
    c = _case("65")
    want = _bytes(_run(ctx, "65"))
    L = len(c["a"])
    base = dict(poses=c["poses"], a=c["a"], b=c["b"], Z=c["Z"], var_t=np.full(L, c["var_t"]), var_r=np.full(L, c["var_r"]))
    good = dict(q_t=c["q_t"], q_r=c["q_r"], gamma=c["gamma"])

    def changed(key, index, value):
        arr = np.array(base[key], copy=True)
        arr[index] = value
        return {**base, key: arr}

    bad_inputs = [
        (changed("a", 3, lcases.CHAIN_N), {}, "index outside"), (changed("b", 0, -1), {}, "index outside"),
        (changed("a", 5, int(c["b"][5])), {}, "a == b"), (changed("poses", (7, 1, 3), np.nan), {}, "non-finite pose"),
        (changed("Z", (2, 0, 0), np.inf), {}, "non-finite Z"), (changed("var_t", 4, np.nan), {}, "non-finite variance"),
        (changed("var_t", 4, 0.0), {}, "variance <= 0"), (changed("var_r", 64, -1.0), {}, "variance <= 0"),
        (base, dict(q_t=-1e-12), "q_t and q_r"), (base, dict(q_r=np.nan), "q_t and q_r"), (base, dict(gamma=0.0), "gamma"),
        (base, dict(gamma=-3.0), "gamma"), (base, dict(gamma=np.inf), "gamma"), (base, dict(steps_per_batch=0), "steps_per_batch"),
    ]
    for inputs, cfg_change, text in bad_inputs:
        with pytest.raises(ElmError, match=r"\(-1\).*elm_loops_consistency: .*" + text):
            LoopConsistency(inputs["poses"], inputs["a"], inputs["b"], inputs["Z"], inputs["var_t"], inputs["var_r"],
                            LoopConsistencyConfig(**{**good, **cfg_change}), ctx)
        # the call after it succeeds, with the bytes it always gives
        assert _bytes(_call(ctx, c)) == want, text
    # NULL arguments, by the raw call: refused with a text, the outputs untouched
    lib, cfg, res = _lib.lib(), LoopConsistencyConfig(**good), _lib.LoopsResultC()
    res.size = 7
    P, Z = np.ascontiguousarray(c["poses"].transpose(0, 2, 1)).ravel(), np.ascontiguousarray(c["Z"].transpose(0, 2, 1)).ravel()
    member, degree = np.full(L, 9, np.uint8), np.full(L, 9, np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(x.dtype)))
    args = [P, lcases.CHAIN_N, c["a"], c["b"], Z, base["var_t"], base["var_r"], L, cfg, res, member, degree]
    for drop in (0, 2, 3, 4, 5, 6, 8, 9, 10, 11):
        a = [None if k == drop else (C.byref(x) if isinstance(x, C.Structure) else (x if isinstance(x, int) else ptr(x))) for k, x in enumerate(args)]
        assert lib.elm_loops_consistency(ctx._h, *a, None, None) == -1, drop
        assert b"NULL" in lib.elm_last_error(ctx._h)
    assert res.size == 7 and (member == 9).all() and (degree == 9).all()
    assert _bytes(_call(ctx, c)) == want


def test_no_loops_and_the_limit_of_s_out(ctx):
    poses = _case("2")["poses"]
    out = LoopConsistency(poses, [], [], np.zeros((0, 4, 4)), [], [], None, ctx, adjacency=True, s=True)
    assert (out["size"], out["steps"], out["adjacent_pairs"]) == (0, 0, 0) and out["members"].size == 0 and out["mask"].size == 0
    assert out["adjacency"].shape == (0, 0) and out["s"].shape == (0, 0) and out["degree"].size == 0
    L = _lib.LOOPS_MAX_S + 1
    rng = np.random.default_rng(5)
    a = rng.integers(0, lcases.CHAIN_N, L)
    b = (a + rng.integers(1, lcases.CHAIN_N, L)) % lcases.CHAIN_N
    Z = np.tile(np.eye(4), (L, 1, 1))
    with pytest.raises(ElmError, match=r"\(-1\).*ELM_LOOPS_MAX_S"):
        LoopConsistency(poses, a, b, Z, 1.0, 1.0, None, ctx, s=True)
    big = LoopConsistency(poses, a, b, Z, 1.0, 1.0, LoopConsistencyConfig(gamma=1e-300), ctx)  # without s_out the same loops are served
    assert big["size"] >= 1 and big["mask"].shape == (L,)
    with pytest.raises(ElmError, match=r"\(-1\).*ELM_LOOPS_MAX\b"):
        n = _lib.LOOPS_MAX + 1
        LoopConsistency(poses, np.zeros(n, np.int32), np.ones(n, np.int32), np.tile(np.eye(4), (n, 1, 1)), 1.0, 1.0, None, ctx)


def test_a_device_group_and_a_batch_in_flight_are_refused(ctx):
    """refused as every pose-graph call that takes ctx is (tests/test_posegraph.py), and served again once the batch is finished"""
    from elimaloc_amd.context import Scan
    from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig
    from elimaloc_amd.voxel_map import VoxelHashMap
    c = _case("2")
    want = _bytes(_run(ctx, "2"))
    grp = Context.multi([0, 0])
    try:
        with pytest.raises(ElmError, match="one rank only"):
            _call(grp, c)
    finally:
        grp.close()
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(_scan_points(2000, 77))
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    reg.EnqueueBatch([Scan(ctx, _scan_points(300, 78))], vm, [np.eye(4)])
    try:
        with pytest.raises(ElmError, match=r"\(-1\)"):
            _call(ctx, c)
    finally:
        reg.FinishBatch()
    assert _bytes(_call(ctx, c)) == want


# ---------------------------------------------------------------- the C++ face
def test_the_cpp_harness_agrees_on_the_planted_fixture(ctx, tmp_path):
    p, out = lcases.planted(), _run(ctx, "planted")
    L = len(p["a"])
    exe, data = tmp_path / "loop_consistency_calls", tmp_path / "planted.f64"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                           "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_harness", "loop_consistency_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    np.concatenate([[lcases.PLANTED_N, L, p["cfg"]["q_t"], p["cfg"]["q_r"], p["cfg"]["gamma"]], p["poses"].transpose(0, 2, 1).ravel(),
                    p["a"].astype(np.float64), p["b"].astype(np.float64), p["Z"].transpose(0, 2, 1).ravel(), np.full(L, p["var_t"]),
                    np.full(L, p["var_r"])]).astype(np.float64).tofile(str(data))
    lines = subprocess.run([str(exe), str(data)], check=True, capture_output=True, timeout=120).stdout.decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [out["size"], out["adjacent_pairs"], out["steps"]]
    assert [int(x) for x in lines[1].split()] == out["members"].tolist() and [int(x) for x in lines[2].split()] == out["degree"].tolist()
