"""Map growth on the GPU (elm_growth_*): the candidate cells, hit, through, the fixed-point sums, every per-beam event count and every stats
field against the numpy mirror of the contract (tests/growth_ref.py), exactly and call by call; job order inside a call; contended
inserts and counters; long probe chains and the capacity guard; the stats against MapEvidence's and the end classes against the free-space
check's; every search index form; misuse; and on
a world with a box that the map does not hold, that the box is what appears and that the grown map explains the scans."""
import ctypes as C
import math

import numpy as np
import pytest

import growth_ref
import ray_ref  # tests/ is on sys.path via conftest
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import (Context, EvidenceConfig, FreeSpaceConfig, GrowthConfig, GrowthRule, IcpMethod, Registration,
                                        RegistrationConfig, Scan, VoxelHashMap)

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
FIELDS = growth_ref.FIELDS


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def field300k():
    return synth.make_field_world(300_000, seed=4242)


@pytest.fixture(scope="module")
def lattice300k():
    return synth.make_world(300_000, seed=77)


@pytest.fixture(scope="module")
def field_map(ctx, field300k):
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(field300k)
    return vm, vm.Pointcloud()


def _random_poses(T, n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    poses = np.empty((n, 4, 4))
    for h in range(n):
        poses[h] = np.eye(4)
        rpy = rng.uniform(-0.3, 0.3, 2)
        poses[h][:3, :3] = synth.rot_zyx(rpy[0], rpy[1], rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:3, 3] = T[:3, 3] + rng.uniform(-spread, spread, 3)
    return poses


def _noisy(scan, seed, far=0):
    """a scan of map points made to end everywhere: a third as drawn (in the map: END-HIT), a third with 0.15 m of noise (next to it:
    END-NEAR), a third with 2 m (free space: END-NEW), and `far` points 2 000 - 3 000 km out (beyond the key range: END-OUT)"""
    rng = np.random.default_rng(seed)
    out = np.array(scan, dtype=np.float64)
    k = np.arange(len(out)) % 3
    out[k == 1] += rng.normal(0.0, 0.15, ((k == 1).sum(), 3))
    out[k == 2] += rng.normal(0.0, 2.0, ((k == 2).sum(), 3))
    if far:
        d = rng.normal(size=(far, 3))
        out[rng.choice(len(out), far, replace=False)] = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(2e6, 3e6, (far, 1))
    return out.astype(np.float32)


def _same(g, ref):
    cells, hit, through, sums = g.Cells()
    rc, rh, rt, rs = ref.cells()
    assert cells.dtype == np.int32 and hit.dtype == np.uint32 and through.dtype == np.uint32 and sums.dtype == np.uint64
    assert np.array_equal(cells, rc), (cells.shape, rc.shape)
    assert np.array_equal(hit, rh), int(np.count_nonzero(hit != rh))
    assert np.array_equal(through, rt), int(np.count_nonzero(through != rt))
    assert np.array_equal(sums, rs), int(np.count_nonzero(sums != rs))
    assert g.Count() == len(rc)
    return cells, hit, through, sums


def _check_one(g, ref, cfg, pts, T):
    """Two observations from zero, each its own call, GPU == mirror after each: the cells, the counters, the sums, the per-beam events
    (resident order) and every stats field.  (The second call's beams see the first call's candidates.)"""
    g.Reset()
    ref.reset()
    sc = Scan(g.ctx, pts)
    res = sc.points()
    rst, rev, _ = ref.call(cfg, [res], np.asarray(T)[None])
    st, events = g.Accumulate(sc, T, cfg, events=True)
    print(st)
    assert events.dtype == np.uint16 and st == rst[0] and st["n_dropped"] == 0
    assert np.array_equal(events, rev[0]), int(np.count_nonzero(events != rev[0]))
    out = _same(g, ref)
    rst2, _, _ = ref.call(cfg, [res], np.asarray(T)[None])
    assert g.Accumulate(sc, T, cfg) == rst2[0]
    _same(g, ref)
    return st, events, out, res


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("world_name,vs", [("field", 1.0), ("field", 0.5), ("field", 0.3), ("lattice", 1.0), ("lattice", 0.5), ("lattice", 0.3)])
def test_exact_against_mirror(ctx, field300k, lattice300k, world_name, vs):
    world = field300k if world_name == "field" else lattice300k
    scan, T = synth.make_scan(world, 3001, seed=int(10 * vs))  # the worlds are centred on the origin
    scan = _noisy(scan, seed=int(10 * vs) + 1)
    far = _noisy(scan, seed=int(10 * vs) + 2, far=6)
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    stored = vm.Pointcloud()
    poses = _random_poses(T, 5, seed=int(vs * 10) + 3)
    for sub in (1, 2, 4):
        g = vm.Growth(8192, sub)
        ref = growth_ref.Growth(stored, vs, sub)
        origin = (0.4, -0.3, 0.25) if sub != 1 else (0.0, 0.0, 0.0)
        for k, n in enumerate((1, 255, 256, 257)):
            _check_one(g, ref, GrowthConfig(sub=sub, origin=origin, clearance_cells=k % 3), scan[:n], poses[k])
        for clearance in (0, 1, 2):  # the far points observe too (and are truncated: they would walk for ever)
            cfg = GrowthConfig(sub=sub, origin=origin, clearance_cells=clearance, obs_max_range_m=1e7)
            st, events, (cells, hit, through, sums), _ = _check_one(g, ref, cfg, far, poses[4])
            assert st["n_cast"] == 3001 and st["n_observing"] > 1500 and st["n_walked"] > 1000 and st["n_steps"] > 3001
            # the comparison cannot pass on an empty table: every end class occurs
            assert st["n_end_hit"] > 0 and st["n_end_new"] > 0 and st["n_end_out"] == 6 and (st["n_end_near"] > 0) == (clearance > 0)
            assert st["n_end_hit"] + st["n_end_near"] + st["n_end_new"] + st["n_end_out"] == st["n_observing"]
            assert int(hit.sum()) == st["n_end_new"] and len(cells) > 100 and st["n_truncated"] >= 6
            assert int(events.sum()) == st["n_through_events"]
        g.close()
    # a short margin, a walk from the origin itself, another observing band: beams see through the cells of their neighbours' end points
    g = vm.Growth(8192, 4)
    ref = growth_ref.Growth(stored, vs, 4)
    st, _, (_, _, through, _), _ = _check_one(g, ref, GrowthConfig(sub=4, min_range_m=0.0, obs_min_range_m=0.0, obs_max_range_m=25.0, end_margin_m=0.05,
                                                                 end_margin_frac=0.0, origin=(-0.2, 0.1, 0.3)), scan, poses[0])
    assert st["n_through_events"] > 0 and through.sum() > 0
    g.close()


# ---------------------------------------------------------------- 2. a batch is one call
def test_batch_order_and_calls(ctx, field300k, field_map):
    vm, stored = field_map
    scan, T = synth.make_scan(field300k, 2000, seed=5)
    scan = _noisy(scan, seed=6)
    sizes = (0, 1, 256, 257, 1000)
    lo = np.cumsum((0,) + sizes)
    scs = [Scan(ctx, scan[a:a + n]) for a, n in zip(lo, sizes)]
    jobs = scs + [scs[2]]  # the 256-point scan a second time, at another pose
    poses = _random_poses(T, len(jobs), seed=6, spread=1.5)
    poses[3], poses[4] = T, T
    cfg = GrowthConfig(origin=(0.1, 0.0, -0.2), min_range_m=0.0, end_margin_m=0.1, end_margin_frac=0.0)  # short margins: through events
    pts = [s.points() for s in jobs]
    ref = growth_ref.Growth(stored, 1.0, 4)
    rst, _, _ = ref.call(cfg, pts, poses)
    g = vm.Growth(8192)
    got = g.Accumulate(jobs, poses, cfg)
    print(got)
    assert got == rst and got[0] == dict.fromkeys(FIELDS, 0) and got[2] != got[5]
    cells, hit, through, sums = _same(g, ref)
    assert through.sum() > 0 and hit.sum() > 300 and all(s["n_dropped"] == 0 for s in got)
    # the same jobs in reversed order inside one call: the same counters, the same stats per job
    g.Reset()
    rev = g.Accumulate(jobs[::-1], poses[::-1], cfg)
    assert rev[::-1] == got
    _same(g, ref)
    # split into two calls: the mirror's call-by-call result, which differs from the single call's (later candidates are not seen)
    ref.reset()
    g.Reset()
    a = ref.call(cfg, pts[:3], poses[:3])[0] + ref.call(cfg, pts[3:], poses[3:])[0]
    b = g.Accumulate(jobs[:3], poses[:3], cfg) + g.Accumulate(jobs[3:], poses[3:], cfg)
    assert a == b
    _, _, through2, _ = _same(g, ref)
    assert through2.sum() <= through.sum()
    # arrays instead of resident scans; events are for a single scan only
    ref.call(cfg, pts, poses)
    g.Accumulate(pts, poses, cfg)
    _same(g, ref)
    with pytest.raises(ElmError):
        g.Accumulate(jobs, poses, cfg, events=True)
    g.close()


# ---------------------------------------------------------------- 3. contention
def test_contended_inserts_and_counters_are_exact(ctx):
    """4 096 copies of one beam: +x from the centre of cell (0, 0, 0) of a 0.25 m lattice to x = 3.2 (float32), cell (12, 0, 0), which the
    map does not hold (nor anything near it): one candidate, hit 4 096, and the sums 4 096 times one beam's k.  A second job in the same
    call: 4 096 copies of the beam to x = 6.125, L = 6, reach 4.8, which leaves cell 12 at 3.125: through 4 096."""
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(np.array([(1.3, 0.1, 0.2), (0.1, -0.9, 0.1), (2.1, 0.9, 0.1)], np.float32))
    o = (0.125, 0.125, 0.125)
    end = np.array([(3.2, 0.125, 0.125)], np.float32)
    kx = int(math.floor((float(end[0, 0]) * 4.0 - 12.0) * 65536.0))
    ends = np.tile(end, (4096, 1))
    crossing = np.tile(np.array([(6.125, 0.125, 0.125)], np.float32), (4096, 1))
    cfg = GrowthConfig(origin=o)
    ref = growth_ref.Growth(vm.Pointcloud(), 1.0, 4)
    rst, _, _ = ref.call(cfg, [ends, crossing], np.stack([np.eye(4)] * 2))
    rc, rh, rt, rs = ref.cells()
    assert rc.tolist() == [[12, 0, 0], [24, 0, 0]] and rh.tolist() == [4096, 4096] and rt.tolist() == [4096, 0]  # the mirror agrees with the hand count
    assert rs.tolist() == [[4096 * kx, 4096 * 32768, 4096 * 32768], [4096 * 32768] * 3]
    g = vm.Growth(40000)
    sa, sb = Scan(ctx, ends), Scan(ctx, crossing)
    for _ in range(2):
        g.Reset()
        st = g.Accumulate([sa, sb], np.stack([np.eye(4)] * 2), cfg)
        assert st == rst and st[0]["n_end_new"] == 4096 and st[1]["n_through_events"] == 4096 and st[0]["n_dropped"] == 0
        _same(g, ref)
    # 4 x 4 096 copies on top, in one call with the crossing job
    ref.call(cfg, [ends] * 4 + [crossing], np.stack([np.eye(4)] * 5))
    g.Accumulate([sa] * 4 + [sb], np.stack([np.eye(4)] * 5), cfg)
    cells, hit, through, sums = _same(g, ref)
    assert hit.tolist() == [5 * 4096, 2 * 4096] and through.tolist() == [2 * 4096, 0] and sums[0].tolist() == [5 * 4096 * kx, 5 * 4096 * 32768, 5 * 4096 * 32768]
    # 64 lanes of one wave end in the 64 distinct fine cells of one coarse cell: 64 inserts under one coarse key, one mask of 64 bits; a
    # second job in the same call walks from the origin through every one of these end points to 1.6 times its range
    ax = np.arange(4)
    X, Y, Zz = np.meshgrid(ax, ax, ax, indexing="ij")
    cells64 = np.stack([X.ravel() + 40, Y.ravel() + 40, Zz.ravel() + 40], 1)
    centres = ((cells64 + 0.5) * 0.25).astype(np.float32)
    cfg0 = GrowthConfig(origin=(0.0, 0.0, 0.0), obs_max_range_m=100.0)
    lanes, walkers = Scan(ctx, centres), Scan(ctx, centres * np.float32(1.6))
    ref.reset()
    g.Reset()
    rst = ref.call(cfg0, [lanes.points(), walkers.points()], np.stack([np.eye(4)] * 2))[0]
    st = g.Accumulate([lanes, walkers], np.stack([np.eye(4)] * 2), cfg0)
    assert st == rst and st[0]["n_end_new"] == 64 and st[1]["n_through_beams"] == 64
    cells, hit, through, _ = _same(g, ref)
    at = np.searchsorted(ray_ref.codes(cells), ray_ref.codes(cells64))
    assert np.array_equal(cells[at], cells64) and (hit[at] == 1).all() and (through[at] >= 1).all()
    g.close()


# ---------------------------------------------------------------- 4. table edges
def test_long_probe_chains_and_the_capacity_guard(ctx, field_map):
    vm, stored = field_map
    # 60 distinct candidate cells in 128 slots: cells in the air over the map, one beam each, four beams per call (count + beams <= 64)
    rng = np.random.default_rng(3)
    cells = np.unique(rng.integers(-200, 200, (80, 3)) + (0, 0, 400), axis=0)[:60]
    pts = ((cells + rng.uniform(0.1, 0.9, cells.shape)) * 0.25).astype(np.float32)
    cfg = GrowthConfig(obs_max_range_m=1000.0)
    g = vm.Growth(64)
    ref = growth_ref.Growth(stored, 1.0, 4)
    for a in range(0, 60, 4):
        assert g.Accumulate(pts[a:a + 4], np.eye(4), cfg) == ref.call(cfg, [pts[a:a + 4]], np.eye(4)[None])[0][0]
    got, hit, through, _ = _same(g, ref)
    assert len(got) == 60 and np.array_equal(got, cells[np.lexsort(cells.T[::-1])]) and (hit == 1).all() and g.Count() == 60
    # the guard: 60 + 5 > 64 is refused before anything is launched, the table is unchanged, and the next fitting call is correct
    five = np.concatenate([pts[:3], ((cells[:2] + (0, 0, 700) + 0.5) * 0.25).astype(np.float32)])
    L = _lib.lib()
    sc = Scan(ctx, five)
    st = _lib.GrowthStatsC()
    T16 = np.ascontiguousarray(np.eye(4)).ravel()
    rc = L.elm_growth_accumulate(ctx._h, g._h, sc._h, T16.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cfg), C.byref(st), None)
    assert rc == UNSUPPORTED and "capacity" in L.elm_last_error(ctx._h).decode()
    with pytest.raises(ElmError):
        g.Accumulate(five, np.eye(4), cfg)
    _same(g, ref)
    assert g.Accumulate(five[:4], np.eye(4), cfg) == ref.call(cfg, [five[:4]], np.eye(4)[None])[0][0]
    got, hit, _, _ = _same(g, ref)
    assert len(got) == 61 and hit.sum() == 64
    with pytest.raises(ElmError):  # 61 + 4 > 64 although only known cells would be hit: the guard counts beams
        g.Accumulate(pts[:4], np.eye(4), cfg)
    g.Reset()
    ref.reset()
    assert g.Accumulate(pts[:64 - 4], np.eye(4), cfg) == ref.call(cfg, [pts[:60]], np.eye(4)[None])[0][0]  # after a reset there is room again
    _same(g, ref)
    g.close()


# ---------------------------------------------------------------- 5. the evidence walk
def test_stats_agree_with_map_evidence(ctx, field300k, field_map):
    vm, stored = field_map
    scan, T = synth.make_scan(field300k, 3001, seed=21)
    scan = _noisy(scan, seed=22)
    poses = _random_poses(T, 3, seed=4, spread=0.5)
    jobs = [Scan(ctx, scan), Scan(ctx, scan[:700]), Scan(ctx, scan[700:1500])]
    kw = dict(origin=(0.1, -0.1, 0.2), max_steps=40)
    ev, g = vm.Evidence(), vm.Growth(8192)
    a, b = ev.Accumulate(jobs, poses, EvidenceConfig(**kw)), g.Accumulate(jobs, poses, GrowthConfig(**kw))
    for x, y in zip(a, b):
        assert all(x[k] == y[k] for k in ("n_cast", "n_observing", "n_walked", "n_truncated", "n_steps", "n_end_hit"))
        assert y["n_end_near"] + y["n_end_new"] + y["n_end_out"] == x["n_end_free"] and y["n_truncated"] > 0 and y["n_end_new"] > 0
    ev.close()
    g.close()


def test_end_classes_agree_with_the_free_space_check(ctx, lattice300k):
    """The end point's neighbourhood test is one function for both calls: with a clearance of one cell and the same range window and origin,
    the free-space check's supported end points are growth's END-HIT and END-NEAR ones, at every pose.  (Chosen on the mirrors,
    growth_ref and test_free_space.mirror, with the first 20 world points of every voxel as the stored points: 98 hit / 81 near / 75
    neither of 254 observing beams at the first pose, 7 / 14 / 233 at the second, none out of range, the three equalities holding.  On
    the map itself the classes are 93 / 86 / 75 and 6 / 15 / 233.)"""
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(lattice300k)
    scan, T = synth.make_scan(lattice300k, 300, seed=21)  # one full 256-beam chunk and a tail of 44
    sc = Scan(ctx, _noisy(scan, seed=22))
    poses = _random_poses(T, 2, seed=23, spread=0.5)
    poses[0] = T
    fcfg = FreeSpaceConfig()
    gcfg = GrowthConfig(sub=fcfg.sub, origin=fcfg.origin, clearance_cells=1, obs_min_range_m=fcfg.min_range_m, obs_max_range_m=fcfg.max_range_m)
    g = vm.Growth(1024, fcfg.sub)
    free, grow = vm.CheckFreeSpace(sc, poses, fcfg), g.Accumulate([sc, sc], poses, gcfg)
    for f, y in zip(free, grow):
        assert y["n_end_out"] == 0 and y["n_end_hit"] > 0 and y["n_end_near"] > 0 and y["n_end_new"] > 0, y  # hit, near and neither all occur
        assert f["n_supported"] == y["n_end_hit"] + y["n_end_near"], (f, y)
        assert f["n_counted"] == y["n_observing"] and f["n_end_occupied"] == y["n_end_hit"], (f, y)
    g.close()


# ---------------------------------------------------------------- 6. edges
def test_edge_cases(ctx, lattice300k):
    world = lattice300k
    scan, T = synth.make_scan(world, 1500, seed=10)
    scan = _noisy(scan, seed=11)
    # an empty map: nothing is HIT or NEAR, every in-range end point is a candidate
    empty = VoxelHashMap(1.0, 20, ctx)
    g = empty.Growth(4096)
    ref = growth_ref.Growth(np.zeros((0, 3)), 1.0, 4)
    st, _, (cells, _, _, _), _ = _check_one(g, ref, GrowthConfig(), scan, T)
    assert st["n_end_hit"] == 0 and st["n_end_near"] == 0 and st["n_end_new"] == st["n_observing"] > 500 and len(cells) > 400
    g.close()
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(world)
    stored = vm.Pointcloud()
    g = vm.Growth(8192)
    ref = growth_ref.Growth(stored, 1.0, 4)
    # an empty scan
    assert g.Accumulate(np.zeros((0, 3), np.float32), T) == dict.fromkeys(FIELDS, 0)
    st0, e0 = g.Accumulate(np.zeros((0, 3), np.float32), T, events=True)
    assert e0.shape == (0,) and g.Count() == 0
    # zero-length, NaN and inf points between real ones: those lanes observe nothing, the other lanes of their waves are unchanged
    o = (0.5, 0.25, -0.125)
    nan, inf = float("nan"), float("inf")
    bad = np.array([o, (nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 2.0, -inf), o, (nan, nan, nan), (inf, -inf, 0.0)], np.float32)
    cfg = GrowthConfig(origin=o)
    st_clean, _, clean, _ = _check_one(g, ref, cfg, scan[:700], T)
    mixed = np.concatenate([bad[:3], scan[:300], bad[3:5], scan[300:700], bad[5:]])
    st_mix, ev_mix, mix, res_mix = _check_one(g, ref, cfg, mixed, T)
    is_bad = ~np.isfinite(res_mix).all(1) | np.all(res_mix == np.array(o, np.float32), axis=1)
    assert is_bad.sum() == len(bad) and not ev_mix[is_bad].any() and st_mix == st_clean and st_mix["n_cast"] == 700
    assert all(np.array_equal(x, y) for x, y in zip(mix, clean))
    # end points exactly on a cell face, both signs: the lower face belongs to the cell (k = 0), the upper face to the next one.  Identity
    # rotation and a translation on the 0.25 m lattice: q = p + t is exact
    G = np.eye(4)
    G[:3, 3] = (3.0, -2.5, 1.25)
    rng = np.random.default_rng(5)
    pick = np.unique(np.concatenate([rng.integers(-300, -20, (60, 3)), rng.integers(20, 300, (60, 3)), rng.integers(-300, 300, (60, 3))]) + (0, 0, 500), axis=0)
    lower = (pick * 0.25 - G[:3, 3]).astype(np.float32)
    cfg0 = GrowthConfig(obs_min_range_m=0.0, obs_max_range_m=1000.0)
    st, _, (cells, hit, _, sums), _ = _check_one(g, ref, cfg0, lower, G)
    assert st["n_end_new"] == len(pick) and np.array_equal(cells, pick[np.lexsort(pick.T[::-1])]) and not sums.any() and (pick < 0).any()
    upper = ((pick + 1) * 0.25 - G[:3, 3]).astype(np.float32)
    st, _, (cells, _, _, sums), _ = _check_one(g, ref, cfg0, upper, G)
    assert np.array_equal(cells, np.unique(pick + 1, axis=0)) and not sums.any()
    # axis-parallel beams (w = 0 on two axes), beams along cell faces and through cell corners (the tie rule), among candidates made by
    # shorter beams of the same directions in the same call
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (1, 1, 1), (-1, -1, -1),
                     (1, 0, 1), (0, -1, 1), (2, 1, 0), (1, 2, 2), (-3, 4, 0), (1, 1, -1)], np.float32)
    events_seen = 0
    for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (0.25, -0.5, 0.0)):
        for margin in (1.0, 0.25):
            both = np.concatenate([axes * 8.0, axes * 3.0, axes * 4.5]) + np.float32(origin)
            G2 = np.eye(4)
            G2[:3, 3] = (3.0, -2.5, 125.0)  # in the air over the map: every end point is new
            st, _, _, _ = _check_one(g, ref, GrowthConfig(min_range_m=0.0, obs_min_range_m=0.0, origin=origin, end_margin_m=margin, end_margin_frac=0.0),
                                     both, G2)
            assert st["n_observing"] == len(both) == st["n_walked"] == st["n_end_new"]
            events_seen += st["n_through_events"]
    assert events_seen > 0
    # max_steps 1 and 7: truncation counted, the cells left before it counted
    short = dict(min_range_m=0.0, end_margin_m=0.1, end_margin_frac=0.0)
    full, _, _, _ = _check_one(g, ref, GrowthConfig(**short), scan, T)
    for ms in (1, 7):
        st, events, _, _ = _check_one(g, ref, GrowthConfig(max_steps=ms, **short), scan, T)
        assert st["n_truncated"] > 300 and st["n_steps"] <= ms * st["n_walked"] and st["n_walked"] == full["n_walked"]
        assert st["n_through_events"] <= full["n_through_events"] and int(events.max()) <= ms and st["n_end_new"] == full["n_end_new"]
    assert full["n_truncated"] == 0 and full["n_through_events"] > 0
    # a scan entirely outside the observing band: cast, and nothing else
    g.Reset()
    st = g.Accumulate(scan, T, GrowthConfig(obs_min_range_m=70.0, obs_max_range_m=80.0))
    assert st == dict(dict.fromkeys(FIELDS, 0), n_cast=1500) and g.Count() == 0 and g.Cells()[0].shape == (0, 3)
    # Reset, then the same input: the same output
    a = g.Accumulate(scan, T)
    ca = g.Cells()
    pa = g.AppearedPoints(GrowthRule(min_hit=1))
    g.Reset()
    assert g.Accumulate(scan, T) == a and all(np.array_equal(x, y) for x, y in zip(g.Cells(), ca))
    assert np.array_equal(g.AppearedPoints(GrowthRule(min_hit=1)), pa) and len(pa) > 0
    ref.reset()
    ref.call(GrowthConfig(), [Scan(ctx, scan).points()], T[None])
    assert np.array_equal(pa, ref.appeared_points(1, 4))
    g.close()


# ---------------------------------------------------------------- 7. index forms
@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled")])
def test_same_result_under_every_index_form(monkeypatch, field300k, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    scan, T = synth.make_scan(field300k, 3000, seed=31)
    scan = _noisy(scan, seed=32)
    vm = VoxelHashMap(1.0, 20, c)
    vm.AddPoints(field300k)
    vm.BuildNeighbourhoods()
    poses = _random_poses(T, 3, seed=9, spread=1.0)
    scs = [Scan(c, j) for j in (scan[:1000], scan[1000:1300], scan)]
    cfg = GrowthConfig()
    ref = growth_ref.Growth(vm.Pointcloud(), 1.0, 4)
    rst = ref.call(cfg, [s.points() for s in scs], poses)[0]
    g = vm.Growth(8192)
    assert g.Accumulate(scs, poses, cfg) == rst
    _, hit, _, _ = _same(g, ref)
    assert hit.sum() > 300
    g.close()
    del vm
    c.close()


# ---------------------------------------------------------------- 8. misuse
def test_misuse_is_refused_and_the_context_stays_usable(ctx, field_map):
    vm, stored = field_map
    world = synth.make_world(30_000, seed=11)
    scan, T = synth.make_scan(world, 2048, seed=12)
    scan = _noisy(scan, seed=13)
    L = _lib.lib()
    T16 = np.ascontiguousarray(T.T).ravel()
    dp = T16.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.GrowthStatsC * 2)()
    cfg = GrowthConfig()
    small = VoxelHashMap(1.0, 30, ctx)
    small.AddPoints(world)
    g = small.Growth(8192, 4)
    sc = Scan(ctx, scan)

    def acc(c, e, s, pose=dp, cf=cfg):
        return L.elm_growth_accumulate(c._h, e._h, s._h, pose, C.byref(cf), st, None)

    # cfg.sub must equal the object's
    assert acc(ctx, g, sc, cf=GrowthConfig(sub=2)) == INVALID
    g2 = small.Growth(8192, 2)
    assert acc(ctx, g2, sc) == INVALID and acc(ctx, g2, sc, cf=GrowthConfig(sub=2)) == 0
    g2.close()
    # a non-finite pose entry
    for bad in (float("nan"), float("inf")):
        B16 = T16.copy()
        B16[13] = bad
        assert acc(ctx, g, sc, pose=B16.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    # map, scan and growth object of another context
    other = Context(0)
    osc = Scan(other, scan)
    omap = VoxelHashMap(1.0, 30, other)
    omap.AddPoints(world)
    out = C.c_void_p()
    assert L.elm_growth_create(ctx._h, omap._handle(), 4, 100, C.byref(out)) == INVALID and not out.value
    assert acc(ctx, g, osc) == INVALID and acc(other, g, osc) == INVALID
    hs = (C.c_void_p * 2)(sc._h.value, osc._h.value)
    two = np.concatenate([T16, T16])
    assert L.elm_growth_accumulate_batch(ctx._h, g._h, hs, two.ctypes.data_as(C.POINTER(C.c_double)), 2, C.byref(cfg), st) == INVALID
    n = C.c_size_t(0)
    rule = GrowthRule()
    assert L.elm_growth_cells(other._h, g._h, None, None, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_growth_reset(other._h, g._h) == INVALID
    assert L.elm_growth_appeared_points(other._h, g._h, C.byref(rule), None, 0, C.byref(n)) == INVALID
    # nothing was recorded by any refused call
    assert g.Count() == 0
    # a batch in flight
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx=ctx)
    reg.EnqueueBatch([sc], small, T[None])
    assert acc(ctx, g, sc) == INVALID
    assert L.elm_growth_cells(ctx._h, g._h, None, None, None, None, 0, C.byref(n)) == INVALID and L.elm_growth_reset(ctx._h, g._h) == INVALID
    assert L.elm_growth_create(ctx._h, small._handle(), 4, 100, C.byref(out)) == INVALID
    reg.FinishBatch()
    # a communicator hook attached
    other.set_allreduce_hook(lambda p, n_, s: 0)
    og_h = C.c_void_p()
    assert L.elm_growth_create(other._h, omap._handle(), 4, 100, C.byref(og_h)) == UNSUPPORTED
    other.set_allreduce_hook(None)
    og = omap.Growth(8192)
    other.set_allreduce_hook(lambda p, n_, s: 0)
    assert acc(other, og, osc) == UNSUPPORTED and "one rank" in L.elm_last_error(other._h).decode()
    assert L.elm_growth_cells(other._h, og._h, None, None, None, None, 0, C.byref(n)) == UNSUPPORTED
    other.set_allreduce_hook(None)
    assert acc(other, og, osc) == 0 and st[0].n_cast == 2048
    og.close()
    del omap, osc
    other.close()
    # a device group's lead
    grp = Context.multi([0, 0])
    gvm = VoxelHashMap(1.0, 30, grp)
    gvm.AddPoints(world)
    assert L.elm_growth_create(grp._h, gvm._handle(), 4, 100, C.byref(out)) == UNSUPPORTED and "one rank" in L.elm_last_error(grp._h).decode()
    del gvm
    grp.close()
    # the Python layer: a rebuilt map invalidates its growth object; a closed object is refused; WithAppeared wants this map's object
    tmp = VoxelHashMap(1.0, 30, ctx)
    tmp.AddPoints(world[:1000])
    tg = tmp.Growth(4096)
    tmp.AddPoints(world[1000:2000])
    with pytest.raises(ElmError):
        tg.Accumulate(sc, T)
    with pytest.raises(ElmError):
        tmp.WithAppeared(tg)
    tg.close()
    with pytest.raises(ElmError):
        tg.Cells()
    with pytest.raises(ElmError):
        small.WithAppeared(vm.Growth(16))
    # the context and the object are usable afterwards, with the answer of the mirror
    _check_one(g, growth_ref.Growth(small.Pointcloud(), 1.0, 4), cfg, scan, T)
    g.close()


# ---------------------------------------------------------------- 9. it finds what appeared, and the grown map explains the scans
# The mirror's figures for this scene (the contract, not the kernel), default config and rule, as recorded in DESIGN.md section 16:
# seed -> (a) share of the box's cells flagged appeared, (b) share flagged among all other candidates (there are none: 0), (c) END-NEW beams
# on WithAppeared(A) / on A
RECORDED = {1: (0.6643, 0.0, 0.0083), 2: (0.0532, 0.0, 0.3951), 3: (0.3437, 0.0, 0.0504)}
TEST_SEED = 1


def box_scene(vm_a, seed):
    """The box of DESIGN.md section 15's scene (surfaces at 0.1 m spacing, 4 x 3 x 2.5 m, standing on the ground near the map's centre) and 12
    poses on a ring of 12 m around it, 1.8 m over the ground, each with its own yaw and a small tilt."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-8.0, 8.0, 2)
    found, gz = vm_a.FindGroundHeight(centre)
    assert found
    sx, sy, sz = 4.0, 3.0, 2.5
    gx, gy, gzs = np.arange(0.0, sx + 1e-9, 0.1), np.arange(0.0, sy + 1e-9, 0.1), np.arange(0.0, sz + 1e-9, 0.1)
    faces = []
    for x in (0.0, sx):
        Y, Z = np.meshgrid(gy, gzs, indexing="ij")
        faces.append(np.stack([np.full(Y.size, x), Y.ravel(), Z.ravel()], 1))
    for y in (0.0, sy):
        X, Z = np.meshgrid(gx, gzs, indexing="ij")
        faces.append(np.stack([X.ravel(), np.full(X.size, y), Z.ravel()], 1))
    X, Y = np.meshgrid(gx, gy, indexing="ij")
    faces.append(np.stack([X.ravel(), Y.ravel(), np.full(X.size, sz)], 1))
    box = rng.permutation(np.concatenate(faces)) + (centre[0] - sx / 2, centre[1] - sy / 2, gz)  # shuffled: the voxel cap keeps an even sample
    poses = np.empty((12, 4, 4))
    for k in range(12):
        a = 2.0 * math.pi * k / 12 + rng.uniform(-0.1, 0.1)
        xy = centre + 12.0 * np.array([math.cos(a), math.sin(a)])
        found, g = vm_a.FindGroundHeight(xy)
        assert found
        poses[k] = np.eye(4)
        poses[k][:3, :3] = synth.rot_zyx(rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-math.pi, math.pi))
        poses[k][:3, 3] = (xy[0], xy[1], g + 1.8)
    return box.astype(np.float32), poses


def box_cells(stored_a, stored_b, cell=0.25, clearance=1):
    """the fine cells of B that A lacks and that are END-NEW-eligible: no occupied cell of A within the clearance"""
    occ_a = ray_ref.occupancy(stored_a, cell)
    cells_b = np.unique(np.floor(np.asarray(stored_b, dtype=np.float64) / cell).astype(np.int64), axis=0)
    cand = cells_b[~ray_ref.is_in(occ_a, ray_ref.codes(cells_b))]
    near = np.zeros(len(cand), bool)
    r = np.arange(-clearance, clearance + 1)
    for off in np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3):
        near |= ray_ref.is_in(occ_a, ray_ref.codes(cand + off))
    return cand[~near]


def box_figures(box, cells, appeared, new_before, new_after):
    """(a), (b), (c) from the candidate cells and their appeared flags"""
    bc = np.sort(ray_ref.codes(box))
    gc = ray_ref.codes(cells)
    a = float(ray_ref.is_in(np.sort(gc[appeared]), bc).mean())
    others = ~ray_ref.is_in(bc, gc)
    b = float(appeared[others].mean()) if others.any() else 0.0
    return a, b, new_after / new_before


def test_it_finds_what_appeared_and_the_grown_map_explains_it(ctx, field300k, field_map):
    vm_a, stored_a = field_map
    box, poses = box_scene(vm_a, TEST_SEED)
    vm_b = VoxelHashMap(1.0, 20, ctx)
    vm_b.AddPoints(np.concatenate([field300k, box]))
    stored_b = vm_b.Pointcloud()
    beams = synth.lidar_beams(32, 512)
    scans = [Scan(ctx, vm_b.RenderScan(P, beams)) for P in poses]  # what a sensor sees in the world WITH the box
    n_beams = sum(s.n for s in scans)
    cfg = GrowthConfig()
    g = vm_a.Growth(n_beams)
    st = g.Accumulate(scans, poses, cfg)
    pts = [s.points() for s in scans]
    ref = growth_ref.Growth(stored_a, 1.0, 4)
    assert st == ref.call(cfg, pts, poses)[0]
    cells, hit, through, sums = _same(g, ref)
    new = g.AppearedPoints()
    assert np.array_equal(new, ref.appeared_points()) and len(new) > 0
    appeared = growth_ref.appeared_cells(hit, through)
    bx = box_cells(stored_a, stored_b)
    assert len(bx) > 200
    # (d) the grown map holds exactly A's points plus the appeared points that the ordinary build keeps: A's points first and unchanged, then
    # a subset of the appeared points in their order, and every one left out is excused by the build's rule (its voxel is full, or a kept
    # point of its voxel lies within sqrt(voxel^2 / cap))
    grown = vm_a.WithAppeared(g)
    kept = grown.Pointcloud()
    assert (grown.voxel_size_, grown.max_points_per_voxel_) == (1.0, 20) and grown.ctx is ctx
    new32 = new.astype(np.float32).astype(np.float64)
    key = lambda p: set(map(tuple, np.asarray(p).tolist()))
    kept_new = key(kept) - key(stored_a)
    assert key(stored_a) <= key(kept) and kept_new <= key(new32) and len(kept) == len(stored_a) + len(kept_new) and len(kept_new) > 0
    res = math.sqrt(1.0 / 20)
    by_voxel = {}
    for p in kept:
        by_voxel.setdefault(tuple(np.trunc(p).astype(int)), []).append(p)
    for p in new32:
        if tuple(p.tolist()) not in kept_new:
            mates = np.array(by_voxel[tuple(np.trunc(p).astype(int))])
            assert len(mates) >= 20 or (np.linalg.norm(mates - p, axis=1) < res).any()
    # (c) the same scans on the grown map: fewer END-NEW beams
    g2 = grown.Growth(n_beams)
    st2 = g2.Accumulate(scans, poses, cfg)
    ref2 = growth_ref.Growth(kept, 1.0, 4)
    assert st2 == ref2.call(cfg, pts, poses)[0]
    _same(g2, ref2)
    before, after = sum(s["n_end_new"] for s in st), sum(s["n_end_new"] for s in st2)
    a, b, c = box_figures(bx, cells, appeared, before, after)
    print("seed", TEST_SEED, "box cells", len(bx), "candidates", len(cells), "appeared", int(appeared.sum()), "(a)", round(a, 4), "(b)", round(b, 5),
          "(c)", round(c, 4), "END-NEW", before, "->", after, "kept of the appeared points", len(kept_new), "of", len(new))
    g.close()
    g2.close()
    rec = RECORDED[TEST_SEED]
    assert a > b  # otherwise the rule's defaults are wrong for this scene: say so, do not hide it in a threshold
    assert after < before
    assert a >= rec[0] / 2 and b <= 2 * rec[1] and c <= 2 * rec[2]
