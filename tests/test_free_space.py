"""The free-space check on the GPU (elm_map_check_free_space): every count and the whole per-ray array against a numpy mirror written from
the contract in include/elimaloc_hip.h ("free-space check"), the fine occupancy against the stored points, the edge cases, every search
index form, the end test against the occupancy score where the two contracts coincide, the separation of wrong poses from the truth on the
field world, and the opt-in arguments of Relocalize / CallbackPointCloud."""
import ctypes as C
import math

import numpy as np
import pytest

from elimaloc_amd import _lib, synth
from elimaloc_amd.registration import (Context, FreeSpaceConfig, IcpMethod, Registration, RegistrationConfig, RelocConfig, Scan,
                                       VoxelHashMap)
from elimaloc_amd._lib import ElmError

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
FIELDS = ("n_counted", "n_pierced", "n_end_occupied", "n_supported", "n_samples", "n_hit_samples")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _codes(k):
    k = np.asarray(k, dtype=np.int64) + (1 << 20)
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def _in(occ, c):
    if occ.size == 0:
        return np.zeros(c.shape, bool)
    i = np.searchsorted(occ, c)
    return occ[np.minimum(i, occ.size - 1)] == c


def _transform(T, a):
    return np.stack([((T[r, 0] * a[:, 0] + T[r, 1] * a[:, 1]) + T[r, 2] * a[:, 2]) + T[r, 3] for r in range(3)], 1)


def mirror(stored, vs, cfg, scan, poses):
    """The contract, step by step, in float64 numpy.  stored: the map's stored points (DownloadPoints); scan: float32 points in the order
    the hits are wanted in.  Returns (list of stats dicts, hits uint16 [n_poses, n])."""
    cell = vs / cfg.sub
    step = cfg.step_m if cfg.step_m > 0.0 else cell / 2.0
    occ = np.unique(_codes(np.floor(stored.astype(np.float64) / cell)))
    p = scan.astype(np.float64)
    o = np.array(list(cfg.origin))
    d = p - o
    L2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        Ln = np.sqrt(L2)
        counted = (L2 >= cfg.min_range_m * cfg.min_range_m) & (L2 <= cfg.max_range_m * cfg.max_range_m) & (L2 > 0.0)
        reach = Ln - np.maximum(cfg.end_margin_m, cfg.end_margin_frac * Ln)
        K = np.where(counted & (reach > 0.0), np.minimum(np.floor(reach / step), float(cfg.max_samples)), 0.0)
        u = d / Ln[:, None]
    K = np.nan_to_num(K).astype(np.int64)
    k0 = int(math.floor(cfg.start_m / step)) + 1
    n_s = np.where(K >= k0, K - k0 + 1, 0)
    nb = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.int64)
    stats, hits_all = [], np.zeros((len(poses), len(p)), np.uint16)
    for h, T in enumerate(np.asarray(poses, dtype=np.float64)):
        hits = np.zeros(len(p), np.int64)
        for k in range(k0, int(K.max(initial=0)) + 1):
            act = np.flatnonzero(K >= k)
            s = float(k) * step
            a = o + u[act] * s
            f = np.floor(_transform(T, a) / cell)
            hits[act] += _in(occ, _codes(f))
        ci = np.flatnonzero(counted)
        fe = np.floor(_transform(T, p[ci]) / cell).astype(np.int64)
        end_occ = _in(occ, _codes(fe))
        sup = np.zeros(len(ci), bool)
        for off in nb:
            sup |= _in(occ, _codes(fe + off))
        stats.append(dict(n_counted=int(counted.sum()), n_pierced=int(np.count_nonzero(hits >= cfg.min_hits)),
                          n_end_occupied=int(end_occ.sum()), n_supported=int(sup.sum()), n_samples=int(n_s.sum()),
                          n_hit_samples=int(hits.sum())))
        hits_all[h] = np.minimum(hits, 65535)
    return stats, hits_all


def _strip(st):
    return {k: st[k] for k in FIELDS}


def _check(vm, vs, cfg, scan, poses):
    """GPU == mirror on a resident scan: every stats field and the whole hits array (resident order)."""
    sc = Scan(vm.ctx, scan)
    res = sc.points()
    stored = vm.Pointcloud() if not vm.Empty() else np.zeros((0, 3))
    ref, ref_hits = mirror(stored, vs, cfg, res, poses)
    got, hits = vm.CheckFreeSpace(sc, poses, cfg, hits=True)
    print([(_strip(g), r) for g, r in zip(got, ref)][:2])
    assert [_strip(g) for g in got] == ref
    assert hits.dtype == np.uint16 and hits.shape == ref_hits.shape and np.array_equal(hits, ref_hits)
    only = vm.CheckFreeSpace(sc, poses, cfg)
    assert only == got
    return got, hits, res


def _random_poses(T, n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    poses = np.empty((n, 4, 4))
    for h in range(n):
        poses[h] = np.eye(4)
        rpy = rng.uniform(-0.3, 0.3, 2)
        poses[h][:3, :3] = synth.rot_zyx(rpy[0], rpy[1], rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:3, 3] = T[:3, 3] + rng.uniform(-spread, spread, 3)
    poses[0] = T
    return poses


@pytest.fixture(scope="module")
def field300k():
    return synth.make_field_world(300_000, seed=4242)


@pytest.fixture(scope="module")
def lattice300k():
    return synth.make_world(300_000, seed=77)


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("world_name,vs,sub", [("field", 1.0, 4), ("field", 0.5, 2), ("field", 0.3, 4), ("lattice", 1.0, 1),
                                               ("lattice", 0.5, 4), ("lattice", 0.3, 2)])
def test_exact_against_mirror(ctx, field300k, lattice300k, world_name, vs, sub):
    world = field300k if world_name == "field" else lattice300k
    scan, T = synth.make_scan(world, 3001, seed=5 + sub)  # not a multiple of 256; the worlds are centred on the origin (negative coordinates)
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    poses = _random_poses(T, 19, seed=int(vs * 10) + sub)  # two pose blocks, the second one partial
    got, hits, _ = _check(vm, vs, FreeSpaceConfig(sub=sub), scan, poses)
    assert got[0]["n_counted"] > 1000 and got[0]["n_samples"] > 10 * got[0]["n_counted"] and hits.max() > 0
    # a non-zero origin, one-hit piercing, a shorter start
    _check(vm, vs, FreeSpaceConfig(sub=sub, origin=(0.4, -0.3, 0.25), min_hits=1, start_m=0.3, min_range_m=1.0), scan, poses[:3])


def test_hits_come_back_in_the_callers_order(ctx, lattice300k):
    scan, T = synth.make_scan(lattice300k, 2000, seed=3)
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(lattice300k)
    sc = Scan(ctx, scan)
    _, resident = vm.CheckFreeSpace(sc, T[None], hits=True)
    _, own = vm.CheckFreeSpace(scan, T[None], hits=True)
    ref = mirror(vm.Pointcloud(), 1.0, FreeSpaceConfig(), scan, T[None])[1]
    assert np.array_equal(own, ref) and np.array_equal(resident, mirror(vm.Pointcloud(), 1.0, FreeSpaceConfig(), sc.points(), T[None])[1])


# ---------------------------------------------------------------- 2. fine occupancy
def test_fine_cells_are_the_stored_points_cells(ctx, field300k):
    half = len(field300k) // 2
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(field300k[:half])
    scan, T = synth.make_scan(field300k, 500, seed=1)

    def expect(sub):
        f = np.floor(vm.Pointcloud() / (1.0 / sub)).astype(np.int64)
        return np.unique(f, axis=0).astype(np.int32)

    for sub in (4, 2):  # two tables on one map
        got = vm.FineCells(sub)
        assert got.dtype == np.int32 and np.array_equal(got, expect(sub))
        vm.CheckFreeSpace(scan, T[None], FreeSpaceConfig(sub=sub))
        assert np.array_equal(vm.FineCells(sub), got)
    n4 = len(vm.FineCells(4))
    vm.AddPoints(field300k[half:])  # the map is rebuilt: so is the table
    assert np.array_equal(vm.FineCells(4), expect(4)) and len(vm.FineCells(4)) > n4
    _check(vm, 1.0, FreeSpaceConfig(), scan, T[None])
    with pytest.raises(ElmError):
        vm.FineCells(3)
    assert VoxelHashMap(1.0, 20, ctx).FineCells(4).shape == (0, 3)


# ---------------------------------------------------------------- 3. edges
def test_edge_cases(ctx, lattice300k):
    world = lattice300k
    scan, T = synth.make_scan(world, 1500, seed=10)
    empty = VoxelHashMap(1.0, 20, ctx)
    got, hits, _ = _check(empty, 1.0, FreeSpaceConfig(), scan, _random_poses(T, 2, 1))
    assert all(g["n_pierced"] == 0 and g["n_supported"] == 0 and g["n_hit_samples"] == 0 and g["n_counted"] > 0 for g in got) and not hits.any()
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(world)
    assert vm.CheckFreeSpace(scan, np.zeros((0, 4, 4))) == []
    out, h0 = vm.CheckFreeSpace(scan, np.zeros((0, 4, 4)), hits=True)
    assert out == [] and h0.shape == (0, 1500)
    # points at L = 0 (the origin itself), beyond max_range_m, and shorter than the margins (K = 0)
    o = (0.5, 0.25, -0.125)
    odd = np.array([o, o, (200.0, 0.0, 0.0), (0.5, 0.25, 0.9), (0.5 + 1.5, 0.25, -0.125), (0.5, 0.25 - 2.5, -0.125)], np.float32)
    mixed = np.concatenate([odd, scan[:700]])
    cfg = FreeSpaceConfig(origin=o, min_range_m=0.0)
    got, hits, res = _check(vm, 1.0, cfg, mixed, _random_poses(T, 3, 2))
    at_origin = np.all(res == np.array(o, np.float32), axis=1)
    assert at_origin.sum() == 2 and not hits[:, at_origin].any()
    assert got[0]["n_counted"] == np.count_nonzero(((res.astype(np.float64) - np.array(o)) ** 2).sum(1) <= 2500.0) - 2
    # max_samples cuts K
    a, _, _ = _check(vm, 1.0, FreeSpaceConfig(max_samples=40), scan, T[None])
    b, _, _ = _check(vm, 1.0, FreeSpaceConfig(), scan, T[None])
    assert a[0]["n_samples"] < b[0]["n_samples"] and a[0]["n_samples"] <= 40 * a[0]["n_counted"]
    # saturation: a tiny step on a short scan through a solid block of the map
    rng = np.random.default_rng(5)
    block = VoxelHashMap(1.0, 30, ctx)
    block.AddPoints(rng.uniform(-6.0, 6.0, (400_000, 3)).astype(np.float32))
    short = np.array([(5.0, 0.0, 0.0), (0.0, -4.0, 1.0), (3.0, 3.0, 3.0), (30.0, 1.0, 0.0)], np.float32)
    cfg = FreeSpaceConfig(sub=1, step_m=2.0e-5, max_samples=65536, start_m=0.0, end_margin_m=0.5, end_margin_frac=0.0, min_range_m=0.0)
    got, hits, _ = _check(block, 1.0, cfg, short, np.eye(4)[None])
    assert hits.max() == 65535 and got[0]["n_hit_samples"] > 3 * 65535
    # min_hits 1 against 2
    one, _, _ = _check(vm, 1.0, FreeSpaceConfig(min_hits=1), scan, T[None])
    assert one[0]["n_pierced"] >= b[0]["n_pierced"] and one[0]["n_hit_samples"] == b[0]["n_hit_samples"]
    # the same call twice gives the same answer
    assert vm.CheckFreeSpace(scan, T[None]) == vm.CheckFreeSpace(scan, T[None])


# ---------------------------------------------------------------- 4. index forms
@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled"), ("ELM_CHECK", "free_wave")])
def test_same_answer_under_every_index_form(monkeypatch, field300k, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    scan, T = synth.make_scan(field300k, 3000, seed=31)
    vm = VoxelHashMap(1.0, 20, c)
    vm.AddPoints(field300k)
    vm.BuildNeighbourhoods()
    _check(vm, 1.0, FreeSpaceConfig(), scan, _random_poses(T, 5, 9))
    _, ok, _, _ = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), c).RunRegister(scan, vm, T)
    assert ok
    del vm
    c.close()


# ---------------------------------------------------------------- 5. the end test and the occupancy score
@pytest.mark.parametrize("vs", [1.0, 0.5])
def test_end_occupied_equals_the_score_where_the_contracts_coincide(ctx, lattice300k, vs):
    world = (lattice300k.astype(np.float64) + 500.0).astype(np.float32)  # every coordinate positive: floor and truncation agree
    scan, T = synth.make_scan(lattice300k, 4000, seed=8)
    T = T.copy()
    T[:3, 3] += 500.0
    poses = _random_poses(T, 20, seed=4, spread=2.0)
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    sc = Scan(ctx, scan)
    p = scan.astype(np.float64)
    assert min(_transform(P, p).min() for P in poses) > 0.0
    score = vm.ScorePoses(sc, poses, RelocConfig(score_max_range_m=50.0))
    got = vm.CheckFreeSpace(sc, poses, FreeSpaceConfig(sub=1, min_range_m=0.0, max_range_m=50.0))
    assert [g["n_end_occupied"] for g in got] == [int(s) for s in score] and score.max() > 1000


# ---------------------------------------------------------------- 6. it separates
@pytest.fixture(scope="module")
def field2m(ctx):
    world = synth.make_field_world(2_000_000, seed=2027)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    return world, vm, vm.Pointcloud()


def _truth_and_scan(world, vm, seed):
    """the truth of test_relocalize._case: ~1.8 m above the ground inside the inner part of the map, and an 8 192-point scan"""
    rng = np.random.default_rng(seed)
    T = synth.make_pose(world, seed)
    ext = float(np.max(np.abs(world[:, :2])))
    T[:2, 3] = rng.uniform(-0.4 * ext, 0.4 * ext, 2)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    assert found
    T[2, 3] = gz + 1.8
    scan, _ = synth.make_scan(world, 8192, seed=seed + 1, T_true=T)
    return T, scan


def _offset(vm, T, dist, yaw_deg, bearing):
    G = np.eye(4)
    G[:3, :3] = synth.rot_zyx(0.0, 0.0, math.radians(yaw_deg)) @ T[:3, :3]
    G[:2, 3] = T[:2, 3] + dist * np.array([math.cos(bearing), math.sin(bearing)])
    found, gz = vm.FindGroundHeight(G[:2, 3])
    G[2, 3] = (gz if found else T[2, 3] - 1.8) + 1.8  # re-seated 1.8 m over the ground
    return G


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_wrong_poses_pierce_the_map(ctx, field2m, seed):
    """synth.make_scan draws map points near the sensor without ray casting, so the test first takes the visible subset: the rays with no
    occupied sample at the truth (by the mirror).  On it the pierced share (min_hits 2) at every offset of 2 m or more must be at least
    10 x the share at the truth + 0.1.  The GPU's counts equal the mirror's exactly: that is the real check."""
    world, vm, stored = field2m
    T, scan = _truth_and_scan(world, vm, seed)
    cfg = FreeSpaceConfig()
    sc = Scan(ctx, scan)
    res = sc.points()
    _, h_truth = mirror(stored, 1.0, cfg, res, T[None])
    d2 = (res.astype(np.float64) ** 2).sum(1)
    counted = (d2 >= 4.0) & (d2 <= 2500.0)
    visible = counted & (h_truth[0] == 0)
    print("seed", seed, "counted", int(counted.sum()), "visible", int(visible.sum()))
    assert visible.sum() >= 1000, "the inputs of this test must keep 1 000 visible rays"
    vis = np.ascontiguousarray(res[visible])
    bearing = 0.7 + seed
    offsets = [("truth", T), ("0.5 m", _offset(vm, T, 0.5, 0.0, bearing)), ("2 m", _offset(vm, T, 2.0, 0.0, bearing)),
               ("5 deg", _offset(vm, T, 0.0, 5.0, bearing)), ("4 m + 90 deg", _offset(vm, T, 4.0, 90.0, bearing)),
               ("30 m + 40 deg", _offset(vm, T, 30.0, 40.0, bearing))]
    poses = np.stack([P for _, P in offsets])
    vsc = Scan(ctx, vis)
    ref, ref_hits = mirror(stored, 1.0, cfg, vsc.points(), poses)
    got, hits = vm.CheckFreeSpace(vsc, poses, cfg, hits=True)
    share = [r["n_pierced"] / r["n_counted"] for r in ref]
    print({name: round(s, 3) for (name, _), s in zip(offsets, share)})
    assert [_strip(g) for g in got] == ref and np.array_equal(hits, ref_hits)
    assert ref[0]["n_pierced"] == 0 and ref[0]["n_counted"] == int(visible.sum())
    for (name, _), s in zip(offsets, share):
        if name in ("2 m", "4 m + 90 deg", "30 m + 40 deg"):
            assert s >= 10.0 * share[0] + 0.1, (name, s, share[0])


# ---------------------------------------------------------------- 7. opt-in arguments
PARENT_KEYS = {"T0", "T", "score", "hyp_index", "is_success", "iterations", "fitness_score"}


def test_relocalize_opt_in(ctx, field300k):
    world = field300k
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    scan, T = synth.make_scan(world, 4096, seed=77)
    G = T.copy()
    G[:2, 3] += (1.0, -0.5)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    rc = RelocConfig(radius_xy_m=1.5, step_xy_m=0.5, yaw_range_deg=20.0, step_yaw_deg=5.0, top_k=4)
    plain = reg.Relocalize(scan, vm, G, rc)
    fs = FreeSpaceConfig(min_hits=1)
    with_fs = reg.Relocalize(scan, vm, G, rc, free_space=fs)
    assert all(set(c) == PARENT_KEYS for c in plain[4]) and len(plain[4]) == len(with_fs[4]) >= 1
    assert np.array_equal(plain[0], with_fs[0]) and plain[1:3] == with_fs[1:3] and np.array_equal(plain[3], with_fs[3])
    for a, b in zip(plain[4], with_fs[4]):
        assert set(b) == PARENT_KEYS | {"free_space"}
        assert all(np.array_equal(a[k], b[k]) for k in PARENT_KEYS)
        assert b["free_space"] == vm.CheckFreeSpace(scan, b["T"][None], fs)[0]
    from elimaloc_amd.registration import GlobalRelocConfig
    tilt = np.eye(4)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    tilt[2, 3] = T[2, 3] - gz
    gc = GlobalRelocConfig(x_min=T[0, 3] - 3.0, x_max=T[0, 3] + 3.0, y_min=T[1, 3] - 3.0, y_max=T[1, 3] + 3.0, step_yaw_deg=10.0, top_k=3,
                           score_min_height_m=-math.inf)
    g_plain = reg.RelocalizeGlobal(scan, vm, tilt, gc)
    g_fs = reg.RelocalizeGlobal(scan, vm, tilt, gc, free_space=fs)
    assert all(set(c) == PARENT_KEYS for c in g_plain[4]) and len(g_plain[4]) == len(g_fs[4])
    for a, b in zip(g_plain[4], g_fs[4]):
        assert all(np.array_equal(a[k], b[k]) for k in PARENT_KEYS)
        assert b["free_space"] == vm.CheckFreeSpace(scan, b["T"][None], fs)[0]


def test_one_rank_only(ctx):
    world = synth.make_world(30_000, seed=11)
    scan, T = synth.make_scan(world, 2048, seed=12)
    L = _lib.lib()
    poses = np.ascontiguousarray(T.T).ravel()
    cfg = FreeSpaceConfig()
    st = (_lib.FreeSpaceStatsC * 1)()

    def code(c, vm):
        sc = Scan(c, scan)
        return L.elm_map_check_free_space(c._h, vm._handle(), sc._h, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(cfg), st, None)

    grp = Context.multi([0, 0])
    gvm = VoxelHashMap(1.0, 30, grp)
    gvm.AddPoints(world)
    assert code(grp, gvm) == UNSUPPORTED and "one rank" in L.elm_last_error(grp._h).decode()
    del gvm
    grp.close()
    hc = Context(0)
    hc.set_allreduce_hook(lambda p, n, s: 0)
    hvm = VoxelHashMap(1.0, 30, hc)
    hvm.AddPoints(world)
    assert code(hc, hvm) == UNSUPPORTED
    hc.set_allreduce_hook(None)
    assert code(hc, hvm) == 0 and st[0].n_counted > 0
    del hvm
    hc.close()
