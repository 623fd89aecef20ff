"""Map ray casting on the GPU (elm_map_raycast): every count and every per-beam output against the numpy mirror of the contract
(tests/ray_ref.py), bit for bit; the walk checked as a walk and against dense sampling of the same rays; the edge cases; every search
index form; beam order; agreement with the free-space check where the two contracts meet; RenderScan and the separation of wrong poses
from the truth on the field world."""
import ctypes as C
import math

import numpy as np
import pytest

import ray_ref  # tests/ is on sys.path via conftest
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import Context, FreeSpaceConfig, RayCastConfig, Scan, VoxelHashMap

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
FIELDS = ray_ref.FIELDS
FACE_EPS = 1e-9   # samples closer than this to a cell face are decided by rounding, not geometry: left out (tests 2 and 6)
LEFT_OUT_CAP = 1e-4


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


def _strip(st):
    return {k: st[k] for k in FIELDS}


def _stored(vm):
    return vm.Pointcloud() if not vm.Empty() else np.zeros((0, 3))


def _same(got, arr, ref, ref_arr):
    assert [_strip(g) for g in got] == ref
    for k in ("flag", "cell", "range_in", "range_out"):
        assert arr[k].dtype == ref_arr[k].dtype and arr[k].shape == ref_arr[k].shape, k
        assert np.array_equal(arr[k], ref_arr[k]), (k, int(np.count_nonzero(arr[k] != ref_arr[k])))


def _check(vm, vs, cfg, beams, poses):
    """GPU == mirror on a resident scan: every stats field and every per-beam array (resident order), ranges bit for bit."""
    sc = Scan(vm.ctx, beams)
    res = sc.points()
    ref, ref_arr, _ = ray_ref.mirror(_stored(vm), vs, cfg, res, poses)
    got, arr = vm.RayCast(sc, poses, cfg, ranges=True, cells=True, flags=True)
    print([(_strip(g), r) for g, r in zip(got, ref)][:1])
    _same(got, arr, ref, ref_arr)
    assert vm.RayCast(sc, poses, cfg) == got  # the stats do not depend on the arrays asked for
    only_flags = vm.RayCast(sc, poses, cfg, flags=True)
    assert only_flags[0] == got and list(only_flags[1]) == ["flag"] and np.array_equal(only_flags[1]["flag"], arr["flag"])
    return got, arr, res


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


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("world_name,vs", [("field", 1.0), ("field", 0.5), ("field", 0.3), ("lattice", 1.0), ("lattice", 0.5), ("lattice", 0.3)])
def test_exact_against_mirror(ctx, field300k, lattice300k, world_name, vs):
    world = field300k if world_name == "field" else lattice300k
    scan, T = synth.make_scan(world, 3001, seed=int(10 * vs))  # not a multiple of 256; the worlds are centred on the origin
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    poses = _random_poses(T, 19, seed=int(vs * 10) + 3)  # more than one pose block of any size up to 16, the last one partial
    for sub in (1, 2, 4):
        origin = (0.4, -0.3, 0.25) if sub == 2 else (0.0, 0.0, 0.0)
        got, arr, _ = _check(vm, vs, RayCastConfig(sub=sub, origin=origin), scan, poses)
        assert got[0]["n_cast"] == 3001 and got[0]["n_hit"] > 1500 and got[0]["n_compared"] > 1000 and got[0]["n_steps"] > 3001
        assert (arr["range_out"][arr["flag"] == 1] >= arr["range_in"][arr["flag"] == 1]).all()
    # a short walk, a tight tolerance, another compared band
    _check(vm, vs, RayCastConfig(sub=4, min_range_m=0.0, max_range_m=30.0, cmp_min_range_m=0.0, cmp_max_range_m=25.0, tol_m=0.05, tol_frac=0.0,
                                 origin=(-0.2, 0.1, 0.3)), scan, poses[:3])


# ---------------------------------------------------------------- 2. the traversal is a traversal
def test_the_walk_is_a_walk_and_dense_sampling_agrees(ctx, field300k):
    vs, sub = 1.0, 4
    cell = vs / sub
    scan, T = synth.make_scan(field300k, 3001, seed=21)
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(field300k)
    cfg = RayCastConfig(sub=sub, max_range_m=60.0)
    sc = Scan(ctx, scan)
    res = sc.points()
    pose = T.copy()[None]  # near the truth, where most beams end on the map: a small turn and shift
    pose[0][:3, :3] = synth.rot_zyx(0.02, -0.03, 0.3) @ T[:3, :3]
    pose[0][:3, 3] += (0.37, -0.21, 0.1)
    ref, ref_arr, vis = ray_ref.mirror(_stored(vm), vs, cfg, res, pose, trace=True)
    got, arr = vm.RayCast(sc, pose, cfg, ranges=True, cells=True, flags=True)
    _same(got, arr, ref, ref_arr)
    occ = ray_ref.codes(vm.FineCells(sub))
    assert np.array_equal(occ, np.sort(occ))
    # (a) from the mirror's list of visited cells
    n = len(res)
    last = np.full((n, 3), np.iinfo(np.int64).min)
    tests = np.zeros(n, np.int64)
    for idx, cells in vis[0]:
        seen_before = tests[idx] > 0
        step = np.abs(cells[seen_before] - last[idx[seen_before]])
        assert (step.sum(1) == 1).all() and (step.max(1) == 1).all()  # one step on one axis
        is_hit = (arr["flag"][0][idx] == 1) & (cells == arr["cell"][0][idx]).all(1)
        # no cell of the search phase is occupied but the hit cell (with which the search phase ends)
        assert np.array_equal(ray_ref.is_in(occ, ray_ref.codes(cells)), is_hit)
        last[idx] = cells
        tests[idx] += 1
    hit = np.flatnonzero(arr["flag"][0] == 1)
    print("hit beams", hit.size, "steps", got[0]["n_steps"])
    assert hit.size > 1500 and ray_ref.is_in(occ, ray_ref.codes(arr["cell"][0][hit])).all()
    assert (last[hit] == arr["cell"][0][hit]).all() and int((tests[arr["flag"][0] > 0] - 1).sum()) == got[0]["n_steps"]
    # (b) independently of the walk: points every cell / 64 along [min_range, range_in) find no occupied cell
    _, _, _, s, w = ray_ref.rays(cfg, res, pose[0])
    total = left_out = 0
    for lo in range(0, hit.size, 128):
        b = hit[lo:lo + 128]
        cnt = np.ceil((arr["range_in"][0][b] - cfg.min_range_m) / (cell / 64.0)).astype(np.int64)
        which = np.repeat(np.arange(b.size), cnt)
        t = cfg.min_range_m + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)) * (cell / 64.0)
        assert (t < arr["range_in"][0][b][which]).all()
        q = (s + w[b][which] * t[:, None]) / cell
        f = np.floor(q)
        near = (np.minimum(q - f, 1.0 - (q - f)) * cell < FACE_EPS).any(1)
        total += t.size
        left_out += int(near.sum())
        assert not ray_ref.is_in(occ, ray_ref.codes(f[~near])).any()
    print("dense samples", total, "left out", left_out)
    assert total > 1_000_000 and left_out < LEFT_OUT_CAP * total


# ---------------------------------------------------------------- 3. edges
def test_edge_cases(ctx, lattice300k):
    world = lattice300k
    scan, T = synth.make_scan(world, 1500, seed=10)
    empty = VoxelHashMap(1.0, 20, ctx)
    got, arr, _ = _check(empty, 1.0, RayCastConfig(), scan, _random_poses(T, 2, 1))
    assert all(g["n_hit"] == 0 and g["n_miss"] == g["n_cast"] == 1500 and g["n_match"] == g["n_through"] == 0 for g in got)
    assert (arr["flag"] == 2).all() and (arr["range_in"] == -1.0).all() and not arr["cell"].any()
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(world)
    # no poses, no beams
    assert vm.RayCast(scan, np.zeros((0, 4, 4))) == []
    out, a0 = vm.RayCast(scan, np.zeros((0, 4, 4)), ranges=True, cells=True, flags=True)
    assert out == [] and a0["range_in"].shape == (0, 1500) and a0["cell"].shape == (0, 1500, 3) and a0["flag"].shape == (0, 1500)
    out, a0 = vm.RayCast(np.zeros((0, 3), np.float32), T[None], flags=True)
    assert _strip(out[0]) == dict.fromkeys(FIELDS, 0) and a0["flag"].shape == (1, 0)
    # zero-length beams (the origin itself) between real ones: flag 0, in no count
    o = (0.5, 0.25, -0.125)
    mixed = np.concatenate([np.array([o, o], np.float32), scan[:700]])
    got, arr, res = _check(vm, 1.0, RayCastConfig(origin=o), mixed, _random_poses(T, 3, 2))
    at_origin = np.all(res == np.array(o, np.float32), axis=1)
    assert at_origin.sum() == 2 and not arr["flag"][:, at_origin].any() and (arr["flag"][:, ~at_origin] > 0).all()
    assert got[0]["n_cast"] == 700 and (arr["range_in"][:, at_origin] == -1.0).all()
    # axis-parallel beams (w = 0 on two axes), beams along cell faces and through cell corners (the tie rule): the pose has an identity
    # rotation and a translation on the 0.25 m lattice, so origins and faces coincide exactly
    G = np.eye(4)
    G[:3, 3] = (3.0, -2.5, 1.25)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (1, 1, 1), (-1, -1, -1),
                     (1, 0, 1), (0, -1, 1), (2, 1, 0), (1, 2, 2), (-3, 4, 0), (1, 1, -1)], np.float32) * 8.0
    for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (0.25, -0.5, 0.0)):
        got, arr, _ = _check(vm, 1.0, RayCastConfig(min_range_m=0.0, max_range_m=40.0, origin=origin, cmp_min_range_m=0.0), axes + np.float32(origin),
                             G[None])
        assert got[0]["n_cast"] == len(axes) and got[0]["n_hit"] >= 6
    # a beam that starts inside an occupied cell: the hit is at min_range_m, after no step
    inside = vm.Pointcloud()[:200].astype(np.float32)
    D = np.eye(4)
    cfg = RayCastConfig(min_range_m=0.0, origin=(0.0, 0.0, 0.0))
    beams = np.array([(1.0, 0.5, 0.25)], np.float32)
    for q in inside[::40]:
        D[:3, 3] = q
        got, arr, _ = _check(vm, 1.0, cfg, beams, D[None])
        assert arr["flag"][0, 0] == 1 and arr["range_in"][0, 0] == 0.0 and got[0]["n_steps"] == 0
        assert np.array_equal(arr["cell"][0, 0], np.floor(q.astype(np.float64) / 0.25).astype(np.int32))
    # a run that reaches max_range_m (down into the ground from just above it), and max_steps small enough to truncate
    down = np.array([(0.0, 0.0, -1.0), (0.01, 0.0, -1.0)], np.float32)
    pc = vm.Pointcloud()
    fr = pc[:, :2] - np.floor(pc[:, :2])
    ground = pc[(pc[:, 2] < 0.5) & (fr > 0.2).all(1) & (fr < 0.8).all(1)][0]  # a ground point (z ~ 0.3) well inside its 1 m cell in x and y
    D[:3, 3] = ground + (0.0, 0.0, 0.3)
    got, arr, _ = _check(vm, 1.0, RayCastConfig(sub=1, min_range_m=0.0, max_range_m=0.4), down, D[None])
    assert got[0]["n_hit"] == 2 and (arr["range_out"] == 0.4).all()
    a, _, _ = _check(vm, 1.0, RayCastConfig(max_steps=6), scan, T[None])
    b, _, _ = _check(vm, 1.0, RayCastConfig(), scan, T[None])
    assert a[0]["n_truncated"] > 100 and b[0]["n_truncated"] == 0 and a[0]["n_hit"] < b[0]["n_hit"] and a[0]["n_steps"] <= 6 * 1500
    _check(vm, 1.0, RayCastConfig(max_steps=1), scan, T[None])
    # bad configurations
    for kw in [dict(min_range_m=3.0, max_range_m=2.0), dict(sub=3), dict(max_steps=0), dict(tol_m=-1.0), dict(cmp_min_range_m=5.0, cmp_max_range_m=4.0),
               dict(origin=(0.0, float("nan"), 0.0))]:
        with pytest.raises(ElmError):
            vm.RayCast(scan, T[None], RayCastConfig(**kw))
    bad = T.copy()
    bad[0, 3] = float("inf")
    with pytest.raises(ElmError):
        vm.RayCast(scan, bad[None])
    # the same call twice gives the same answer
    assert vm.RayCast(scan, T[None]) == vm.RayCast(scan, T[None])


def test_one_rank_only(ctx):
    world = synth.make_world(30_000, seed=11)
    scan, T = synth.make_scan(world, 2048, seed=12)
    L = _lib.lib()
    poses = np.ascontiguousarray(T.T).ravel()
    cfg = RayCastConfig()
    st = (_lib.RayCastStatsC * 1)()

    def code(c, vm):
        sc = Scan(c, scan)
        return L.elm_map_raycast(c._h, vm._handle(), sc._h, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(cfg), st, None, None, None, None)

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
    assert code(hc, hvm) == 0 and st[0].n_cast == 2048 and st[0].n_hit > 0
    del hvm
    hc.close()


# ---------------------------------------------------------------- 4. index forms (and the pose block: the same outputs for every size)
@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled"), ("ELM_CHECK", "ray_poses=1"), ("ELM_CHECK", "ray_poses=4"),
                                 ("ELM_CHECK", "ray_poses=16")])
def test_same_answer_under_every_index_form(monkeypatch, field300k, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    scan, T = synth.make_scan(field300k, 3000, seed=31)
    vm = VoxelHashMap(1.0, 20, c)
    vm.AddPoints(field300k)
    vm.BuildNeighbourhoods()
    _check(vm, 1.0, RayCastConfig(), scan, _random_poses(T, 19, 9))
    del vm
    c.close()


# ---------------------------------------------------------------- 5. order
def test_arrays_come_back_in_the_callers_order(ctx, lattice300k):
    scan, T = synth.make_scan(lattice300k, 2000, seed=3)
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(lattice300k)
    sc = Scan(ctx, scan)
    assert not np.array_equal(sc.points(), scan)  # the resident order is not the caller's
    cfg = RayCastConfig()
    st_res, resident = vm.RayCast(sc, T[None], cfg, ranges=True, cells=True, flags=True)
    st_own, own = vm.RayCast(scan, T[None], cfg, ranges=True, cells=True, flags=True)
    ref_own = ray_ref.mirror(vm.Pointcloud(), 1.0, cfg, scan, T[None])
    ref_res = ray_ref.mirror(vm.Pointcloud(), 1.0, cfg, sc.points(), T[None])
    _same(st_own, own, ref_own[0], ref_own[1])
    _same(st_res, resident, ref_res[0], ref_res[1])
    assert st_own == st_res and not np.array_equal(own["range_in"], resident["range_in"])


# ---------------------------------------------------------------- 6. the free-space check
def test_free_space_samples_before_the_hit_are_free(ctx, field300k):
    """The free-space check's samples q = R (o + u k step) + t below range_in lie in cells the walk has tested and found empty.  The two
    calls round differently (R (o + u s) + t against (R o + t) + (R u) s), so samples within 1e-9 m of a cell face are left out."""
    vs, cell = 1.0, 0.25
    scan, T = synth.make_scan(field300k, 3001, seed=61)
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(field300k)
    sc = Scan(ctx, scan)
    res = sc.points()
    pose = _random_poses(T, 2, seed=8, spread=1.0)[1]
    fs, rc = FreeSpaceConfig(), RayCastConfig()  # samples start beyond 1 m, the walk starts at 1 m
    assert fs.start_m == rc.min_range_m and fs.sub == rc.sub and rc.max_range_m > fs.max_range_m
    ref, ref_arr, _ = ray_ref.mirror(vm.Pointcloud(), vs, rc, res, pose[None])
    got, arr = vm.RayCast(sc, pose[None], rc, ranges=True, cells=True, flags=True)
    _same(got, arr, ref, ref_arr)
    _, hits = vm.CheckFreeSpace(sc, pose[None], fs, hits=True)
    # the free-space contract's samples, from the header
    occ = ray_ref.occupancy(vm.Pointcloud(), cell)
    p = res.astype(np.float64)
    L2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    Ln = np.sqrt(L2)
    counted = (L2 >= fs.min_range_m ** 2) & (L2 <= fs.max_range_m ** 2)
    step = cell / 2.0
    reach = Ln - np.maximum(fs.end_margin_m, fs.end_margin_frac * Ln)
    K = np.where(counted & (reach > 0.0), np.minimum(np.floor(reach / step), float(fs.max_samples)), 0.0).astype(np.int64)
    k0 = int(math.floor(fs.start_m / step)) + 1
    u = p / Ln[:, None]
    rin = np.where(arr["flag"][0] == 1, arr["range_in"][0], np.inf)  # a beam that missed: all its samples
    assert not (arr["flag"][0] == 3).any()
    mine, beyond, clean = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64), np.ones(len(p), bool)
    total = left_out = 0
    for k in range(k0, int(K.max()) + 1):
        act = np.flatnonzero(K >= k)
        sd = float(k) * step
        a = u[act] * sd
        q = np.stack([((pose[r, 0] * a[:, 0] + pose[r, 1] * a[:, 1]) + pose[r, 2] * a[:, 2]) + pose[r, 3] for r in range(3)], 1) / cell
        f = np.floor(q)
        o_k = ray_ref.is_in(occ, ray_ref.codes(f))
        near = (np.minimum(q - f, 1.0 - (q - f)) * cell < FACE_EPS).any(1)
        before = sd < rin[act]
        total += int(before.sum())
        left_out += int((before & near).sum())
        assert not (o_k & before & ~near).any(), k
        clean[act[before & near]] = False
        mine[act] += o_k
        beyond[act] += o_k & ~before
    print("samples below range_in", total, "left out", left_out)
    assert total > 100_000 and left_out < LEFT_OUT_CAP * total
    assert np.array_equal(hits[0], np.minimum(mine, 65535).astype(np.uint16))  # GPU free-space check == its contract
    assert np.array_equal(mine[clean], beyond[clean]) and mine.sum() > 1000     # ... and counts only samples at or beyond range_in


# ---------------------------------------------------------------- 7. it renders and it separates
@pytest.fixture(scope="module")
def field2m(ctx):
    world = synth.make_field_world(2_000_000, seed=2027)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    return world, vm, vm.Pointcloud()


def _truth(world, vm, seed):
    """the truth of test_free_space's separation test: ~1.8 m above the ground inside the inner part of the map"""
    rng = np.random.default_rng(seed)
    T = synth.make_pose(world, seed)
    ext = float(np.max(np.abs(world[:, :2])))
    T[:2, 3] = rng.uniform(-0.4 * ext, 0.4 * ext, 2)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    assert found
    T[2, 3] = gz + 1.8
    return T


def _offset(vm, T, dist, yaw_deg, bearing):
    G = np.eye(4)
    G[:3, :3] = synth.rot_zyx(0.0, 0.0, math.radians(yaw_deg)) @ T[:3, :3]
    G[:2, 3] = T[:2, 3] + dist * np.array([math.cos(bearing), math.sin(bearing)])
    found, gz = vm.FindGroundHeight(G[:2, 3])
    G[2, 3] = (gz if found else T[2, 3] - 1.8) + 1.8  # re-seated 1.8 m over the ground
    return G


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_it_renders_and_it_separates(ctx, field2m, seed):
    """Mirror figures of this test (2 M-point field world, 32 x 512 beams; seeds 11 / 12 / 13), as recorded in DESIGN.md section 14:
    see the table there.  The assertions are the issue's: RenderScan == the mirror's pick; the rendered scan's pierced share at the truth
    below a quarter of make_scan's; MATCH at the truth strictly above MATCH at every wrong pose."""
    world, vm, stored = field2m
    T = _truth(world, vm, seed)
    beams = synth.lidar_beams(32, 512)
    cfg = RayCastConfig()
    # (a) RenderScan without noise is the mirror's pick, beam for beam
    _, ref_arr, _ = ray_ref.mirror(stored, 1.0, cfg, beams, T[None])
    bi, si = ray_ref.render_pick(stored, 1.0, cfg, beams, T, ref_arr["cell"][0], ref_arr["flag"][0])
    pts, beam_idx, map_idx = vm.RenderScan(T, beams, cfg, return_index=True)
    assert len(bi) > 8000 and np.array_equal(beam_idx, bi) and np.array_equal(map_idx, si)
    q = stored[si] - T[:3, 3]
    R = T[:3, :3]
    local = np.stack([(q[:, 0] * R[0, j] + q[:, 1] * R[1, j]) + q[:, 2] * R[2, j] for j in range(3)], 1).astype(np.float32)
    assert pts.dtype == np.float32 and np.array_equal(pts, local) and np.array_equal(vm.RenderScan(T, beams, cfg), pts)
    # (b) the rendered scan respects occlusion: its rays pierce the map far less than make_scan's at the same pose
    rendered = vm.RenderScan(T, beams, cfg, noise=0.01, seed=seed)
    assert rendered.shape == pts.shape and np.abs(rendered - pts).max() < 0.1 and not np.array_equal(rendered, pts)
    drawn, _ = synth.make_scan(world, 16384, seed=seed + 1, T_true=T)
    fs = FreeSpaceConfig()
    p_r = vm.CheckFreeSpace(rendered, T[None], fs)[0]
    p_d = vm.CheckFreeSpace(drawn, T[None], fs)[0]
    print("seed", seed, "pierced share: rendered", round(p_r["pierced_share"], 4), "of", p_r["n_counted"], "make_scan", round(p_d["pierced_share"], 4),
          "of", p_d["n_counted"])
    assert p_r["n_counted"] > 4000 and p_d["n_counted"] > 4000
    assert p_r["pierced_share"] < p_d["pierced_share"] / 4.0
    # (c) the expected ranges separate the truth from wrong poses
    bearing = 0.7 + seed
    offsets = [("truth", T), ("0.5 m", _offset(vm, T, 0.5, 0.0, bearing)), ("2 m", _offset(vm, T, 2.0, 0.0, bearing)),
               ("5 deg", _offset(vm, T, 0.0, 5.0, bearing)), ("4 m + 90 deg", _offset(vm, T, 4.0, 90.0, bearing))]
    poses = np.stack([P for _, P in offsets])
    sc = Scan(ctx, rendered)
    ref, ref_arr, _ = ray_ref.mirror(stored, 1.0, cfg, sc.points(), poses)
    got, arr = vm.RayCast(sc, poses, cfg, ranges=True, cells=True, flags=True)
    _same(got, arr, ref, ref_arr)
    share = {name: (r["n_match"] / r["n_compared"], r["n_through"] / r["n_compared"], r["n_front"] / r["n_compared"]) for (name, _), r in zip(offsets, ref)}
    print("seed", seed, "match / through / front:", {k: tuple(round(x, 3) for x in v) for k, v in share.items()}, "compared", ref[0]["n_compared"])
    assert ref[0]["n_compared"] > 4000
    for name, _ in offsets[1:]:
        assert share["truth"][0] > share[name][0], (name, share)
