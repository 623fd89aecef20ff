"""Map change evidence on the GPU (elm_evidence_*): every counter, every per-beam event count and every stats field against the numpy
mirror of the contract (tests/evidence_ref.py), exactly; a batch against the same jobs one by one; contended counters; the edge cases; the
walk against the ray cast's; every search index form; misuse; and on a map with a phantom box, that the box is what gets flagged and
that pruning removes it."""
import ctypes as C
import math

import numpy as np
import pytest

import evidence_ref
import ray_ref  # tests/ is on sys.path via conftest
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import (Context, EvidenceConfig, EvidenceRule, IcpMethod, RayCastConfig, Registration, RegistrationConfig, Scan,
                                        VoxelHashMap)

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
FIELDS = evidence_ref.FIELDS


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


def _stored(vm):
    return vm.Pointcloud() if not vm.Empty() else np.zeros((0, 3))


def _random_poses(T, n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    poses = np.empty((n, 4, 4))
    for h in range(n):
        poses[h] = np.eye(4)
        rpy = rng.uniform(-0.3, 0.3, 2)
        poses[h][:3, :3] = synth.rot_zyx(rpy[0], rpy[1], rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:3, 3] = T[:3, 3] + rng.uniform(-spread, spread, 3)
    return poses


def _check_one(vm, stored, vs, cfg, pts, T, ev=None):
    """One observation from zero, GPU == mirror: the cells, both counters, the per-beam events (resident order) and every stats field."""
    own = ev is None
    ev = vm.Evidence(cfg.sub) if own else ev
    ev.Reset()
    sc = Scan(vm.ctx, pts)
    res = sc.points()
    cells, through, hit, ref, ref_ev, _ = evidence_ref.mirror(stored, vs, cfg, [res], np.asarray(T)[None])
    st, events = ev.Accumulate(sc, T, cfg, events=True)
    t, h = ev.Counts()
    print(st, ref[0])
    assert np.array_equal(vm.FineCells(cfg.sub), cells)
    assert t.dtype == np.uint32 and h.dtype == np.uint32 and events.dtype == np.uint16
    assert st == ref[0]
    assert np.array_equal(events, ref_ev[0]), int(np.count_nonzero(events != ref_ev[0]))
    assert np.array_equal(t, through), int(np.count_nonzero(t != through))
    assert np.array_equal(h, hit), int(np.count_nonzero(h != hit))
    assert ev.Accumulate(sc, T, cfg) == st  # the stats do not depend on the events being asked for ...
    t2, h2 = ev.Counts()
    assert np.array_equal(t2, 2 * through) and np.array_equal(h2, 2 * hit)  # ... and a second observation adds to the first
    if own:
        ev.close()
    return st, events, t, h, res


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("world_name,vs", [("field", 1.0), ("field", 0.5), ("field", 0.3), ("lattice", 1.0), ("lattice", 0.5), ("lattice", 0.3)])
def test_exact_against_mirror(ctx, field300k, lattice300k, world_name, vs):
    world = field300k if world_name == "field" else lattice300k
    scan, T = synth.make_scan(world, 3001, seed=int(10 * vs))  # the worlds are centred on the origin
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    stored = vm.Pointcloud()
    poses = _random_poses(T, 5, seed=int(vs * 10) + 3)
    for sub in (1, 2, 4):
        ev = vm.Evidence(sub)
        origin = (0.4, -0.3, 0.25) if sub != 1 else (0.0, 0.0, 0.0)
        cfg = EvidenceConfig(sub=sub, origin=origin)
        for k, n in enumerate((1, 255, 256, 257, 3001)):
            st, events, t, h, _ = _check_one(vm, stored, vs, cfg, scan[:n], poses[k], ev)
        assert st["n_cast"] == 3001 and st["n_observing"] > 1500 and st["n_walked"] > 1000 and st["n_steps"] > 3001
        assert st["n_end_hit"] + st["n_end_free"] == st["n_observing"] and st["n_truncated"] == 0
        # make_scan draws map points through walls: plenty of through events to compare
        assert st["n_through_events"] > 0 and int(events.sum()) == st["n_through_events"] and int(t.sum()) == st["n_through_events"]
        assert int(h.sum()) == st["n_end_hit"]
        ev.close()
    # a short margin, a walk from the origin itself, another observing band
    _check_one(vm, stored, vs, EvidenceConfig(sub=4, min_range_m=0.0, obs_min_range_m=0.0, obs_max_range_m=25.0, end_margin_m=0.05,
                                              end_margin_frac=0.0, origin=(-0.2, 0.1, 0.3)), scan, poses[0])
    # the truth itself, where most end points lie in occupied cells
    st, _, _, h, _ = _check_one(vm, stored, vs, EvidenceConfig(sub=4), scan, T)
    assert st["n_end_hit"] > 500 and int(h.sum()) == st["n_end_hit"]


# ---------------------------------------------------------------- 2. batch = sum
def test_batch_is_the_sum_of_its_jobs(ctx, field300k, field_map):
    vm, stored = field_map
    scan, T = synth.make_scan(field300k, 2000, seed=5)
    sizes = (0, 1, 256, 257, 1000)
    lo = np.cumsum((0,) + sizes)
    scs = [Scan(ctx, scan[a:a + n]) for a, n in zip(lo, sizes)]
    jobs = scs + [scs[2]]  # the 256-point scan a second time, at another pose
    poses = _random_poses(T, len(jobs), seed=6, spread=1.5)
    poses[3], poses[4] = T, T  # two jobs at the truth, where the end points lie in the map: the hit counters are fed too
    cfg = EvidenceConfig(origin=(0.1, 0.0, -0.2))
    cells, through, hit, ref, _, _ = evidence_ref.mirror(stored, 1.0, cfg, [s.points() for s in jobs], poses)
    ev = vm.Evidence()
    got = ev.Accumulate(jobs, poses, cfg)
    t, h = ev.Counts()
    print(got, ref)
    assert got == ref and got[0] == dict.fromkeys(FIELDS, 0) and got[2] != got[5]
    assert np.array_equal(t, through) and np.array_equal(h, hit) and through.sum() > 0 and hit.sum() > 100
    ev.Reset()
    t0, h0 = ev.Counts()
    assert not t0.any() and not h0.any() and t0.shape == t.shape
    one_by_one = [ev.Accumulate(jobs[j], poses[j], cfg) for j in reversed(range(len(jobs)))][::-1]
    t1, h1 = ev.Counts()
    assert one_by_one == got and np.array_equal(t1, t) and np.array_equal(h1, h)
    # arrays instead of resident scans give the same counters; the batch adds to what is there
    ev.Accumulate([s.points() for s in jobs], poses, cfg)
    t2, h2 = ev.Counts()
    assert np.array_equal(t2, 2 * through) and np.array_equal(h2, 2 * hit)
    ev.Reset()
    assert not ev.Counts()[0].any() and not ev.Counts()[1].any()
    with pytest.raises(ElmError):
        ev.Accumulate(jobs, poses, cfg, events=True)
    ev.close()


# ---------------------------------------------------------------- 3. contention
def test_contended_counters_are_exact(ctx):
    """4 096 copies of one beam: +x from the centre of cell (0, 0, 0) of a 0.25 m lattice, L = 3, default config: the walk starts in cell 4
    (1.125 / 0.25) and leaves cells 4 .. 7 (at 1.125 .. 1.875 <= reach 2.0); cells 5 and 6 are occupied, and so is cell 12, where it ends."""
    vm = VoxelHashMap(1.0, 20, ctx)
    stored_in = np.array([(1.3, 0.1, 0.2), (1.6, 0.2, 0.1), (3.1, 0.1, 0.1), (0.1, -0.9, 0.1), (2.1, 0.9, 0.1)], np.float32)
    vm.AddPoints(stored_in)
    o = (0.125, 0.125, 0.125)
    beams = np.tile(np.array([(3.125, 0.125, 0.125)], np.float32), (4096, 1))
    cfg = EvidenceConfig(origin=o)
    cells = vm.FineCells(4)
    idx = {tuple(c): i for i, c in enumerate(cells.tolist())}
    expect_t, expect_h = np.zeros(len(cells), np.uint32), np.zeros(len(cells), np.uint32)
    expect_t[[idx[(5, 0, 0)], idx[(6, 0, 0)]]] = 4096
    expect_h[idx[(12, 0, 0)]] = 4096
    _, through, hit, ref, _, _ = evidence_ref.mirror(vm.Pointcloud(), 1.0, cfg, [beams], np.eye(4)[None])
    assert np.array_equal(through, expect_t) and np.array_equal(hit, expect_h)  # the mirror agrees with the hand count
    ev = vm.Evidence()
    sc = Scan(ctx, beams)
    runs = []
    for _ in range(2):
        ev.Reset()
        st, events = ev.Accumulate(sc, np.eye(4), cfg, events=True)
        t, h = ev.Counts()
        assert st == ref[0] and st["n_through_events"] == 2 * 4096 and st["n_end_hit"] == 4096 and st["n_steps"] == 4 * 4096
        assert (events == 2).all() and np.array_equal(t, expect_t) and np.array_equal(h, expect_h)
        runs.append((st, t, h))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # the same scan four times in one batch, on top
    ev.Accumulate([sc] * 4, np.stack([np.eye(4)] * 4), cfg)
    t, h = ev.Counts()
    assert np.array_equal(t, 5 * expect_t) and np.array_equal(h, 5 * expect_h)
    ev.close()


# ---------------------------------------------------------------- 4. edges
def test_edge_cases(ctx, lattice300k):
    world = lattice300k
    scan, T = synth.make_scan(world, 1500, seed=10)
    # an empty map: zero cells, accumulation runs and counts nothing
    empty = VoxelHashMap(1.0, 20, ctx)
    ev = empty.Evidence()
    st = ev.Accumulate([scan, scan[:10]], np.stack([T, T]))
    t, h = ev.Counts()
    assert t.shape == (0,) and h.shape == (0,) and ev.StalePoints().shape == (0,)
    assert st[0]["n_cast"] == 1500 and st[0]["n_end_hit"] == 0 and st[0]["n_end_free"] == st[0]["n_observing"] > 500
    assert st[0]["n_through_events"] == 0 and st[0]["n_steps"] > 1500
    _check_one(empty, np.zeros((0, 3)), 1.0, EvidenceConfig(), scan, T, ev)
    ev.close()
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(world)
    stored = vm.Pointcloud()
    ev = vm.Evidence()
    # an empty scan
    assert ev.Accumulate(np.zeros((0, 3), np.float32), T) == dict.fromkeys(FIELDS, 0)
    st0, e0 = ev.Accumulate(np.zeros((0, 3), np.float32), T, events=True)
    assert e0.shape == (0,) and not ev.Counts()[0].any()
    # zero-length, NaN and inf points between real ones: those lanes observe nothing, the other lanes of their waves are unchanged
    o = (0.5, 0.25, -0.125)
    nan, inf = float("nan"), float("inf")
    bad = np.array([o, (nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 2.0, -inf), o, (nan, nan, nan), (inf, -inf, 0.0)], np.float32)
    cfg = EvidenceConfig(origin=o)
    st_clean, ev_clean, t_clean, h_clean, res_clean = _check_one(vm, stored, 1.0, cfg, scan[:700], T, ev)
    mixed = np.concatenate([bad[:3], scan[:300], bad[3:5], scan[300:700], bad[5:]])
    st_mix, ev_mix, t_mix, h_mix, res_mix = _check_one(vm, stored, 1.0, cfg, mixed, T, ev)
    is_bad = ~np.isfinite(res_mix).all(1) | np.all(res_mix == np.array(o, np.float32), axis=1)
    assert is_bad.sum() == len(bad) and not ev_mix[is_bad].any()
    assert st_mix["n_cast"] == 700 and {k: v for k, v in st_mix.items()} == st_clean
    assert np.array_equal(t_mix, t_clean) and np.array_equal(h_mix, h_clean)
    key = np.dtype((np.void, 12))
    by_point = dict(zip(np.ascontiguousarray(res_clean).view(key).ravel().tolist(), ev_clean.tolist()))
    assert [by_point[k] for k in np.ascontiguousarray(res_mix[~is_bad]).view(key).ravel().tolist()] == ev_mix[~is_bad].tolist()
    # end points exactly on a cell face, both signs: the lower face belongs to the cell, the upper face to the next one.  Identity rotation and
    # a translation on the 0.25 m lattice: q = p + t is exact
    G = np.eye(4)
    G[:3, 3] = (3.0, -2.5, 1.25)
    cells = vm.FineCells(4)
    pick = np.unique(np.concatenate([cells[(cells[:, 0] > 20)][:40], cells[(cells[:, 0] < -20)][:40], cells[(cells[:, 1] < -20)][:40]]), axis=0)
    lower = (pick * 0.25 - G[:3, 3]).astype(np.float32)          # the cell's own corner: inside it
    upper = ((pick + 1) * 0.25 - G[:3, 3]).astype(np.float32)    # the opposite corner: the cell (+1, +1, +1)
    cfg0 = EvidenceConfig(obs_min_range_m=0.0, obs_max_range_m=1000.0)
    st, _, t, h, _ = _check_one(vm, stored, 1.0, cfg0, lower, G, ev)
    assert st["n_observing"] == len(pick) and st["n_end_hit"] == len(pick) and (pick < 0).any() and (pick > 0).any()
    codes = ray_ref.codes(cells)
    assert np.array_equal(np.flatnonzero(h), np.sort(np.searchsorted(codes, ray_ref.codes(pick)))) and (h[h > 0] == 1).all()
    st, _, t, h, _ = _check_one(vm, stored, 1.0, cfg0, upper, G, ev)
    assert st["n_end_hit"] == int(ray_ref.is_in(codes, ray_ref.codes(pick + 1)).sum())
    # axis-parallel beams (w = 0 on two axes), beams along cell faces and through cell corners (the tie rule)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (1, 1, 1), (-1, -1, -1),
                     (1, 0, 1), (0, -1, 1), (2, 1, 0), (1, 2, 2), (-3, 4, 0), (1, 1, -1)], np.float32) * 8.0
    events_seen = 0
    for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (0.25, -0.5, 0.0)):
        for margin in (1.0, 0.25):
            st, _, _, _, _ = _check_one(vm, stored, 1.0, EvidenceConfig(min_range_m=0.0, obs_min_range_m=0.0, origin=origin, end_margin_m=margin,
                                                                      end_margin_frac=0.0), axes + np.float32(origin), G, ev)
            assert st["n_observing"] == len(axes) == st["n_walked"]
            events_seen += st["n_through_events"]
    assert events_seen > 0
    # max_steps 1 and 7: truncation counted, the cells left before it counted
    full, _, _, _, _ = _check_one(vm, stored, 1.0, EvidenceConfig(), scan, T, ev)
    for ms in (1, 7):
        st, events, _, _, _ = _check_one(vm, stored, 1.0, EvidenceConfig(max_steps=ms), scan, T, ev)
        assert st["n_truncated"] > 300 and st["n_steps"] <= ms * st["n_walked"] and st["n_walked"] == full["n_walked"]
        assert st["n_through_events"] <= full["n_through_events"] and int(events.max()) <= ms
    assert full["n_truncated"] == 0
    # a scan entirely outside the observing band: cast, and nothing else
    ev.Reset()
    st = ev.Accumulate(scan, T, EvidenceConfig(obs_min_range_m=70.0, obs_max_range_m=80.0))
    assert st == dict(dict.fromkeys(FIELDS, 0), n_cast=1500) and not ev.Counts()[0].any() and not ev.Counts()[1].any()
    # the same call twice gives the same answer
    a = ev.Accumulate(scan, T)
    ta, ha = ev.Counts()
    ev.Reset()
    assert ev.Accumulate(scan, T) == a and np.array_equal(ev.Counts()[0], ta) and np.array_equal(ev.Counts()[1], ha)
    ev.close()


# ---------------------------------------------------------------- 5. the ray cast
def test_the_walk_agrees_with_the_ray_cast(ctx, field300k, field_map):
    """Same start, same steps: RayCast with the same min_range_m and max_steps and a max_range_m above every reach walks the same cells.
    reach is that of the beams that walk; a beam that does not walk (not observing, or reach <= min_range_m) has none: -inf below, so that
    no beam is left out of any check."""
    vm, stored = field_map
    scan, T = synth.make_scan(field300k, 3001, seed=21)
    pose = _random_poses(T, 1, seed=4, spread=0.5)[0]
    sc = Scan(ctx, scan)
    res = sc.points()
    ec = EvidenceConfig(origin=(0.1, -0.1, 0.2))
    rc = RayCastConfig(min_range_m=ec.min_range_m, max_range_m=100.0, max_steps=ec.max_steps, origin=tuple(ec.origin))
    ev = vm.Evidence()
    st, events = ev.Accumulate(sc, pose, ec, events=True)
    through, _ = ev.Counts()
    ray, arr = vm.RayCast(sc, pose[None], rc, ranges=True, cells=True, flags=True)
    flag, rin, rout, hc = arr["flag"][0], arr["range_in"][0], arr["range_out"][0], arr["cell"][0]
    assert st["n_truncated"] == 0 and ray[0]["n_truncated"] == 0 and rc.max_range_m > ec.obs_max_range_m
    L2, L, cast, _, _ = ray_ref.rays(ec, res, pose)
    obs = cast & (L2 >= ec.obs_min_range_m ** 2) & (L2 <= ec.obs_max_range_m ** 2)
    reach = L - np.fmax(ec.end_margin_m, ec.end_margin_frac * L)
    reach = np.where(obs & (reach > ec.min_range_m), reach, -np.inf)
    seen = events >= 1
    print("beams", len(res), "seen through", int(seen.sum()), "ray hits", int((flag == 1).sum()))
    assert seen.any()
    assert ((flag[seen] == 1) & (rin[seen] <= reach[seen])).all()
    assert seen[(flag == 1) & (rout <= reach)].all() and ((flag == 1) & (rout <= reach)).any()
    cells = vm.FineCells(4)
    k = np.searchsorted(ray_ref.codes(cells), ray_ref.codes(hc[seen]))
    assert np.array_equal(cells[k], hc[seen])
    assert (np.bincount(k, minlength=len(cells)) <= through).all()
    ev.close()


# ---------------------------------------------------------------- 6. index forms
@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled")])
def test_same_counters_under_every_index_form(monkeypatch, field300k, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    scan, T = synth.make_scan(field300k, 3000, seed=31)
    vm = VoxelHashMap(1.0, 20, c)
    vm.AddPoints(field300k)
    vm.BuildNeighbourhoods()
    poses = _random_poses(T, 3, seed=9, spread=1.0)
    jobs = [scan[:1000], scan[1000:1300], scan]
    scs = [Scan(c, j) for j in jobs]
    cfg = EvidenceConfig()
    cells, through, hit, ref, _, _ = evidence_ref.mirror(vm.Pointcloud(), 1.0, cfg, [s.points() for s in scs], poses)
    ev = vm.Evidence()
    assert ev.Accumulate(scs, poses, cfg) == ref
    t, h = ev.Counts()
    assert np.array_equal(t, through) and np.array_equal(h, hit) and through.sum() > 0
    ev.close()
    del vm
    c.close()


# ---------------------------------------------------------------- 7. misuse
def test_misuse_is_refused_and_the_context_stays_usable(ctx, field_map):
    vm, stored = field_map
    world = synth.make_world(30_000, seed=11)
    scan, T = synth.make_scan(world, 2048, seed=12)
    L = _lib.lib()
    T16 = np.ascontiguousarray(T.T).ravel()
    dp = T16.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.EvidenceStatsC * 2)()
    cfg = EvidenceConfig()
    small = VoxelHashMap(1.0, 30, ctx)
    small.AddPoints(world)
    ev = small.Evidence(4)
    sc = Scan(ctx, scan)

    def acc(c, e, s, pose=dp, cf=cfg):
        return L.elm_evidence_accumulate(c._h, e._h, s._h, pose, C.byref(cf), st, None)

    # cfg.sub must equal the object's
    assert acc(ctx, ev, sc, cf=EvidenceConfig(sub=2)) == INVALID
    ev2 = small.Evidence(2)
    assert acc(ctx, ev2, sc) == INVALID and acc(ctx, ev2, sc, cf=EvidenceConfig(sub=2)) == 0
    ev2.close()
    # a non-finite pose entry
    for bad in (float("nan"), float("inf")):
        B16 = T16.copy()
        B16[13] = bad
        assert acc(ctx, ev, sc, pose=B16.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    # map, scan and evidence of another context
    other = Context(0)
    osc = Scan(other, scan)
    omap = VoxelHashMap(1.0, 30, other)
    omap.AddPoints(world)
    out = C.c_void_p()
    assert L.elm_evidence_create(ctx._h, omap._handle(), 4, C.byref(out)) == INVALID and not out.value
    assert acc(ctx, ev, osc) == INVALID and acc(other, ev, osc) == INVALID
    hs = (C.c_void_p * 2)(sc._h.value, osc._h.value)
    two = np.concatenate([T16, T16])
    assert L.elm_evidence_accumulate_batch(ctx._h, ev._h, hs, two.ctypes.data_as(C.POINTER(C.c_double)), 2, C.byref(cfg), st) == INVALID
    n = C.c_size_t(0)
    assert L.elm_evidence_counts(other._h, ev._h, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_evidence_reset(other._h, ev._h) == INVALID
    rule = EvidenceRule()
    assert L.elm_evidence_stale_points(other._h, ev._h, C.byref(rule), None, 0, C.byref(n)) == INVALID
    # nothing was counted by any refused call
    assert not ev.Counts()[0].any() and not ev.Counts()[1].any()
    # a batch in flight
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx=ctx)
    reg.EnqueueBatch([sc], small, T[None])
    assert acc(ctx, ev, sc) == INVALID
    assert L.elm_evidence_counts(ctx._h, ev._h, None, None, 0, C.byref(n)) == INVALID and L.elm_evidence_reset(ctx._h, ev._h) == INVALID
    assert L.elm_evidence_create(ctx._h, small._handle(), 4, C.byref(out)) == INVALID
    reg.FinishBatch()
    # a communicator hook attached
    other.set_allreduce_hook(lambda p, n_, s: 0)
    oev_h = C.c_void_p()
    assert L.elm_evidence_create(other._h, omap._handle(), 4, C.byref(oev_h)) == UNSUPPORTED
    other.set_allreduce_hook(None)
    oev = omap.Evidence()
    other.set_allreduce_hook(lambda p, n_, s: 0)
    assert acc(other, oev, osc) == UNSUPPORTED and "one rank" in L.elm_last_error(other._h).decode()
    assert L.elm_evidence_counts(other._h, oev._h, None, None, 0, C.byref(n)) == UNSUPPORTED
    other.set_allreduce_hook(None)
    assert acc(other, oev, osc) == 0 and st[0].n_cast == 2048
    oev.close()
    del omap, osc
    other.close()
    # a device group's lead
    grp = Context.multi([0, 0])
    gvm = VoxelHashMap(1.0, 30, grp)
    gvm.AddPoints(world)
    assert L.elm_evidence_create(grp._h, gvm._handle(), 4, C.byref(out)) == UNSUPPORTED and "one rank" in L.elm_last_error(grp._h).decode()
    del gvm
    grp.close()
    # the Python layer: a rebuilt map invalidates its evidence; a closed object is refused
    tmp = VoxelHashMap(1.0, 30, ctx)
    tmp.AddPoints(world[:1000])
    tev = tmp.Evidence()
    tmp.AddPoints(world[1000:2000])
    with pytest.raises(ElmError):
        tev.Accumulate(sc, T)
    tev.close()
    with pytest.raises(ElmError):
        tev.Counts()
    with pytest.raises(ElmError):
        small.WithoutStale(vm.Evidence())
    # the context and the object are usable afterwards, with the answer of the mirror
    _check_one(small, small.Pointcloud(), 1.0, cfg, scan, T, ev)
    ev.close()


# ---------------------------------------------------------------- 8. it finds what is gone, and pruning removes it
# The mirror's figures for this scene (the contract, not the kernel), default rule, as recorded in DESIGN.md section 15:
# seed -> (a) share of the box's cells flagged, (b) share of flagged cells among the counted non-box cells, (c) through events after / before
RECORDED = {1: (0.8826, 0.000525, 0.6044), 2: (0.1904, 0.003513, 0.8663), 3: (0.4208, 0.002109, 0.8452)}
TEST_SEED = 1


def box_scene(vm_a, seed):
    """The phantom box (surfaces at 0.1 m spacing, 4 x 3 x 2.5 m, standing on the ground near the map's centre) and 12 poses on a ring of
    12 m around it, 1.8 m over the ground, each with its own yaw and a small tilt."""
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


def box_figures(cells_b, is_box, through, hit, events_before, events_after):
    """(a), (b), (c) from counters aligned with cells_b"""
    stale = evidence_ref.stale_cells(through, hit)
    counted = (through > 0) | (hit > 0)
    a = float(stale[is_box].mean())
    b = float(stale[~is_box & counted].mean())
    return a, b, events_after / events_before


def test_it_finds_what_is_gone_and_pruning_removes_it(ctx, field300k, field_map):
    vm_a, stored_a = field_map
    box, poses = box_scene(vm_a, TEST_SEED)
    vm_b = VoxelHashMap(1.0, 20, ctx)
    vm_b.AddPoints(np.concatenate([field300k, box]))
    stored_b = vm_b.Pointcloud()
    beams = synth.lidar_beams(32, 512)
    scans = [Scan(ctx, vm_a.RenderScan(P, beams)) for P in poses]  # what a sensor sees in the world WITHOUT the box
    cfg = EvidenceConfig()
    ev = vm_b.Evidence()
    st = ev.Accumulate(scans, poses, cfg)
    through, hit = ev.Counts()
    cells_b, ref_t, ref_h, ref_st, _, _ = evidence_ref.mirror(stored_b, 1.0, cfg, [s.points() for s in scans], poses)
    assert st == ref_st and np.array_equal(through, ref_t) and np.array_equal(hit, ref_h) and np.array_equal(vm_b.FineCells(4), cells_b)
    is_box = ~ray_ref.is_in(ray_ref.codes(vm_a.FineCells(4)), ray_ref.codes(cells_b))
    assert is_box.sum() > 200
    # pruning: the new map holds exactly B's unflagged points
    flags = ev.StalePoints()
    pruned = vm_b.WithoutStale(ev)
    assert flags.shape == (len(stored_b),) and flags.any()
    cell_of_pt = np.searchsorted(ray_ref.codes(cells_b), ray_ref.codes(np.floor(stored_b / 0.25)))
    assert np.array_equal(flags, evidence_ref.stale_cells(through, hit)[cell_of_pt])
    kept = pruned.Pointcloud()
    assert (pruned.voxel_size_, pruned.max_points_per_voxel_) == (1.0, 20) and pruned.ctx is ctx
    assert len(kept) == int((~flags).sum()) and set(map(tuple, kept.tolist())) == set(map(tuple, stored_b[~flags].tolist()))  # (d)
    ev_p = pruned.Evidence()
    st_p = ev_p.Accumulate(scans, poses, cfg)
    before, after = sum(s["n_through_events"] for s in st), sum(s["n_through_events"] for s in st_p)
    a, b, c = box_figures(cells_b, is_box, through, hit, before, after)
    print("seed", TEST_SEED, "box cells", int(is_box.sum()), "(a)", round(a, 4), "(b)", round(b, 5), "(c)", round(c, 4), "events", before, "->", after,
          "stale points", int(flags.sum()))
    ev.close()
    ev_p.close()
    rec = RECORDED[TEST_SEED]
    assert rec is not None, "no recorded figures"
    assert a > b  # otherwise the rule's defaults are wrong for this scene: say so, do not hide it in a threshold
    assert a >= rec[0] / 2 and b <= 2 * rec[1] and c <= 2 * rec[2]
