"""The rolling local map and the LiDAR odometry on the GPU.

The primitive (elm_map_build_device_from), byte for byte: against elm_map_build_device fed the mirror's drop / xyz (tests/local_map_ref.py),
against elm_map_build of P, against the mirror map -- Pointcloud(), keys, counts and info(), in order -- with the stats equal to the
mirror's counts, over the scan sizes, job tables, poses, bases and keep variants of tests/local_map_cases.py; repeats; one GICP
registration under ELM_GRID=tiled and ELM_KERNEL=lists; the refusals that need a device, each followed by a correct build.

The loop (LidarOdometry) on the fixed inputs: against the same loop written here from the host primitives (Pointcloud(), the mirror's
sources, elm_map_build_device with host arrays, RunRegisterBatch) in pose bytes, iterations and is_success; against the oracle's loop
(tests/golden/local_map_loop.npz) within the HIP-vs-oracle tolerance of tests/test_gpu_parity.py; the rules at their boundaries."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import build_cases  # tests/ is on sys.path via conftest
import build_ref
import local_map_cases as cases
import local_map_ref as ref
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import Context, IcpMethod, LidarOdometry, OdometryConfig, Registration, RegistrationConfig, Scan, VoxelHashMap
from test_gpu_parity import POSE_TOL_M, POSE_TOL_RAD  # the project's HIP-vs-oracle pose tolerance: 1e-4 m / 1e-5 rad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5
INFO = ("n_input_points", "n_points", "n_voxels", "hash_capacity", "voxel_size", "max_points_per_voxel", "device_bytes")
STATS = ("n_base_kept", "n_base_dropped", "n_scan_points", "n_points", "n_voxels")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _read(vm):
    """what the contract compares: the stored points, the voxels' keys and counts, the info fields"""
    pts = vm.Pointcloud()
    keys, counts = vm.Voxels()[:2]
    mi = vm.info()
    return pts, keys, counts, tuple(getattr(mi, f) for f in INFO)


def _same_maps(a, b):
    assert a[3] == b[3], (a[3], b[3])
    assert a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes()  # (bytes: -0.0 is not 0.0 here)
    assert np.array_equal(a[1], b[1]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


def _same_content(a, b):
    """_same_maps but for device_bytes: a registration in between has built the map's search index"""
    _same_maps(a[:3] + (a[3][:6],), b[:3] + (b[3][:6],))


def _as_map(ctx, h, vs, cap):
    vm = VoxelHashMap(vs, cap, ctx)
    vm._h, vm._derived = h, True
    return vm


def _host_built(ctx, pts, vs, cap, device=False):
    vm = VoxelHashMap(vs, cap, ctx, device_build=device)
    vm.AddPoints(pts)
    vm._handle()
    return vm


def _derived(ctx, base, drop, extra, vs, cap):
    """elm_map_build_device with host arrays"""
    extra = np.ascontiguousarray(extra, dtype=np.float32).reshape(-1, 3)
    h = C.c_void_p()
    dptr = None if drop is None else np.ascontiguousarray(drop, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    rc = _lib.lib().elm_map_build_device(ctx._h, base._handle() if base is not None else None, dptr,
                                         extra.ctypes.data_as(C.POINTER(C.c_float)), len(extra), vs, cap, C.byref(h))
    assert rc == 0, _lib.lib().elm_last_error(ctx._h).decode()
    return _as_map(ctx, h, vs, cap)


def _call_from(ctx, base, keep, scans, poses, vs, cap):
    """elm_map_build_device_from itself -> (status, handle, stats dict)"""
    src = _lib.BuildSourcesC()
    src.base = base._handle() if base is not None else None
    src.keep_within = 0 if keep is None else 1
    if keep is not None:
        src.keep_center = (C.c_double * 3)(*[float(x) for x in keep[0]])
        src.keep_radius_m = float(keep[1])
    n = len(scans)
    hs = (C.c_void_p * max(n, 1))(*[s._h.value for s in scans])
    P = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)
    src.scans = hs
    src.poses16 = P.ctypes.data_as(C.POINTER(C.c_double)) if n else None
    src.n_jobs = n
    st = _lib.BuildSourcesStatsC()
    h = C.c_void_p(1)
    rc = _lib.lib().elm_map_build_device_from(ctx._h, C.byref(src), vs, cap, C.byref(h), C.byref(st))
    if rc != 0:
        assert h.value is None  # *out is NULL after a refusal
    return rc, h, {k: int(getattr(st, k)) for k in STATS}


def _resident(ctx, name, cache={}):
    """the job table `name` as resident scans (equal keys share one Scan), their resident points and the poses"""
    pts, poses, keys = cases.jobs(name)
    scans = []
    for p, k in zip(pts, keys):
        if (id(ctx), k) not in cache:
            cache[(id(ctx), k)] = Scan(ctx, p)
        scans.append(cache[(id(ctx), k)])
    return scans, [s.points() for s in scans], poses


def _check_primitive(ctx, base, keep, scans, scan_pts, poses, vs, cap):
    """device producers == host arrays == host build of P == mirror, and the stats; -> the device map's read-back"""
    base_pts = base.Pointcloud() if base is not None else np.zeros((0, 3))
    (mp, mk, mc), mstats = ref.build(base_pts, keep, scan_pts, poses, vs, cap)
    P, drop, xyz = ref.input_points(base_pts, keep, scan_pts, poses)
    rc, h, stats = _call_from(ctx, base, keep, scans, poses, vs, cap)
    assert rc == 0, _lib.lib().elm_last_error(ctx._h).decode()
    got = _read(_as_map(ctx, h, vs, cap))
    print("base", len(base_pts), "keep", keep, "jobs", [len(p) for p in scan_pts], "->", stats)
    assert stats == mstats
    _same_maps(got, _read(_derived(ctx, base, drop if base is not None else None, xyz, vs, cap)))
    _same_maps(got, _read(_host_built(ctx, P, vs, cap)))
    assert np.array_equal(got[0], mp) and np.array_equal(got[1], mk) and np.array_equal(got[2], mc)
    assert got[3][:3] == (len(P), len(mp), len(mk)) and got[3][4:6] == (vs, cap)
    return got


# ---------------------------------------------------------------- the primitive
def test_a_scan_in_resident_order_stays_where_it_is(ctx):
    """what lets the CPU loop on the oracle and the GPU loop insert the same points in the same order"""
    for n in cases.SCAN_SIZES:
        p = cases.scan_points(n)
        assert np.array_equal(Scan(ctx, p).points(), p), n
    _, scans = cases.loop_inputs()
    assert np.array_equal(Scan(ctx, scans[3]).points(), scans[3])
    raw = np.random.default_rng(3).uniform(-3.5, 3.5, size=(1025, 3)).astype(np.float32)
    assert np.array_equal(Scan(ctx, raw).points(), cases.in_resident_order(raw))


@pytest.mark.parametrize("name", list(cases.JOBS))
def test_from_scans_alone(ctx, name):
    scans, pts, poses = _resident(ctx, name)
    _check_primitive(ctx, None, None, scans, pts, poses, cases.VOXEL, cases.CAP)


@pytest.fixture(scope="module")
def bases(ctx):
    cloud = cases.base_cloud()
    return {"host": _host_built(ctx, cloud, 1.0, 30), "device": _host_built(ctx, cloud, 1.0, 30, device=True),
            "vs05": _host_built(ctx, cloud, 0.5, 30)}


@pytest.mark.parametrize("which", ["host", "device", "vs05"])
@pytest.mark.parametrize("keep", [None, ([0.5, -0.25, 0.25], 2.5)])
@pytest.mark.parametrize("name", ["one_257", "five_mixed", "zero_middle"])
def test_on_a_resident_base(ctx, bases, which, keep, name):
    """a host-built base, a device-built base, a base of another voxel size (0.5 -> 1.0)"""
    base = bases[which]
    before = _read(base)
    scans, pts, poses = _resident(ctx, name)
    _check_primitive(ctx, base, keep, scans, pts, poses, 1.0, 30)
    _same_maps(_read(base), before)  # the base is not modified


def test_keep_variants(ctx, bases):
    base = bases["host"]
    stored = base.Pointcloud()
    scans, pts, poses = _resident(ctx, "two_mixed")
    # radius 0 with the centre on a stored point keeps exactly that point
    centre = stored[1234]
    got = _check_primitive(ctx, base, (centre, 0.0), [], [], [], 1.0, 30)
    assert got[0].tolist() == [centre.tolist()]
    _check_primitive(ctx, base, (centre, 0.0), scans, pts, poses, 1.0, 30)
    # a radius that drops everything, without and with jobs
    got = _check_primitive(ctx, base, ([100.0, 0.0, 0.0], 1.0), [], [], [], 1.0, 30)
    assert len(got[0]) == 0 and got[3][:3] == (0, 0, 0)
    _check_primitive(ctx, base, ([100.0, 0.0, 0.0], 1.0), scans, pts, poses, 1.0, 30)
    # keep everything: by keep_within = 0, by a sphere around it all, and without jobs (the base's own bytes)
    got = _check_primitive(ctx, base, None, [], [], [], 1.0, 30)
    assert np.array_equal(got[0], stored)
    _same_maps(_check_primitive(ctx, base, ([0.0, 0.0, 0.0], 50.0), scans, pts, poses, 1.0, 30),
               _check_primitive(ctx, base, None, scans, pts, poses, 1.0, 30))
    # an empty base with a sphere; nothing at all
    empty = _host_built(ctx, np.zeros((0, 3), np.float32), 1.0, 30)
    _check_primitive(ctx, empty, ([0.0, 0.0, 0.0], 5.0), scans, pts, poses, 1.0, 30)
    got = _check_primitive(ctx, None, None, [], [], [], 1.0, 30)
    assert len(got[0]) == 0


def test_the_hand_worked_thresholds(ctx):
    """radius 5 about the origin: (3, 4, 0) stays (25 <= 25), (3, nextafter32(4), 0) goes; float32 ties, -0.0 and a voxel face"""
    base = _host_built(ctx, cases.THRESHOLD_POINTS, 1.0, 30)
    assert np.array_equal(base.Pointcloud(), cases.THRESHOLD_POINTS.astype(np.float64))  # one voxel each: stored in input order
    got = _check_primitive(ctx, base, cases.THRESHOLD_KEEP, [], [], [], 1.0, 30)
    assert np.array_equal(got[0], cases.THRESHOLD_POINTS[np.array(cases.THRESHOLD_KEPT)].astype(np.float64))
    tie = Scan(ctx, cases.TIE_POINTS)
    got = _check_primitive(ctx, None, None, [tie], [tie.points()], [cases.TIE_POSE], 1.0, 30)
    want = ref.transform(tie.points(), cases.TIE_POSE)
    assert sorted(map(tuple, want.tolist())) == sorted(map(tuple, cases.TIE_EXPECTED.tolist()))
    assert got[0].tobytes() == build_ref.build(want, 1.0, 30)[0].tobytes()


def test_a_contended_build_repeats_byte_for_byte(ctx, bases):
    scans, pts, poses = _resident(ctx, "five_mixed")
    runs = []
    for _ in range(5):
        rc, h, stats = _call_from(ctx, bases["device"], ([0.5, -0.25, 0.25], 3.0), scans, poses, 1.0, 30)
        assert rc == 0
        runs.append((_read(_as_map(ctx, h, 1.0, 30)), stats))
    for r, st in runs[1:]:
        _same_maps(r, runs[0][0])
        assert r[2].tobytes() == runs[0][0][2].tobytes() and st == runs[0][1]


@pytest.mark.parametrize("env", [("ELM_GRID", "tiled"), ("ELM_KERNEL", "lists")])
def test_a_gicp_registration_on_the_result(monkeypatch, env):
    """the map of the device producers and the host-path map of the same points: pose bytes, iterations and flags"""
    monkeypatch.setenv(*env)
    c = Context(0)
    poses, scans = cases.loop_inputs()
    res = [Scan(c, s) for s in scans[:4]]
    dev = VoxelHashMap(1.0, 30, c, device_index=True).UpdatedFromScans(res[:3], poses[:3])
    P = ref.input_points(np.zeros((0, 3)), None, [s.points() for s in res[:3]], poses[:3])[0]
    host = _host_built(c, P, 1.0, 30)
    _same_maps(_read(dev), _read(host))
    out = []
    for vm in (dev, host):
        vm.CalPointCovAll(0.4)
        r = Registration(RegistrationConfig(icp_method=IcpMethod.GICP, **cases.LOOP_REG), c).RunRegisterBatch([res[3]], vm, [poses[2]])[0]
        out.append((r["T"].tobytes(), r["iterations"], r["is_success"], r["gate"], r["fitness_score"], r["n_corr_last"]))
    print(env, out[0][1:])
    assert out[0] == out[1] and out[0][1] > 0
    c.close()


def test_updated_from_scans_wrapper(ctx, bases):
    base = bases["device"]
    scans, pts, poses = _resident(ctx, "two_mixed")
    keep = ([0.5, -0.25, 0.25], 2.5)
    up, stats = base.UpdatedFromScans(scans, poses, keep_center=keep[0], keep_radius=keep[1], stats=True)
    assert up._derived and up.device_build_ and (up.voxel_size_, up.max_points_per_voxel_, up.ctx) == (1.0, 30, ctx)
    (mp, mk, mc), mstats = ref.build(base.Pointcloud(), keep, pts, poses, 1.0, 30)
    assert stats == mstats and np.array_equal(up.Pointcloud(), mp) and np.array_equal(up.Voxels()[0], mk)
    alone = VoxelHashMap(1.0, 30, ctx).UpdatedFromScans(scans, poses)
    assert np.array_equal(alone.Pointcloud(), ref.build(np.zeros((0, 3)), None, pts, poses, 1.0, 30)[0][0])
    with pytest.raises(ElmError):
        base.UpdatedFromScans(scans, poses[:1])
    with pytest.raises(ElmError):
        base.UpdatedFromScans(scans, poses, keep_center=[0, 0, 0])
    with pytest.raises(ElmError):
        base.UpdatedFromScans([pts[0], pts[1]], poses)  # resident scans only


# ---------------------------------------------------------------- refusals with a device
def test_refusals_leave_the_context_usable(ctx, bases):
    L = _lib.lib()
    scans, pts, poses = _resident(ctx, "two_mixed")
    base = bases["host"]

    def still_good():
        _check_primitive(ctx, base, ([0.5, -0.25, 0.25], 2.5), scans, pts, poses, 1.0, 30)

    def refused(rc_h_st, code, text=None):
        rc, h, _ = rc_h_st
        assert rc == code and h.value is None
        if text:
            assert text in L.elm_last_error(ctx._h).decode()
        still_good()

    bad = pts[0].copy()
    bad[100, 1] = np.nan
    refused(_call_from(ctx, base, None, [scans[1], Scan(ctx, bad)], poses, 1.0, 30), UNSUPPORTED, "2^20")
    far = np.array(poses[:1])
    far[0][:3, 3] = (0.0, float(2 ** 20) + 8.0, 0.0)  # every point of the scan lands at |q / vs| >= 2^20
    refused(_call_from(ctx, base, None, scans[:1], far, 1.0, 30), UNSUPPORTED, "2^20")
    one = np.array(poses[:1])
    one[0] = np.eye(4)
    edge = Scan(ctx, np.array([[0.0, 0.0, 0.0], [float(2 ** 19), 1.0, 1.0]], np.float32))
    refused(_call_from(ctx, None, None, [edge], one, 0.5, 30), UNSUPPORTED, "2^20")  # 2^19 / 0.5 = 2^20: one point does not pack
    other = Context(0)
    foreign = Scan(other, pts[0])
    refused(_call_from(ctx, base, None, [scans[0], foreign], poses, 1.0, 30), INVALID)
    foreign_base = _host_built(other, pts[1], 1.0, 30)
    refused(_call_from(ctx, foreign_base, None, scans, poses, 1.0, 30), INVALID)
    foreign.close()
    foreign_base.Clear()
    other.close()
    # a batch in flight
    vm = _host_built(ctx, cases.base_cloud(), 1.0, 30)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    reg.EnqueueBatch([scans[1]], vm, [np.eye(4)])
    rc, h, _ = _call_from(ctx, base, None, scans, poses, 1.0, 30)
    assert rc == INVALID and h.value is None
    reg.FinishBatch()
    still_good()


# ---------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", cases.LOOP_GOLDEN)))


def _config(method, **kw):
    kw = dict(cases.LOOP_REG, **kw)
    return OdometryConfig(voxel_size=cases.VOXEL, max_points_per_voxel=cases.CAP, max_range_m=cases.LOOP_MAX_RANGE, icp_method=method, **kw)


def _finish(vm, method, cov_dist):
    """what an insert does to its new map: the device index build and the covariances the method reads"""
    _lib.check(_lib.lib().elm_map_set_index_build(vm._h, _lib.INDEX_BUILD_DEVICE), vm.ctx._h, "elm_map_set_index_build")
    if method == IcpMethod.GICP:
        vm.CalPointCovAll(cov_dist)
    elif method in (IcpMethod.VGICP, IcpMethod.AVGICP):
        vm.CalVoxelCovAll()
    return vm


def _host_loop(ctx, cfg, scans, guesses):
    """the odometry loop from the host primitives: Pointcloud(), the mirror's sources, elm_map_build_device with host arrays,
    RunRegisterBatch; every guess is given"""
    method = IcpMethod(cfg.reg.icp_method)
    reg = Registration(cfg.reg, ctx)
    vm, T_key, steps = None, None, []
    for scan, guess in zip(scans, guesses):
        st = dict(T=np.array(guess, dtype=np.float64), registered=False, is_success=True, inserted=False, iterations=0)
        if vm is not None:
            r = reg.RunRegisterBatch([scan], vm, [guess])[0]
            st.update(T=r["T"], registered=True, is_success=r["is_success"], iterations=r["iterations"])
        if st["is_success"] and (vm is None or ref.is_keyframe(T_key, st["T"], cfg.key_min_trans_m, cfg.key_min_rot_rad)):
            stored = vm.Pointcloud() if vm is not None else np.zeros((0, 3))
            drop, xyz = ref.sources(stored, (st["T"][:3, 3], cfg.max_range_m) if vm is not None else None, [scan.points()], [st["T"]])
            vm = _finish(_derived(ctx, vm, drop if vm is not None else None, xyz, cfg.voxel_size, cfg.max_points_per_voxel), method,
                         cfg.reg.gicp_cov_search_dist)
            T_key = st["T"]
            st["inserted"] = True
        steps.append(st)
    return steps, vm


def _device_loop(ctx, cfg, scans, guesses):
    od = LidarOdometry(cfg, ctx)
    steps = [od.Step(s, g) for s, g in zip(scans, guesses)]
    return steps, od


@pytest.fixture(scope="module")
def loop(ctx):
    poses, pts = cases.loop_inputs()
    scans = [Scan(ctx, p) for p in pts]
    for s, p in zip(scans, pts):
        assert np.array_equal(s.points(), p)
    return poses, scans, cases.loop_guesses(poses)


@pytest.mark.parametrize("name,steps", [("p2p", 8), ("gicp", 8), ("vgicp", 3)])
def test_the_loop(ctx, loop, name, steps):
    poses, scans, guesses = loop
    method = {"p2p": IcpMethod.P2P, "gicp": IcpMethod.GICP, "vgicp": IcpMethod.VGICP}[name]
    cfg = _config(method)
    dev, od = _device_loop(ctx, cfg, scans[:steps], guesses[:steps])
    host, host_map = _host_loop(ctx, cfg, scans[:steps], guesses[:steps])
    gold = _gold()
    for k, (d, h) in enumerate(zip(dev, host)):
        dt, dr = synth.pose_error(gold[name + "_T"][k], d["T"])
        print(name, k, "ok", d["is_success"], "inserted", d["inserted"], "iterations", d["reg"]["iterations"] if d["reg"] else 0,
              "oracle", int(gold[name + "_iterations"][k]), "dt %.3g dr %.3g" % (dt, dr), d["build"])
    for k, (d, h) in enumerate(zip(dev, host)):
        assert d["T"].tobytes() == h["T"].tobytes(), k
        assert (d["registered"], d["is_success"], d["inserted"]) == (h["registered"], h["is_success"], h["inserted"]) == (k > 0, True, True)
        assert (d["reg"]["iterations"] if d["reg"] else 0) == h["iterations"]
        assert d["build"]["n_scan_points"] == scans[k].n and d["build"]["n_base_dropped"] >= 0
    assert dev[-1]["build"]["n_points"] == od.Map().info().n_points and dev[-1]["build"]["n_voxels"] == od.Map().info().n_voxels
    assert dev[0]["T"].tobytes() == np.array(guesses[0]).tobytes() and dev[0]["reg"] is None
    _same_maps(_read(od.Map()), _read(host_map))
    assert od.Map().info().layout_flags == host_map.info().layout_flags
    # the oracle's loop
    for k, d in enumerate(dev):
        dt, dr = synth.pose_error(gold[name + "_T"][k], d["T"])
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD, (k, dt, dr)
    od.close()


def test_keyframes_at_their_boundary(ctx, loop):
    """a scan that is registered but not inserted leaves the map handle as it was; the same pose a hair over the threshold inserts"""
    poses, scans, guesses = loop
    free = LidarOdometry(_config(IcpMethod.P2P), ctx)
    free.Step(scans[0], guesses[0])
    T1 = free.Step(scans[1], guesses[1])["T"]
    free.close()
    d = T1[:3, 3] - guesses[0][:3, 3]
    dist = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    for th, want in ((dist, True), (np.nextafter(dist, np.inf), False)):
        od = LidarOdometry(_config(IcpMethod.P2P, key_min_trans_m=th, key_min_rot_rad=math.pi), ctx)
        od.Step(scans[0], guesses[0])
        h0, before = od.Map()._h.value, _read(od.Map())
        st = od.Step(scans[1], guesses[1])
        assert st["T"].tobytes() == T1.tobytes() and st["registered"] and st["is_success"]
        assert st["inserted"] == want == ref.is_keyframe(guesses[0], T1, th, math.pi)
        assert (od.Map()._h.value == h0) == (not want) and (st["build"] is None) == (not want)
        if not want:
            _same_content(_read(od.Map()), before)
        od.close()
    # the rotation, by its cosine
    R = [(guesses[0][0, i] * T1[0, i] + guesses[0][1, i] * T1[1, i]) + guesses[0][2, i] * T1[2, i] for i in range(3)]
    c = (((R[0] + R[1]) + R[2]) - 1.0) / 2.0
    angle = math.acos(min(c, 1.0))
    for th in (angle * (1 - 1e-6), angle * (1 + 1e-6)):
        od = LidarOdometry(_config(IcpMethod.P2P, key_min_trans_m=100.0, key_min_rot_rad=th), ctx)
        od.Step(scans[0], guesses[0])
        st = od.Step(scans[1], guesses[1])
        assert st["inserted"] == (c <= math.cos(th)) == ref.is_keyframe(guesses[0], T1, 100.0, th), (th, angle)
        od.close()


def test_a_failed_step_changes_nothing(ctx, loop):
    poses, scans, guesses = loop
    good = LidarOdometry(_config(IcpMethod.P2P), ctx)
    want = [good.Step(scans[k], guesses[k]) for k in range(3)]
    od = LidarOdometry(_config(IcpMethod.P2P), ctx)
    od.Step(scans[0], guesses[0])
    od.Step(scans[1], guesses[1])
    h0, before, pred = od.Map()._h.value, _read(od.Map()), od.Predict()
    # the same object with max_fitness_score = 0: the step fails at the fitness gate
    strict = LidarOdometry(_config(IcpMethod.P2P, max_fitness_score=0.0), ctx)
    strict.Step(scans[0], guesses[0])
    hs, bs = strict.Map()._h.value, _read(strict.Map())
    st = strict.Step(scans[1], guesses[1])
    assert st["registered"] and not st["is_success"] and not st["inserted"] and st["build"] is None
    assert strict.Map()._h.value == hs and strict.Predict().tobytes() == np.array(guesses[0]).tobytes()  # one pose in the history: the first
    _same_content(_read(strict.Map()), bs)
    st = strict.Step(scans[1], guesses[1])  # again: the same failure, from the same state
    assert not st["is_success"] and strict.Map()._h.value == hs
    strict.close()
    # the next step of the untouched object is the undisturbed one
    assert od.Map()._h.value == h0 and od.Predict().tobytes() == pred.tobytes()
    _same_maps(_read(od.Map()), before)
    st = od.Step(scans[2], guesses[2])
    assert st["T"].tobytes() == want[2]["T"].tobytes() and st["inserted"] and st["reg"]["iterations"] == want[2]["reg"]["iterations"]
    _same_maps(_read(od.Map()), _read(good.Map()))
    od.close()
    good.close()


def test_reset_and_predict(ctx, loop):
    poses, scans, guesses = loop
    od = LidarOdometry(_config(IcpMethod.P2P), ctx)
    assert od.Map() is None and np.array_equal(od.Predict(), np.eye(4))
    first = od.Step(scans[0], None)  # no guess, no history: identity
    assert np.array_equal(first["T"], np.eye(4)) and not first["registered"] and first["is_success"] and first["inserted"]
    od.Reset()
    assert od.Map() is None and np.array_equal(od.Predict(), np.eye(4))
    # guess = None is Predict() fed back, byte for byte; Predict() is the numpy formula
    a, b = LidarOdometry(_config(IcpMethod.P2P), ctx), od
    history = []
    for k in range(4):
        g = b.Predict() if k else np.array(guesses[0])
        want = ref.predict(history) if k else g
        assert np.allclose(g, want, rtol=0, atol=1e-9) and np.abs(g[:3, 3]).max() <= 100.0
        assert np.array_equal(g[3], [0.0, 0.0, 0.0, 1.0])
        sa, sb = a.Step(scans[k], None if k else guesses[0]), b.Step(scans[k], g)
        assert sa["T"].tobytes() == sb["T"].tobytes() and sa["is_success"] == sb["is_success"] and sa["inserted"] == sb["inserted"]
        assert (sa["reg"]["iterations"] if k else 0) == (sb["reg"]["iterations"] if k else 0)
        if sb["is_success"]:
            history.append(sb["T"])
    assert len(history) >= 2  # the constant-velocity branch ran
    _same_maps(_read(a.Map()), _read(b.Map()))
    # after Reset the next scan is a first scan again
    b.Reset()
    again = b.Step(scans[0], guesses[0])
    assert not again["registered"] and again["inserted"] and again["T"].tobytes() == np.array(guesses[0]).tobytes()
    assert np.array_equal(b.Predict(), guesses[0])
    a.close()
    b.close()


def test_a_whole_log_in_one_call(ctx):
    """64 scans x 2 048 points at 64 poses, no base, against the mirror"""
    world = synth.make_world(100_000)
    poses = cases.loop_poses(64, 0.25, 1.0)
    scans = [Scan(ctx, synth.make_scan(world, 2048, 9000 + k, T_true=poses[k], max_range=cases.LOOP_SCAN_RANGE)[0]) for k in range(64)]
    pts = [s.points() for s in scans]
    vm, stats = VoxelHashMap(1.0, 30, ctx).UpdatedFromScans(scans, poses, stats=True)
    (mp, mk, mc), mstats = ref.build(np.zeros((0, 3)), None, pts, poses, 1.0, 30)
    print("whole log:", stats)
    assert stats == mstats and stats["n_scan_points"] == 64 * 2048
    got = _read(vm)
    assert np.array_equal(got[0], mp) and np.array_equal(got[1], mk) and np.array_equal(got[2], mc)
