"""The rolling local map and the LiDAR odometry (include/elimaloc_hip.h, "device map build from resident sources" and "LiDAR odometry on a
rolling local map") on the CPU: the numpy mirror of the two device producers (tests/local_map_ref.py) on thresholds worked out by hand
and against the oracle's two add_points; the keyframe rule and the prediction formula on the mirror; the odometry loop's fixed inputs
(tests/local_map_cases.py) run with the oracle, every step succeeding, and equal to the committed fixture; the symbols, the struct
layouts, the argument errors without a device; the C++ shim's call lines compiling."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import build_cases  # tests/ is on sys.path via conftest
import build_ref
import local_map_cases as cases
import local_map_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the mirror, by hand
def test_keep_thresholds_worked_out_by_hand():
    """radius 5 about the origin: (3, 4, 0) gives 9 + 16 = 25 <= 25 and stays; the next float32 above 4 gives more and goes"""
    drop = ref.keep_flags(cases.THRESHOLD_POINTS, cases.THRESHOLD_KEEP)
    assert drop.dtype == np.uint8 and (drop == 0).tolist() == cases.THRESHOLD_KEPT
    assert ref.keep_flags(cases.THRESHOLD_POINTS, None).tolist() == [0] * len(cases.THRESHOLD_POINTS)
    x = float(cases.NEXT4)
    assert x > 4.0 and (9.0 + x * x) > 25.0 and np.float32(x) == cases.NEXT4
    # radius 0 with the centre on a stored point keeps exactly that point; a NaN radius is the caller's error, a NaN point is dropped
    assert (ref.keep_flags(cases.THRESHOLD_POINTS, (cases.THRESHOLD_POINTS[6].astype(np.float64), 0.0)) == 0).tolist() == \
        [False] * 6 + [True, False]
    assert ref.keep_flags(np.array([[np.nan, 0, 0]], np.float32), ([0, 0, 0], 5.0)).tolist() == [1]


def test_transform_rounding_worked_out_by_hand():
    """float32 ties go to even, -0.0 stays in voxel 0, 0.5 + 0.5 lands on the face and belongs to voxel 1"""
    q = ref.transform(cases.TIE_POINTS, cases.TIE_POSE)
    assert q.dtype == np.float32 and np.array_equal(q, cases.TIE_EXPECTED)
    assert float(q[0, 0]) == 1.0 and float(q[1, 0]) == 1.0 + 2.0 ** -22  # both ties: to the even neighbour
    keys = build_ref.voxel_keys(q, 1.0)
    assert keys.tolist() == [[1, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]
    # a general pose: the contract's association against a longer-precision product, within one rounding of float32
    P = cases.scan_points(257)
    T = cases.POSES["general"]
    exact = (P.astype(np.longdouble) @ T[:3, :3].astype(np.longdouble).T + T[:3, 3].astype(np.longdouble)).astype(np.float64)
    got = ref.transform(P, T).astype(np.float64)
    assert np.abs(got - exact).max() <= np.spacing(np.float32(np.abs(exact).max()))
    # the job order and the stats
    scans, poses, _ = cases.jobs("zero_middle")
    drop, xyz = ref.sources(cases.THRESHOLD_POINTS, cases.THRESHOLD_KEEP, scans, poses)
    assert len(xyz) == 257 + 256 and np.array_equal(xyz[257:], scans[3]) and np.array_equal(xyz[:257], ref.transform(scans[0], poses[0]))


def test_the_resident_order_is_a_stable_sort():
    p = cases.scan_points(1025)
    assert np.array_equal(cases.resident_order(p), np.arange(1025))  # already ordered: an upload keeps it
    raw = np.random.default_rng(3).uniform(-3.5, 3.5, size=(1025, 3)).astype(np.float32)
    o = cases.resident_order(raw)
    assert sorted(o.tolist()) == list(range(1025)) and not np.array_equal(o, np.arange(1025))


# ---------------------------------------------------------------- the mirror map against the oracle
@pytest.mark.parametrize("keep", [None, ([0.5, -0.25, 0.0], 2.5), ([0.0, 0.0, 0.0], 100.0), ([50.0, 0.0, 0.0], 1.0)])
@pytest.mark.parametrize("vs", [1.0, 0.5])
def test_the_mirror_map_is_the_oracles_two_adds(oracle, keep, vs):
    """base = the +-3 m family of tests/build_cases.py; the oracle adds the kept stored points, then the transformed scans"""
    base = build_ref.build(build_cases.dense3(), 1.0, 30)[0]
    scans, poses, _ = cases.jobs("five_mixed")
    scans, poses = scans[:3], poses[:3]  # (the far poses belong to another map)
    (mp, mk, mc), stats = ref.build(base, keep, scans, poses, vs, 30)
    drop, xyz = ref.sources(base, keep, scans, poses)
    om = oracle.Map(vs, 30)
    kept = base[drop == 0].astype(np.float32)
    for cloud in (kept, xyz):
        if len(cloud):
            om.add_points(cloud)
    keys, counts = om.voxels()[:2]
    want = build_ref.canonical(om.pointcloud()[0], keys, counts)
    got = build_ref.canonical(mp, mk, mc)
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    assert stats["n_base_kept"] + stats["n_base_dropped"] == len(base) and stats["n_scan_points"] == len(xyz)
    assert stats["n_points"] == om.num_points and stats["n_voxels"] == om.num_voxels
    if keep is not None and keep[1] == 100.0:
        assert stats["n_base_dropped"] == 0
    if keep is not None and keep[1] == 1.0:
        assert stats["n_base_kept"] == 0


# ---------------------------------------------------------------- keyframe rule and prediction
def _pose(yaw=0.0, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = t
    return T


def test_the_keyframe_rule_at_its_thresholds():
    key = _pose()
    never_rot = math.pi  # cos = -1: the rotation test cannot fire for these poses
    d = 0.75  # dyadic: the distance is exact
    assert ref.is_keyframe(key, _pose(t=(d, 0, 0)), d, never_rot)
    assert not ref.is_keyframe(key, _pose(t=(np.nextafter(d, 0.0), 0, 0)), d, never_rot)
    assert ref.is_keyframe(key, _pose(t=(0.25, 0.5, 0.5)), d, never_rot)  # 1/16 + 1/4 + 1/4 = 9/16: sqrt = 0.75 exactly
    # the rotation by its cosine: R = R_key^T R_new has (trace - 1) / 2 = cos(yaw) for a yaw; it inserts iff that is <= cos(threshold)
    big = 10.0  # the translation test cannot fire
    for yaw in (0.05, 0.3, 1.0):
        c = ((math.cos(yaw) + math.cos(yaw)) + 1.0 - 1.0) / 2.0  # as the rule sums the diagonal of a yaw
        th_at = math.acos(c)
        new = _pose(yaw)
        assert ref.is_keyframe(key, new, big, th_at) == (c <= math.cos(th_at))
        lo, hi = th_at * (1 - 1e-9), th_at * (1 + 1e-9)
        assert math.cos(lo) > c > math.cos(hi)
        assert ref.is_keyframe(key, new, big, lo) and not ref.is_keyframe(key, new, big, hi)
    # against a key pose that is itself rotated and moved: only the relative motion counts
    key2 = _pose(0.7, (3.0, -2.0, 1.0))
    new2 = key2 @ _pose(0.2, (0.5, 0.0, 0.0))
    assert ref.is_keyframe(key2, new2, 0.4999, never_rot) and not ref.is_keyframe(key2, new2, 0.5001, never_rot)
    assert ref.is_keyframe(key2, new2, big, 0.1999) and not ref.is_keyframe(key2, new2, big, 0.2001)
    assert ref.is_keyframe(key, key, 0.0, 0.0)  # both thresholds 0: every scan


def test_the_prediction_formula():
    assert np.array_equal(ref.predict([]), np.eye(4))
    a = _pose(0.3, (1.0, 2.0, 0.5))
    assert np.array_equal(ref.predict([a]), a)
    step = _pose(0.05, (0.5, 0.02, 0.0))
    b = a @ step
    assert np.allclose(ref.predict([a, b]), b @ step, atol=1e-13)  # constant velocity: the same step again
    assert np.allclose(ref.rigid_inverse(a) @ a, np.eye(4), atol=1e-15)
    assert np.allclose(ref.predict([_pose(), a, b]), b @ step, atol=1e-13)  # only the last two count


# ---------------------------------------------------------------- the loop's inputs, with the oracle
def test_the_loop_inputs():
    poses, scans = cases.loop_inputs()
    assert len(poses) == len(scans) == cases.LOOP_STEPS == 8
    for k in range(1, len(poses)):
        D = ref.rigid_inverse(poses[k - 1]) @ poses[k]
        assert abs(np.linalg.norm(poses[k][:3, 3] - poses[k - 1][:3, 3]) - 0.5) < 1e-12
        assert abs(math.degrees(math.acos((np.trace(D[:3, :3]) - 1) / 2)) - 2.0) < 1e-6
    for s in scans:
        assert s.shape == (cases.LOOP_SCAN_POINTS, 3) and s.dtype == np.float32
        assert np.array_equal(cases.resident_order(s), np.arange(len(s)))
        assert np.sqrt((s.astype(np.float64) ** 2).sum(1)).max() < cases.LOOP_SCAN_RANGE + 0.1


@pytest.mark.parametrize("name,steps", [("p2p", 8), ("gicp", 8), ("vgicp", 3)])
def test_the_oracle_loop_succeeds_and_is_the_fixture(oracle, name, steps):
    """the condition the GPU loop tests rest on: every step of the oracle's loop succeeds and inserts; its poses are the fixture's"""
    method = {"p2p": oracle.P2P, "gicp": oracle.GICP, "vgicp": oracle.VGICP}[name]
    poses, scans = cases.loop_inputs()
    got, stored = ref.oracle_loop(oracle, method, poses[:steps], scans[:steps], cases.loop_guesses(poses)[:steps], cases.VOXEL, cases.CAP,
                                  cases.LOOP_MAX_RANGE, **cases.LOOP_REG)
    assert [s["is_success"] for s in got] == [True] * steps and [s["inserted"] for s in got] == [True] * steps
    assert [s["registered"] for s in got] == [False] + [True] * (steps - 1)
    gold = np.load(os.path.join(ROOT, "tests", "golden", cases.LOOP_GOLDEN))
    assert np.allclose(np.stack([s["T"] for s in got]), gold[name + "_T"], rtol=0, atol=1e-12)
    assert gold[name + "_is_success"].all() and gold[name + "_iterations"].tolist() == [s["iterations"] for s in got]
    assert int(gold[name + "_n_stored"]) == len(stored)


# ---------------------------------------------------------------- header, layouts, arguments, shim
NEW_SYMBOLS = ("elm_map_build_device_from", "elm_odometry_config_default", "elm_odometry_create", "elm_odometry_destroy", "elm_odometry_reset",
               "elm_odometry_predict", "elm_odometry_step_scan", "elm_odometry_map")


def test_the_symbols_are_in_the_header(L):
    from elimaloc_amd import _lib
    raw = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+elm_map_build_device_from\s*\(\s*elm_ctx\*\s*ctx,\s*const elm_build_sources\*\s*src,\s*double voxel_size,"
                     r"\s*int max_points_per_voxel,\s*elm_map\*\*\s*out,\s*elm_build_sources_stats\*\s*stats\)", src)
    assert re.search(r"int\s+elm_odometry_step_scan\s*\(\s*elm_odometry\*\s*odom,\s*const elm_scan\*\s*scan,\s*const double T_guess\[16\]\s*,"
                     r"\s*elm_odometry_step\*\s*out\)", src)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.EXPORTS and re.search(r"\b%s\s*\(" % s, src)
    for rule in ("first scan", "later scans", "keyframe test", "insert", "history", "scope"):
        assert rule in raw


def test_struct_layouts_match_the_header(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(elm_build_sources), sizeof(elm_build_sources_stats), sizeof(elm_odometry_config), sizeof(elm_odometry_step));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(elm_build_sources, keep_within), offsetof(elm_build_sources, keep_center),
         offsetof(elm_build_sources, keep_radius_m), offsetof(elm_build_sources, scans), offsetof(elm_build_sources, poses16),
         offsetof(elm_build_sources, n_jobs));
  printf("%zu %zu %zu %zu\n", offsetof(elm_odometry_config, max_points_per_voxel), offsetof(elm_odometry_config, max_range_m),
         offsetof(elm_odometry_config, key_min_rot_rad), offsetof(elm_odometry_config, reg));
  printf("%zu %zu %zu %zu\n", offsetof(elm_odometry_step, registered), offsetof(elm_odometry_step, inserted), offsetof(elm_odometry_step, reg),
         offsetof(elm_odometry_step, build));
  return 0; }
'''
    src = tmp_path / "p.c"
    src.write_text(probe)
    exe = tmp_path / "p"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    S, St, Cf, Sp = _lib.BuildSourcesC, _lib.BuildSourcesStatsC, _lib.OdometryConfigC, _lib.OdometryStepC
    assert out[:4] == [C.sizeof(S), C.sizeof(St), C.sizeof(Cf), C.sizeof(Sp)]
    assert out[4:10] == [S.keep_within.offset, S.keep_center.offset, S.keep_radius_m.offset, S.scans.offset, S.poses16.offset, S.n_jobs.offset]
    assert out[10:14] == [Cf.max_points_per_voxel.offset, Cf.max_range_m.offset, Cf.key_min_rot_rad.offset, Cf.reg.offset]
    assert out[14:] == [Sp.registered.offset, Sp.inserted.offset, Sp.reg.offset, Sp.build.offset]
    assert [n for n, _ in St._fields_] == ["n_base_kept", "n_base_dropped", "n_scan_points", "n_points", "n_voxels"]


def _sources(**kw):
    from elimaloc_amd import _lib
    s = _lib.BuildSourcesC()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_argument_errors_without_a_device(L):
    """every ELM_ERR_INVALID case that needs no device: never-dereferenced handles stand in for the context, the base and the scans"""
    from elimaloc_amd import _lib
    one = C.c_void_p(1)  # a context that is never dereferenced: these arguments are refused before it is looked at
    T = (C.c_double * 32)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] * 2))
    scans = (C.c_void_p * 2)(1, 1)
    stats = _lib.BuildSourcesStatsC()

    def build(ctx, src, vs=1.0, cap=30, with_out=True):
        out = C.c_void_p(1)
        rc = L.elm_map_build_device_from(ctx, C.byref(src) if src is not None else None, vs, cap, C.byref(out) if with_out else None,
                                         C.byref(stats))
        if with_out:
            assert out.value is None  # *out is NULL after a refusal
        return rc

    ok = dict(scans=scans, poses16=T, n_jobs=2)
    assert build(None, _sources(**ok)) == INVALID
    assert build(one, None) == INVALID
    assert build(one, _sources(**ok), with_out=False) == INVALID
    assert build(one, _sources(**ok), vs=0.0) == INVALID and build(one, _sources(**ok), vs=float("nan")) == INVALID
    assert build(one, _sources(**ok), cap=0) == INVALID
    assert build(one, _sources(scans=scans, poses16=T, n_jobs=-1)) == INVALID
    assert build(one, _sources(scans=scans, poses16=T, n_jobs=4097)) == INVALID
    assert build(one, _sources(poses16=T, n_jobs=2)) == INVALID and build(one, _sources(scans=scans, n_jobs=2)) == INVALID
    assert build(one, _sources(scans=(C.c_void_p * 2)(1, None), poses16=T, n_jobs=2)) == INVALID
    assert build(one, _sources(keep_within=2, **ok)) == INVALID and build(one, _sources(keep_within=-1, **ok)) == INVALID
    assert build(one, _sources(keep_within=1, keep_radius_m=1.0, **ok)) == INVALID  # no base
    assert build(one, _sources(keep_radius_m=-1.0, **ok)) == INVALID
    assert build(one, _sources(keep_radius_m=float("inf"), **ok)) == INVALID and build(one, _sources(keep_radius_m=float("nan"), **ok)) == INVALID
    assert build(one, _sources(keep_center=(C.c_double * 3)(0.0, float("nan"), 0.0), **ok)) == INVALID
    bad = (C.c_double * 32)(*T)
    bad[16 + 13] = float("inf")
    assert build(one, _sources(scans=scans, poses16=bad, n_jobs=2)) == INVALID
    # the odometry object
    cfg = _lib.OdometryConfigC()
    L.elm_odometry_config_default(C.byref(cfg))
    assert (cfg.voxel_size, cfg.max_points_per_voxel, cfg.max_range_m, cfg.key_min_trans_m, cfg.key_min_rot_rad) == (1.0, 30, 100.0, 0.0, 0.0)
    ref_reg = _lib.RegConfig()
    L.elm_reg_config_default(C.byref(ref_reg))
    assert bytes(cfg.reg) == bytes(ref_reg)
    out = C.c_void_p(1)
    assert L.elm_odometry_create(None, C.byref(cfg), C.byref(out)) == INVALID and out.value is None
    assert L.elm_odometry_create(one, None, C.byref(out)) == INVALID and L.elm_odometry_create(one, C.byref(cfg), None) == INVALID
    for field, value in (("voxel_size", 0.0), ("voxel_size", float("nan")), ("max_points_per_voxel", 0), ("max_range_m", -1.0),
                         ("max_range_m", float("inf")), ("key_min_trans_m", -0.5), ("key_min_rot_rad", float("nan"))):
        c2 = _lib.OdometryConfigC.from_buffer_copy(cfg)
        setattr(c2, field, value)
        assert L.elm_odometry_create(one, C.byref(c2), C.byref(out)) == INVALID, field
    for method in (-1, 4):
        c2 = _lib.OdometryConfigC.from_buffer_copy(cfg)
        c2.reg.icp_method = method
        assert L.elm_odometry_create(one, C.byref(c2), C.byref(out)) == INVALID
    step = _lib.OdometryStepC()
    G = (C.c_double * 16)()
    assert L.elm_odometry_step_scan(None, one, None, C.byref(step)) == INVALID
    assert L.elm_odometry_predict(None, G) == INVALID and L.elm_odometry_reset(None) == INVALID
    assert L.elm_odometry_map(None) is None
    L.elm_odometry_destroy(None)


def test_python_wrappers_refuse_what_they_can_see():
    from elimaloc_amd.registration import OdometryConfig, IcpMethod
    cfg = OdometryConfig(voxel_size=0.5, max_points_per_voxel=20, max_range_m=25.0, key_min_trans_m=0.5, icp_method=IcpMethod.P2P,
                         max_fitness_score=1.0)
    assert (cfg.voxel_size, cfg.max_points_per_voxel, cfg.max_range_m, cfg.key_min_trans_m, cfg.reg.icp_method, cfg.reg.max_fitness_score) == \
        (0.5, 20, 25.0, 0.5, 0, 1.0)
    with pytest.raises(AttributeError):
        OdometryConfig(no_such_field=1)


def test_shim_odometry_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/odometry_calls.cpp, built as tests/test_map_build_device_abi.py builds build_calls.cpp"""
    exe = tmp_path / "odometry_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "odometry_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
