"""Relocalization on the GPU (elm_map_score_poses / elm_relocalize): the occupancy scores against a numpy mirror in all three kernel forms and
under every search-index form, the edge cases, recovery from guesses metres and tens of degrees off (P2P and GICP), the node's
CallbackInitialPose with a RelocConfig, and the one-rank-only refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from elimaloc_amd import _lib, synth
from elimaloc_amd.registration import (Context, IcpMethod, MakeHypotheses, Registration, RegistrationConfig, RelocConfig, Scan,
                                       VoxelHashMap)
from elimaloc_amd._lib import ElmError
from reloc_ref import _codes, mirror_scores  # noqa: F401  (the numpy mirror of the score contract)

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
FORMS = [dict(), dict(lds_budget_bytes=0), dict(lds_budget_bytes=0, bitmap_max_bytes=0)]  # default (LDS when it fits), global bitmap, probes


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _small_hyps(T, **kw):
    return MakeHypotheses(T, RelocConfig(**({"radius_xy_m": 1.0, "step_xy_m": 0.5, "yaw_range_deg": 180.0, "step_yaw_deg": 24.0} | kw)))


@pytest.fixture(scope="module")
def field1m():
    return synth.make_field_world(1_000_000, seed=4242)


def _check_all_forms(vm, scan, poses, ref, r_max=50.0):
    sc = Scan(vm.ctx, scan)
    for f in FORMS:
        got = vm.ScorePoses(sc, poses, RelocConfig(score_max_range_m=r_max, **f))
        assert np.array_equal(got, ref), (f, np.flatnonzero(got != ref)[:10])


def test_scores_exact_field_world(ctx, field1m):
    world = field1m
    scan, T = synth.make_scan(world, 6001, seed=5)
    poses = _small_hyps(T)
    ref = mirror_scores(world, 1.0, scan, poses, 50.0)
    assert ref.max() > 0.9 * np.count_nonzero(np.einsum("ij,ij->i", scan.astype(np.float64), scan.astype(np.float64)) <= 2500.0)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    _check_all_forms(vm, scan, poses, ref)


@pytest.mark.parametrize("vs", [0.5, 0.3])
def test_scores_exact_lattice_world(ctx, vs):
    world = synth.make_world(300_000, seed=77)
    scan, T = synth.make_scan(world, 4099, seed=8, max_range=40.0)
    poses = _small_hyps(T, step_yaw_deg=40.0)
    ref = mirror_scores(world, vs, scan, poses, 30.0)  # some points lie beyond 30 m: the range test is exercised
    vm = VoxelHashMap(vs, 20, ctx)
    vm.AddPoints(world)
    _check_all_forms(vm, scan, poses, ref, r_max=30.0)


def test_scores_exact_random_rotations(ctx, field1m):
    world = field1m
    scan, T = synth.make_scan(world, 5003, seed=21)  # not a multiple of 256
    rng = np.random.default_rng(3)
    poses = np.empty((2000, 4, 4))
    for h in range(2000):
        v = rng.normal(size=3)
        poses[h] = np.eye(4)
        poses[h][:3, :3] = synth.rotvec_to_matrix(v / np.linalg.norm(v) * rng.uniform(0.0, math.pi))
        poses[h][:3, 3] = T[:3, 3] + rng.uniform(-3.0, 3.0, 3)
    poses[0] = T
    ref = mirror_scores(world, 1.0, scan, poses, 50.0)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    _check_all_forms(vm, scan, poses, ref)


@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled")])
def test_scores_same_under_every_index_form(monkeypatch, field1m, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    world = field1m
    scan, T = synth.make_scan(world, 3000, seed=31)
    poses = _small_hyps(T, step_yaw_deg=60.0)
    ref = mirror_scores(world, 1.0, scan, poses, 50.0)
    vm = VoxelHashMap(1.0, 30, c)
    vm.AddPoints(world)
    vm.BuildNeighbourhoods()
    _check_all_forms(vm, scan, poses, ref)
    # a registration still runs on that index afterwards
    _, ok, _, _ = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), c).RunRegister(scan, vm, T)
    assert ok
    del vm
    c.close()


def test_score_edge_cases(ctx):
    world = synth.make_world(50_000, seed=9)
    scan, T = synth.make_scan(world, 1000, seed=10)
    empty = VoxelHashMap(1.0, 30, ctx)
    assert np.array_equal(empty.ScorePoses(scan, _small_hyps(T)), np.zeros(len(_small_hyps(T)), np.uint32))
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    far = scan.astype(np.float64)
    r_min = float(np.sqrt(np.min(np.einsum("ij,ij->i", far, far))))
    assert not np.any(vm.ScorePoses(scan, _small_hyps(T), RelocConfig(score_max_range_m=0.5 * r_min)))
    one = vm.ScorePoses(scan, T[None])
    assert one.shape == (1,) and one[0] == mirror_scores(world, 1.0, scan, T[None], 50.0)[0] and one[0] > 0
    poses = _small_hyps(T)
    sc = Scan(ctx, scan)
    a, b = vm.ScorePoses(sc, poses), vm.ScorePoses(sc, poses)
    assert np.array_equal(a, b) and a.dtype == np.uint32
    # empty map: elm_relocalize answers like elm_register (gate 1)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    pose, ok, fit, _, cands = reg.Relocalize(scan, empty, T, RelocConfig(radius_xy_m=1.0, step_yaw_deg=30.0, top_k=3))
    assert not ok and fit is None and reg.last_relocalize_["gate"] == 1 and len(cands) == 3
    assert all(c["score"] == 0 for c in cands)


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def field2m(ctx):
    world = synth.make_field_world(2_000_000, seed=2027)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    vm.CalPointCovAll(0.4)
    return world, vm


def _case(world, vm, seed):
    """truth at ~1.8 m above the ground, a scan, and a guess 3-4.5 m and 30-170 deg of yaw off (z from the ground under the guess)."""
    rng = np.random.default_rng(seed)
    T = synth.make_pose(world, seed)
    ext = float(np.max(np.abs(world[:, :2])))
    T[:2, 3] = rng.uniform(-0.4 * ext, 0.4 * ext, 2)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    assert found
    T[2, 3] = gz + 1.8
    scan, _ = synth.make_scan(world, 16384, seed=seed + 1, T_true=T)
    d, a = rng.uniform(3.0, 4.5), rng.uniform(0.0, 2 * math.pi)
    dyaw = math.radians(rng.uniform(30.0, 170.0)) * rng.choice([-1.0, 1.0])
    G = np.eye(4)
    G[:3, :3] = synth.rot_zyx(0.0, 0.0, dyaw) @ T[:3, :3]
    G[:2, 3] = T[:2, 3] + d * np.array([math.cos(a), math.sin(a)])
    found, gz = vm.FindGroundHeight(G[:2, 3])
    G[2, 3] = (gz if found else T[2, 3] - 1.8) + 1.8
    return T, scan, G


def _yaw_of(R):
    return math.atan2(R[1, 0], R[0, 0])


@pytest.mark.parametrize("method", [IcpMethod.P2P, IcpMethod.GICP])
def test_relocalize_recovers(ctx, field2m, method):
    world, vm = field2m
    reg = Registration(RegistrationConfig(icp_method=method), ctx)
    # the best hypothesis lies up to half a step from the truth.  GICP converges from the default grid to ICP-from-the-truth's pose.  P2P on
    # this ground-dominated world stops where its 0.02 m step test fires, 0.13-0.28 m short even from 0.13 m (measured, DESIGN.md section
    # 11): it runs on the finer 0.25 m / 1 deg grid and must land inside ICP's basin (0.25 m / 1 deg), not on the truth's own ICP pose
    gicp = method == IcpMethod.GICP
    rcfg = RelocConfig() if gicp else RelocConfig(step_xy_m=0.25, step_yaw_deg=1.0)
    tol_m, tol_deg = (0.05, 0.2) if gicp else (0.25, 1.0)
    for seed in (101, 202, 303):
        T, scan, G = _case(world, vm, seed)
        # premise: plain ICP from the guess does not recover
        p0, ok0, _, _ = reg.RunRegister(scan, vm, G)
        dt0, dr0 = synth.pose_error(T, p0)
        assert (not ok0) or dt0 > 1.0 or dr0 > math.radians(5.0), (seed, dt0, dr0)
        ref, ok_ref, _, _ = reg.RunRegister(scan, vm, T)
        assert ok_ref
        pose, ok, fit, cov, cands = reg.Relocalize(scan, vm, G, rcfg)
        assert ok, (seed, cands[:3])
        dt, dr = synth.pose_error(ref, pose)
        assert dt <= tol_m and dr <= math.radians(tol_deg), (seed, dt, dr, [(c["score"], c["is_success"], c["iterations"], c["fitness_score"],
                                                                     synth.pose_error(T, c["T"])) for c in cands])
        # bit-identical to elm_register_batch on the same resident scan from the winner's T0
        win = [c for c in cands if np.array_equal(c["T"], pose)]
        assert win
        again = reg.RunRegisterBatch([Scan(ctx, scan)], vm, [win[0]["T0"]])[0]
        assert np.array_equal(again["T"], pose) and again["fitness_score"] == fit and again["is_success"]
        # candidates: sorted by (score desc, index asc), NMS spacing between every kept pair
        assert 1 <= len(cands) <= rcfg.top_k
        keys = [(-c["score"], c["hyp_index"]) for c in cands]
        assert keys == sorted(keys)
        for i in range(len(cands)):
            for j in range(i):
                a, b = cands[i]["T0"], cands[j]["T0"]
                dxy = float(np.hypot(*(a[:2, 3] - b[:2, 3])))
                dy = abs((math.degrees(_yaw_of(a[:3, :3] @ b[:3, :3].T)) + 180.0) % 360.0 - 180.0)
                assert dxy > rcfg.nms_xy_m - 1e-9 or dy > rcfg.nms_yaw_deg - 1e-9, (i, j, dxy, dy)
        # every candidate's T0 is hypothesis hyp_index of the grid around the guess
        H = MakeHypotheses(G, rcfg)
        assert all(np.array_equal(H[c["hyp_index"]], c["T0"]) for c in cands)


def test_callback_initial_pose_relocalizes(ctx, field2m):
    from elimaloc_amd.pcm_matching import PcmMatching, PcmMatchingConfig
    world, vm = field2m
    tf = np.eye(4)
    tf[2, 3] = 1.8
    node = PcmMatching(PcmMatchingConfig(tf_ego_to_lidar=tf), ctx)
    node.Init(world)
    T, scan, G = _case(world, vm, 404)
    rviz = G @ np.linalg.inv(tf)
    plain = node.CallbackInitialPose(rviz, scan)
    if plain is not None:
        dt, dr = synth.pose_error(T, plain["pose_lidar"])
        assert dt > 1.0 or dr > math.radians(5.0)
    out = node.CallbackInitialPose(rviz, scan, relocalize=RelocConfig())
    assert out is not None and out["candidates"]
    from elimaloc_amd.pcm_matching import voxel_downsample
    src, _ = voxel_downsample(scan, node.cfg_.d_input_voxel_ds_m)
    ref, ok, _, _ = node.registration_.RunRegister(src, node.local_map_, T)
    assert ok
    dt, dr = synth.pose_error(ref, out["pose_lidar"])
    assert dt <= 0.05 and dr <= math.radians(0.2), (dt, dr)
    assert np.allclose(out["pose_ego"], out["pose_lidar"] @ np.linalg.inv(tf))


def test_one_rank_only(ctx):
    world = synth.make_world(30_000, seed=11)
    scan, T = synth.make_scan(world, 2048, seed=12)
    L = _lib.lib()
    poses = np.ascontiguousarray(T.T).ravel()
    cfg = RelocConfig(radius_xy_m=0.5, step_yaw_deg=90.0, top_k=2)
    reg = RegistrationConfig(icp_method=IcpMethod.P2P)

    def codes(c, vm):
        sc = Scan(c, scan)
        out = np.zeros(1, np.uint32)
        a = L.elm_map_score_poses(c._h, vm._handle(), sc._h, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(cfg),
                                  out.ctypes.data_as(C.POINTER(C.c_uint32)))
        Tout, res, cands, n = np.empty(16), _lib.RegResult(), (_lib.RelocCandidate * 2)(), C.c_int(0)
        b = L.elm_relocalize(c._h, vm._handle(), scan.ctypes.data_as(C.POINTER(C.c_float)), scan.shape[0],
                             poses.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cfg), C.byref(reg),
                             Tout.ctypes.data_as(C.POINTER(C.c_double)), C.byref(res), cands, 2, C.byref(n))
        return a, b, L.elm_last_error(c._h).decode()

    grp = Context.multi([0, 0])
    gvm = VoxelHashMap(1.0, 30, grp)
    gvm.AddPoints(world)
    a, b, msg = codes(grp, gvm)
    assert (a, b) == (UNSUPPORTED, UNSUPPORTED) and "one rank" in msg
    with pytest.raises(ElmError):
        gvm.ScorePoses(scan, T[None], cfg)
    del gvm
    grp.close()
    hc = Context(0)
    hc.set_allreduce_hook(lambda p, n, s: 0)
    hvm = VoxelHashMap(1.0, 30, hc)
    hvm.AddPoints(world)
    assert codes(hc, hvm)[:2] == (UNSUPPORTED, UNSUPPORTED)
    hc.set_allreduce_hook(None)
    assert codes(hc, hvm)[:2] == (0, 0)  # without the hook the same calls run
    del hvm
    hc.close()
