"""BASELINE config 5 in closed loop: deskew + VGICP on the GPU, 27-state EKF on the CPU, at 10 Hz LiDAR / 200 Hz IMU.

Parity: the product chain (LocalizationStream = PcmMatching over the C ABI + csrc/elm_ekf.cpp) against a second chain
assembled only from checker parts (oracle deskew / pose sync / downsample / register + tests/np_ekf.py), both fed the
same simulated drive.  Every ICP pose must agree within the north-star tolerance (1e-4 m / 1e-5 rad) although the loop
is closed (each pose feeds the filter that seeds and deskews the next scan).
"""
import collections

import numpy as np
import pytest

from elimaloc_amd import synth

import np_ekf

pytestmark = pytest.mark.gpu


class OracleStream:
    """The same topology as elimaloc_amd.stream.LocalizationStream, from oracle calls and the numpy EKF."""

    def __init__(self, oracle, world, cfg, ekf_cfg):
        self.o, self.cfg = oracle, cfg
        self.map = oracle.Map(cfg.d_pcm_voxel_size, cfg.i_pcm_voxel_max_point)
        self.map.add_points(world)
        self.map.cal_voxel_cov_all()
        self.ekf = np_ekf.NpEkf(ekf_cfg)
        self.imu, self.odom = collections.deque(), collections.deque()

    def CallbackImu(self, t, gyro, acc):
        self.ekf.predict_imu(t, gyro, acc)
        e = self.ekf.publish()
        if "x_m" not in e:
            return
        q = np_ekf.quat_mul(np_ekf.quat_mul(np_ekf.aa_quat(e["yaw_rad"], [0, 0, 1]), np_ekf.aa_quat(e["pitch_rad"], [0, 1, 0])),
                            np_ekf.aa_quat(e["roll_rad"], [1, 0, 0]))
        row = np.array([e["timestamp"], e["x_m"], e["y_m"], e["z_m"], q[1], q[2], q[3], q[0], e["vx"], e["vy"], e["vz"], e["roll_vel"],
                        e["pitch_vel"], e["yaw_vel"]])
        self.imu.append(np.array([t, *gyro]))
        if abs(row[1]) < 1e-9 or abs(row[2]) < 1e-9:
            return
        self.odom.append(row)

    def CallbackPointCloud(self, raw, point_time, stamp):
        o, cfg = self.o, self.cfg
        if not self.odom:
            return None
        while self.imu and self.imu[0][0] < stamp - 1.0:
            self.imu.popleft()
        while self.odom and self.odom[0][0] < stamp - 1.0:
            self.odom.popleft()
        imu, od = np.array(self.imu), np.array(self.odom)
        scan_end = stamp - cfg.d_lidar_time_delay
        keep = o.filter_points_by_distance(raw, cfg.d_input_max_dist)
        xyz, tt = raw[keep], point_time[keep]
        front = float(tt[0])
        s_cur = scan_end + front
        iok, itime, irot = o.imu_deskew_info(imu[:, 0].copy(), imu[:, 1:].copy(), s_cur, scan_end)
        ook, inc = o.odom_deskew_info(od, s_cur, scan_end)
        if not (iok and ook):
            return None
        und = o.deskew_points(xyz, tt - np.float32(front), itime, irot, s_cur, scan_end, inc)
        pok, sync_ego = o.get_interpolated_pose(od, scan_end)
        if not pok:
            return None
        src = und[o.voxel_downsample(und, cfg.d_input_voxel_ds_m)]
        ref = o.register(self.map, src, sync_ego.astype(np.float64) @ cfg.tf_ego_to_lidar, o.default_config(2))
        if not ref["is_success"]:
            return None
        ego = ref["T"] @ np.linalg.inv(cfg.tf_ego_to_lidar)
        cov = o.shape_odom_covariance(ref["local_cov"], ego, ref["fitness"])
        from elimaloc_amd.stream import rot_to_quat_xyzw
        self.ekf.update_pcm_odom(scan_end, ego[:3, 3], rot_to_quat_xyzw(ego[:3, :3]), cov, np_ekf.PCM)
        return dict(pose_ego=ego, time=scan_end, n_source=len(src))


def _closed_loop(oracle, map_points, n_pts, n_scans, native, max_range=40.0, crop_m=None):
    from elimaloc_amd import _lib
    from elimaloc_amd.ekf import EkfAlgorithm, EkfConfig
    from elimaloc_amd.pcm_matching import PcmMatching, PcmMatchingConfig
    from elimaloc_amd.registration import Context, IcpMethod, RegistrationConfig
    from elimaloc_amd.stream import LocalizationStream, rot_to_quat_xyzw
    world = synth.make_world(map_points, seed=1001)
    tf = np.eye(4)
    tf[:3, :3] = synth.rot_zyx(0.0, 0.01, 0.02)
    tf[:3, 3] = [1.2, 0.0, 1.6]
    cfg = PcmMatchingConfig(tf_ego_to_lidar=tf, registration=RegistrationConfig(icp_method=IcpMethod.VGICP))
    ctx = Context(0)
    node = PcmMatching(cfg, ctx)
    node.Init(world)
    ecfg = EkfConfig()
    prod = LocalizationStream(node, EkfAlgorithm(ecfg), native=native)
    drive = synth.Drive()
    # the checker's CPU map: the whole world, or (full-size runs) the part of it the drive's scans can reach
    cworld = world
    if crop_m is not None:
        x0, y0, *_ = drive.at(0.0)
        d = world[:, :2].astype(np.float64) - np.array([float(x0), float(y0)])
        cworld = world[(d * d).sum(axis=1) < crop_m * crop_m]
    chk = OracleStream(oracle, cworld, cfg, {n: getattr(ecfg.c, n) for n, _ in _lib.EkfConfig._fields_})
    rng = np.random.default_rng(42)
    imu_hz, t0 = 200, 500.0
    # initial pose: the truth (what a converged CallbackInitialPose hands over), as PCM_INIT to both filters
    P0 = drive.ego_pose(0.0)
    q0 = rot_to_quat_xyzw(P0[:3, :3])
    k_imu, errs, n_done = 0, [], 0
    for k in range(int(n_scans * imu_hz / 10) + 1):
        t = k / imu_hz
        g, f = drive.imu(t, rng)
        if k == 2:
            prod.ekf.CallbackPcmInitOdom(t0 + t, P0[:3, 3], q0)
            chk.ekf.update_pcm_odom(t0 + t, P0[:3, 3], q0, np.eye(6) * 1e-9, np_ekf.PCM_INIT)
        prod.CallbackImu(t0 + t, g, f)
        chk.CallbackImu(t0 + t, g, f)
        if k > 10 and k % (imu_hz // 10) == 0:
            t_end = t - cfg.d_lidar_time_delay - 0.005   # the scan ended a sensor delay ago
            raw, rel = drive.scan(world, n_pts, t_end, tf, seed=7000 + k, max_range=max_range)
            stamp = t0 + t_end + cfg.d_lidar_time_delay
            a = prod.CallbackPointCloud(raw, rel, stamp)
            b = chk.CallbackPointCloud(raw, rel, stamp)
            assert (a is None) == (b is None)
            if a is None:
                continue
            n_done += 1
            dt, dr = synth.pose_error(b["pose_ego"], a["pose_ego"])
            assert dt <= 1e-4 and dr <= 1e-5, (k, dt, dr)
            assert a["n_source"] == b["n_source"]
            et, er = synth.pose_error(drive.ego_pose(t_end), a["pose_ego"])
            errs.append((et, er))
    assert n_done >= n_scans - 2
    s = prod.ekf.State()
    assert not s["pcm_init_on_going"] and s["state_initialized"]      # the 10-update warm-up is over, prediction runs
    np.testing.assert_allclose(s["x"][:3], chk.ekf.pos, rtol=0, atol=1e-4)
    np.testing.assert_allclose(s["x"][6:9], chk.ekf.vel, rtol=0, atol=1e-3)
    errs = np.array(errs)
    # localisation quality against ground truth (not a parity statement): ICP poses stay within a few cm / 0.2 deg
    assert np.median(errs[:, 0]) < 0.05 and errs[:, 0].max() < 0.15 and errs[:, 1].max() < 0.5 * np.pi / 180
    # the filter follows the drive: final speed and position close to truth
    x, y, yaw, v, *_ = drive.at(k / imu_hz)
    assert abs(np.linalg.norm(s["x"][6:9]) - v) < 0.5 and np.hypot(s["x"][0] - x, s["x"][1] - y) < 0.2
    ctx.close()


def test_closed_loop_stream_matches_checker_chain(oracle):
    _closed_loop(oracle, 100000, 20000, 32, native=False)


def test_closed_loop_stream_native_callback(oracle):
    """The same loop with the node callback as ONE C-ABI call (deskew + VoxelDownsample fused on the device)."""
    _closed_loop(oracle, 100000, 20000, 32, native=True)


def test_closed_loop_stream_full_size_c5(oracle):
    """BASELINE config 5 at its stated size: 131 072-point raw scans against the 10 M-point map, 24 scans in closed loop through
    elm_pcm_callback_point_cloud; the checker chain registers against the part of the map within 90 m of the drive (the scans
    reach 60 m, the drive moves a few metres)."""
    _closed_loop(oracle, 10_000_000, 131072, 24, native=True, max_range=60.0, crop_m=90.0)


def test_deskew_downsample_full_size_kept_in_input_order(oracle):
    """elm_deskew_downsample on a 131 072-point scan: the kept points equal the oracle's deskew -> VoxelDownsample ROW FOR ROW IN INPUT
    ORDER (the reference emits unordered_map order; the device promises input order, and the summation tree of the registration that
    follows depends on it), at the shipped 1.5 m and at a fine 0.2 m voxel."""
    from elimaloc_amd.deskew import PcmDeskew
    from elimaloc_amd.registration import Context
    st = synth.make_deskew_stream(131072, seed=77)
    ctx = Context(0)
    dk = PcmDeskew(ctx)
    front = float(st["time"][0])
    scan_end = st["stamp"]
    scan_cur = scan_end + front
    imu = np.concatenate([st["imu_t"][:, None], st["imu_w"]], axis=1)
    ok_i, itime, irot = oracle.imu_deskew_info(st["imu_t"], st["imu_w"], scan_cur, scan_end)
    ok_o, inc = oracle.odom_deskew_info(st["odom"], scan_cur, scan_end)
    assert ok_i and ok_o
    und = oracle.deskew_points(st["xyz"], st["time"] - np.float32(front), itime, irot, scan_cur, scan_end, inc)
    ok, und_gpu = dk.DeskewPointCloud(st["xyz"], st["time"], st["stamp"], imu, st["odom"])
    assert ok
    # bit for bit, as at 20 000 points (test_deskew_matches_oracle): sinf / cosf by glibc's own algorithm, the rest float32 in the reference's order
    assert np.array_equal(und_gpu, und), f"{int((und_gpu != und).any(axis=1).sum())} of {len(und)} deskewed points differ from the oracle's"
    for vs in (1.5, 0.2):
        ok, kept = dk.DeskewDownsample(st["xyz"], st["time"], st["stamp"], imu, st["odom"], vs)
        assert ok
        # the device downsamples ITS undistorted cloud: compare with the oracle's rule applied to the same cloud
        ref = und_gpu[np.sort(oracle.voxel_downsample(und_gpu, vs))]
        assert kept.shape == ref.shape
        assert np.array_equal(kept, ref)
    ctx.close()
