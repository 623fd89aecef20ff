"""Registration information on the GPU (elm_register_information) against the numpy mirror (tests/reginfo_ref.py),
which is fed the pairs of the public correspondence call at its own g = T p: the sums, the information and the eigenvalues to the
project's sums contract (1e-9 of the largest magnitude of each block), the eigenvectors by their residual and orthogonality, every count
and flag; the chunk and wavefront edges; the identity with the first iteration of the registration; the bytes; the corridor; the misuse;
and the three callers (LoopCloser.Verify, PcmMatching.CallbackPointCloud, the C++ shim)."""
import os
import subprocess

import numpy as np
import pytest

import reginfo_cases as cases
import reginfo_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH = 5.0  # the shipped max_search_dist
COMBOS = [(ref.P2P, 0), (ref.GICP, 0), (ref.VGICP, 0), (ref.AVGICP, 0), (ref.P2P, 1), (ref.GICP, 1)]
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 700]
# At min_eigen_ratio 0 the rank of an exactly singular H (one or two pairs) is decided by rounding, which the sums contract does not pin:
# the small jobs ask with a ratio far above rounding and far below any real eigenvalue ratio.
ROBUST = 1e-9


class Scene:
    """a map with both kinds of covariance and what the mirror needs of it, downloaded once"""

    def __init__(self, ctx, world):
        from elimaloc_amd.registration import VoxelHashMap
        self.ctx, self.world = ctx, world
        self.vm = VoxelHashMap(1.0, 30, ctx)
        self.vm.AddPoints(world)
        self.vm.CalVoxelCovAll()
        self.vm.CalPointCovAll(0.4)
        self.xyz, cov, self.mean = self.vm.Pointcloud(with_cov=True)
        self.cov = cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        self.Sinv = np.linalg.inv(cov)
        self.normal = np.linalg.eigh(cov)[1][:, :, 0]
        _, _, vcov, self.vmean = self.vm.Voxels()
        self.vSinv = np.linalg.inv(vcov)

    def pairs(self, g, method):
        """the pairs of elm_map_get_correspondences at g, as reginfo_ref.job takes them"""
        what = {ref.P2P: 0, ref.GICP: 0, ref.VGICP: 1, ref.AVGICP: 2}[method]
        _, si, ti = self.vm._correspondences(what, g, TH)
        out = []
        for i, t in zip(si.tolist(), ti.tolist()):
            if t < 0:
                out.append((i, np.zeros(3), None, None, True))
            elif method == ref.P2P:
                out.append((i, self.xyz[t], None, self.normal[t], False))
            elif method == ref.GICP:
                out.append((i, self.mean[t], self.Sinv[t], self.normal[t], False))
            else:
                out.append((i, self.vmean[t], self.vSinv[t], None, False))
        return out


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def room(ctx):
    return Scene(ctx, cases.room_points())


def _reg(ctx, method, **kw):
    from elimaloc_amd.registration import Registration, RegistrationConfig
    return Registration(RegistrationConfig(icp_method=int(method), **kw), ctx)


def _room_pose(seed, off=0.04):
    rng = np.random.default_rng(seed)
    return cases.pose(cases.general_rotation(seed, 170.0), cases.ROOM_CENTRE + rng.uniform(-1.0, 1.0, 3) * [2.0, 1.5, 0.5]), off


def _job_inputs(scene, n, seed):
    """(resident scan, pose a few centimetres off the pose the scan was drawn at)"""
    from elimaloc_amd.registration import Scan
    T, off = _room_pose(seed)
    pts = cases.scan_of(scene.world, T, n, seed + 1)
    rng = np.random.default_rng(seed + 2)
    d = np.eye(4)
    d[:3, :3] = ref.exp_so3(rng.normal(0, 0.004, 3))
    d[:3, 3] = rng.normal(0, off, 3)
    return Scan(scene.ctx, pts), T @ d


def block_close(a, b, what, rel=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.abs(b).max()) if b.size else 0.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    assert err <= rel * scale, (what, err, scale)


def compare(got, want, what):
    """a result of the library against the mirror's, by the rules of the issue"""
    for k in ("n_points", "n_pairs", "n_default", "dof", "rank", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("H", "g", "information", "eigenvalues"):
        block_close(got[k], want[k], (what, k))
    for k in ("chi2", "sigma2", "length_scale"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got["H"], got["H"].T) and np.array_equal(got["information"], got["information"].T), what
    if got["n_pairs"]:
        l = got["length_scale"]
        D = np.diag([1.0, 1.0, 1.0, 1.0 / l, 1.0 / l, 1.0 / l])
        S6, lam, V = D @ got["H"] @ D, got["eigenvalues"], got["eigenvectors"]
        assert np.all(np.diff(lam) >= 0), what
        assert np.abs(S6 @ V - V * lam).max() <= 1e-9 * np.abs(lam).max(), what
        assert np.abs(V.T @ V - np.eye(6)).max() <= 1e-12, what
        for k in range(6):
            assert V[int(np.argmax(np.abs(V[:, k]))), k] > 0.0, what


def mirror(scene, sc, T, method, metric, **cfg):
    pts = sc.points()
    return ref.job(T, pts, scene.pairs(ref.transform(T, pts), method), TH, method, metric, **cfg)


def _no_flagged_covariance(scene):
    flags = int(scene.vm.info().layout_flags)
    assert flags & 8 and flags & 16, flags  # bits 3 / 4: no point / voxel covariance outside the compact form, so Sbar is that form


# ---------------------------------------------------------------- against the mirror
@pytest.mark.parametrize("method,metric", COMBOS)
def test_every_size_alone_against_the_mirror(room, method, metric):
    from elimaloc_amd.registration import RegInfoConfig
    reg = _reg(room.ctx, method)
    for n in SIZES:
        sc, T = _job_inputs(room, n, 100 + n)
        got = reg.Information([sc], room.vm, T[None], RegInfoConfig(metric=metric, min_eigen_ratio=ROBUST))[0]
        want = mirror(room, sc, T, method, metric, min_eigen_ratio=ROBUST)
        assert got["n_points"] == n and got["n_pairs"] >= n
        compare(got, want, (method, metric, n))
    _no_flagged_covariance(room)


@pytest.mark.parametrize("method,metric", COMBOS)
def test_three_ragged_jobs_in_one_call(room, method, metric):
    from elimaloc_amd.registration import RegInfoConfig
    reg = _reg(room.ctx, method)
    jobs = [_job_inputs(room, n, 300 + n) for n in (257, 3, 700)]
    got = reg.Information([j[0] for j in jobs], room.vm, np.stack([j[1] for j in jobs]), RegInfoConfig(metric=metric, min_eigen_ratio=ROBUST))
    for k, (sc, T) in enumerate(jobs):
        want = mirror(room, sc, T, method, metric, min_eigen_ratio=ROBUST)
        compare(got[k], want, (method, metric, k))
        if k != 1:
            assert got[k]["rank"] == 6 and got[k]["status"] == 0 and got[k]["sigma2"] > 0.0


def test_no_pair_few_pairs_and_the_default_target(room):
    from elimaloc_amd.registration import RegInfoConfig, Scan
    for method, metric in COMBOS:
        reg = _reg(room.ctx, method)
        sc, T = _job_inputs(room, 65, 41)
        far = T.copy()
        far[:3, 3] += [500.0, 300.0, 0.0]  # no map and no origin within reach
        one, T1 = _job_inputs(room, 1, 42)
        two, T2 = _job_inputs(room, 2, 43)
        near0 = Scan(room.ctx, np.random.default_rng(5).uniform(-1.5, 1.5, (40, 3)).astype(np.float32))  # around the origin: the default target
        T0 = cases.pose(cases.general_rotation(44, 90.0), [0.3, -0.2, 0.1])
        scans, poses = [sc, one, two, near0, sc], np.stack([far, T1, T2, T0, T])
        for sigma2 in (0.0, 0.0025):
            got = reg.Information(scans, room.vm, poses, RegInfoConfig(metric=metric, min_eigen_ratio=ROBUST, sigma2=sigma2))
            want = [mirror(room, s, P, method, metric, min_eigen_ratio=ROBUST, sigma2=sigma2) for s, P in zip(scans, poses)]
            for k in range(5):
                compare(got[k], want[k], (method, metric, sigma2, k))
            assert got[0]["status"] == ref.NO_PAIRS | ref.DEGENERATE and got[0]["n_points"] == 65 and not got[0]["H"].any() and got[0]["no_pairs"]
            if method != ref.AVGICP:  # (AVGICP pairs a point with up to seven voxels)
                assert got[1]["n_pairs"] == 1 and got[2]["n_pairs"] == 2
            if method == ref.P2P and metric == 0:
                assert got[1]["rank"] == 3 and got[1]["dof"] == 0 and got[2]["rank"] == 5 and got[2]["dof"] == 1
                assert got[1]["no_dof"] == (sigma2 == 0.0) and got[1]["information"].any() == (sigma2 > 0.0) and got[1]["H"].any()
            if metric == 0 and method != ref.AVGICP:  # the plane metric drops the default target; AVGICP has none
                assert got[3]["n_default"] == got[3]["n_pairs"] == 40
            else:
                assert got[3]["n_default"] == 0 and got[3]["n_pairs"] == 0
            assert got[4]["status"] == 0


def test_an_empty_map(ctx):
    from elimaloc_amd.registration import RegInfoConfig, Scan, VoxelHashMap
    empty = VoxelHashMap(1.0, 30, ctx)
    empty.AddPoints(np.zeros((0, 3), np.float32))
    sc = Scan(ctx, np.random.default_rng(1).uniform(-2, 2, (70, 3)).astype(np.float32))
    for method in (ref.P2P, ref.GICP, ref.VGICP, ref.AVGICP):
        got = _reg(ctx, method).Information([sc, sc], empty, np.stack([np.eye(4)] * 2), RegInfoConfig())
        for r in got:
            assert r["status"] == ref.NO_PAIRS | ref.DEGENERATE and r["n_points"] == 70 and r["n_pairs"] == 0 and not r["H"].any()


@pytest.mark.parametrize("form", ["tiled", "direct"])
def test_the_tiled_grid_and_a_map_without_a_search_index(form, monkeypatch):
    from elimaloc_amd.registration import Context, RegInfoConfig
    if form == "tiled":
        monkeypatch.setenv("ELM_KERNEL", "grid")
        monkeypatch.setenv("ELM_GRID", "tiled")
    else:
        monkeypatch.setenv("ELM_KERNEL", "direct")
    c = Context(0)
    try:
        scene = Scene(c, cases.room_points())
        jobs = [_job_inputs(scene, n, 500 + n) for n in (257, 64, 700)]
        for method, metric in COMBOS:
            got = _reg(c, method).Information([j[0] for j in jobs], scene.vm, np.stack([j[1] for j in jobs]), RegInfoConfig(metric=metric))
            for k, (sc, T) in enumerate(jobs):
                compare(got[k], mirror(scene, sc, T, method, metric), (form, method, metric, k))
        info = scene.vm.info()
        assert bool(int(info.layout_flags) & 4) == (form == "tiled")
        if form == "direct":
            assert int(info.index_bytes) == 0  # nothing was built: the plain walk paired the points
    finally:
        c.close()


# ---------------------------------------------------------------- the identity with the registration
@pytest.mark.parametrize("method", [ref.P2P, ref.GICP, ref.VGICP, ref.AVGICP])
def test_the_first_iteration_of_the_registration_has_these_sums(room, method):
    """trace[0] of RunRegister(max_iteration = 1) at the same pose: J^T J is H, J^T r is g, n_corr is n_pairs"""
    from elimaloc_amd.registration import RegInfoConfig, Scan
    T, _ = _room_pose(77)
    pts = cases.scan_of(room.world, T, 700, 78)
    T0 = T.copy()
    T0[:3, 3] += [0.03, -0.02, 0.025]
    T0[:3, :3] = T0[:3, :3] @ ref.exp_so3([0.003, -0.002, 0.004])
    reg = _reg(room.ctx, method, max_iteration=1)
    assert reg.config_.max_search_dist == TH
    det = reg.RunRegister(pts, room.vm, T0, trace=True)[4]
    it = det["iters"][0]
    got = reg.Information([Scan(room.ctx, pts)], room.vm, T0[None], RegInfoConfig())[0]
    block_close(it["JTJ"], got["H"], (method, "JTJ"))
    block_close(it["JTr"], got["g"], (method, "JTr"))
    assert int(it["n_corr"]) == got["n_pairs"] and got["n_default"] == 0
    assert not int(room.vm.info().layout_flags) & (128 | 256)  # no asymmetric stored inverse
    _no_flagged_covariance(room)


# ---------------------------------------------------------------- bytes
@pytest.mark.parametrize("method,metric", [(ref.P2P, 0), (ref.GICP, 1), (ref.AVGICP, 0)])
def test_bytes_are_the_job_s_own(room, method, metric):
    from elimaloc_amd.registration import RegInfoConfig
    reg = _reg(room.ctx, method)
    cfg = RegInfoConfig(metric=metric)
    jobs = [_job_inputs(room, n, 600 + n) for n in (700, 257, 65, 300)]
    scans, poses = [j[0] for j in jobs], np.stack([j[1] for j in jobs])
    raw = lambda idx: [bytes(r) for r in list(reg.Information([scans[k] for k in idx], room.vm, poses[idx], cfg, raw=True))[:len(idx)]]
    a, b = raw([0, 1, 2, 3]), raw([0, 1, 2, 3])
    assert a == b  # the same bytes on every run
    alone = raw([0])[0]
    assert alone == a[0] == raw([3, 2, 0])[2] == raw([1, 0, 3])[1]  # alone, first, last, in the middle
    assert raw([2, 1])[0] == a[2] and len(set(a)) == 4


# ---------------------------------------------------------------- degeneracy
@pytest.fixture(scope="module")
def corridor(ctx):
    return Scene(ctx, cases.corridor_points())


@pytest.mark.parametrize("method", [ref.P2P, ref.GICP])
def test_the_corridor_is_free_along_its_axis(corridor, method):
    from elimaloc_amd.posegraph import PoseGraph
    from elimaloc_amd.registration import RegInfoConfig, Scan
    T = cases.pose(cases.rot_x(0.1), [0.5, 0.2, 0.3])
    sc = Scan(corridor.ctx, cases.scan_of(corridor.world, T, 600, 9, noise=0.01, within=8.0))
    assert not corridor.cov[:, 0, 1:].any()  # no neighbourhood covariance couples x with y or z: every plane normal has an x component of 0
    got = _reg(corridor.ctx, method).Information([sc], corridor.vm, T[None], RegInfoConfig(metric=1, min_eigen_ratio=1e-6))[0]
    compare(got, mirror(corridor, sc, T, method, 1, min_eigen_ratio=1e-6), ("corridor", method))
    assert got["rank"] == 5 and got["degenerate"] and got["status"] == ref.DEGENERATE
    assert got["eigenvalues"][0] <= 1e-9 * got["eigenvalues"][5] and np.array_equal(np.abs(got["eigenvectors"][:, 0]), cases.CORRIDOR_AXIS)
    info = got["information"]
    assert not (info @ cases.CORRIDOR_AXIS).any() and info.any()  # exactly zero along the axis
    assert np.linalg.eigvalsh(info)[1] > 0.0
    pg = PoseGraph(4, 4, corridor.ctx, prior_capacity=4)  # both calls require exact symmetry
    pg.AddNodes(np.stack([np.eye(4), T]), [1, 0])
    pg.AddEdges([0], [1], T[None], info)
    pg.AddPriors([1], T[None], info)
    assert pg.Size()[1] == 1 and pg.PriorCount() == 1


def test_the_room_is_constrained(room):
    from elimaloc_amd.registration import RegInfoConfig
    sc, T = _job_inputs(room, 700, 900)
    for method, metric in COMBOS:
        got = _reg(room.ctx, method).Information([sc], room.vm, T[None], RegInfoConfig(metric=metric, min_eigen_ratio=1e-6))[0]
        assert got["rank"] == 6 and got["status"] == 0 and got["eigenvalues"][0] > 1e-6 * got["eigenvalues"][5], (method, metric)
        np.testing.assert_array_equal(got["information"], got["H"] / got["sigma2"])


# ---------------------------------------------------------------- misuse
def test_misuse_is_refused_and_the_context_stays_usable(room):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import Context, ElmError, RegInfoConfig, RegistrationConfig, Scan, VoxelHashMap
    ctx = room.ctx
    sc, T = _job_inputs(room, 65, 1000)
    reg = _reg(ctx, ref.P2P)

    def good():
        r = reg.Information([sc], room.vm, T[None], RegInfoConfig())[0]
        assert r["status"] == 0 and r["n_pairs"] >= 65

    def refused(code, scans, vm, poses, cfg=None, m_config=None, r=reg):
        with pytest.raises(ElmError) as e:
            r.Information(scans, vm, poses, cfg, m_config)
        assert f"({code})" in str(e.value), str(e.value)
        good()

    good()
    other = Context(0)
    try:
        foreign_map = VoxelHashMap(1.0, 30, other)
        foreign_map.AddPoints(room.world[:500])
        refused(-1, [sc], foreign_map, T[None])
        refused(-1, [Scan(other, sc.points())], room.vm, T[None])
    finally:
        other.close()
    bad = T.copy()
    bad[1, 3] = np.nan
    refused(-1, [sc], room.vm, bad[None])
    refused(-1, [], room.vm, np.zeros((0, 4, 4)))
    refused(-1, [sc], room.vm, T[None], RegInfoConfig(min_eigen_ratio=1.0))
    refused(-1, [sc], room.vm, T[None], RegInfoConfig(metric=1), RegistrationConfig(icp_method=ref.VGICP))
    refused(-5, [sc], room.vm, T[None], None, RegistrationConfig(icp_method=ref.GICP, use_radar_cov=1))
    # missing covariances: the registration's own code and text
    plain = VoxelHashMap(1.0, 30, ctx)
    plain.AddPoints(room.world)
    for method, text in ((ref.GICP, "GICP needs elm_map_cal_point_cov_all()"), (ref.VGICP, "VGICP/AVGICP need elm_map_cal_voxel_cov_all()")):
        with pytest.raises(ElmError, match=r"\(-1\).*" + text.replace("(", r"\(").replace(")", r"\)").replace("/", "/")):
            _reg(ctx, method).Information([sc], plain, T[None])
        good()
    with pytest.raises(ElmError, match=r"\(-1\).*GICP needs"):
        reg.Information([sc], plain, T[None], RegInfoConfig(metric=1))  # the plane metric reads the point covariances
    good()
    # a batch in flight owns the context's stream and scratch
    reg.EnqueueBatch([sc], room.vm, T[None])
    with pytest.raises(ElmError) as e:
        reg.Information([sc], room.vm, T[None])
    assert "(-1)" in str(e.value)
    reg.FinishBatch()
    good()
    # a device group, a hook
    grp = Context.multi([0, 0])
    try:
        gvm = VoxelHashMap(1.0, 30, grp)
        gvm.AddPoints(room.world[:2000])
        with pytest.raises(ElmError) as e:
            _reg(grp, ref.P2P).Information([Scan(grp, sc.points())], gvm, T[None])
        assert "(-5)" in str(e.value)
        del gvm
    finally:
        grp.close()
    good()
    ctx.set_allreduce_hook(lambda buf, n, stream: 0)
    try:
        with pytest.raises(ElmError) as e:
            reg.Information([sc], room.vm, T[None])
        assert "(-5)" in str(e.value)
    finally:
        ctx.set_allreduce_hook(None)
    good()
    assert _lib.REGINFO_MAX_JOBS == 4096


# ---------------------------------------------------------------- the callers
def test_loop_closer_verify_with_information(room):
    from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
    from elimaloc_amd.registration import RegInfoConfig
    ctx = room.ctx
    lc = LoopCloser(PlaceDatabase(PlaceConfig(), 16, ctx), 1.0, 30, window=8)
    yaw = lambda a: np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    poses = [cases.pose(yaw(0.9 * k), cases.ROOM_CENTRE + [1.5 * np.cos(k), 1.0 * np.sin(k), 0.1 * k - 0.3]) for k in range(6)]
    for k, P in enumerate(poses):  # a small ring of entries inside the room
        lc.Insert(cases.scan_of(room.world, P, 700, 1200 + k), P)
    Tq = poses[2] @ cases.pose(yaw(0.05), [0.2, -0.1, 0.02])
    query = cases.scan_of(room.world, Tq, 700, 1300)
    cand = dict(entry=2, yaw_rad=0.05)
    plain = lc.Verify(query, cand)
    assert set(plain) == {"T", "is_success", "fitness_score", "local_cov", "candidates", "T_entry_query"}  # today's keys
    res = lc.Verify(query, cand, information=RegInfoConfig())
    assert set(res) == set(plain) | {"information", "reginfo"} and res["T"].tobytes() == plain["T"].tobytes()
    info = res["information"]
    assert res["is_success"] and res["reginfo"]["status"] == 0 and res["reginfo"]["n_points"] == 700
    assert np.array_equal(info, info.T) and np.linalg.eigvalsh(info)[0] >= -1e-9 * np.abs(info).max() and info.any()
    entry, _ = lc.Insert(query, res["T"])
    lc.AddLoop(2, entry, res["T_entry_query"], info)
    closed, out = lc.Close()
    assert closed.shape == (7, 4, 4) and np.isfinite(closed).all()
    assert lc.Verify(query, cand, information=RegInfoConfig(metric=1))["reginfo"]["dof"] == res["reginfo"]["n_pairs"] - 6


def test_callback_point_cloud_with_information():
    from elimaloc_amd import synth
    from elimaloc_amd.pcm_matching import PcmMatching, PcmMatchingConfig
    from elimaloc_amd.registration import Context, IcpMethod, RegInfoConfig, RegistrationConfig, Scan
    world = synth.make_world(20000, seed=1001)
    c = Context(0)
    try:
        tf = np.eye(4)
        tf[:3, 3] = [1.2, 0.0, 1.6]
        node = PcmMatching(PcmMatchingConfig(tf_ego_to_lidar=tf, registration=RegistrationConfig(icp_method=IcpMethod.VGICP)), c)
        node.Init(world)
        st = synth.make_deskew_stream(700, seed=9, stamp=2000.0)
        od = st["odom"].copy()
        od[:, 1:4] += [-8.0, 3.0, 0.3]
        from elimaloc_amd.pcm_matching import get_interpolated_pose
        ok, ego_end = get_interpolated_pose(od, st["stamp"] - node.cfg_.d_lidar_time_delay)
        lidar_end = ego_end.astype(np.float64) @ tf
        near = world[np.linalg.norm(world - lidar_end[:3, 3].astype(np.float32), axis=1) < 40.0]
        pick = near[np.random.default_rng(4).choice(len(near), 700, replace=False)].astype(np.float64)
        raw = ((pick - lidar_end[:3, 3]) @ lidar_end[:3, :3]).astype(np.float32)
        imu = np.concatenate([st["imu_t"][:, None], st["imu_w"]], axis=1)
        a = node.CallbackPointCloud(raw, st["time"], st["stamp"], imu, od)
        b = node.CallbackPointCloud(raw, st["time"], st["stamp"], imu, od, information=RegInfoConfig())
        assert ok and a is not None and b is not None and set(b) == set(a) | {"information"}
        assert b["pose_lidar"].tobytes() == a["pose_lidar"].tobytes() and "information_ms" in node.timings_
        r = b["information"]
        assert r["n_points"] == b["n_source"] and r["n_pairs"] > 0 and np.array_equal(r["information"], r["information"].T)
    finally:
        c.close()


def test_the_cpp_shim_gives_the_python_call_s_bytes(room, tmp_path):
    """tests/shim_harness/registration_information_calls.cpp: the shim's call on the points, poses and map points it is handed, its
    results written out raw, against Registration.Information on the same inputs"""
    from elimaloc_amd.registration import RegInfoConfig, Scan
    exe = tmp_path / "registration_information_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                           "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_harness", "registration_information_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                           "-Wl,-rpath," + libdir, "-o", str(exe)])
    jobs = [_job_inputs(room, n, 1500 + n) for n in (300, 65)]
    room.world.astype(np.float32).tofile(tmp_path / "map.f32")
    for k, (sc, T) in enumerate(jobs):
        sc.points().tofile(tmp_path / f"scan{k}.f32")
        np.ascontiguousarray(T.T).tofile(tmp_path / f"pose{k}.f64")
    subprocess.check_call([str(exe), str(tmp_path), "2"], timeout=120)
    got = (tmp_path / "results.bin").read_bytes()
    # the harness: GICP, the plane metric, min_eigen_ratio 1e-6; it uploads the points it was handed as this process does
    scans = [Scan(room.ctx, sc.points()) for sc, _ in jobs]
    want = _reg(room.ctx, ref.GICP).Information(scans, room.vm, np.stack([T for _, T in jobs]), RegInfoConfig(metric=1, min_eigen_ratio=1e-6), raw=True)
    assert got == b"".join(bytes(want[k]) for k in range(2)) and len(got) == 2 * 1008
