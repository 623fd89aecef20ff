"""The reference's public correspondence calls -- VoxelHashMap::GetCorrespondencePoints / GetCorrespondencesCov /
GetCorrespondencesAllCov / GetAdjacentVoxels (vhm.cpp:31-243) -- as calls of their own: the PAIRS of the production search (the QUERY
instantiations of the grid / voxel-list kernels, i.e. the code the fused accumulate kernels run) against the oracle, pair for pair,
index for index, on every index form; the plain 27-probe walk (ELM_CHECK=query_direct) as the in-product checker."""
import numpy as np
import pytest

from elimaloc_amd import synth


def _queries(world, seed, n=6000):
    """float64 MAP-frame points: transformed scan points (not float32-representable), points beyond the map, points whose 27 voxels are
    all empty but that lie within range of the ORIGIN (the reference's default target, QUIRK), negative coordinates, exact map points."""
    rng = np.random.default_rng(seed)
    scan, Tt = synth.make_scan(world, n, seed=seed)
    T = synth.perturb(Tt, seed=seed + 1, max_trans=0.4, max_rot_deg=1.5)
    g = scan.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    far = rng.uniform(-400, 400, size=(300, 3))
    near0 = rng.uniform(-4.5, 4.5, size=(300, 3)) * np.array([1.0, 1.0, 1.0]) + np.array([0.0, 0.0, 30.0]) * (rng.random((300, 1)) < 0.5)
    exact = world[rng.choice(len(world), 300, replace=False)].astype(np.float64)
    tight0 = rng.uniform(-0.6, 0.6, size=(60, 3))
    odd = np.array([[np.nan, 0.0, 0.0], [np.inf, 1.0, 1.0], [1.0, -np.inf, 2.0], [1e300, 0.0, 0.0], [3e9, -3e9, 1.0]])  # pair with nothing
    return np.concatenate([g, far, near0, tight0, exact, -np.abs(g[:200]), odd])


def _set_env(monkeypatch, kernel_env):
    if kernel_env == "tiled":
        monkeypatch.setenv("ELM_KERNEL", "grid"); monkeypatch.setenv("ELM_GRID", "tiled")
    elif kernel_env == "grid":
        monkeypatch.setenv("ELM_KERNEL", "grid")
    elif kernel_env == "query_direct":
        monkeypatch.setenv("ELM_CHECK", "query_direct")
    else:
        monkeypatch.setenv("ELM_KERNEL", kernel_env)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel_env", ["grid", "tiled", "lists", "direct", "query_direct"])
def test_correspondence_calls_match_the_oracle_pair_for_pair(oracle, kernel_env, monkeypatch):
    from elimaloc_amd.registration import Context, VoxelHashMap
    _set_env(monkeypatch, kernel_env)
    rng = np.random.default_rng(3)
    world = np.concatenate([synth.make_world(80000, seed=31), rng.uniform(-40, 40, size=(4000, 3)) * np.array([1.0, 1.0, 0.1])]).astype(np.float32)
    world = world[(np.abs(world[:, :2]) > 6.0).any(axis=1)]  # nothing near the origin: the default target is reachable
    c = Context(0)
    try:
        for vs, th in ((1.0, 5.0), (0.7, 1.2)):
            vm = VoxelHashMap(vs, 30, c)
            vm.AddPoints(world)
            vm.CalVoxelCovAll()
            om = oracle.Map(vs, 30)
            om.add_points(world)
            om.cal_voxel_cov_all()
            q = _queries(world, seed=100 + int(vs * 10))
            # GetCorrespondencePoints
            acc, tgt, _ = om.nearest_points(q, th)
            sp, tp, si, ti = vm.GetCorrespondencePoints(q, th, indices=True)
            assert np.array_equal(si, np.flatnonzero(acc))
            assert np.array_equal(sp, q[acc]) and np.array_equal(tp, tgt[acc])
            assert (ti == -1).sum() == int((acc & (np.abs(tgt).sum(axis=1) == 0)).sum()) and (ti == -1).sum() > 0
            # GetCorrespondencesCov
            acc, mean, cov = om.nearest_voxel(q, th)
            sp, tm, tc, si, ti = vm.GetCorrespondencesCov(q, th, indices=True)
            assert np.array_equal(si, np.flatnonzero(acc))
            assert np.array_equal(tm, mean[acc])
            np.testing.assert_allclose(tc, cov[acc], rtol=1e-9, atol=1e-12)
            assert (ti == -1).any()
            # GetCorrespondencesAllCov
            osrc, omean, ocov = om.all_cov_pairs(q, th)
            sp, tm, tc, si, ti = vm.GetCorrespondencesAllCov(q, th, indices=True)
            assert np.array_equal(si, osrc) and np.array_equal(tm, omean)
            np.testing.assert_allclose(tc, ocov, rtol=1e-9, atol=1e-12)
            assert len(si) > len(q)  # several pairs per point
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel_env", ["grid", "tiled", "query_direct"])
def test_exact_ties_pick_the_reference_s_neighbour(oracle, kernel_env, monkeypatch):
    """Query points exactly half-way between lattice points: 2, 4 or 8 candidates at bit-identical distance; the pair is the FIRST strict
    minimum of the reference's walk (bucket visiting order, insertion order inside a bucket)."""
    from elimaloc_amd.registration import Context, VoxelHashMap
    from test_gpu_parity import _tie_world
    _set_env(monkeypatch, kernel_env)
    lattice, scan = _tie_world()
    c = Context(0)
    try:
        vm = VoxelHashMap(1.0, 30, c)
        vm.AddPoints(lattice)
        om = oracle.Map(1.0, 30)
        om.add_points(lattice)
        q = scan.astype(np.float64)
        acc, tgt, _ = om.nearest_points(q, 5.0)
        sp, tp, si, ti = vm.GetCorrespondencePoints(q, 5.0, indices=True)
        assert np.array_equal(si, np.flatnonzero(acc)) and np.array_equal(tp, tgt[acc])
    finally:
        c.close()


@pytest.mark.gpu
def test_empty_and_degenerate_queries(oracle):
    from elimaloc_amd.registration import Context, VoxelHashMap
    c = Context(0)
    try:
        vm = VoxelHashMap(1.0, 30, c)
        vm.AddPoints(synth.make_world(5000, seed=2))
        sp, tp = vm.GetCorrespondencePoints(np.zeros((0, 3)), 5.0)
        assert sp.shape == (0, 3) and tp.shape == (0, 3)
        one = np.array([[1000.0, 1000.0, 1000.0]])
        assert vm.GetCorrespondencePoints(one, 5.0)[0].shape == (0, 3)
        with pytest.raises(Exception):
            vm.GetCorrespondencesCov(one, 5.0)  # no CalVoxelCovAll yet: the same refusal as a VGICP registration
    finally:
        c.close()


def test_get_adjacent_voxels_is_key_arithmetic(oracle):
    """vhm.cpp:208-243: range 0 the voxel itself, 1 the seven (0, +x, -x, +y, -y, +z, -z), anything else the 27 (x slowest)."""
    from elimaloc_amd.registration import VoxelHashMap
    vm = VoxelHashMap.__new__(VoxelHashMap)
    vm.voxel_size_ = 0.7
    p = np.array([-0.1, 3.6, 0.69])
    v = np.floor(p / 0.7).astype(int)
    assert np.array_equal(vm.GetAdjacentVoxels(p, 0), v[None])
    a1 = vm.GetAdjacentVoxels(p, 1)
    assert np.array_equal(a1 - v, [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    for r in (2, 5):
        a = vm.GetAdjacentVoxels(p, r)
        assert a.shape == (27, 3) and np.array_equal(a[0] - v, [-1, -1, -1]) and np.array_equal(a[1] - v, [-1, -1, 0]) and np.array_equal(a[9] - v, [0, -1, -1])


def test_oracle_all_cov_pairs_against_brute_force(oracle):
    """The oracle's GetCorrespondencesAllCov call against plain numpy: floor key of the query, the seven neighbour keys in the
    reference's order, voxels looked up by their STORED (truncated) keys, mean within range."""
    world = synth.make_world(20000, seed=9)
    om = oracle.Map(1.0, 30)
    om.add_points(world)
    om.cal_voxel_cov_all()
    keys, npts, covs, means = om.voxels()
    table = {tuple(int(x) for x in k): i for i, k in enumerate(keys)}
    rng = np.random.default_rng(4)
    q = np.concatenate([world[rng.choice(len(world), 500)].astype(np.float64) + rng.normal(0, 0.3, (500, 3)), rng.uniform(-3, 3, (100, 3))])
    src, mean, cov = om.all_cov_pairs(q, 1.1)
    exp_src, exp_mean = [], []
    for i, p in enumerate(q):
        f = np.floor(p / 1.0).astype(int)
        for off in ([0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]):
            v = table.get(tuple(int(x) for x in f + np.array(off)))
            if v is None or npts[v] == 0:
                continue
            d = means[v] - p
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] < 1.1 * 1.1:
                exp_src.append(i); exp_mean.append(means[v])
    assert np.array_equal(src, np.array(exp_src)) and np.array_equal(mean, np.array(exp_mean))
    assert len(src) > 600


def _pairs_for_align(seed, n=4000):
    rng = np.random.default_rng(seed)
    src = rng.uniform(-40, 40, (n, 3)) * np.array([1.0, 1.0, 0.1])
    T = synth.perturb(np.eye(4), seed=seed + 1, max_trans=2.0, max_rot_deg=20.0)
    tgt = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.08, (n, 3))
    tgt[::50] += rng.normal(0, 6.0, (len(tgt[::50]), 3))  # some pairs far out: tiny weights, the VGICP skip (reg.cpp:201)
    A = rng.normal(0, 0.3, (n, 3, 3))
    cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    cov[::7] = np.eye(3)                                   # identity covariances (a neighbourhood of the point alone)
    cov[3::11] += rng.normal(0, 0.02, (len(cov[3::11]), 3, 3))  # NOT symmetric (the regularised covariance of a rank-deficient neighbourhood)
    return src, tgt, cov, T


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1, 2])
def test_align_clouds_local_on_explicit_pairs(oracle, method):
    """Registration::AlignCloudsLocal / PointCov / VoxelCov (reg.cpp:15-225) as calls of their own, against the oracle's restatement:
    step, local_cov (GICP), d_fitness_score_; symmetric and non-symmetric covariances, identity covariances, use_radar_cov."""
    from elimaloc_amd.registration import Context, Registration, RegistrationConfig, IcpMethod
    c = Context(0)
    try:
        for seed in (1, 2):
            src, tgt, cov, T = _pairs_for_align(10 * seed + method)
            for radar in ((False, True) if method else (False,)):
                rng = np.random.default_rng(seed)
                scov = rng.normal(0, 0.05, (len(src), 3, 3)) if radar else None
                cfg = RegistrationConfig(icp_method=IcpMethod(method), use_radar_cov=int(radar))
                reg = Registration(cfg, c)
                ref = oracle.align_clouds_local(method, src, tgt, None if method == 0 else cov, T, 5.0,
                                                oracle.default_config(method, use_radar_cov=int(radar)), src_cov=scov)
                if method == 0:
                    step = reg.AlignCloudsLocal(src, tgt, T, 5.0)
                elif method == 1:
                    step, lc = reg.AlignCloudsLocalPointCov(src, tgt, cov, T, 5.0, source_cov=scov)
                    np.testing.assert_allclose(lc, ref["local_cov"], rtol=1e-7, atol=1e-12)
                else:
                    step = reg.AlignCloudsLocalVoxelCov(src, tgt, cov, T, 5.0, source_cov=scov)
                np.testing.assert_allclose(step, ref["T"], rtol=0, atol=1e-10)
                assert abs(reg.d_fitness_score_ - ref["fitness"]) <= 1e-9 * max(abs(ref["fitness"]), 1e-12)
        # no pairs at all: the zero system -> the identity step, fitness 0 / 0
        step = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), c).AlignCloudsLocal(np.zeros((0, 3)), np.zeros((0, 3)), np.eye(4), 5.0)
        assert np.array_equal(step, np.eye(4))
    finally:
        c.close()


def _singular_pair_sets():
    """(name, source points, residuals target - source, lm_lambda, components of x = (t, w) that the rule zeroes).  last_icp_pose is the
    identity, so the residual of a pair is target - source.
    * every source point on the sensor's x axis: the row and column of the rotation about x are exact zeros (every term has a factor 0),
      whatever the weights; every source point at the origin: the whole rotation block is.  Both survive the shipped damping
      (h + lambda h = 0 for h = 0) and arbitrary coordinates.
    * one pair (rank 3) and two pairs (rank 5) are singular only without damping (the damped diagonal is 1.5 times the original), and
      their zero pivots are Schur complements: lambda = 0, dyadic coordinates and residuals of squared length 5 (weight 25 / (5 + 5)^2 =
      1 / 4 exactly), so that no operation rounds and the zeros are exact in any elimination order."""
    rng = np.random.default_rng(5)
    on_x = np.zeros((7, 3)); on_x[:, 0] = rng.uniform(-30, 30, 7)
    return [
        ("x-axis", on_x, rng.normal(0, 0.3, (7, 3)), None, [3]),
        ("x-axis-no-damping", on_x, rng.normal(0, 0.3, (7, 3)), 0.0, [3]),
        ("origin", np.zeros((5, 3)), rng.normal(0, 0.3, (5, 3)), None, [3, 4, 5]),
        ("origin-no-damping", np.zeros((5, 3)), rng.normal(0, 0.3, (5, 3)), 0.0, [3, 4, 5]),
        ("one-pair", np.array([[2.0, 2.0, 0.0]]), np.array([[1.0, 2.0, 0.0]]), 0.0, [0, 2, 4]),
        ("two-pairs", np.array([[2.0, 2.0, 0.0], [-2.0, -2.0, 0.0]]), np.array([[1.0, 2.0, 0.0], [2.0, 0.0, -1.0]]), 0.0, [4]),
        ("one-pair-damped", np.array([[2.0, 2.0, 0.0]]), np.array([[1.0, 2.0, 0.0]]), None, []),
        ("two-pairs-damped", np.array([[2.0, 2.0, 0.0], [-2.0, -2.0, 0.0]]), np.array([[1.0, 2.0, 0.0], [2.0, 0.0, -1.0]]), None, []),
    ]


@pytest.mark.gpu
def test_align_clouds_local_on_structurally_singular_pairs(oracle):
    """elm_align_clouds_local (k_align_solve: the scalar elm::ldlt_solve6 on the device) on P2P pair sets whose normal equations are
    singular by construction: the step against oracle.align_clouds_local at the atol 1e-10 of test_align_clouds_local_on_explicit_pairs,
    and the components the rule zeroes exactly 0 -- translations read off the step, a zero rotation vector as the identity rotation in
    bytes, a zero rotation about one axis as the symmetry of the opposite off-diagonal pair (R[1][2] and R[2][1] are c_y a_z -+ sin(angle) a_x
    in rotvec_to_matrix: equal exactly when the x component is 0)."""
    import np_ref
    from elimaloc_amd.registration import Context, Registration, RegistrationConfig, IcpMethod
    c = Context(0)
    try:
        for name, src, res, lam, zeroed in _singular_pair_sets():
            kw = {} if lam is None else {"lm_lambda": lam}
            cfg = RegistrationConfig(icp_method=IcpMethod.P2P, **kw)
            ocfg = oracle.default_config(0, **kw)
            tgt = src + res
            ref = oracle.align_clouds_local(0, src, tgt, None, np.eye(4), 5.0, ocfg)
            reg = Registration(cfg, c)
            step = reg.AlignCloudsLocal(src, tgt, np.eye(4), 5.0)
            np.testing.assert_allclose(step, ref["T"], rtol=0, atol=1e-10, err_msg=name)
            assert abs(reg.d_fitness_score_ - ref["fitness"]) <= 1e-9 * max(abs(ref["fitness"]), 1e-12), name
            # the rule's own zeros for this system (the numpy statement on the oracle's sums) are the ones listed
            D = np.array(ref["JTJ"])
            D[np.diag_indices(6)] = np.diag(D) + cfg.lm_lambda * np.diag(D)
            x = np_ref.eigen_ldlt_solve(D, ref["JTr"])
            assert [i for i in zeroed if x[i] != 0.0] == [], (name, x)
            for i in zeroed:
                if i < 3:
                    assert step[i, 3] == 0.0, (name, i, step[i, 3])
            if all(i in zeroed for i in (3, 4, 5)):
                assert np.array_equal(step[:3, :3], np.eye(3)), name
            else:
                assert not np.array_equal(step[:3, :3], np.eye(3)), name
                for i, (r, q) in ((3, (1, 2)), (4, (0, 2)), (5, (0, 1))):
                    if i in zeroed:
                        assert step[r, q] == step[q, r], (name, i)
            np.testing.assert_allclose(step[:3, 3], x[:3], rtol=1e-11, atol=1e-13, err_msg=name)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,method", [(255, 0), (256, 0), (257, 0), (255, 1), (256, 1), (257, 1), (255, 2), (256, 2), (257, 2), (1024 * 256 + 1, 0)])
def test_align_clouds_local_at_the_block_edges(oracle, method, n):
    """k_align_pairs at the edges of its launch: 255 / 256 / 257 pairs (one workgroup of 256 threads less one, full, and one thread of
    a second) for all three methods, and 1024 * 256 + 1 pairs (P2P): the grid is capped at 1024 workgroups, so one thread takes a second
    trip through the grid-stride loop.  Same assertions as test_align_clouds_local_on_explicit_pairs."""
    from elimaloc_amd.registration import Context, Registration, RegistrationConfig, IcpMethod
    c = Context(0)
    try:
        src, tgt, cov, T = _pairs_for_align(300 + method, n=n)
        reg = Registration(RegistrationConfig(icp_method=IcpMethod(method)), c)
        ref = oracle.align_clouds_local(method, src, tgt, None if method == 0 else cov, T, 5.0, oracle.default_config(method))
        if method == 0:
            step = reg.AlignCloudsLocal(src, tgt, T, 5.0)
        elif method == 1:
            step, lc = reg.AlignCloudsLocalPointCov(src, tgt, cov, T, 5.0)
            np.testing.assert_allclose(lc, ref["local_cov"], rtol=1e-7, atol=1e-12)
        else:
            step = reg.AlignCloudsLocalVoxelCov(src, tgt, cov, T, 5.0)
        np.testing.assert_allclose(step, ref["T"], rtol=0, atol=1e-10)
        assert abs(reg.d_fitness_score_ - ref["fitness"]) <= 1e-9 * max(abs(ref["fitness"]), 1e-12)
        assert not np.array_equal(step, np.eye(4))
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [1, 2])
def test_run_register_with_radar_cov_equals_its_public_pieces(oracle, method):
    """use_radar_cov = 1 (reg.cpp:302-305, 109-111, 188-190): CalFramePointCov on the points under the initial guess feeds the FIRST iteration's
    metric; the re-transform at the end of every iteration leaves the default identity covariance for the later ones."""
    from elimaloc_amd.registration import Context, VoxelHashMap, Registration, RegistrationConfig, IcpMethod
    m = IcpMethod(method)
    world = synth.make_world(60000, seed=87)
    scan, Tt = synth.make_scan(world, 3000, seed=88)
    T0 = synth.perturb(Tt, seed=89, max_trans=0.3, max_rot_deg=1.0)
    rv, av, ev = 0.5, 2.0, 1.0
    c = Context(0)
    try:
        vm = VoxelHashMap(1.0, 30, c)
        vm.AddPoints(world)
        if m == IcpMethod.GICP:
            vm.CalPointCovAll(0.4)
            _, pcov, pmean = vm.Pointcloud(with_cov=True)
        else:
            vm.CalVoxelCovAll()
        cfg = RegistrationConfig(icp_method=m, use_radar_cov=1, range_variance_m=rv, azimuth_variance_deg=av, elevation_variance_deg=ev)
        reg = Registration(cfg, c)
        *_, det = reg.RunRegister(scan, vm, T0, trace=True)
        assert det["iterations"] >= 2
        th = cfg.max_search_dist
        local = scan.astype(np.float64)
        T = np.array(T0, dtype=np.float64)
        for it in range(det["iterations"]):
            x, y, z = local[:, 0], local[:, 1], local[:, 2]
            g = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
            scov = Registration.CalFramePointCov(g, rv, av, ev) if it == 0 else np.broadcast_to(np.eye(3), (len(g), 3, 3))
            if method == 1:
                _, tp, si, ti = vm.GetCorrespondencePoints(g, th, indices=True)
                ok = ti >= 0
                tm = np.where(ok[:, None], pmean[np.maximum(ti, 0)], 0.0)
                tc = np.where(ok[:, None, None], pcov[np.maximum(ti, 0)], np.eye(3))
                step, _ = reg.AlignCloudsLocalPointCov(local[si], tm, tc, T, th, source_cov=scov[si])
            else:
                _, tm, tc, si, ti = vm.GetCorrespondencesCov(g, th, indices=True)
                step = reg.AlignCloudsLocalVoxelCov(local[si], tm, tc, T, th, source_cov=scov[si])
            assert len(si) == int(det["iters"][it]["n_corr"])
            T = T @ step
            np.testing.assert_allclose(T, det["iters"][it]["T"], rtol=0, atol=5e-9)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_run_register_equals_its_public_pieces(oracle, method):
    """RunRegister (one fused kernel per iteration) against the reference's own loop built from the public calls (reg.cpp:317-378):
    TransformPoints -> GetCorrespondence* -> AlignCloudsLocal* -> T <- T * step, iteration by iteration."""
    from elimaloc_amd.registration import Context, VoxelHashMap, Registration, RegistrationConfig, IcpMethod
    m = IcpMethod(method)
    world = synth.make_world(60000, seed=77)
    scan, Tt = synth.make_scan(world, 5000, seed=78)
    T0 = synth.perturb(Tt, seed=79, max_trans=0.3, max_rot_deg=1.0)
    c = Context(0)
    try:
        vm = VoxelHashMap(1.0, 30, c)
        vm.AddPoints(world)
        if m == IcpMethod.GICP:
            vm.CalPointCovAll(0.4)
        if m in (IcpMethod.VGICP, IcpMethod.AVGICP):
            vm.CalVoxelCovAll()
        reg = Registration(RegistrationConfig(icp_method=m), c)
        *_, det = reg.RunRegister(scan, vm, T0, trace=True)
        assert det["iterations"] >= 2
        if m == IcpMethod.GICP:
            _, pcov, pmean = vm.Pointcloud(with_cov=True)
        th = reg.config_.max_search_dist
        local = scan.astype(np.float64)
        T = np.array(T0, dtype=np.float64)
        for it in range(det["iterations"]):
            x, y, z = local[:, 0], local[:, 1], local[:, 2]
            g = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)  # reg.hpp:141-146
            if method == 0:
                _, tp, si, ti = vm.GetCorrespondencePoints(g, th, indices=True)
                step = reg.AlignCloudsLocal(local[si], tp, T, th)
            elif method == 1:
                _, tp, si, ti = vm.GetCorrespondencePoints(g, th, indices=True)
                ok = ti >= 0
                tm = np.where(ok[:, None], pmean[np.maximum(ti, 0)], 0.0)
                tc = np.where(ok[:, None, None], pcov[np.maximum(ti, 0)], np.eye(3))
                step, _ = reg.AlignCloudsLocalPointCov(local[si], tm, tc, T, th)
            else:
                f = vm.GetCorrespondencesCov if method == 2 else vm.GetCorrespondencesAllCov
                _, tm, tc, si, ti = f(g, th, indices=True)
                step = reg.AlignCloudsLocalVoxelCov(local[si], tm, tc, T, th)
            assert len(si) == int(det["iters"][it]["n_corr"])
            T = T @ step
            np.testing.assert_allclose(T, det["iters"][it]["T"], rtol=0, atol=2e-9)
        assert abs(reg.d_fitness_score_ - det["d_fitness"]) <= 1e-8 * max(abs(det["d_fitness"]), 1e-9)
    finally:
        c.close()


def test_cal_frame_point_cov_matches_the_oracle(oracle):
    """Registration::CalFramePointCov (reg.hpp:186-217): R S per point, not symmetric; points on the z axis and at the origin included."""
    from elimaloc_amd.registration import Registration
    rng = np.random.default_rng(8)
    p = rng.uniform(-60, 60, (3000, 3))
    p[:4] = [[0, 0, 0], [0, 0, 5], [-3, 0, 0], [1e-9, -1e-9, 2]]
    for rv, av, ev in ((0.5, 2.0, 1.0), (0.05, 0.4, 0.4), (1.0, 0.0, 30.0)):
        a = oracle.cal_frame_point_cov(p, rv, av, ev)
        b = Registration.CalFramePointCov(p, rv, av, ev)
        np.testing.assert_allclose(b, a, rtol=0, atol=2e-15 * max(1.0, np.abs(a).max()))
        assert np.abs(a - a.transpose(0, 2, 1)).max() > 0.1  # R S, not R S R^T
