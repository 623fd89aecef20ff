"""The production solve step on the device -- k_solve: the world-to-sensor congruence of the covariance methods, the LM damping, wave_ldlt6,
rotvec_to_matrix, the pose update, matrix_to_angle, GICP's local_cov -- fed with the systems of tests/solve_cases.py.

How the sums get in: with an exchange hook installed (elm_comm_set_hook) every iteration runs as reduce-only launch, hook, solve-only
launch, and the hook is handed the device pointer of the packed sums in between: 32 doubles per slot, 21 upper-triangle J^T J entries in
tri(i, j) order, 6 J^T r, the residual sum, n_corr, and three words that carry the rank check.  The hook here overwrites words 0..28 of
every slot with a case (hipMemcpyAsync on the stream it is given, from host arrays that outlive the call; n_corr = the scan's size so the
overlap gate passes, residual sum 0), checks n_doubles == 32 * slots first and never writes outside [0, n_doubles).  max_iteration = 1:
one solve per registration.  The expectations are np_ref.eigen_ldlt_solve's, the compositions are mpmath's at 50 digits.

The worst errors observed on the MI355X are printed by the tests and recorded in their docstrings."""
import ctypes as C

import numpy as np
import pytest

import gate_cases
import np_ref
import solve_cases as SC

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-13     # the oracle / numpy-statement bound of tests/test_oracle.py
POSE_ATOL = 1e-14             # per entry of T for |t| <= 10, and for step_norm: about a dozen roundings of O(1) .. O(10) quantities
EPS = 2.0 ** -52


def _tri(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def _pack(A, b, n_corr):
    w = np.zeros(29)
    for i in range(6):
        for j in range(i, 6):
            w[_tri(i, j)] = A[i, j]
    w[21:27] = b
    w[27] = 0.0
    w[28] = float(n_corr)
    return w


class Rig:
    """one context, one tiny map (343 lattice points, identity covariances: no asymmetric side sums), scans of 1 and 64 stored points"""

    def __init__(self):
        from elimaloc_amd.registration import Context, Scan, VoxelHashMap
        self.ctx = Context(0)
        world = gate_cases.world()[:343]
        self.vm = VoxelHashMap(1.0, 30, self.ctx)
        self.vm.AddPoints(world)
        self.vm.CalVoxelCovAll()
        self.vm.CalPointCovAll(0.4)
        self.scans = {1: Scan(self.ctx, world[:1]), 64: Scan(self.ctx, world[10:74])}
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.hip.hipMemcpyAsync.restype = C.c_int

    def close(self):
        self.scans = None
        self.vm = None
        self.ctx.close()

    def run(self, method, systems, T0s, lam, driver, slots=None):
        """systems: [(A, b)] -- one registration each, scan sizes alternate 1 / 64.  driver "batch" or "stream" (`slots` device slots: in
        the hook form slot s serves the registrations s, s + S, ... of a call whose registrations all end after one iteration)."""
        from elimaloc_amd.registration import IcpMethod, Registration, RegistrationConfig
        B = len(systems)
        sizes = [1 if i % 2 == 0 else 64 for i in range(B)]
        S = B if driver == "batch" else min(slots, B)
        rounds = (B + S - 1) // S
        host = np.zeros((rounds, S, 29))  # stays alive until the call has returned
        for r in range(B):
            host[r // S, r % S] = _pack(systems[r][0], systems[r][1], sizes[r])
        calls = []

        def hook(ptr, n_doubles, stream):
            k = len(calls)
            calls.append(n_doubles)
            if n_doubles != 32 * S:
                raise AssertionError(f"the exchange carries {n_doubles} doubles, expected 32 * {S}")
            if k >= rounds:
                return 0  # (a stream looks once more after its last registration: nothing is iterating)
            for s in range(S):
                if k * S + s >= B:
                    continue
                first = 32 * s
                assert 0 <= first and first + 29 <= n_doubles
                rc = self.hip.hipMemcpyAsync(C.c_void_p(ptr + 8 * first), C.c_void_p(host[k, s].ctypes.data), 29 * 8, 1, C.c_void_p(stream))
                if rc != 0:
                    raise AssertionError(f"hipMemcpyAsync: {rc}")
            return 0

        cfg = RegistrationConfig(icp_method=IcpMethod(method), max_iteration=1, lm_lambda=float(lam))
        reg = Registration(cfg, self.ctx)
        scans = [self.scans[n] for n in sizes]
        self.ctx.set_allreduce_hook(hook)
        try:
            if driver == "batch":
                out = reg.RunRegisterBatch(scans, self.vm, T0s, trace=True)
            else:
                out = reg.RunRegisterStream(scans, self.vm, T0s, slots=slots, trace=True)
        except Exception:
            if self.ctx.hook_error is not None:
                raise self.ctx.hook_error
            raise
        finally:
            err = self.ctx.hook_error
            self.ctx.set_allreduce_hook(None)
        assert err is None, err
        assert len(calls) >= rounds and host.shape == (rounds, S, 29)
        for r, (o, n) in enumerate(zip(out, sizes)):
            assert o["iterations"] == 1 and len(o["iters"]) == 1 and o["gate"] == 0 and o["is_success"], (r, o["gate"])
            assert o["iters"][0]["n_corr"] == n and o["iters"][0]["residual_sum"] == 0.0
        return out


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def cases():
    return SC.cases()


def _bytes_equal(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def _same_results(a, b):
    for p, q in zip(a, b):
        for key in ("x", "T", "JTJ", "JTr"):
            if not _bytes_equal(p["iters"][0][key], q["iters"][0][key]):
                return False
        if not (_bytes_equal(p["T"], q["T"]) and _bytes_equal(p["local_cov"], q["local_cov"]) and _bytes_equal(p["iters"][0]["step_norm"], q["iters"][0]["step_norm"])):
            return False
    return True


def _general_T0(seed):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = np_ref.exp_so3(rng.normal(size=3))
    T[:3, 3] = rng.uniform(-0.5, 0.5, size=3)   # |t0| <= 1
    return T


def _quarter_turn(axis):
    """an exact signed permutation: +90 degrees about `axis`"""
    R = {0: [[1, 0, 0], [0, 0, -1], [0, 1, 0]], 1: [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], 2: [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}[axis]
    T = np.eye(4)
    T[:3, :3] = np.array(R, dtype=np.float64)
    T[:3, 3] = (0.25, -0.5, 0.125)
    return T


def _mp_pose(T0, x):
    """(T0 . [Exp(x[3:]) | x[:3]], angle of Exp(x[3:]) in [0, pi] + |x[:3]|) at 50 digits, rounded to float64"""
    import mpmath as mp
    with mp.workdps(50):
        w = [mp.mpf(float(v)) for v in x[3:]]
        t = [mp.mpf(float(v)) for v in x[:3]]
        th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
        R = mp.eye(3)
        if th != 0:
            a = [v / th for v in w]
            K = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R = mp.eye(3) + mp.sin(th) * K + (1 - mp.cos(th)) * (K * K)
        dT = mp.eye(4)
        for i in range(3):
            for j in range(3):
                dT[i, j] = R[i, j]
            dT[i, 3] = t[i]
        T = mp.matrix([[float(v) for v in row] for row in np.asarray(T0)]) * dT
        ang = th - 2 * mp.pi * mp.floor(th / (2 * mp.pi))
        if ang > mp.pi:
            ang = 2 * mp.pi - ang
        step = ang + mp.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
        return np.array([[float(T[i, j]) for j in range(4)] for i in range(4)]), float(step)


def _chunks(items):
    """batches of 1, 3 and 9 registrations, in turn"""
    out, k, sizes = [], 0, (1, 3, 9)
    while items:
        n = sizes[k % 3]
        out.append(items[:n])
        items = items[n:]
        k += 1
    return out


STREAM_SLOTS = {1: 1, 2: 2, 3: 2, 9: 3}   # 3 registrations through 2 slots: the second round leaves a slot idle


def _drive(rig, method, systems, T0s, lam):
    """both drivers, twice each: the same bytes every time (one solve workgroup per slot; neither the slot index nor the driver leaks)"""
    B = len(systems)
    slots = STREAM_SLOTS.get(B, min(B, 3))
    runs = [rig.run(method, systems, T0s, lam, "batch"), rig.run(method, systems, T0s, lam, "batch"),
            rig.run(method, systems, T0s, lam, "stream", slots), rig.run(method, systems, T0s, lam, "stream", slots)]
    assert _same_results(runs[0], runs[1]) and _same_results(runs[2], runs[3]), "two runs of one batch differ"
    assert _same_results(runs[0], runs[2]), "batch and stream differ"
    return runs[0]


def _check_x(c_name, got, want, zeroed):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=c_name)
    for i in zeroed:
        assert got[i] == 0.0, (c_name, i, got[i])


def _check_pose(name, T0, it, worst):
    T, step = _mp_pose(T0, it["x"])
    assert np.abs(T[:3, 3]).max() <= 10.0, name
    worst[0] = max(worst[0], float(np.abs(it["T"] - T).max()))
    worst[1] = max(worst[1], abs(it["step_norm"] - step))
    np.testing.assert_allclose(it["T"], T, rtol=0, atol=POSE_ATOL, err_msg=name)
    assert abs(it["step_norm"] - step) <= POSE_ATOL, (name, it["step_norm"], step)


def test_p2p_every_case(rig, cases):
    """P2P: the sums are sensor-frame, nothing stands between the injected system and wave_ldlt6.  Every case of solve_cases, grouped by
    LM factor, in batches of 1, 3 and 9 with another case and another T0 per slot, through RunRegisterBatch and RunRegisterStream.
    x within rtol 1e-11 / atol 1e-13 of the numpy statement of Eigen's routine, exact zeros where the rule zeroes, the trace's JTJ / JTr
    the injected bytes, T and step_norm within 1e-14 of the 50-digit composition from the device's own x.
    (solve_cases.ROUNDING_DECIDED -- one case -- is run for its pose composition and determinism only.)
    Observed on the MI355X: worst |T - T_mp| = 6.9e-16, worst |step - step_mp| = 8.9e-16, worst x error = 1.8e-2 of the bound."""
    worst = [0.0, 0.0, 0.0]
    for lam in sorted({c.lam for c in cases}):
        group = [c for c in cases if c.lam == lam]
        seed = 0
        for chunk in _chunks(group):
            T0s = []
            for c in chunk:
                T0s.append([np.eye(4), _quarter_turn(seed % 3), _general_T0(1000 + seed)][seed % 3])
                seed += 1
            out = _drive(rig, 0, [(c.A, c.b) for c in chunk], T0s, lam)
            for c, T0, o in zip(chunk, T0s, out):
                it = o["iters"][0]
                assert _bytes_equal(it["JTJ"], c.A) and _bytes_equal(it["JTr"], c.b), c.name
                assert _bytes_equal(o["T"], it["T"]), c.name
                if c.name not in SC.ROUNDING_DECIDED:
                    _check_x(c.name, it["x"], c.x, SC.zeroed(c))
                    worst[2] = max(worst[2], float(np.max(np.abs(it["x"] - c.x) / (ATOL + RTOL * np.abs(c.x)))))
                _check_pose(c.name, T0, it, worst)
    print(f"P2P: worst |T - T_mp| = {worst[0]:.3e}, worst |step - step_mp| = {worst[1]:.3e}, worst x error / bound = {worst[2]:.3e}")


def test_wave_and_scalar_solves_agree(rig, cases, tmp_path):
    """The same sums through both implementations: wave_ldlt6 (k_solve, on the device) and elm::ldlt_solve6 (the function k_align_solve
    runs, compiled for the host here) agree within the same bound, zeros included."""
    host = SC.build_host_la(tmp_path)
    use = [c for c in cases if c.name not in SC.ROUNDING_DECIDED]
    xs, _ = host([(SC.damped(c.A, c.lam), c.b) for c in use], [])
    k = 0
    for lam in sorted({c.lam for c in use}):
        group = [(i, c) for i, c in enumerate(use) if c.lam == lam]
        for s in range(0, len(group), 9):
            chunk = group[s:s + 9]
            out = rig.run(0, [(c.A, c.b) for _, c in chunk], [np.eye(4)] * len(chunk), lam, "batch")
            for (i, c), o in zip(chunk, out):
                _check_x(c.name, o["iters"][0]["x"], xs[i], [j for j in SC.zeroed(c)])
                k += 1
    assert k == len(use)


def _congruence(T0, A, b):
    R = np.asarray(T0)[:3, :3]
    P = np.zeros((6, 6))
    P[:3, :3] = R
    P[3:, 3:] = R
    return P, P.T @ A @ P, P.T @ b


def _mp_congruence(T0, A, b):
    import mpmath as mp
    with mp.workdps(50):
        P = mp.zeros(6, 6)
        for i in range(3):
            for j in range(3):
                P[i, j] = P[3 + i, 3 + j] = mp.mpf(float(T0[i, j]))
        H = P.T * mp.matrix(A.tolist()) * P
        v = P.T * mp.matrix([float(q) for q in b])
        return np.array([[float(H[i, j]) for j in range(6)] for i in range(6)]), np.array([float(q) for q in v])


def _cov_subset(cases):
    """every case of the discrete families, and four of each larger family"""
    out, seen = [], {}
    for c in cases:
        seen[c.rule] = seen.get(c.rule, 0) + 1
        if c.rule in (SC.PIVOT_ORDER, SC.ZERO_PIVOT, SC.CUTOFF, SC.DAMPING) or seen[c.rule] <= 4:
            out.append(c)
    return out


@pytest.mark.parametrize("method", [1, 2])
def test_covariance_methods_congruence_and_solve(rig, cases, method):
    """GICP and VGICP: the injected sums are world-frame and k_solve applies H_l = P^T H_w P, b_l = P^T b_w, P = diag(R, R), before the
    damping.  R = identity and the three quarter turns (exact signed permutations): the trace's JTJ / JTr equal P^T H P / P^T b in bytes
    -- every entry's destination -- and x follows the rule on H_l (the pivot order moves with the permutation).  One general rotation:
    H_l within 33 eps max|H_w| and b_l within 6 eps max|b_w| of the 50-digit congruence (an entry is a sum of 9 (3) products of three
    (two) factors: at most 11 (4) roundings on terms whose absolute sum is at most 3 max|H_w| (sqrt(3) max|b_w|)), then x against the rule
    on the device's own H_l for the nonsingular cases (a general rotation turns an exact zero pivot into a rounding residue).
    GICP's local_cov: the 50-digit inverse of the damped H_l within rtol 1e-7 / atol 1e-12 where no pivot is zero (observed worst error /
    bound printed); on exactly singular systems the device's LDL^T-based inverse is finite (the reference's PartialPivLU inverse is not:
    DESIGN.md section 7), symmetric, with exactly zero rows and columns at the zero pivots whose column of L is zero.
    Observed on the MI355X: worst local_cov error = 3.9e-6 of the bound (GICP), worst |T - T_mp| = 6.9e-16, worst |step - step_mp| =
    8.9e-16 (both methods)."""
    sub = _cov_subset(cases)
    worst_cov, worst_pose = 0.0, [0.0, 0.0]
    poses = [("identity", np.eye(4)), ("turn-x", _quarter_turn(0)), ("turn-y", _quarter_turn(1)), ("turn-z", _quarter_turn(2)),
             ("general", _general_T0(77))]
    for tag, T0 in poses:
        exact = tag != "general"
        for lam in sorted({c.lam for c in sub}):
            group = [c for c in sub if c.lam == lam and (exact or (SC.nonsingular(c) and c.rule != SC.CUTOFF))]
            for s in range(0, len(group), 9):
                chunk = group[s:s + 9]
                out = _drive(rig, method, [(c.A, c.b) for c in chunk], [T0] * len(chunk), lam)
                for c, o in zip(chunk, out):
                    name = f"{c.name} {tag}"
                    it = o["iters"][0]
                    P, Hl, bl = _congruence(T0, c.A, c.b)
                    if exact:
                        assert np.array_equal(it["JTJ"], Hl) and np.array_equal(it["JTr"], bl), name
                    else:
                        Hm, bm = _mp_congruence(T0, c.A, c.b)
                        np.testing.assert_allclose(it["JTJ"], Hm, rtol=0, atol=33 * EPS * np.abs(c.A).max(), err_msg=name)
                        np.testing.assert_allclose(it["JTr"], bm, rtol=0, atol=6 * EPS * np.abs(c.b).max(), err_msg=name)
                        assert np.array_equal(np.triu(it["JTJ"]), np.tril(it["JTJ"]).T), name
                    Hd = np.triu(it["JTJ"]) + np.triu(it["JTJ"], 1).T   # the solve reads the packed upper triangle
                    D = SC.damped(Hd, lam)
                    if c.name not in SC.ROUNDING_DECIDED:
                        want = np_ref.eigen_ldlt_solve(D, it["JTr"])
                        perm, d, _ = SC.ldlt(D, it["JTr"])
                        zero = [perm[k] for k in range(6) if not abs(d[k]) > SC.TOL and want[perm[k]] == 0.0]
                        _check_x(name, it["x"], want, zero)
                    _check_pose(name, T0, it, worst_pose)
                    cov = o["local_cov"]
                    if method != 1:
                        pass
                    elif SC.nonsingular(c) and c.rule != SC.CUTOFF:
                        inv = SC.mp_solve_matrix(D, it["JTr"])[1]
                        worst_cov = max(worst_cov, float(np.max(np.abs(cov - inv) / (1e-12 + 1e-7 * np.abs(inv)))))
                        np.testing.assert_allclose(cov, inv, rtol=1e-7, atol=1e-12, err_msg=name)
                    elif exact and c.name not in SC.ROUNDING_DECIDED:
                        assert np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T), name
                        for i in SC.isolated_zero_pivots(D):
                            assert not np.any(cov[i, :]) and not np.any(cov[:, i]), (name, i)
    print(f"method {method}: worst local_cov error / bound = {worst_cov:.3e}, worst |T - T_mp| = {worst_pose[0]:.3e}, "
          f"worst |step - step_mp| = {worst_pose[1]:.3e}")


def _rotation_vectors():
    """(label, x): H = I, lam = 0 and b = x, so the solve returns x in bytes"""
    t = np.array([0.25, -0.5, 0.125])
    axes = {"x-largest": np.array([0.8, 0.36, 0.48]), "y-largest": np.array([0.36, 0.8, 0.48]), "z-largest": np.array([0.48, 0.36, 0.8])}
    out = [("angle-0", np.zeros(6))]
    for label, ang in (("1e-170", 1e-170), ("1e-9", 1e-9), ("1", 1.0)):   # 1e-170: the squared norm underflows to 0
        out.append((f"angle-{label}", np.concatenate([t, ang * axes["z-largest"]])))
    for label, ang in (("pi-1e-9", np.pi - 1e-9), ("pi", np.pi), ("4", 4.0)):  # trace <= 0: the quaternion branch by the largest diagonal entry
        for a, axis in axes.items():
            out.append((f"angle-{label}-{a}", np.concatenate([t, ang * axis])))
    return out


def test_rotvec_to_matrix_and_matrix_to_angle_on_the_device(rig):
    """rotvec_to_matrix, the pose update and matrix_to_angle as k_solve runs them: rotation vectors of angle 0, 1e-170, 1e-9, 1,
    pi - 1e-9, pi and 4 (beyond pi: the angle of the matrix is 2 pi - 4), the last three about axes that make each diagonal entry of the
    rotation the largest.  T and step_norm = angle + |x_t| within 1e-14 of the 50-digit values; angle 0 from the identity pose returns the
    identity and a step of 0 in bytes.  Batches of 9, 3 and 1.
    Observed on the MI355X: worst |T - T_mp| = 2.2e-16, worst |step - step_mp| = 4.4e-16."""
    vec = _rotation_vectors()
    assert len(vec) == 13
    worst = [0.0, 0.0]
    T0s_all = [np.eye(4)] + [_general_T0(500 + i) if i % 2 else np.eye(4) for i in range(1, 13)]
    for lo, hi in ((0, 9), (9, 12), (12, 13)):
        chunk, T0s = vec[lo:hi], T0s_all[lo:hi]
        out = _drive(rig, 0, [(np.eye(6), x) for _, x in chunk], T0s, 0.0)
        for (label, x), T0, o in zip(chunk, T0s, out):
            it = o["iters"][0]
            assert _bytes_equal(it["x"], x), label
            _check_pose(label, T0, it, worst)
            if label == "angle-0":
                assert _bytes_equal(it["T"], np.eye(4)) and _bytes_equal(it["step_norm"], 0.0)
            if label == "angle-1e-170":
                assert np.array_equal(it["T"][:3, :3], T0[:3, :3])
    print(f"rotations: worst |T - T_mp| = {worst[0]:.3e}, worst |step - step_mp| = {worst[1]:.3e}")
