"""Registration information (include/elimaloc_hip_reginfo.h) on the CPU: the header against its signature table,
the struct layouts, the argument errors that need no device, the host's call of the pair terms (the code the kernel runs, compiled for
the host) against the numpy mirror (tests/reginfo_ref.py), and the mirror itself against plain matrix algebra, finite differences,
numpy.linalg.eigh and two constructed scenes: a corridor whose axis it must name, and a closed room."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reginfo_cases as cases
import reginfo_ref as ref
import test_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_reginfo.h"
NAMES = {"elm_reginfo_config_default", "elm_register_information", "elm_reginfo_pair_terms"}
METHODS_METRICS = [(ref.P2P, 0), (ref.GICP, 0), (ref.VGICP, 0), (ref.AVGICP, 0), (ref.P2P, 1), (ref.GICP, 1)]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def lib_pair_terms(L, T, p, mu, S, normal, th, method, metric):
    T16 = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).ravel()
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel()
    p, mu, S, normal = arr(p), arr(mu), arr(S), arr(normal)
    w, H, g, chi = np.zeros(1), np.zeros(36), np.zeros(6), np.zeros(1)
    rc = L.elm_reginfo_pair_terms(_dp(T16), _dp(p), _dp(mu), _dp(S), _dp(normal), float(th), method, metric, _dp(w), _dp(H), _dp(g), _dp(chi))
    return rc, float(w[0]), H.reshape(6, 6), g, float(chi[0])


def close_per_entry(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b)))


# ---------------------------------------------------------------- the ABI
def test_the_new_header_against_its_signature_table(L):
    from elimaloc_amd import _lib
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_REGINFO
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_REGINFO == list(table)
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params and (restype is None) == (ret == "void") and (ret == "void" or (restype is C.c_int and ret == "int")), name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    top = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    assert '#include "elimaloc_hip_posegraph_init_prior.h"\n#include "elimaloc_hip_reginfo.h"\n' in top
    others = (set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT) | set(_lib.EXPORTS_LOOPS) | set(_lib.EXPORTS_LOOPCOV)
              | set(_lib.EXPORTS_PGCOV) | set(_lib.EXPORTS_PGPRIOR) | set(_lib.EXPORTS_PGINITP))
    assert not NAMES & others
    import __graft_entry__ as g
    assert "EXPORTS_REGINFO" in open(g.__file__).read()  # build()'s missing-symbol check reads the new table
    strip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    for name, value in (("MAX_JOBS", _lib.REGINFO_MAX_JOBS), ("METRIC_METHOD", _lib.REGINFO_METRIC_METHOD), ("METRIC_PLANE", _lib.REGINFO_METRIC_PLANE),
                        ("NO_PAIRS", _lib.REGINFO_NO_PAIRS), ("NO_DOF", _lib.REGINFO_NO_DOF), ("DEGENERATE", _lib.REGINFO_DEGENERATE),
                        ("NON_FINITE", _lib.REGINFO_NON_FINITE)):
        assert re.search(r"#define ELM_REGINFO_%s %d\b" % (name, value), strip), name
    assert (ref.NO_PAIRS, ref.NO_DOF, ref.DEGENERATE, ref.NON_FINITE) == (1, 2, 4, 8)


def test_the_header_compiles_as_c():
    probe = ('#include "elimaloc_hip.h"\nint main(void) { elm_reginfo_config c; elm_reginfo_result r; elm_reg_config reg;\n'
             '  elm_reginfo_config_default(&c); elm_reg_config_default(&reg); r.status = 0;\n'
             '  return elm_register_information(0, 0, 0, 0, 1, &reg, &c, &r) == ELM_ERR_INVALID && c.metric == ELM_REGINFO_METRIC_METHOD ? r.status : 1; }\n')
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=probe.encode(), check=True)


def test_struct_layouts_and_defaults(L, tmp_path):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RegInfoConfig
    structs = {"elm_reginfo_config": _lib.RegInfoConfigC, "elm_reginfo_result": _lib.RegInfoResultC}
    lines = []
    for name, cls in structs.items():
        offs = ", ".join("offsetof(%s, %s)" % (name, f) for f, _ in cls._fields_)
        lines.append('  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs))
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for row, (name, cls) in zip(rows, structs.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name
    assert [r[0] for r in rows] == [32, 1008]
    raw = _lib.RegInfoConfigC()
    C.memset(C.byref(raw), 0xAB, C.sizeof(raw))
    L.elm_reginfo_config_default(C.byref(raw))
    c = RegInfoConfig()
    assert bytes(c) == bytes(raw) == bytes(32)  # the factory's bytes are the C default's: the method metric and three zeros
    c = RegInfoConfig(metric=1, sigma2=0.25, length_scale_m=2.0, min_eigen_ratio=1e-6)
    assert (c.metric, c.sigma2, c.length_scale_m, c.min_eigen_ratio) == (1, 0.25, 2.0, 1e-6)
    with pytest.raises(AttributeError, match="RegInfoConfig has no field lambda_init"):
        RegInfoConfig(lambda_init=1.0)
    with pytest.raises(AttributeError):
        RegInfoConfig(_pad=1)
    L.elm_reginfo_config_default(None)


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RegInfoConfig, RegistrationConfig
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    scans = (C.c_void_p * 1)(1)
    T = np.eye(4).ravel()
    res = _lib.RegInfoResultC()
    res.status = 77
    reg, good = RegistrationConfig(), RegInfoConfig()
    call = lambda ctx, m, s, p, n, r, c, out: L.elm_register_information(ctx, m, s, _dp(p), n, None if r is None else C.byref(r),
                                                                         None if c is None else C.byref(c), None if out is None else C.byref(out))
    assert call(None, one, scans, T, 1, reg, good, res) == INVALID and call(one, None, scans, T, 1, reg, good, res) == INVALID
    assert call(one, one, None, T, 1, reg, good, res) == INVALID and call(one, one, scans, None, 1, reg, good, res) == INVALID
    assert call(one, one, scans, T, 1, None, good, res) == INVALID and call(one, one, scans, T, 1, reg, None, res) == INVALID
    assert call(one, one, scans, T, 1, reg, good, None) == INVALID
    for n in (0, -1, _lib.REGINFO_MAX_JOBS + 1):
        assert call(one, one, scans, T, n, reg, good, res) == INVALID, n
    for bad in (dict(metric=2), dict(metric=-1), dict(sigma2=-1.0), dict(sigma2=float("nan")), dict(sigma2=float("inf")), dict(length_scale_m=-0.5),
                dict(length_scale_m=float("nan")), dict(min_eigen_ratio=-1e-9), dict(min_eigen_ratio=1.0), dict(min_eigen_ratio=float("nan"))):
        assert call(one, one, scans, T, 1, reg, RegInfoConfig(**bad), res) == INVALID, bad
    for bad in (dict(icp_method=4), dict(icp_method=-1), dict(max_search_dist=0.0), dict(max_search_dist=float("nan"))):
        assert call(one, one, scans, T, 1, RegistrationConfig(**bad), good, res) == INVALID, bad
    for method in (ref.VGICP, ref.AVGICP):  # the plane metric is for the point methods
        assert call(one, one, scans, T, 1, RegistrationConfig(icp_method=method), RegInfoConfig(metric=1), res) == INVALID
    assert res.status == 77
    # the host's pair terms
    p, mu, n = np.array([1.0, 2.0, 3.0]), np.array([1.1, 2.0, 3.0]), np.array([0.0, 0.0, 1.0])
    ok = lambda **k: L.elm_reginfo_pair_terms(*[k.get(a, d) for a, d in (("T", _dp(T)), ("p", _dp(p)), ("mu", _dp(mu)), ("S", None), ("n", _dp(n)), ("th", 5.0),
                                                                         ("method", 0), ("metric", 0), ("w", None), ("H", None), ("g", None), ("chi", None))])
    assert ok() == 0
    assert ok(T=None) == INVALID and ok(p=None) == INVALID and ok(mu=None) == INVALID
    assert ok(method=4) == INVALID and ok(metric=2) == INVALID and ok(th=0.0) == INVALID and ok(th=float("nan")) == INVALID
    assert ok(metric=1, n=None) == INVALID and ok(metric=1, method=2) == INVALID and ok(metric=1, method=1) == 0


def test_shim_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/registration_information_calls.cpp, built as the other harnesses are; without arguments it touches no device"""
    exe = tmp_path / "registration_information_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "registration_information_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the pair terms: the library's host code against the mirror
def _pair_case(seed, big_rotation=False):
    rng = np.random.default_rng(seed)
    R = cases.general_rotation(seed, 179.0) if big_rotation else cases.general_rotation(seed, 40.0)
    T = cases.pose(R, rng.uniform(-30, 30, 3))
    p = rng.uniform(-20, 20, 3).astype(np.float32).astype(np.float64)
    mu = T[:3, :3] @ p + T[:3, 3] + rng.normal(0, 0.3, 3)
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    S = np.eye(3) + 999.0 * np.outer(n, n) + rng.normal(0, 1e-3, (3, 3))  # a stored inverse, not exactly symmetric
    return T, p, mu, S, n


@pytest.mark.parametrize("method,metric", METHODS_METRICS)
def test_pair_terms_match_the_mirror_entry_by_entry(L, method, metric):
    for seed in range(12):
        T, p, mu, S, n = _pair_case(seed, big_rotation=seed % 2 == 0)
        rc, w, H, g, chi = lib_pair_terms(L, T, p, mu, S, n, 5.0, method, metric)
        mw, mH, mg, mchi = ref.pair_terms(T, p, mu, S, n, 5.0, method, metric)
        assert rc == 0 and w > 0.0
        assert close_per_entry(w, mw) and close_per_entry(H, mH) and close_per_entry(g, mg) and close_per_entry(chi, mchi), (method, metric, seed)
        assert np.array_equal(H, H.T)


def test_pair_terms_at_a_rotation_beyond_120_degrees(L):
    R = ref.exp_so3(np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8]) * np.deg2rad(170.0))
    assert np.degrees(np.arccos((np.trace(R) - 1) / 2)) > 120.0
    T = cases.pose(R, [4.0, -7.0, 1.5])
    _, p, _, S, n = _pair_case(3)
    mu = R @ p + T[:3, 3] + np.array([0.2, -0.1, 0.05])
    for method, metric in METHODS_METRICS:
        rc, w, H, g, chi = lib_pair_terms(L, T, p, mu, S, n, 5.0, method, metric)
        mw, mH, mg, mchi = ref.pair_terms(T, p, mu, S, n, 5.0, method, metric)
        assert rc == 0 and close_per_entry(w, mw) and close_per_entry(H, mH) and close_per_entry(g, mg) and close_per_entry(chi, mchi)
        # ... and the mirror is the contract's matrices
        J, M, e = ref.jacobian(p), ref.metric_plain(T, S, n, method, metric), ref.residual(T, p, mu)
        np.testing.assert_allclose(mH, J.T @ M @ J, rtol=0, atol=1e-12 * np.abs(J.T @ M @ J).max())
        np.testing.assert_allclose(mg, J.T @ M @ e, rtol=0, atol=1e-12 * max(np.abs(J.T @ M @ e).max(), 1e-300))
        np.testing.assert_allclose(mchi, e @ M @ e, rtol=1e-12)
        np.testing.assert_allclose(mw, ref.weight_plain(T, p, mu, 5.0, method), rtol=1e-14)


def test_pair_terms_on_either_side_of_the_weight_threshold(L):
    """w0 = th^2 / (th + |e|^2)^2 = 0.01 at |e|^2 = 9 th, reachable inside the search radius only for th > 9: th = 12, |e|^2 = 108 -+"""
    th = 12.0
    T = cases.pose(cases.general_rotation(4, 90.0), [1.0, 2.0, 3.0])
    p = np.array([3.0, -2.0, 0.5])
    d = np.array([2.0, -1.0, 2.0]) / 3.0  # unit
    for e2, inside in ((9 * th * 0.999, True), (9 * th * 1.001, False)):
        assert e2 < th * th  # a pair the search accepts
        mu = T[:3, :3] @ (p + d * np.sqrt(e2)) + T[:3, 3]
        for method in (ref.VGICP, ref.AVGICP):
            rc, w, H, g, chi = lib_pair_terms(L, T, p, mu, np.eye(3) * 2.0, None, th, method, 0)
            m = ref.pair_terms(T, p, mu, np.eye(3) * 2.0, None, th, method, 0)
            assert rc == 0 and (m is not None) == inside
            if inside:
                assert abs(w - 0.01) < 1e-4 and w >= 0.01 and close_per_entry(w, m[0]) and close_per_entry(H, m[1]) and close_per_entry(g, m[2])
            else:
                assert w == 0.0 and not H.any() and not g.any() and chi == 0.0
        for method in (ref.P2P, ref.GICP):  # no threshold for the point methods
            rc, w, H, g, chi = lib_pair_terms(L, T, p, mu, np.eye(3), None, th, method, 0)
            m = ref.pair_terms(T, p, mu, np.eye(3), None, th, method, 0)
            assert rc == 0 and w > 0.0 and close_per_entry(w, m[0]) and close_per_entry(H, m[1])


def test_the_default_target_pair(L):
    """the reference's default target: the origin with the identity, whatever the method"""
    T = cases.pose(cases.general_rotation(9, 100.0), [0.5, -0.3, 0.2])
    p = np.array([1.0, 0.5, -0.25])
    for method in (ref.P2P, ref.GICP, ref.VGICP):
        rc, w, H, g, chi = lib_pair_terms(L, T, p, np.zeros(3), None, None, 5.0, method, 0)
        mw, mH, mg, mchi = ref.pair_terms(T, p, np.zeros(3), None, None, 5.0, method, 0)
        assert rc == 0 and close_per_entry(w, mw) and close_per_entry(H, mH) and close_per_entry(g, mg) and close_per_entry(chi, mchi)
        J, e = ref.jacobian(p), ref.residual(T, p, np.zeros(3))
        np.testing.assert_allclose(mH, J.T @ J, rtol=0, atol=1e-14)
        np.testing.assert_allclose(mchi, e @ e, rtol=1e-13)


# ---------------------------------------------------------------- the mirror's own algebra
def test_the_jacobian_is_the_derivative_of_the_residual():
    """central differences of e under the right perturbation T <- T [Exp(w) | v] acting on the scan point: de/dx = -J.  Step 1e-6: the
    truncation error is O(h^2 |p|) ~ 1e-11, the rounding error eps |p| / h ~ 1e-9."""
    for seed in range(6):
        T, p, mu, _, _ = _pair_case(seed, big_rotation=True)
        J, h = ref.jacobian(p), 1e-6
        fd = np.empty((3, 6))
        for k in range(6):
            x = np.zeros(6)
            x[k] = h
            fd[:, k] = (ref.residual(T, p, mu, x) - ref.residual(T, p, mu, -x)) / (2 * h)
        np.testing.assert_allclose(fd, -J, rtol=0, atol=1e-7 * max(1.0, np.abs(p).max()))


def test_the_jacobi_against_eigh():
    rng = np.random.default_rng(12)
    mats = []
    for k in range(20):
        A = rng.normal(size=(6, 6)) * (10.0 ** rng.uniform(-3, 3, 6))
        mats.append(A @ A.T)
    mats += [np.zeros((6, 6)), np.eye(6), np.diag([5.0, 1.0, 1.0, 3.0, 0.0, 2.0]), np.outer(np.arange(1.0, 7.0), np.arange(1.0, 7.0))]
    for A in mats:
        lam, V = ref.eig6_sym_asc(A)
        scale = max(np.abs(A).max(), 1e-300)
        np.testing.assert_allclose(lam, np.linalg.eigh(A)[0], rtol=0, atol=1e-13 * scale * 6)
        assert np.all(np.diff(lam) >= 0)
        assert np.abs(V.T @ V - np.eye(6)).max() <= 1e-13
        assert np.abs(A @ V - V * lam).max() <= 1e-13 * scale * 6
        for k in range(6):  # the sign rule: the first largest-magnitude component is positive
            assert V[int(np.argmax(np.abs(V[:, k]))), k] > 0.0


def test_finish_flags_and_the_variance_factor():
    T = cases.pose(cases.general_rotation(2, 60.0), cases.ROOM_CENTRE)
    pts, pairs = cases.room_pairs(T, n=50)
    r = ref.job(T, pts, pairs, 5.0, ref.P2P)
    assert r["status"] == 0 and r["rank"] == 6 and r["dof"] == 3 * 50 - 6 and r["n_pairs"] == 50
    np.testing.assert_allclose(r["sigma2"], r["chi2"] / r["dof"], rtol=1e-15)
    np.testing.assert_allclose(r["information"], r["H"] / r["sigma2"], rtol=1e-15)
    assert np.array_equal(r["information"], r["information"].T) and np.array_equal(r["H"], r["H"].T)
    np.testing.assert_allclose(ref.job(T, pts, pairs, 5.0, ref.P2P, sigma2=0.04)["information"], r["H"] / 0.04, rtol=1e-15)
    assert ref.job(T, pts, pairs, 5.0, ref.P2P, length_scale_m=2.0)["length_scale"] == 2.0
    # no pair; one pair: rank 3 of 3 residuals, no degree of freedom left
    none = ref.job(T, pts, [], 5.0, ref.P2P)
    assert none["status"] == ref.NO_PAIRS | ref.DEGENERATE and not none["H"].any() and none["n_points"] == 50
    one = ref.job(T, pts, pairs[:1], 5.0, ref.P2P, min_eigen_ratio=1e-9)
    assert one["rank"] == 3 and one["dof"] == 0 and one["status"] == ref.NO_DOF | ref.DEGENERATE and one["sigma2"] == 0.0
    assert not one["information"].any() and one["H"].any()
    one = ref.job(T, pts, pairs[:1], 5.0, ref.P2P, min_eigen_ratio=1e-9, sigma2=0.01)
    assert one["status"] == ref.DEGENERATE and one["information"].any() and np.array_equal(one["information"], one["information"].T)
    # the plane metric counts one residual per pair
    assert ref.job(T, pts, pairs, 5.0, ref.P2P, metric=1)["dof"] == 50 - 6


# ---------------------------------------------------------------- two constructed scenes
def test_the_corridor_names_its_axis():
    T = cases.pose(cases.rot_x(0.2), [1.5, 0.3, 0.4])
    pts, pairs = cases.corridor_pairs(T)
    for method in (ref.P2P, ref.GICP):
        r = ref.job(T, pts, pairs, 5.0, method, metric=1, min_eigen_ratio=1e-6)
        lam, V = r["eigenvalues"], r["eigenvectors"]
        assert lam[0] / lam[5] < 1e-9 and lam[1] / lam[5] > 1e-3
        assert np.array_equal(np.abs(V[:, 0]), cases.CORRIDOR_AXIS)  # the null direction is the corridor's axis
        assert r["rank"] == 5 and r["status"] == ref.DEGENERATE
        assert not (r["information"] @ cases.CORRIDOR_AXIS).any() and np.array_equal(r["information"], r["information"].T)
        assert np.linalg.eigvalsh(r["information"])[1] > 0.0
        # ... at a general rotation the axis is R^T e_x, no longer exact
        Tg = cases.pose(cases.general_rotation(21, 150.0), [1.5, 0.3, 0.4])
        pts_g, pairs_g = cases.corridor_pairs(Tg)
        rg = ref.job(Tg, pts_g, pairs_g, 5.0, method, metric=1, min_eigen_ratio=1e-6)
        axis = np.concatenate([Tg[:3, :3].T @ [1.0, 0.0, 0.0], np.zeros(3)])
        assert rg["eigenvalues"][0] / rg["eigenvalues"][5] < 1e-9 and rg["rank"] == 5
        assert abs(abs(rg["eigenvectors"][:, 0] @ axis) - 1.0) < 1e-9
        assert np.abs(rg["information"] @ axis).max() < 1e-9 * np.abs(rg["information"]).max()


def test_the_closed_room_is_constrained():
    T = cases.pose(cases.general_rotation(5, 120.0), cases.ROOM_CENTRE + [0.5, -0.4, 0.1])
    pts, pairs = cases.room_pairs(T)
    for method, metric in ((ref.P2P, 0), (ref.P2P, 1), (ref.GICP, 1)):
        r = ref.job(T, pts, pairs, 5.0, method, metric=metric, min_eigen_ratio=1e-6)
        assert r["eigenvalues"][0] / r["eigenvalues"][5] > 1e-2 and r["rank"] == 6 and r["status"] == 0
        np.testing.assert_allclose(r["information"], r["H"] / r["sigma2"], rtol=1e-15)
