"""CPU checks of the relocalization ABI (include/elimaloc_hip.h, relocalization): the config defaults, the hypothesis grid against a numpy
mirror, the struct layouts against the ctypes mirrors, argument errors without a device, and the C++ shim's RunRelocalize compiling."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _guess(yaw=0.7, t=(12.5, -31.25, 2.1), roll=0.02, pitch=-0.015):
    from elimaloc_amd.synth import rot_zyx
    T = np.eye(4)
    T[:3, :3] = rot_zyx(roll, pitch, yaw)
    T[:3, 3] = t
    return T


def _mirror(T, radius, step, yaw_range, step_yaw):
    """numpy mirror of elm_reloc_make_hypotheses: T_h = [Rz(dyaw_k) R0 | t0 + (i step, j step, 0)], h = (k W + (i + m)) W + (j + m)."""
    m = int(math.floor(radius / step + 1e-9))
    W = 2 * m + 1
    if yaw_range >= 180.0:
        dy = [k * step_yaw for k in range(int(math.ceil(360.0 / step_yaw - 1e-9)))]
    else:
        kk = int(math.floor(yaw_range / step_yaw + 1e-9))
        dy = [0.0] + [s * a * step_yaw for a in range(1, kk + 1) for s in (1.0, -1.0)]
    out = []
    for d in dy:
        a = d * (math.pi / 180.0)
        c, s = math.cos(a), math.sin(a)
        R = T[:3, :3].copy()
        R[0], R[1] = c * T[0, :3] - s * T[1, :3], s * T[0, :3] + c * T[1, :3]
        for i in range(-m, m + 1):
            for j in range(-m, m + 1):
                H = np.eye(4)
                H[:3, :3] = R
                H[:3, 3] = T[:3, 3] + np.array([i * step, j * step, 0.0])
                out.append(H)
    return np.array(out), W, dy


def test_reloc_config_defaults(L):
    from elimaloc_amd.registration import RelocConfig
    c = RelocConfig()
    assert (c.radius_xy_m, c.step_xy_m, c.yaw_range_deg, c.step_yaw_deg) == (5.0, 0.5, 180.0, 2.0)
    assert (c.score_max_range_m, c.max_score_points, c.top_k) == (50.0, 8192, 16)
    assert (c.nms_xy_m, c.nms_yaw_deg) == (1.0, 6.0)
    assert (c.lds_budget_bytes, c.bitmap_max_bytes) == (64 << 10, 64 << 20)
    assert RelocConfig(top_k=3, step_xy_m=0.25).top_k == 3
    with pytest.raises(AttributeError):
        RelocConfig(no_such_field=1)


@pytest.mark.parametrize("radius,step,yaw_range,step_yaw", [(5.0, 0.5, 180.0, 2.0), (1.0, 0.5, 30.0, 10.0), (0.0, 1.0, 0.0, 5.0),
                                                             (1.5, 0.5, 200.0, 7.0), (0.3, 0.1, 359.0, 90.0)])
def test_make_hypotheses_matches_mirror(L, radius, step, yaw_range, step_yaw):
    from elimaloc_amd.registration import MakeHypotheses, RelocConfig
    T = _guess()
    cfg = RelocConfig(radius_xy_m=radius, step_xy_m=step, yaw_range_deg=yaw_range, step_yaw_deg=step_yaw)
    H = MakeHypotheses(T, cfg)
    M, W, dy = _mirror(T, radius, step, yaw_range, step_yaw)
    assert H.shape == M.shape
    np.testing.assert_allclose(H, M, rtol=0, atol=1e-12)
    # the guess itself is hypothesis k = 0, i = j = 0, bit for bit
    m = (W - 1) // 2
    assert np.array_equal(H[m * W + m], T)
    # every rotation orthonormal, det +1; bottom rows exact
    R = H[:, :3, :3]
    np.testing.assert_allclose(np.einsum("nij,nkj->nik", R, R), np.broadcast_to(np.eye(3), R.shape), atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
    assert np.array_equal(H[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (H.shape[0], 4)))
    # z and the third row are the guess's (a yaw about the world z axis)
    assert np.array_equal(H[:, 2, :3], np.broadcast_to(T[2, :3], (H.shape[0], 3))) and np.all(H[:, 2, 3] == T[2, 3])
    # no duplicate yaw (360 deg is 0 deg)
    wrapped = sorted(round(d % 360.0, 9) for d in dy)
    assert len(set(wrapped)) == len(wrapped)


def test_make_hypotheses_default_count_and_order(L):
    from elimaloc_amd.registration import MakeHypotheses
    T = _guess(yaw=-2.0)
    H = MakeHypotheses(T)
    assert H.shape[0] == 180 * 21 * 21
    W, m = 21, 10
    # index order: j fastest (y), then i (x), then k (yaw)
    h = (3 * W + (2 + m)) * W + (-4 + m)
    np.testing.assert_allclose(H[h][:2, 3], T[:2, 3] + [2 * 0.5, -4 * 0.5], atol=1e-12)
    yaw = math.atan2(H[h][1, 0], H[h][0, 0]) - math.atan2(T[1, 0], T[0, 0])
    assert abs((math.degrees(yaw) - 6.0 + 180.0) % 360.0 - 180.0) < 1e-9


def test_make_hypotheses_size_query_and_cap(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RelocConfig
    T = np.ascontiguousarray(_guess().T).ravel()
    cfg = RelocConfig(radius_xy_m=1.0, step_xy_m=0.5, yaw_range_deg=10.0, step_yaw_deg=5.0)
    n = C.c_size_t(0)
    assert L.elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), None, 0, C.byref(n)) == _lib.ELM_OK
    assert n.value == 5 * 5 * 5
    out = np.full(16 * 7, -9.0)
    assert L.elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), _dp(out), 6, C.byref(n)) == _lib.ELM_OK
    assert n.value == 125 and np.all(out[16 * 6:] == -9.0) and out[15] == 1.0


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_reloc_config), offsetof(elm_reloc_config, score_max_range_m),
         offsetof(elm_reloc_config, max_score_points), offsetof(elm_reloc_config, top_k), offsetof(elm_reloc_config, nms_xy_m),
         offsetof(elm_reloc_config, lds_budget_bytes), offsetof(elm_reloc_config, bitmap_max_bytes));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_reloc_candidate), offsetof(elm_reloc_candidate, T),
         offsetof(elm_reloc_candidate, score), offsetof(elm_reloc_candidate, hyp_index), offsetof(elm_reloc_candidate, is_success),
         offsetof(elm_reloc_candidate, iterations), offsetof(elm_reloc_candidate, fitness_score));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    R, K = _lib.RelocConfigC, _lib.RelocCandidate
    assert a == [C.sizeof(R), R.score_max_range_m.offset, R.max_score_points.offset, R.top_k.offset, R.nms_xy_m.offset,
                 R.lds_budget_bytes.offset, R.bitmap_max_bytes.offset]
    assert b == [C.sizeof(K), K.T.offset, K.score.offset, K.hyp_index.offset, K.is_success.offset, K.iterations.offset,
                 K.fitness_score.offset]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RegistrationConfig, RelocConfig
    INVALID = -1
    T = np.ascontiguousarray(np.eye(4)).ravel()
    n = C.c_size_t(0)
    bad = [dict(step_xy_m=0.0), dict(step_yaw_deg=-1.0), dict(radius_xy_m=-1.0), dict(score_max_range_m=0.0), dict(top_k=0),
           dict(max_score_points=0), dict(nms_xy_m=-0.5), dict(lds_budget_bytes=-1), dict(radius_xy_m=float("nan")),
           dict(radius_xy_m=1e6, step_xy_m=0.01)]
    for kw in bad:
        cfg = RelocConfig(**kw)
        assert L.elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), None, 0, C.byref(n)) == INVALID, kw
    cfg = RelocConfig()
    assert L.elm_reloc_make_hypotheses(None, C.byref(cfg), None, 0, C.byref(n)) == INVALID
    assert L.elm_reloc_make_hypotheses(_dp(T), None, None, 0, C.byref(n)) == INVALID
    assert L.elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), None, 4, C.byref(n)) == INVALID
    assert L.elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), None, 0, None) == INVALID
    Tn = T.copy()
    Tn[13] = float("inf")
    assert L.elm_reloc_make_hypotheses(_dp(Tn), C.byref(cfg), None, 0, C.byref(n)) == INVALID
    sc = np.zeros(4, np.uint32)
    P = np.tile(T, 4)
    assert L.elm_map_score_poses(None, None, None, _dp(P), 4, C.byref(cfg), sc.ctypes.data_as(C.POINTER(C.c_uint32))) == INVALID
    reg = RegistrationConfig()
    pts = np.zeros((8, 3), np.float32)
    Tout = np.empty(16)
    res = _lib.RegResult()
    cands = (_lib.RelocCandidate * 4)()
    nc = C.c_int(0)
    fp = pts.ctypes.data_as(C.POINTER(C.c_float))
    assert L.elm_relocalize(None, None, fp, 8, _dp(T), C.byref(cfg), C.byref(reg), _dp(Tout), C.byref(res), cands, 4, C.byref(nc)) == INVALID
    assert L.elm_relocalize(None, None, None, 0, None, None, None, None, None, None, 0, None) == INVALID


def test_shim_run_relocalize_compiles_and_links(L, tmp_path):
    src = tmp_path / "reloc_shim.cpp"
    src.write_text(r'''
#include "registration.hpp"
// RunRelocalize next to RunRegister, as a node's CallbackInitialPose would call it
int relocalize_from(const std::vector<PointStruct>& scan, const VoxelHashMap& map, const Eigen::Matrix4d& clicked) {
    Registration reg;
    RegistrationConfig rc;
    RelocConfig reloc;
    reloc.radius_xy_m = 4.0;
    bool ok = false;
    double fitness = 0.0;
    Eigen::Matrix<double, 6, 6> cov;
    std::vector<elm_reloc_candidate> cands;
    Eigen::Matrix4d pose = reg.RunRelocalize(scan, map, clicked, rc, reloc, ok, fitness, cov, &cands);
    return ok && pose(3, 3) == 1.0 ? (int)cands.size() : -1;
}
int main(int argc, char**) {
    if (argc > 1) { std::vector<PointStruct> s; VoxelHashMap m; return relocalize_from(s, m, Eigen::Matrix4d::Identity()); }
    return 0;
}
''')
    exe = tmp_path / "reloc_shim"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"), str(src),
                               "-L", libdir, "-lelimaloc_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


@pytest.mark.gpu
def test_score_poses_return_codes(L):
    """elm_map_score_poses: every refusal before the device is touched is ELM_ERR_INVALID, the null check comes before the one-rank check,
    and valid arguments on a context with a hook attached are ELM_ERR_UNSUPPORTED."""
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import Context, RelocConfig, Scan, VoxelHashMap
    INVALID, UNSUPPORTED = -1, -5
    rng = np.random.default_rng(5)
    world = rng.uniform(-3.0, 3.0, (200, 3)).astype(np.float32)
    pts = world[:10].copy()
    T = np.ascontiguousarray(np.eye(4)).ravel()
    two = np.tile(T, 2)
    nan2 = two.copy()
    nan2[16 + 13] = float("nan")
    cfg = RelocConfig()
    out = np.zeros(2, np.uint32)
    u32 = out.ctypes.data_as(C.POINTER(C.c_uint32))
    ctx, other = Context(0), Context(0)
    vm, ovm = VoxelHashMap(1.0, 30, ctx), VoxelHashMap(1.0, 30, other)
    vm.AddPoints(world)
    ovm.AddPoints(world)
    sc, osc = Scan(ctx, pts), Scan(other, pts)

    def code(c=ctx, m=vm, s=sc, poses=T, n=1, config=cfg, scores=u32):
        return L.elm_map_score_poses(c._h, m._handle(), s._h, None if poses is None else _dp(poses), n,
                                     None if config is None else C.byref(config), scores)

    assert code() == _lib.ELM_OK and out[0] > 0
    assert code(n=0) == INVALID and code(n=-1) == INVALID
    assert code(scores=None) == INVALID and code(poses=None) == INVALID
    assert code(poses=two, n=2) == _lib.ELM_OK and code(poses=nan2, n=2) == INVALID
    assert code(config=RelocConfig(score_max_range_m=0.0)) == INVALID and code(config=None) == INVALID
    assert code(m=ovm) == INVALID and code(s=osc) == INVALID
    ctx.set_allreduce_hook(lambda p, n, s: 0)
    assert code(scores=None) == INVALID and code(poses=None) == INVALID and code(n=0) == INVALID  # the null check comes first
    assert code() == UNSUPPORTED and "one rank" in L.elm_last_error(ctx._h).decode()
    assert code(m=ovm) == UNSUPPORTED  # ... and the one-rank check before the owners'
    ctx.set_allreduce_hook(None)
    assert code() == _lib.ELM_OK
    del vm, ovm, sc, osc
    ctx.close()
    other.close()
