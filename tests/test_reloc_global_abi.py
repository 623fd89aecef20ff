"""CPU checks of the global-relocalization ABI (include/elimaloc_hip.h, global relocalization): config defaults, struct layouts against the
ctypes mirrors, argument errors without a device, and the C++ shim's RunRelocalizeGlobal / FindGroundHeights compiling."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_global_config_defaults(L):
    from elimaloc_amd.registration import GlobalRelocConfig
    c = GlobalRelocConfig()
    assert all(math.isnan(v) for v in (c.x_min, c.x_max, c.y_min, c.y_max))
    assert (c.step_xy_m, c.step_yaw_deg, c.score_max_range_m, c.score_min_height_m) == (0.5, 2.0, 50.0, 1.0)
    assert (c.max_score_points, c.top_k, c.nms_xy_m, c.nms_yaw_deg) == (8192, 16, 1.0, 6.0)
    assert (c.pool_min, c.max_kz_span, c.bitmap_max_bytes) == (64, 64, 256 << 20)
    assert GlobalRelocConfig(top_k=3, score_min_height_m=-math.inf).score_min_height_m == -math.inf
    with pytest.raises(AttributeError):
        GlobalRelocConfig(no_such_field=1)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
#define O(T, f) (unsigned long)offsetof(T, f)
int main(void) {
  printf("%zu %lu %lu %lu %lu %lu %lu %lu %lu\n", sizeof(elm_reloc_global_config), O(elm_reloc_global_config, step_xy_m),
         O(elm_reloc_global_config, score_min_height_m), O(elm_reloc_global_config, max_score_points), O(elm_reloc_global_config, top_k),
         O(elm_reloc_global_config, nms_xy_m), O(elm_reloc_global_config, pool_min), O(elm_reloc_global_config, max_kz_span),
         O(elm_reloc_global_config, bitmap_max_bytes));
  printf("%zu %lu %lu %lu %lu %lu %lu %lu %lu\n", sizeof(elm_reloc_global_stats), O(elm_reloc_global_stats, nx),
         O(elm_reloc_global_stats, levels), O(elm_reloc_global_stats, tau), O(elm_reloc_global_stats, nodes_bounded),
         O(elm_reloc_global_stats, nodes_kept), O(elm_reloc_global_stats, leaves_scored), O(elm_reloc_global_stats, point_evals),
         O(elm_reloc_global_stats, ms_refine));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    G, S = _lib.GlobalRelocConfigC, _lib.GlobalRelocStats
    assert a == [C.sizeof(G), G.step_xy_m.offset, G.score_min_height_m.offset, G.max_score_points.offset, G.top_k.offset,
                 G.nms_xy_m.offset, G.pool_min.offset, G.max_kz_span.offset, G.bitmap_max_bytes.offset]
    assert b == [C.sizeof(S), S.nx.offset, S.levels.offset, S.tau.offset, S.nodes_bounded.offset, S.nodes_kept.offset,
                 S.leaves_scored.offset, S.point_evals.offset, S.ms_refine.offset]


def test_invalid_arguments_without_device(L):
    """The lattice-size query of an explicit rectangle needs no device (ctx = map = NULL): a valid config returns ELM_OK and the size, so an
    ELM_ERR_INVALID for each bad case below can only come from the argument checks."""
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import GlobalRelocConfig
    nan = float("nan")
    T = np.ascontiguousarray(np.eye(4)).ravel()
    T[14] = 1.8  # (0, 0, h): valid
    n = C.c_size_t(0)
    rect = dict(x_min=-10.0, x_max=10.0, y_min=0.0, y_max=5.25)

    def size(cfg, Tt=T):
        n.value = 0
        return L.elm_reloc_global_hypotheses(None, None, _dp(Tt), C.byref(cfg), None, None, 0, C.byref(n))

    # the valid config: 41 x 11 x 180
    assert size(GlobalRelocConfig(**rect)) == _lib.ELM_OK and n.value == 41 * 11 * 180
    assert size(GlobalRelocConfig(**rect, step_yaw_deg=7.0, score_min_height_m=-math.inf, top_k=1024)) == _lib.ELM_OK
    assert n.value == 41 * 11 * 52
    bad = [dict(step_xy_m=0.0), dict(step_xy_m=nan), dict(step_yaw_deg=-2.0), dict(score_max_range_m=0.0), dict(top_k=0),
           dict(top_k=1025), dict(max_score_points=0), dict(nms_xy_m=-1.0), dict(nms_yaw_deg=nan), dict(pool_min=0), dict(max_kz_span=0),
           dict(bitmap_max_bytes=-1), dict(score_min_height_m=nan), dict(score_min_height_m=math.inf),
           # NaN mixes in the rectangle, a non-finite side, inverted rectangles
           dict(x_min=nan), dict(y_max=nan), dict(x_min=nan, x_max=nan, y_min=nan), dict(y_max=math.inf), dict(x_min=-math.inf),
           dict(x_min=10.0, x_max=-10.0), dict(y_min=6.0),
           # a lattice above 2^31 - 1 poses: 20001 x 20001 x 180
           dict(x_min=0.0, x_max=10000.0, y_min=0.0, y_max=10000.0)]
    for kw in bad:
        assert size(GlobalRelocConfig(**(rect | kw))) == INVALID, kw
    # T_tilt with an xy translation, a non-finite entry or a bad bottom row
    for idx, v in ((12, 0.5), (13, -1.0), (14, nan), (0, math.inf), (3, 1.0), (7, -0.1), (11, 0.2), (15, 2.0)):
        Tb = T.copy()
        Tb[idx] = v
        assert size(GlobalRelocConfig(**rect), Tb) == INVALID, idx
    # no size pointer; an unset rectangle needs the map (and so a context)
    cfg = GlobalRelocConfig(**rect)
    assert L.elm_reloc_global_hypotheses(None, None, _dp(T), C.byref(cfg), None, None, 0, None) == INVALID
    assert size(GlobalRelocConfig()) == INVALID
    # the other entry points without a context
    q = np.zeros(4)
    z = np.zeros(2)
    f = np.zeros(2, np.int32)
    assert L.elm_map_ground_heights(None, None, _dp(q), 2, _dp(z), f.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    assert L.elm_relocalize_global(None, None, None, 0, None, None, None, None, None, None, 0, None, None) == INVALID


def test_shim_run_relocalize_global_compiles_and_links(L, tmp_path):
    src = tmp_path / "global_shim.cpp"
    src.write_text(r'''
#include "registration.hpp"
// what a node calls when no initial pose arrives
int start_without_pose(const std::vector<PointStruct>& scan, const VoxelHashMap& map, double lidar_height) {
    Registration reg;
    RegistrationConfig rc;
    GlobalRelocConfig reloc;
    reloc.step_yaw_deg = 3.0;
    Eigen::Matrix4d tilt = Eigen::Matrix4d::Identity();
    tilt(2, 3) = lidar_height;
    bool ok = false;
    double fitness = 0.0;
    Eigen::Matrix<double, 6, 6> cov;
    std::vector<elm_reloc_candidate> cands;
    elm_reloc_global_stats stats;
    Eigen::Matrix4d pose = reg.RunRelocalizeGlobal(scan, map, tilt, rc, reloc, ok, fitness, cov, &cands, &stats);
    std::vector<double> xy{0.0, 0.0, 1.0, 2.0}, z;
    std::vector<int32_t> found;
    map.FindGroundHeights(xy, z, found);
    return ok && pose(3, 3) == 1.0 ? (int)cands.size() + (int)found.size() : -1;
}
int main(int argc, char**) {
    if (argc > 1) { std::vector<PointStruct> s; VoxelHashMap m; return start_without_pose(s, m, 1.8); }
    return 0;
}
''')
    exe = tmp_path / "global_shim"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"), str(src),
                               "-L", libdir, "-lelimaloc_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
