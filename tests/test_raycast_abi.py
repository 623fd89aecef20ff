"""CPU checks of the ray-casting ABI (include/elimaloc_hip.h, ray casting): the config defaults, the struct layouts against the ctypes
mirrors, argument errors without a device, the C++ shim's VoxelHashMap::RayCast compiling, synth.lidar_beams, and the numpy mirror of the
contract (tests/ray_ref.py) pinned on a map of three cells whose walks are written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ray_ref  # tests/ is on sys.path via conftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def test_raycast_config_defaults(L):
    from elimaloc_amd.registration import RayCastConfig
    c = RayCastConfig()
    assert (c.sub, c.max_steps) == (4, 4096)
    assert (c.min_range_m, c.max_range_m, c.cmp_min_range_m, c.cmp_max_range_m, c.tol_m, c.tol_frac) == (1.0, 100.0, 2.0, 50.0, 0.5, 0.02)
    assert list(c.origin) == [0.0, 0.0, 0.0]
    c = RayCastConfig(sub=2, origin=(0.5, -1.0, 2.0), max_steps=17, tol_m=0.1)
    assert c.sub == 2 and list(c.origin) == [0.5, -1.0, 2.0] and c.max_steps == 17 and c.tol_m == 0.1
    with pytest.raises(AttributeError):
        RayCastConfig(no_such_field=1)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_raycast_config), offsetof(elm_raycast_config, sub),
         offsetof(elm_raycast_config, max_steps), offsetof(elm_raycast_config, min_range_m), offsetof(elm_raycast_config, max_range_m),
         offsetof(elm_raycast_config, cmp_min_range_m), offsetof(elm_raycast_config, cmp_max_range_m), offsetof(elm_raycast_config, tol_m),
         offsetof(elm_raycast_config, tol_frac), offsetof(elm_raycast_config, origin));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_raycast_stats), offsetof(elm_raycast_stats, n_cast),
         offsetof(elm_raycast_stats, n_hit), offsetof(elm_raycast_stats, n_miss), offsetof(elm_raycast_stats, n_truncated),
         offsetof(elm_raycast_stats, n_compared), offsetof(elm_raycast_stats, n_match), offsetof(elm_raycast_stats, n_through),
         offsetof(elm_raycast_stats, n_front), offsetof(elm_raycast_stats, n_steps));
  printf("%zu %zu\n", sizeof(elm_freespace_config), sizeof(elm_freespace_stats));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    F, S = _lib.RayCastConfigC, _lib.RayCastStatsC
    assert a == [C.sizeof(F), F.sub.offset, F.max_steps.offset, F.min_range_m.offset, F.max_range_m.offset, F.cmp_min_range_m.offset,
                 F.cmp_max_range_m.offset, F.tol_m.offset, F.tol_frac.offset, F.origin.offset]
    assert b == [C.sizeof(S), S.n_cast.offset, S.n_hit.offset, S.n_miss.offset, S.n_truncated.offset, S.n_compared.offset, S.n_match.offset,
                 S.n_through.offset, S.n_front.offset, S.n_steps.offset]
    assert a[0] == 80 and b[0] == 40
    # no existing struct changed size
    assert c == [C.sizeof(_lib.FreeSpaceConfigC), C.sizeof(_lib.FreeSpaceStatsC)]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RayCastConfig
    T = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.RayCastStatsC * 2)()
    cfg = RayCastConfig()
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first

    def call(ctx, m, s, poses, n, c, stats):
        return L.elm_map_raycast(ctx, m, s, poses, n, c, stats, None, None, None, None)

    assert call(None, None, None, dp, 1, C.byref(cfg), st) == INVALID
    assert call(one, one, one, dp, 1, None, st) == INVALID
    assert call(one, one, one, dp, -1, C.byref(cfg), st) == INVALID
    assert call(one, one, one, None, 1, C.byref(cfg), st) == INVALID
    assert call(one, one, one, dp, 1, C.byref(cfg), None) == INVALID
    nan, inf = float("nan"), float("inf")
    for kw in [dict(sub=3), dict(sub=0), dict(sub=8), dict(max_steps=0), dict(max_steps=-4), dict(max_steps=(1 << 20) + 1), dict(min_range_m=-0.1),
               dict(min_range_m=nan), dict(max_range_m=0.5), dict(max_range_m=inf), dict(min_range_m=3.0, max_range_m=2.0),
               dict(cmp_min_range_m=-1.0), dict(cmp_max_range_m=1.0), dict(cmp_max_range_m=nan), dict(tol_m=-0.5), dict(tol_m=inf),
               dict(tol_frac=-0.01), dict(tol_frac=nan), dict(origin=(0.0, nan, 0.0)), dict(origin=(inf, 0.0, 0.0))]:
        assert call(one, one, one, dp, 1, C.byref(RayCastConfig(**kw)), st) == INVALID, kw
    L.elm_raycast_config_default(None)  # a NULL config is ignored


def test_shim_raycast_compiles_and_links(L, tmp_path):
    src = tmp_path / "ray_shim.cpp"
    src.write_text(r'''
#include "registration.hpp"
// the registered pose verified by the expected ranges of its own scan, as a node would after RunRegister
double match_share(const std::vector<PointStruct>& scan, const VoxelHashMap& map, const Eigen::Matrix4d& pose) {
    RayCastConfig rc;
    rc.tol_m = 0.4;
    rc.origin[2] = 0.1;
    VoxelHashMap::RayCastArrays arr;
    const std::vector<elm_raycast_stats> st = map.RayCast(scan, std::vector<Eigen::Matrix4d>(1, pose), rc, &arr);
    const std::vector<elm_raycast_stats> st2 = map.RayCast(scan, std::vector<Eigen::Matrix4d>(2, pose));
    return st[0].n_compared ? (double)st[0].n_match / (double)st[0].n_compared
                            : (double)(st2.size() + arr.range_in.size() + arr.range_out.size() + arr.cell.size() + arr.flag.size());
}
int main(int argc, char**) {
    if (argc > 1) { std::vector<PointStruct> s; VoxelHashMap m; return (int)match_share(s, m, Eigen::Matrix4d::Identity()); }
    return 0;
}
''')
    exe = tmp_path / "ray_shim"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"), str(src),
                               "-L", libdir, "-lelimaloc_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


def test_lidar_beams():
    from elimaloc_amd import synth
    b = synth.lidar_beams(32, 512, -25.0, 15.0)
    assert b.shape == (32 * 512, 3) and b.dtype == np.float32 and b.flags["C_CONTIGUOUS"]
    assert np.abs(np.linalg.norm(b.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(b, synth.lidar_beams(32, 512, -25.0, 15.0))
    el = np.degrees(np.arcsin(b[:, 2].astype(np.float64))).reshape(32, 512)
    assert np.allclose(el[0], -25.0, atol=1e-4) and np.allclose(el[-1], 15.0, atol=1e-4) and np.all(np.diff(el[:, 0]) > 0)
    az = np.degrees(np.arctan2(b[:512, 1], b[:512, 0])) % 360.0
    assert az[0] == 0.0 and np.allclose(np.diff(az), 360.0 / 512, atol=1e-3)
    assert len(np.unique(b, axis=0)) == len(b)
    one = synth.lidar_beams(1, 4, -10.0, 10.0)
    assert np.allclose(one, [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], atol=1e-7)


class _Cfg:
    """a plain object with elm_raycast_config's fields: the mirror needs no library"""

    def __init__(self, **kw):
        self.sub, self.max_steps = 4, 4096
        self.min_range_m, self.max_range_m, self.cmp_min_range_m, self.cmp_max_range_m = 0.5, 2.0, 0.0, 10.0
        self.tol_m, self.tol_frac, self.origin = 0.25, 0.0, (0.125, 0.125, 0.125)
        self.__dict__.update(kw)


# voxel 1.0, sub 4: 0.25 m cells.  Three stored points: cells (5, 0, 0), (6, 0, 0) and (0, -4, 0) (floor(-0.9 / 0.25) = -4).
STORED = np.array([(1.3, 0.1, 0.2), (1.6, 0.2, 0.1), (0.1, -0.9, 0.1)], np.float32)
O = np.array((0.125, 0.125, 0.125))  # the centre of cell (0, 0, 0): every face crossing below is a multiple of 0.25 minus 0.125, exact
BEAMS = np.array([O + (1, 0, 0), O + (0, -2, 0), O + (0, 0, 3), O], np.float32)  # +x (L 1), -y (L 2), +z (L 3), the origin itself (L 0)


def test_the_mirror_on_a_map_worked_out_by_hand():
    """Identity pose, origin at the centre of cell (0, 0, 0), walks from t = 0.5.
    +x: starts in cell x = 2 (0.625 / 0.25), exits at t = 0.625, 0.875, 1.125: cells 2, 3, 4 empty, cell 5 entered at 1.125 = the hit after
        3 steps; cell 6 occupied too (entered at 1.375), cell 7 empty: range_out = 1.625.  L = 1: 1.125 - 0.25 <= 1 -> MATCH.
    -y: starts in cell y = floor(-1.5) = -2, faces at t = 0.625, 0.875: cell -4 entered at 0.875 after 2 steps = the hit; cell -5 (entered
        at 1.125) is empty: range_out = 1.125.  L = 2 > 1.125 + 0.25 -> THROUGH.
    +z: cells 2 .. 8 empty, entered at 0.625 .. 1.875 (6 steps); the next face, 2.125, lies beyond max_range 2 -> MISS, FRONT.
    the origin itself: not cast."""
    st, arr, vis = ray_ref.mirror(STORED, 1.0, _Cfg(), BEAMS, np.eye(4)[None], trace=True)
    assert st == [dict(n_cast=3, n_hit=2, n_miss=1, n_truncated=0, n_compared=3, n_match=1, n_through=1, n_front=1, n_steps=11)]
    assert arr["flag"].tolist() == [[1, 1, 2, 0]]
    assert arr["range_in"].tolist() == [[1.125, 0.875, -1.0, -1.0]] and arr["range_out"].tolist() == [[1.625, 1.125, -1.0, -1.0]]
    assert arr["cell"].tolist() == [[[5, 0, 0], [0, -4, 0], [0, 0, 0], [0, 0, 0]]]
    walk = {i: [tuple(c[list(b).index(i)]) for b, c in vis[0] if i in b] for i in range(4)}
    assert walk[0] == [(2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0)] and walk[1] == [(0, -2, 0), (0, -3, 0), (0, -4, 0)]
    assert walk[2] == [(0, 0, z) for z in range(2, 9)] and walk[3] == []
    # a beam that starts inside an occupied cell: the hit is at min_range_m itself, after no step
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(min_range_m=1.2), BEAMS[:1], np.eye(4)[None])
    assert (st[0]["n_hit"], st[0]["n_steps"]) == (1, 0) and arr["range_in"][0, 0] == 1.2 and arr["range_out"][0, 0] == 1.625
    assert arr["cell"][0, 0].tolist() == [5, 0, 0] and st[0]["n_match"] == 1
    # the run reaches max_range_m: cell 6 is entered at 1.375 <= 1.5, its exit 1.625 lies beyond
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(max_range_m=1.5), BEAMS[:1], np.eye(4)[None])
    assert arr["range_in"][0, 0] == 1.125 and arr["range_out"][0, 0] == 1.5 and st[0]["n_hit"] == 1
    # max_steps 2: cells 2, 3, 4 are tested, the third step is not taken -> truncated (and FRONT); max_steps 3 reaches the hit, and the
    # run then ends by steps at the hit cell's own entry
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(max_steps=2), BEAMS[:1], np.eye(4)[None])
    assert arr["flag"][0, 0] == 3 and st[0] == dict(n_cast=1, n_hit=0, n_miss=0, n_truncated=1, n_compared=1, n_match=0, n_through=0,
                                                    n_front=1, n_steps=2)
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(max_steps=3), BEAMS[:1], np.eye(4)[None])
    assert arr["flag"][0, 0] == 1 and arr["range_in"][0, 0] == 1.125 and arr["range_out"][0, 0] == 1.125 and st[0]["n_steps"] == 3
    # a pose: a quarter turn about z maps the sensor's +x beam onto the world's -y ... from the same origin cell
    T = np.eye(4)
    T[:3, :3] = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]
    T[:3, 3] = O - T[:3, :3] @ O  # keeps the world origin of the beams at O
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(), BEAMS[:1], T[None])
    assert arr["cell"][0, 0].tolist() == [0, -4, 0] and arr["range_in"][0, 0] == 0.875 and arr["range_out"][0, 0] == 1.125
    # sub 1 (1 m cells): +x from t = 0.5 starts in cell 0, enters cell 1 at 0.875 -- occupied (both x points), cell 2 empty at 1.875
    st, arr, _ = ray_ref.mirror(STORED, 1.0, _Cfg(sub=1), BEAMS[:1], np.eye(4)[None])
    assert arr["cell"][0, 0].tolist() == [1, 0, 0] and arr["range_in"][0, 0] == 0.875 and arr["range_out"][0, 0] == 1.875 and st[0]["n_steps"] == 1
    # an empty map: everything cast misses
    st, arr, _ = ray_ref.mirror(np.zeros((0, 3)), 1.0, _Cfg(), BEAMS, np.eye(4)[None])
    assert st[0]["n_miss"] == 3 and st[0]["n_hit"] == 0 and st[0]["n_front"] == 3 and arr["flag"].tolist() == [[2, 2, 2, 0]]
