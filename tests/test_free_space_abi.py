"""CPU checks of the free-space ABI (include/elimaloc_hip.h, free-space check): the config defaults, the struct layouts against the ctypes
mirrors, argument errors without a device, and the C++ shim's VoxelHashMap::CheckFreeSpace compiling."""
import ctypes as C
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


def test_free_space_config_defaults(L):
    from elimaloc_amd.registration import FreeSpaceConfig
    c = FreeSpaceConfig()
    assert (c.sub, c.min_hits, c.max_samples) == (4, 2, 1024)
    assert c.step_m == 0.0  # = cell / 2 of the map the call is made on
    assert (c.start_m, c.min_range_m, c.max_range_m, c.end_margin_m, c.end_margin_frac) == (1.0, 2.0, 50.0, 1.0, 0.2)
    assert list(c.origin) == [0.0, 0.0, 0.0]
    c = FreeSpaceConfig(sub=2, origin=(0.5, -1.0, 2.0), step_m=0.1)
    assert c.sub == 2 and list(c.origin) == [0.5, -1.0, 2.0] and c.step_m == 0.1
    with pytest.raises(AttributeError):
        FreeSpaceConfig(no_such_field=1)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_freespace_config), offsetof(elm_freespace_config, sub),
         offsetof(elm_freespace_config, min_hits), offsetof(elm_freespace_config, max_samples), offsetof(elm_freespace_config, step_m),
         offsetof(elm_freespace_config, start_m), offsetof(elm_freespace_config, min_range_m), offsetof(elm_freespace_config, max_range_m),
         offsetof(elm_freespace_config, end_margin_m), offsetof(elm_freespace_config, end_margin_frac), offsetof(elm_freespace_config, origin));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_freespace_stats), offsetof(elm_freespace_stats, n_counted),
         offsetof(elm_freespace_stats, n_pierced), offsetof(elm_freespace_stats, n_end_occupied), offsetof(elm_freespace_stats, n_supported),
         offsetof(elm_freespace_stats, n_samples), offsetof(elm_freespace_stats, n_hit_samples));
  printf("%zu %zu %zu\n", sizeof(elm_reloc_config), sizeof(elm_reloc_candidate), sizeof(elm_reloc_global_config));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, c = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    F, S = _lib.FreeSpaceConfigC, _lib.FreeSpaceStatsC
    assert a == [C.sizeof(F), F.sub.offset, F.min_hits.offset, F.max_samples.offset, F.step_m.offset, F.start_m.offset, F.min_range_m.offset,
                 F.max_range_m.offset, F.end_margin_m.offset, F.end_margin_frac.offset, F.origin.offset]
    assert b == [C.sizeof(S), S.n_counted.offset, S.n_pierced.offset, S.n_end_occupied.offset, S.n_supported.offset, S.n_samples.offset,
                 S.n_hit_samples.offset]
    assert b[0] == 32
    # no existing struct changed size
    assert c == [C.sizeof(_lib.RelocConfigC), C.sizeof(_lib.RelocCandidate), C.sizeof(_lib.GlobalRelocConfigC)]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import FreeSpaceConfig
    T = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.FreeSpaceStatsC * 2)()
    cfg = FreeSpaceConfig()
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    assert L.elm_map_check_free_space(None, None, None, dp, 1, C.byref(cfg), st, None) == INVALID
    assert L.elm_map_check_free_space(one, one, one, dp, 1, None, st, None) == INVALID
    assert L.elm_map_check_free_space(one, one, one, dp, -1, C.byref(cfg), st, None) == INVALID
    assert L.elm_map_check_free_space(one, one, one, None, 1, C.byref(cfg), st, None) == INVALID
    assert L.elm_map_check_free_space(one, one, one, dp, 1, C.byref(cfg), None, None) == INVALID
    for kw in [dict(sub=3), dict(sub=0), dict(sub=8), dict(min_hits=0), dict(max_samples=0), dict(max_samples=1 << 20), dict(step_m=-0.1),
               dict(step_m=float("nan")), dict(start_m=-1.0), dict(min_range_m=-1.0), dict(max_range_m=1.0), dict(end_margin_m=-0.5),
               dict(end_margin_frac=float("inf")), dict(origin=(0.0, float("nan"), 0.0))]:
        assert L.elm_map_check_free_space(one, one, one, dp, 1, C.byref(FreeSpaceConfig(**kw)), st, None) == INVALID, kw
    n = C.c_size_t(0)
    buf = np.zeros(3, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.elm_map_fine_cells(None, None, 4, None, 0, C.byref(n)) == INVALID
    assert L.elm_map_fine_cells(one, one, 3, None, 0, C.byref(n)) == INVALID
    assert L.elm_map_fine_cells(one, one, 4, None, 0, None) == INVALID
    assert L.elm_map_fine_cells(one, one, 4, None, 1, C.byref(n)) == INVALID
    assert L.elm_map_fine_cells(one, one, 0, buf, 1, C.byref(n)) == INVALID
    L.elm_freespace_config_default(None)  # a NULL config is ignored


def test_shim_check_free_space_compiles_and_links(L, tmp_path):
    src = tmp_path / "free_shim.cpp"
    src.write_text(r'''
#include "registration.hpp"
// the registered pose verified by the rays of its own scan, as a node would after RunRegister
double pierced_share(const std::vector<PointStruct>& scan, const VoxelHashMap& map, const Eigen::Matrix4d& pose) {
    FreeSpaceConfig fs;
    fs.min_hits = 2;
    fs.origin[2] = 0.1;
    std::vector<uint16_t> hits;
    const std::vector<elm_freespace_stats> st = map.CheckFreeSpace(scan, std::vector<Eigen::Matrix4d>(1, pose), fs, &hits);
    const std::vector<elm_freespace_stats> st2 = map.CheckFreeSpace(scan, std::vector<Eigen::Matrix4d>(2, pose));
    return st[0].n_counted ? (double)st[0].n_pierced / (double)st[0].n_counted : (double)(st2.size() + hits.size());
}
int main(int argc, char**) {
    if (argc > 1) { std::vector<PointStruct> s; VoxelHashMap m; return (int)pierced_share(s, m, Eigen::Matrix4d::Identity()); }
    return 0;
}
''')
    exe = tmp_path / "free_shim"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"), str(src),
                               "-L", libdir, "-lelimaloc_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
