"""The growth-objects ABI (include/elimaloc_hip.h, map growth: objects) on the CPU: the numpy mirror of the contract
(tests/objects_ref.py) against cases written out by hand -- every one of the 26 offsets under every connectivity, a small scene with its
records, maps and stats -- and against scipy.ndimage.label on random blocks; the struct layouts against the ctypes mirrors, the rule's
defaults, argument errors without a device, and the C++ shim's FindObjects / Objects / CellObjects / BeamObjects call lines compiling."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import growth_ref  # tests/ is on sys.path via conftest
import objects_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
OFFSETS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
LIMIT = {6: 1, 18: 2, 26: 3}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _objects(cells, hit=None, through=None, **rule):
    """the mirror on a cell set given in any order -> (Objects, the cells in ascending (x, y, z) order)"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    order = np.lexsort(cells.T[::-1])
    hit = np.full(len(cells), 3, np.uint32) if hit is None else np.asarray(hit, dtype=np.uint32)
    through = np.zeros(len(cells), np.uint32) if through is None else np.asarray(through, dtype=np.uint32)
    return objects_ref.Objects(cells[order], hit[order], through[order], objects_ref.Rule(**rule)), cells[order]


# ---------------------------------------------------------------- the mirror, by hand
@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("d", OFFSETS)
def test_the_mirror_on_every_offset(d, connectivity):
    """{c, c + d}: one object of two cells when |d|_1 <= 1 / 2 / 3, else two objects of one cell"""
    assert len(OFFSETS) == 26
    joined = sum(abs(x) for x in d) <= LIMIT[connectivity]
    for c in ((0, 0, 0), (-1, 0, 7), (4, -5, -1)):  # (the second and third straddle 0 and a coarse-cell face for some d)
        o, cells = _objects([c, np.add(c, d)], connectivity=connectivity)
        assert o.stats == dict(n_members=2, n_objects=1 if joined else 2, n_small=0, n_small_cells=0, max_cells=2 if joined else 1)
        assert o.cell_map.tolist() == ([0, 0] if joined else [0, 1])
        assert o.objects["label"].tolist() == (cells[:1] if joined else cells).tolist()
        assert o.objects["n_cells"].tolist() == ([2] if joined else [1, 1])
    assert len(objects_ref.offsets(connectivity)) == connectivity


def test_the_mirror_on_a_scene_worked_out_by_hand():
    """Seven candidate cells.  A = {(0,0,0), (1,0,0), (1,1,0)}: an L of three face-connected cells.  C = (-1,-1,-1): the corner neighbour
    of (0,0,0), d = (1,1,1): joined to A under 26 only.  D = (2,1,1): an edge neighbour of (1,1,0), d = (1,0,1), and of B = (3,2,1),
    d = (1,1,0): under 18 and 26 it bridges A and B, which touch nothing else.  N = (2,1,0), hit 2: a candidate below min_hit 3 that would
    join (1,1,0) and D by faces -- not a member, it connects nothing.  Counters: hit 3, 4, 5, 6, 2, 7, 9 in ascending cell order, through
    0, but D has through 1 (hit 7 >= 4 * 1: a member)."""
    cells = [(-1, -1, -1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 1, 1), (3, 2, 1)]  # ascending
    hit = [3, 4, 5, 6, 2, 7, 9]
    through = [0, 0, 0, 0, 0, 1, 0]
    B = 1 << 20
    o, _ = _objects(cells, hit, through, connectivity=6)
    # 6: A by faces; C, D, B alone
    assert o.cell_map.tolist() == [0, 1, 1, 1, -1, 2, 3]
    assert o.stats == dict(n_members=6, n_objects=4, n_small=0, n_small_cells=0, max_cells=3)
    assert o.objects["label"].tolist() == [[-1, -1, -1], [0, 0, 0], [2, 1, 1], [3, 2, 1]] and o.objects["n_cells"].tolist() == [1, 3, 1, 1]
    assert o.objects["lo"].tolist() == [[-1, -1, -1], [0, 0, 0], [2, 1, 1], [3, 2, 1]] and o.objects["hi"].tolist() == [[-1, -1, -1], [1, 1, 0], [2, 1, 1], [3, 2, 1]]
    assert o.objects["hit"].tolist() == [3, 15, 7, 9] and o.objects["through"].tolist() == [0, 0, 1, 0]
    assert o.objects["cell_sum"].tolist() == [[B - 1] * 3, [3 * B + 2, 3 * B + 1, 3 * B], [B + 2, B + 1, B + 1], [B + 3, B + 2, B + 1]]
    assert all(o.objects[f].dtype == t for f, t in zip(objects_ref.OBJECT_FIELDS, (np.int32, np.uint32, np.int32, np.int32, np.uint64, np.uint64, np.uint64)))
    # 18: A + D + B through the edges; C alone
    o, _ = _objects(cells, hit, through, connectivity=18)
    assert o.cell_map.tolist() == [0, 1, 1, 1, -1, 1, 1] and o.objects["n_cells"].tolist() == [1, 5]
    assert o.objects["lo"].tolist()[1] == [0, 0, 0] and o.objects["hi"].tolist()[1] == [3, 2, 1] and o.objects["hit"].tolist() == [3, 31]
    # 26: everything
    o, _ = _objects(cells, hit, through, connectivity=26)
    assert o.cell_map.tolist() == [0, 0, 0, 0, -1, 0, 0] and o.stats == dict(n_members=6, n_objects=1, n_small=0, n_small_cells=0, max_cells=6)
    assert o.objects["label"].tolist() == [[-1, -1, -1]] and o.objects["through"].tolist() == [1]
    # min_cells 3 under 6: A is listed, the three single cells are small
    o, _ = _objects(cells, hit, through, connectivity=6, min_cells=3)
    assert o.cell_map.tolist() == [-2, 0, 0, 0, -1, -2, -2] and o.stats == dict(n_members=6, n_objects=1, n_small=3, n_small_cells=3, max_cells=3)
    assert o.objects["label"].tolist() == [[0, 0, 0]]
    # min_cells 4: nothing is listed, max_cells is still the largest component's
    o, _ = _objects(cells, hit, through, connectivity=6, min_cells=4)
    assert o.stats == dict(n_members=6, n_objects=0, n_small=4, n_small_cells=6, max_cells=3) and o.objects["label"].shape == (0, 3)
    # the member rule: min_hit 2 makes N a member and joins A and D by faces; hit_per_through 8 drops D (7 < 8 * 1)
    o, _ = _objects(cells, hit, through, connectivity=6, min_hit=2)
    assert o.cell_map.tolist() == [0, 1, 1, 1, 1, 1, 2]
    o, _ = _objects(cells, hit, through, connectivity=26, hit_per_through=8)
    assert o.cell_map.tolist() == [0, 0, 0, 0, -1, -1, 1]
    # the beam map: identity pose, 0.25 m cells, origin far enough from every end point; beam i ends at the centre of cell i; one beam in a
    # cell that is no candidate, one outside the observing window, one NaN, one at the origin itself
    o, _ = _objects(cells, hit, through, connectivity=6, min_cells=3)
    cfg = growth_ref.Cfg(origin=(0.0, 0.0, 5.0), obs_min_range_m=1.0)
    pts = np.concatenate([(np.array(cells) + 0.5) * 0.25, [(2.0, 2.0, 2.0), (0.0, 0.0, 4.5), (np.nan, 0.0, 0.0), (0.0, 0.0, 5.0)]]).astype(np.float32)
    assert o.beams(cfg, 0.25, pts, np.eye(4)).tolist() == [-2, 0, 0, 0, -1, -2, -2, -1, -1, -1, -1]
    G = np.eye(4)
    G[:3, 3] = (0.25, 0.0, 0.0)  # one cell along x: beam i now ends in cell i + (1, 0, 0)
    assert o.beams(cfg, 0.25, pts, G).tolist() == [-1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    # no candidates at all
    o, _ = _objects(np.zeros((0, 3)))
    assert o.stats == dict.fromkeys(objects_ref.STAT_FIELDS, 0) and o.cell_map.shape == (0,) and o.objects["cell_sum"].shape == (0, 3)
    assert o.beams(cfg, 0.25, pts, np.eye(4)).tolist() == [-1] * len(pts)


def test_the_mirror_at_the_key_range():
    """members at +-(2^20 - 1): their neighbours beyond the range are no cells"""
    m = (1 << 20) - 1
    o, _ = _objects([(m, m, m), (m - 1, m, m), (-m, -m, -m), (-m, -m + 1, -m + 1)], connectivity=18)
    assert o.cell_map.tolist() == [0, 0, 1, 1] and o.objects["cell_sum"].tolist() == [[2, 3, 3], [4 * m + 1, 4 * m + 2, 4 * m + 2]]


@pytest.mark.parametrize("connectivity,rank", [(6, 1), (18, 2), (26, 3)])
def test_the_mirror_against_scipy(connectivity, rank):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, rank)
    assert int(structure.sum()) == connectivity + 1
    rng = np.random.default_rng(connectivity)
    for fill in (0.08, 0.2, 0.35, 0.6):
        block = rng.random((12, 12, 12)) < fill
        lab, n = ndimage.label(block, structure=structure)
        cells = np.argwhere(block) - (5, 6, 7)  # C order: ascending (x, y, z); shifted across 0 on every axis
        o = objects_ref.Objects(cells, np.full(len(cells), 3), np.zeros(len(cells)), objects_ref.Rule(connectivity=connectivity))
        # scipy numbers the components in the order it meets them on its raster scan: by their smallest cell, from 1
        assert o.stats["n_objects"] == n and np.array_equal(o.cell_map, lab[block] - 1)
        assert np.array_equal(o.objects["n_cells"], np.bincount(lab[block])[1:])
        boxes = ndimage.find_objects(lab)
        assert o.objects["lo"].tolist() == [[s.start - k for s, k in zip(b, (5, 6, 7))] for b in boxes]
        assert o.objects["hi"].tolist() == [[s.stop - 1 - k for s, k in zip(b, (5, 6, 7))] for b in boxes]


# ---------------------------------------------------------------- the ABI
def test_object_rule_defaults(L):
    from elimaloc_amd.registration import GrowthObjectRule, GrowthRule
    r, g, m = GrowthObjectRule(), GrowthRule(), objects_ref.Rule()
    assert (r.min_hit, r.hit_per_through, r.connectivity, r.min_cells) == (3, 4, 26, 1)
    assert (r.min_hit, r.hit_per_through) == (g.min_hit, g.hit_per_through)  # the member rule is the growth rule's
    assert (m.min_hit, m.hit_per_through, m.connectivity, m.min_cells) == (3, 4, 26, 1)
    r = GrowthObjectRule(min_hit=1, hit_per_through=0, connectivity=6, min_cells=7)
    assert (r.min_hit, r.hit_per_through, r.connectivity, r.min_cells) == (1, 0, 6, 7)
    with pytest.raises(AttributeError):
        GrowthObjectRule(no_such_field=1)
    L.elm_growth_object_rule_default(None)  # a NULL rule is ignored


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(elm_growth_object_rule), offsetof(elm_growth_object_rule, min_hit),
         offsetof(elm_growth_object_rule, hit_per_through), offsetof(elm_growth_object_rule, connectivity), offsetof(elm_growth_object_rule, min_cells));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_growth_object), offsetof(elm_growth_object, label), offsetof(elm_growth_object, n_cells),
         offsetof(elm_growth_object, lo), offsetof(elm_growth_object, hi), offsetof(elm_growth_object, hit), offsetof(elm_growth_object, through),
         offsetof(elm_growth_object, cell_sum));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(elm_growth_object_stats), offsetof(elm_growth_object_stats, n_members),
         offsetof(elm_growth_object_stats, n_objects), offsetof(elm_growth_object_stats, n_small), offsetof(elm_growth_object_stats, n_small_cells),
         offsetof(elm_growth_object_stats, max_cells));
  printf("%zu %zu %zu\n", sizeof(elm_growth_config), sizeof(elm_growth_stats), sizeof(elm_growth_rule));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    r, o, s, old = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    R, O, S = _lib.GrowthObjectRuleC, _lib.GrowthObjectC, _lib.GrowthObjectStatsC
    assert r == [C.sizeof(R), R.min_hit.offset, R.hit_per_through.offset, R.connectivity.offset, R.min_cells.offset]
    assert o == [C.sizeof(O), O.label.offset, O.n_cells.offset, O.lo.offset, O.hi.offset, O.hit.offset, O.through.offset, O.cell_sum.offset]
    assert s == [C.sizeof(S), S.n_members.offset, S.n_objects.offset, S.n_small.offset, S.n_small_cells.offset, S.max_cells.offset]
    assert (r[0], o[0], s[0]) == (16, 80, 24)
    assert o[1:] == [0, 12, 16, 28, 40, 48, 56]
    # the growth structs did not change size
    assert old == [C.sizeof(_lib.GrowthConfigC), C.sizeof(_lib.GrowthStatsC), C.sizeof(_lib.GrowthRuleC)] == [80, 56, 8]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import GrowthConfig, GrowthObjectRule
    T = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    n = C.c_size_t(0)
    st = _lib.GrowthObjectStatsC()
    rule, cfg = GrowthObjectRule(), GrowthConfig()
    objs = (_lib.GrowthObjectC * 2)()
    out = (C.c_int32 * 4)()
    assert L.elm_growth_find_objects(None, one, C.byref(rule), C.byref(st)) == INVALID
    assert L.elm_growth_find_objects(one, None, C.byref(rule), C.byref(st)) == INVALID
    assert L.elm_growth_find_objects(one, one, None, C.byref(st)) == INVALID
    for kw in (dict(connectivity=0), dict(connectivity=7), dict(connectivity=8), dict(connectivity=27), dict(min_cells=0)):
        assert L.elm_growth_find_objects(one, one, C.byref(GrowthObjectRule(**kw)), C.byref(st)) == INVALID, kw
    assert L.elm_growth_objects(one, one, objs, 2, None) == INVALID
    assert L.elm_growth_objects(one, one, None, 2, C.byref(n)) == INVALID
    assert L.elm_growth_objects(None, one, objs, 2, C.byref(n)) == INVALID and L.elm_growth_objects(one, None, objs, 2, C.byref(n)) == INVALID
    assert L.elm_growth_cell_objects(one, one, out, 4, None) == INVALID
    assert L.elm_growth_cell_objects(one, one, None, 4, C.byref(n)) == INVALID
    assert L.elm_growth_cell_objects(None, one, out, 4, C.byref(n)) == INVALID and L.elm_growth_cell_objects(one, None, out, 4, C.byref(n)) == INVALID

    def beams(ctx, g, s, pose, c, o):
        return L.elm_growth_beam_objects(ctx, g, s, pose, c, o)

    assert beams(None, one, one, dp, C.byref(cfg), out) == INVALID
    assert beams(one, None, one, dp, C.byref(cfg), out) == INVALID
    assert beams(one, one, None, dp, C.byref(cfg), out) == INVALID
    assert beams(one, one, one, None, C.byref(cfg), out) == INVALID
    assert beams(one, one, one, dp, None, out) == INVALID
    assert beams(one, one, one, dp, C.byref(cfg), None) == INVALID
    nan, inf = float("nan"), float("inf")
    for kw in [dict(sub=3), dict(max_steps=0), dict(min_range_m=nan), dict(obs_min_range_m=-1.0), dict(obs_max_range_m=1.0), dict(obs_max_range_m=inf),
               dict(end_margin_m=-0.5), dict(end_margin_frac=nan), dict(origin=(0.0, nan, 0.0)), dict(clearance_cells=3)]:
        assert beams(one, one, one, dp, C.byref(GrowthConfig(**kw)), out) == INVALID, kw


def test_shim_objects_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/objects_calls.cpp, built as tests/test_growth_abi.py builds growth_calls.cpp"""
    exe = tmp_path / "objects_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "objects_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
