"""The map-growth ABI (include/elimaloc_hip.h, map growth) on the CPU: the config and rule defaults, the struct layouts against the ctypes
mirrors, argument errors without a device, the C++ shim's MapGrowth / WithAppeared call lines compiling; and the numpy mirror of the
contract (tests/growth_ref.py) pinned on a map of three cells whose end classes, walks and counters are written out by hand -- then the GPU
pinned on the same hand-written numbers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import growth_ref  # tests/ is on sys.path via conftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def test_growth_config_and_rule_defaults(L):
    from elimaloc_amd.registration import EvidenceConfig, GrowthConfig, GrowthRule
    c, e = GrowthConfig(), EvidenceConfig()
    shared = ("sub", "max_steps", "min_range_m", "obs_min_range_m", "obs_max_range_m", "end_margin_m", "end_margin_frac")
    assert all(getattr(c, k) == getattr(e, k) for k in shared) and list(c.origin) == list(e.origin)  # the evidence config's fields ...
    assert c.clearance_cells == 1                                                                    # ... plus the clearance
    m = growth_ref.Cfg()  # the mirror's plain config carries the same defaults
    assert all(getattr(m, k) == getattr(c, k) for k in shared + ("clearance_cells",))
    c = GrowthConfig(sub=2, origin=(0.5, -1.0, 2.0), max_steps=17, clearance_cells=2)
    assert c.sub == 2 and list(c.origin) == [0.5, -1.0, 2.0] and c.max_steps == 17 and c.clearance_cells == 2
    with pytest.raises(AttributeError):
        GrowthConfig(no_such_field=1)
    r = GrowthRule()
    assert (r.min_hit, r.hit_per_through) == (3, 4)
    r = GrowthRule(min_hit=1, hit_per_through=0)
    assert (r.min_hit, r.hit_per_through) == (1, 0)
    with pytest.raises(AttributeError):
        GrowthRule(no_such_field=1)
    L.elm_growth_config_default(None)  # a NULL config / rule is ignored
    L.elm_growth_rule_default(None)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_growth_config), offsetof(elm_growth_config, sub),
         offsetof(elm_growth_config, max_steps), offsetof(elm_growth_config, min_range_m), offsetof(elm_growth_config, obs_min_range_m),
         offsetof(elm_growth_config, obs_max_range_m), offsetof(elm_growth_config, end_margin_m),
         offsetof(elm_growth_config, end_margin_frac), offsetof(elm_growth_config, origin), offsetof(elm_growth_config, clearance_cells));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_growth_stats), offsetof(elm_growth_stats, n_cast),
         offsetof(elm_growth_stats, n_observing), offsetof(elm_growth_stats, n_walked), offsetof(elm_growth_stats, n_truncated),
         offsetof(elm_growth_stats, n_end_hit), offsetof(elm_growth_stats, n_end_near), offsetof(elm_growth_stats, n_end_new),
         offsetof(elm_growth_stats, n_end_out), offsetof(elm_growth_stats, n_through_beams), offsetof(elm_growth_stats, n_dropped),
         offsetof(elm_growth_stats, n_through_events), offsetof(elm_growth_stats, n_steps));
  printf("%zu %zu %zu\n", sizeof(elm_growth_rule), offsetof(elm_growth_rule, min_hit), offsetof(elm_growth_rule, hit_per_through));
  printf("%zu %zu %zu\n", sizeof(elm_evidence_config), sizeof(elm_evidence_stats), sizeof(elm_evidence_rule));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, r, old = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    F, S, R = _lib.GrowthConfigC, _lib.GrowthStatsC, _lib.GrowthRuleC
    assert a == [C.sizeof(F), F.sub.offset, F.max_steps.offset, F.min_range_m.offset, F.obs_min_range_m.offset, F.obs_max_range_m.offset,
                 F.end_margin_m.offset, F.end_margin_frac.offset, F.origin.offset, F.clearance_cells.offset]
    assert b == [C.sizeof(S), S.n_cast.offset, S.n_observing.offset, S.n_walked.offset, S.n_truncated.offset, S.n_end_hit.offset,
                 S.n_end_near.offset, S.n_end_new.offset, S.n_end_out.offset, S.n_through_beams.offset, S.n_dropped.offset,
                 S.n_through_events.offset, S.n_steps.offset]
    assert r == [C.sizeof(R), R.min_hit.offset, R.hit_per_through.offset]
    assert a[0] == 80 and b[0] == 56 and r[0] == 8
    # the evidence structs did not change size
    assert old == [C.sizeof(_lib.EvidenceConfigC), C.sizeof(_lib.EvidenceStatsC), C.sizeof(_lib.EvidenceRuleC)] == [72, 48, 8]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import GrowthConfig, GrowthRule
    T = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.GrowthStatsC * 2)()
    cfg, rule = GrowthConfig(), GrowthRule()
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    scans = (C.c_void_p * 2)(1, 1)
    n = C.c_size_t(0)
    out = C.c_void_p()
    assert L.elm_growth_create(None, one, 4, 100, C.byref(out)) == INVALID
    assert L.elm_growth_create(one, None, 4, 100, C.byref(out)) == INVALID
    assert L.elm_growth_create(one, one, 4, 100, None) == INVALID
    for sub in (0, 3, 8, -1):
        assert L.elm_growth_create(one, one, sub, 100, C.byref(out)) == INVALID
    for cap in (0, (1 << 30) + 1):
        assert L.elm_growth_create(one, one, 4, cap, C.byref(out)) == INVALID
    L.elm_growth_destroy(None)
    assert L.elm_growth_reset(None, one) == INVALID and L.elm_growth_reset(one, None) == INVALID

    def acc(ctx, g, s, pose, c):
        return L.elm_growth_accumulate(ctx, g, s, pose, c, st, None)

    assert acc(None, one, one, dp, C.byref(cfg)) == INVALID
    assert acc(one, None, one, dp, C.byref(cfg)) == INVALID
    assert acc(one, one, None, dp, C.byref(cfg)) == INVALID
    assert acc(one, one, one, None, C.byref(cfg)) == INVALID
    assert acc(one, one, one, dp, None) == INVALID
    nan, inf = float("nan"), float("inf")
    for kw in [dict(sub=3), dict(sub=0), dict(max_steps=0), dict(max_steps=(1 << 20) + 1), dict(min_range_m=-0.1), dict(min_range_m=nan),
               dict(obs_min_range_m=-1.0), dict(obs_max_range_m=1.0), dict(obs_max_range_m=inf), dict(end_margin_m=-0.5), dict(end_margin_m=inf),
               dict(end_margin_frac=-0.01), dict(end_margin_frac=nan), dict(origin=(0.0, nan, 0.0)), dict(origin=(inf, 0.0, 0.0)),
               dict(clearance_cells=-1), dict(clearance_cells=3)]:
        assert acc(one, one, one, dp, C.byref(GrowthConfig(**kw))) == INVALID, kw
    for nj in (0, -1, 4097):
        assert L.elm_growth_accumulate_batch(one, one, scans, dp, nj, C.byref(cfg), st) == INVALID
    assert L.elm_growth_accumulate_batch(one, one, None, dp, 1, C.byref(cfg), st) == INVALID
    assert L.elm_growth_cells(one, one, None, None, None, None, 0, None) == INVALID
    assert L.elm_growth_cells(None, one, None, None, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_growth_appeared_points(one, one, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_growth_appeared_points(one, one, C.byref(rule), None, 5, C.byref(n)) == INVALID
    assert L.elm_growth_appeared_points(one, None, C.byref(rule), None, 0, C.byref(n)) == INVALID


def test_shim_growth_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/growth_calls.cpp, built as tests/test_shim_compile.py builds pcm_calls.cpp"""
    exe = tmp_path / "growth_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "growth_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the hand-made map
# voxel 1.0, sub 4: 0.25 m cells.  Three stored points: the occupied cells are (5, 0, 0), (6, 0, 0) and (0, -4, 0) (floor(-0.9 / 0.25)).
# Identity pose, origin O at the centre of cell (0, 0, 0): cell k along an axis is left at t = 0.25 (k + 1) - 0.125, exact.  Walks start at
# t = 0.5 (cell 2 on the beam's axis), margin 0.25 m without a fractional part, beams of any length observe.  Every coordinate below is a
# float32 value.
#   H   +x, L 1.25: end x = 1.375, cell (5, 0, 0), occupied: END-HIT.  reach 1.0: cells 2 and 3 are left (0.625, 0.875), cell 4 would be
#       left at 1.125.  2 steps.
#   N   +x, L 1: end x = 1.125, cell (4, 0, 0), free, next to the occupied (5, 0, 0): END-NEAR at clearance 1 and 2, END-NEW at clearance
#       0.  reach 0.75: cell 2 is left, cell 3 would be left at 0.875.  1 step.  All three fractions are 0.5: k = 32768.
#   W   +z, L 3: end z = 3.125, cell (0, 0, 12), free and far from everything: END-NEW, k = (32768, 32768, 32768).  reach 2.75: cells
#       2 .. 10 are left (cell 10 at 2.625), cell 11 would be left at 2.875.  9 steps.
#   Z   +z, L 3.375: end z = 3.5, exactly the lower face of cell (0, 0, 14), which owns it: END-NEW, k_z = 0.  reach 3.125 is EXACTLY the
#       parameter at which cell 12 is left: t_next = reach is not beyond it, the step is taken, and cell 12 is W's candidate: one through
#       event -- in the same call (phase 2 sees all of phase 1), or in a later call than W's; none when Z's call comes first.  Cells
#       2 .. 12 are left: 11 steps.
#   X   +x, L 300 000: end cell x = 1 200 000 >= 2^20: END-OUT.  It walks and is TRUNCATED after max_steps steps; on its way it leaves
#       cell (4, 0, 0) (at 1.125), a through event where N made that cell a candidate (clearance 0).
#   K   -y, L 0.125 (the float64 difference -1e-30 - 0.125 rounds to -0.125): end y = -1e-30, v = -4e-30, floor -1: cell (0, -1, 0), free,
#       nothing within 2 cells: END-NEW.  v - floor(v) rounds to exactly 1.0, 65536 after the scaling: k_y is CLAMPED to 65535.  reach < 0:
#       no walk.
#   C   -y, L 0.75: end y = -0.625, cell (0, -3, 0), free, next to the occupied (0, -4, 0): END-NEAR (END-NEW at clearance 0, k_y = 32768:
#       v = -2.5).  reach 0.5 = min_range_m, not beyond it: no walk.
#   the origin itself: not cast.
STORED = np.array([(1.3, 0.1, 0.2), (1.6, 0.2, 0.1), (0.1, -0.9, 0.1)], np.float32)
O = np.array((0.125, 0.125, 0.125))
H, N, W, Z, X = O + (1.25, 0, 0), O + (1, 0, 0), O + (0, 0, 3), O + (0, 0, 3.375), O + (300000, 0, 0)
K, Cb = np.array((0.125, -1e-30, 0.125)), O + (0, -0.75, 0)
BEAMS = np.array([H, N, W, Z, X, K, Cb, O], np.float32)
HALF = 32768
MAIN_CELLS = [[0, -1, 0], [0, 0, 12], [0, 0, 14]]
MAIN = dict(hit=[1, 1, 1], through=[0, 1, 0], sums=[[HALF, 65535, HALF], [HALF, HALF, HALF], [HALF, HALF, 0]], events=[0, 0, 0, 1, 0, 0, 0, 0],
            stats=dict(n_cast=7, n_observing=7, n_walked=5, n_truncated=1, n_end_hit=1, n_end_near=2, n_end_new=3, n_end_out=1, n_through_beams=1,
                       n_dropped=0, n_through_events=1, n_steps=2 + 1 + 9 + 11 + 4096))
ZERO_CELLS = [[0, -3, 0], [0, -1, 0], [0, 0, 12], [0, 0, 14], [4, 0, 0]]
ZERO = dict(hit=[1, 1, 1, 1, 1], through=[0, 0, 1, 0, 1], sums=[[HALF, HALF, HALF], [HALF, 65535, HALF], [HALF, HALF, HALF], [HALF, HALF, 0], [HALF, HALF, HALF]],
            events=[0, 0, 0, 1, 1, 0, 0, 0],
            stats=dict(MAIN["stats"], n_end_near=0, n_end_new=5, n_through_beams=2, n_through_events=2))


def _cfg(**kw):
    c = dict(min_range_m=0.5, obs_min_range_m=0.0, obs_max_range_m=1e6, end_margin_m=0.25, end_margin_frac=0.0, origin=tuple(O))
    c.update(kw)
    return c


def _expect_point(cell, sums, hit, size=0.25):
    return [(float(c) + (float(s) / float(hit) + 0.5) / 65536.0) * size for c, s in zip(cell, sums)]


def _check(cells, hit, through, sums, st, ev, want_cells, want):
    assert cells.tolist() == want_cells
    assert hit.tolist() == want["hit"] and through.tolist() == want["through"] and sums.tolist() == want["sums"]
    assert st == want["stats"] and ev.tolist() == want["events"]


def test_the_mirror_on_a_map_worked_out_by_hand():
    eye = np.eye(4)[None]
    for clearance in (1, 2):
        g = growth_ref.Growth(STORED, 1.0, 4)
        st, ev, left = g.call(growth_ref.Cfg(**_cfg(clearance_cells=clearance)), [BEAMS], eye, trace=True)
        _check(*g.cells(), st[0], ev[0], MAIN_CELLS, MAIN)
    left = left[0]
    assert left[0] == [(2, 0, 0), (3, 0, 0)] and left[1] == [(2, 0, 0)] and left[2] == [(0, 0, z) for z in range(2, 11)]
    assert left[3] == [(0, 0, z) for z in range(2, 13)] and left[4] == [(x, 0, 0) for x in range(2, 4098)] and left[5] == left[6] == left[7] == []
    # the points and the rule: with min_hit 1 all three cells have appeared ((0, 0, 12): hit 1 >= 0 * through); the default needs 3 hits
    assert np.array_equal(g.appeared_points(1, 0), np.array([_expect_point(c, s, 1) for c, s in zip(MAIN_CELLS, MAIN["sums"])]))
    assert g.appeared(1, 1).tolist() == [True, True, True] and g.appeared(1, 2).tolist() == [True, False, True] and not g.appeared().any()
    assert g.appeared_points(1, 0)[0].tolist() == [0.25 * 32768.5 / 65536.0, 0.25 * (-1.0 + 65535.5 / 65536.0), 0.25 * 32768.5 / 65536.0]
    # clearance 0: never NEAR
    g = growth_ref.Growth(STORED, 1.0, 4)
    st, ev, _ = g.call(growth_ref.Cfg(**_cfg(clearance_cells=0)), [BEAMS], eye)
    _check(*g.cells(), st[0], ev[0], ZERO_CELLS, ZERO)
    # order.  One call: both job orders give the same counters.  Two calls: W's cell exists when Z walks, or it does not yet
    cfg = growth_ref.Cfg(**_cfg())
    two = np.stack([np.eye(4)] * 2)
    for jobs in ([BEAMS[2:3], BEAMS[3:4]], [BEAMS[3:4], BEAMS[2:3]]):
        g = growth_ref.Growth(STORED, 1.0, 4)
        st, _, _ = g.call(cfg, jobs, two)
        cells, hit, through, _ = g.cells()
        assert cells.tolist() == [[0, 0, 12], [0, 0, 14]] and hit.tolist() == [1, 1] and through.tolist() == [1, 0]
        assert sorted(s["n_through_events"] for s in st) == [0, 1]
    for first, second, want in ((2, 3, [1, 0]), (3, 2, [0, 0])):
        g = growth_ref.Growth(STORED, 1.0, 4)
        g.call(cfg, [BEAMS[first:first + 1]], eye)
        st, _, _ = g.call(cfg, [BEAMS[second:second + 1]], eye)
        cells, hit, through, _ = g.cells()
        assert cells.tolist() == [[0, 0, 12], [0, 0, 14]] and hit.tolist() == [1, 1] and through.tolist() == want
        assert st[0]["n_through_events"] == want[0] * (second == 3)
    # a second observation adds to the first; reset empties the table
    g = growth_ref.Growth(STORED, 1.0, 4)
    g.call(cfg, [BEAMS], eye)
    g.call(cfg, [BEAMS], eye)
    cells, hit, through, sums = g.cells()
    assert cells.tolist() == MAIN_CELLS and hit.tolist() == [2, 2, 2] and through.tolist() == [0, 2, 0] and sums.tolist() == (2 * np.array(MAIN["sums"])).tolist()
    assert np.array_equal(g.appeared_points(1, 0), np.array([_expect_point(c, 2 * np.array(s), 2) for c, s in zip(MAIN_CELLS, MAIN["sums"])]))
    g.reset()
    assert g.cells()[0].shape == (0, 3) and g.appeared_points().shape == (0, 3)
    # max_steps 8 truncates X after cells 2 .. 9; sub 1 (1 m cells): W and Z both end in cell (0, 0, 3), fractions 0.125 and 0.5
    g = growth_ref.Growth(STORED, 1.0, 4)
    st, _, left = g.call(growth_ref.Cfg(**_cfg(max_steps=8)), [BEAMS[4:5]], eye, trace=True)
    assert left[0][0] == [(x, 0, 0) for x in range(2, 10)] and (st[0]["n_truncated"], st[0]["n_steps"], st[0]["n_end_out"]) == (1, 8, 1)
    g = growth_ref.Growth(STORED, 1.0, 1)
    g.call(growth_ref.Cfg(**_cfg(sub=1, clearance_cells=0)), [BEAMS[[2, 3]]], eye)
    cells, hit, _, sums = g.cells()
    assert cells.tolist() == [[0, 0, 3]] and hit.tolist() == [2] and sums.tolist() == [[16384, 16384, 8192 + 32768]]
    # the rule
    h, t = np.array([2, 3, 3, 4, 8, 7, 0], np.uint32), np.array([0, 0, 1, 1, 2, 2, 0], np.uint32)
    assert growth_ref.appeared_cells(h, t).tolist() == [False, True, False, True, True, False, False]
    assert growth_ref.appeared_cells(np.array([4000000000], np.uint32), np.array([3000000000], np.uint32), 1, 2).tolist() == [False]  # no 32-bit wrap


@pytest.mark.gpu
def test_the_gpu_on_the_map_worked_out_by_hand():
    from elimaloc_amd.registration import Context, GrowthConfig, GrowthRule, VoxelHashMap
    ctx = Context(0)
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(STORED)
    assert vm.FineCells(4).tolist() == [[0, -4, 0], [5, 0, 0], [6, 0, 0]]
    eye = np.eye(4)
    g = vm.Growth(64)
    for clearance in (1, 2):
        g.Reset()
        st, ev = g.Accumulate(BEAMS, eye, GrowthConfig(**_cfg(clearance_cells=clearance)), events=True)
        _check(*g.Cells(), st, ev, MAIN_CELLS, MAIN)
        assert g.Count() == 3
    assert np.array_equal(g.AppearedPoints(GrowthRule(min_hit=1, hit_per_through=0)),
                          np.array([_expect_point(c, s, 1) for c, s in zip(MAIN_CELLS, MAIN["sums"])]))
    assert len(g.AppearedPoints(GrowthRule(min_hit=1, hit_per_through=2))) == 2 and g.AppearedPoints().shape == (0, 3)
    g.Reset()
    assert g.Count() == 0 and g.Cells()[0].shape == (0, 3)
    st, ev = g.Accumulate(BEAMS, eye, GrowthConfig(**_cfg(clearance_cells=0)), events=True)
    _check(*g.Cells(), st, ev, ZERO_CELLS, ZERO)
    cfg = GrowthConfig(**_cfg())
    two = np.stack([eye] * 2)
    for jobs in ([BEAMS[2:3], BEAMS[3:4]], [BEAMS[3:4], BEAMS[2:3]]):
        g.Reset()
        st = g.Accumulate(jobs, two, cfg)
        cells, hit, through, _ = g.Cells()
        assert cells.tolist() == [[0, 0, 12], [0, 0, 14]] and hit.tolist() == [1, 1] and through.tolist() == [1, 0]
        assert sorted(s["n_through_events"] for s in st) == [0, 1]
    for first, second, want in ((2, 3, [1, 0]), (3, 2, [0, 0])):
        g.Reset()
        g.Accumulate(BEAMS[first:first + 1], eye, cfg)
        st = g.Accumulate(BEAMS[second:second + 1], eye, cfg)
        cells, hit, through, _ = g.Cells()
        assert cells.tolist() == [[0, 0, 12], [0, 0, 14]] and hit.tolist() == [1, 1] and through.tolist() == want
        assert st["n_through_events"] == want[0] * (second == 3)
    g.Reset()
    g.Accumulate(BEAMS, eye, cfg)
    g.Accumulate(BEAMS, eye, cfg)
    cells, hit, through, sums = g.Cells()
    assert cells.tolist() == MAIN_CELLS and hit.tolist() == [2, 2, 2] and through.tolist() == [0, 2, 0] and sums.tolist() == (2 * np.array(MAIN["sums"])).tolist()
    g1 = vm.Growth(16, sub=1)
    g1.Accumulate(BEAMS[[2, 3]], eye, GrowthConfig(**_cfg(sub=1, clearance_cells=0)))
    cells, hit, _, sums = g1.Cells()
    assert cells.tolist() == [[0, 0, 3]] and hit.tolist() == [2] and sums.tolist() == [[16384, 16384, 8192 + 32768]]
    g1.close()
    g.close()
    del vm
    ctx.close()
