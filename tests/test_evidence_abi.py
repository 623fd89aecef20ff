"""CPU checks of the map-evidence ABI (include/elimaloc_hip.h, map evidence): the config and rule defaults, the struct layouts against
the ctypes mirrors, argument errors without a device, the C++ shim's MapEvidence compiling, and the numpy mirror of the contract
(tests/evidence_ref.py) pinned on a map of three cells whose walks and counters are written out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import evidence_ref  # tests/ is on sys.path via conftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def test_evidence_config_and_rule_defaults(L):
    from elimaloc_amd.registration import EvidenceConfig, EvidenceRule
    c = EvidenceConfig()
    assert (c.sub, c.max_steps) == (4, 4096)
    assert (c.min_range_m, c.obs_min_range_m, c.obs_max_range_m, c.end_margin_m, c.end_margin_frac) == (1.0, 2.0, 50.0, 1.0, 0.2)
    assert list(c.origin) == [0.0, 0.0, 0.0]
    m = evidence_ref.Cfg()  # the mirror's plain config carries the same defaults
    assert all(getattr(m, k) == getattr(c, k) for k in ("sub", "max_steps", "min_range_m", "obs_min_range_m", "obs_max_range_m", "end_margin_m",
                                                        "end_margin_frac"))
    c = EvidenceConfig(sub=2, origin=(0.5, -1.0, 2.0), max_steps=17, end_margin_frac=0.1)
    assert c.sub == 2 and list(c.origin) == [0.5, -1.0, 2.0] and c.max_steps == 17 and c.end_margin_frac == 0.1
    with pytest.raises(AttributeError):
        EvidenceConfig(no_such_field=1)
    r = EvidenceRule()
    assert (r.min_through, r.through_per_hit) == (3, 4)
    r = EvidenceRule(min_through=1, through_per_hit=0)
    assert (r.min_through, r.through_per_hit) == (1, 0)
    with pytest.raises(AttributeError):
        EvidenceRule(no_such_field=1)
    L.elm_evidence_config_default(None)  # a NULL config / rule is ignored
    L.elm_evidence_rule_default(None)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_evidence_config), offsetof(elm_evidence_config, sub),
         offsetof(elm_evidence_config, max_steps), offsetof(elm_evidence_config, min_range_m), offsetof(elm_evidence_config, obs_min_range_m),
         offsetof(elm_evidence_config, obs_max_range_m), offsetof(elm_evidence_config, end_margin_m),
         offsetof(elm_evidence_config, end_margin_frac), offsetof(elm_evidence_config, origin));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_evidence_stats), offsetof(elm_evidence_stats, n_cast),
         offsetof(elm_evidence_stats, n_observing), offsetof(elm_evidence_stats, n_walked), offsetof(elm_evidence_stats, n_truncated),
         offsetof(elm_evidence_stats, n_through_beams), offsetof(elm_evidence_stats, n_end_hit), offsetof(elm_evidence_stats, n_end_free),
         offsetof(elm_evidence_stats, n_through_events), offsetof(elm_evidence_stats, n_steps));
  printf("%zu %zu %zu\n", sizeof(elm_evidence_rule), offsetof(elm_evidence_rule, min_through), offsetof(elm_evidence_rule, through_per_hit));
  printf("%zu %zu %zu %zu\n", sizeof(elm_raycast_config), sizeof(elm_raycast_stats), sizeof(elm_freespace_config), sizeof(elm_freespace_stats));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    a, b, r, old = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    F, S, R = _lib.EvidenceConfigC, _lib.EvidenceStatsC, _lib.EvidenceRuleC
    assert a == [C.sizeof(F), F.sub.offset, F.max_steps.offset, F.min_range_m.offset, F.obs_min_range_m.offset, F.obs_max_range_m.offset,
                 F.end_margin_m.offset, F.end_margin_frac.offset, F.origin.offset]
    assert b == [C.sizeof(S), S.n_cast.offset, S.n_observing.offset, S.n_walked.offset, S.n_truncated.offset, S.n_through_beams.offset,
                 S.n_end_hit.offset, S.n_end_free.offset, S.n_through_events.offset, S.n_steps.offset]
    assert r == [C.sizeof(R), R.min_through.offset, R.through_per_hit.offset]
    assert a[0] == 72 and b[0] == 48 and r[0] == 8
    # no existing struct changed size
    assert old == [C.sizeof(_lib.RayCastConfigC), C.sizeof(_lib.RayCastStatsC), C.sizeof(_lib.FreeSpaceConfigC), C.sizeof(_lib.FreeSpaceStatsC)]


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import EvidenceConfig, EvidenceRule
    T = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    st = (_lib.EvidenceStatsC * 2)()
    cfg, rule = EvidenceConfig(), EvidenceRule()
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    scans = (C.c_void_p * 2)(1, 1)
    n = C.c_size_t(0)
    out = C.c_void_p()
    assert L.elm_evidence_create(None, one, 4, C.byref(out)) == INVALID
    assert L.elm_evidence_create(one, None, 4, C.byref(out)) == INVALID
    assert L.elm_evidence_create(one, one, 4, None) == INVALID
    for sub in (0, 3, 8, -1):
        assert L.elm_evidence_create(one, one, sub, C.byref(out)) == INVALID
    L.elm_evidence_destroy(None)
    assert L.elm_evidence_reset(None, one) == INVALID and L.elm_evidence_reset(one, None) == INVALID

    def acc(ctx, ev, s, pose, c):
        return L.elm_evidence_accumulate(ctx, ev, s, pose, c, st, None)

    assert acc(None, one, one, dp, C.byref(cfg)) == INVALID
    assert acc(one, None, one, dp, C.byref(cfg)) == INVALID
    assert acc(one, one, None, dp, C.byref(cfg)) == INVALID
    assert acc(one, one, one, None, C.byref(cfg)) == INVALID
    assert acc(one, one, one, dp, None) == INVALID
    nan, inf = float("nan"), float("inf")
    for kw in [dict(sub=3), dict(sub=0), dict(max_steps=0), dict(max_steps=(1 << 20) + 1), dict(min_range_m=-0.1), dict(min_range_m=nan),
               dict(obs_min_range_m=-1.0), dict(obs_max_range_m=1.0), dict(obs_max_range_m=inf), dict(end_margin_m=-0.5), dict(end_margin_m=inf),
               dict(end_margin_frac=-0.01), dict(end_margin_frac=nan), dict(origin=(0.0, nan, 0.0)), dict(origin=(inf, 0.0, 0.0))]:
        assert acc(one, one, one, dp, C.byref(EvidenceConfig(**kw))) == INVALID, kw
    for nj in (0, -1, 4097):
        assert L.elm_evidence_accumulate_batch(one, one, scans, dp, nj, C.byref(cfg), st) == INVALID
    assert L.elm_evidence_accumulate_batch(one, one, None, dp, 1, C.byref(cfg), st) == INVALID
    assert L.elm_evidence_counts(one, one, None, None, 0, None) == INVALID
    assert L.elm_evidence_counts(None, one, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_evidence_stale_points(one, one, None, None, 0, C.byref(n)) == INVALID
    assert L.elm_evidence_stale_points(one, one, C.byref(rule), None, 5, C.byref(n)) == INVALID
    assert L.elm_evidence_stale_points(one, None, C.byref(rule), None, 0, C.byref(n)) == INVALID


def test_shim_map_evidence_compiles_and_links(L, tmp_path):
    src = tmp_path / "evid_shim.cpp"
    src.write_text(r'''
#include "registration.hpp"
// a replayed trajectory accumulated on the map, then the share of stored points that the default rule calls stale
double stale_share(const std::vector<std::vector<PointStruct>>& scans, const std::vector<Eigen::Matrix4d>& poses, const VoxelHashMap& map) {
    MapEvidence ev(map, 4);
    EvidenceConfig cfg;
    cfg.end_margin_frac = 0.25;
    cfg.origin[2] = 0.1;
    const std::vector<elm_evidence_stats> st = ev.Accumulate(scans, poses, cfg);
    const elm_evidence_stats one = ev.Accumulate(scans[0], poses[0]);
    std::vector<uint32_t> through, hit;
    ev.Counts(through, hit);
    EvidenceRule rule;
    rule.min_through = 5;
    const std::vector<uint8_t> flags = ev.StalePoints(rule);
    const std::vector<uint8_t> dflt = ev.StalePoints();
    ev.Reset();
    size_t stale = 0;
    for (uint8_t f : flags) stale += f;
    return flags.empty() ? (double)(st.size() + one.n_cast + through.size() + hit.size() + dflt.size()) : (double)stale / (double)flags.size();
}
int main(int argc, char**) {
    if (argc > 1) {
        std::vector<std::vector<PointStruct>> s(1);
        VoxelHashMap m;
        return (int)stale_share(s, std::vector<Eigen::Matrix4d>(1, Eigen::Matrix4d::Identity()), m);
    }
    return 0;
}
''')
    exe = tmp_path / "evid_shim"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"), str(src),
                               "-L", libdir, "-lelimaloc_hip", "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# voxel 1.0, sub 4: 0.25 m cells.  Three stored points: cells (5, 0, 0), (6, 0, 0) and (0, -4, 0) (floor(-0.9 / 0.25) = -4); in
# elm_map_fine_cells' ascending order: (0, -4, 0), (5, 0, 0), (6, 0, 0).
STORED = np.array([(1.3, 0.1, 0.2), (1.6, 0.2, 0.1), (0.1, -0.9, 0.1)], np.float32)
O = np.array((0.125, 0.125, 0.125))  # the centre of cell (0, 0, 0): cell k along an axis is left at t = 0.25 (k + 1) - 0.125, exact
A, B, Cb, D, E = O + (2, 0, 0), O + (1.625, 0, 0), O + (0, -0.75, 0), O + (0, -1, 0), O + (0, 0, 3)
BEAMS = np.array([A, B, Cb, D, E, O, O + (12, 0, 0)], np.float32)


def _cfg(**kw):
    c = dict(min_range_m=0.5, obs_min_range_m=0.0, obs_max_range_m=10.0, end_margin_m=0.25, end_margin_frac=0.0, origin=tuple(O))
    c.update(kw)
    return evidence_ref.Cfg(**c)


def _one(cfg, beams, T=np.eye(4)):
    cells, through, hit, st, ev, left = evidence_ref.mirror(STORED, 1.0, cfg, [beams], T[None], trace=True)
    assert cells.tolist() == [[0, -4, 0], [5, 0, 0], [6, 0, 0]]
    return through.tolist(), hit.tolist(), st[0], ev[0].tolist(), left[0]


def test_the_mirror_on_a_map_worked_out_by_hand():
    """Identity pose, origin at the centre of cell (0, 0, 0), walks from t = 0.5, margin 0.25 m (no fractional part).
    A  +x, L 2: end point in cell x = 8, empty -> END-FREE.  reach 1.75.  Starts in cell 2 (0.625 / 0.25); cells 2 .. 6 are left at t = 0.625,
       0.875, 1.125, 1.375, 1.625; cell 7 would be left at 1.875 > 1.75: the walk ends there BY REACH.  5 steps; cells 5 and 6 are occupied:
       2 events.
    B  +x, L 1.625: end point in cell 7, empty.  reach 1.375 EXACTLY the parameter at which cell 5 is left: t_next = reach is not beyond
       it, the step is taken and cell 5 counts.  Cell 6 would be left at 1.625 > 1.375.  4 steps, 1 event.
    C  -y, L 0.75: end point y = -0.625, cell -3, empty.  reach 0.5 = min_range_m, not beyond it: no walk, the end point only.
    D  -y, L 1: end point y = -0.875, cell -4, occupied -> END-HIT.  reach 0.75.  Starts in cell -2 (floor(-1.5)), left at 0.625; cell -3
       would be left at 0.875 > 0.75.  1 step, no event.
    E  +z, L 3: end point in cell 12, empty.  reach 2.75: cells 2 .. 10 are left (cell 10 at 2.625), cell 11 would be left at 2.875.  9 steps.
    the origin itself: not cast.  +x, L 12: cast, beyond obs_max_range_m 10: not observing, touches nothing."""
    through, hit, st, ev, left = _one(_cfg(), BEAMS)
    assert through == [0, 2, 1] and hit == [1, 0, 0]
    assert st == dict(n_cast=6, n_observing=5, n_walked=4, n_truncated=0, n_through_beams=2, n_end_hit=1, n_end_free=4, n_through_events=3,
                      n_steps=19)
    assert ev == [2, 1, 0, 0, 0, 0, 0]
    assert left[0] == [(x, 0, 0) for x in range(2, 7)] and left[1] == [(x, 0, 0) for x in range(2, 6)] and left[2] == []
    assert left[3] == [(0, -2, 0)] and left[4] == [(0, 0, z) for z in range(2, 11)] and left[5] == [] and left[6] == []
    # D with a margin of 0.5: reach 0.5 is not beyond min_range_m -> its end point counts, nothing is walked
    through, hit, st, ev, left = _one(_cfg(end_margin_m=0.5), BEAMS[3:4])
    assert through == [0, 0, 0] and hit == [1, 0, 0] and left[0] == []
    assert st == dict(n_cast=1, n_observing=1, n_walked=0, n_truncated=0, n_through_beams=0, n_end_hit=1, n_end_free=0, n_through_events=0,
                      n_steps=0)
    # A with max_steps 2: cells 2 and 3 are left, the third step is not taken -> truncated, no event; with max_steps 4 cells 2 .. 5 are left
    # (cell 5 counts), and the step out of cell 6 (1.625 <= 1.75) is refused: truncated with 1 event
    through, hit, st, ev, left = _one(_cfg(max_steps=2), BEAMS[:1])
    assert through == [0, 0, 0] and (st["n_truncated"], st["n_steps"], st["n_through_events"], st["n_through_beams"]) == (1, 2, 0, 0)
    through, hit, st, ev, left = _one(_cfg(max_steps=4), BEAMS[:1])
    assert through == [0, 1, 0] and (st["n_truncated"], st["n_steps"], st["n_through_events"], st["n_through_beams"]) == (1, 4, 1, 1)
    assert left[0] == [(x, 0, 0) for x in range(2, 6)]
    # max_steps 5 is exactly enough: the walk ends by reach, not truncated
    through, hit, st, ev, left = _one(_cfg(max_steps=5), BEAMS[:1])
    assert through == [0, 1, 1] and (st["n_truncated"], st["n_steps"]) == (0, 5)
    # the fractional margin: 0.5 L = 1 > 0.25 -> reach 1.0: cells 2 and 3 are left (0.625, 0.875), cell 4 would be left at 1.125
    through, hit, st, ev, left = _one(_cfg(end_margin_frac=0.5), BEAMS[:1])
    assert through == [0, 0, 0] and st["n_steps"] == 2 and st["n_walked"] == 1
    # observing band: A (L 2) outside [0, 1.9] is cast and touches nothing
    through, hit, st, ev, left = _one(_cfg(obs_max_range_m=1.9), BEAMS[:1])
    assert through == [0, 0, 0] and (st["n_cast"], st["n_observing"], st["n_end_free"]) == (1, 0, 0)
    # a pose: a quarter turn about z maps the sensor's +x beam onto the world's -y from the same origin cell.  A (L 2): end point y = -1.875,
    # cell -8, empty; reach 1.75; starts in cell -2, cells -2 .. -6 are left at 0.625 .. 1.625; cell -4 is occupied: 1 event
    T = np.eye(4)
    T[:3, :3] = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]
    T[:3, 3] = O - T[:3, :3] @ O  # keeps the world origin of the beams at O
    through, hit, st, ev, left = _one(_cfg(), BEAMS[:1], T)
    assert through == [1, 0, 0] and hit == [0, 0, 0] and left[0] == [(0, y, 0) for y in range(-2, -7, -1)] and st["n_steps"] == 5
    # sub 1 (1 m cells): A starts in cell 0, which is left at t = 0.875; cell 1 (both x points) would be left at 1.875 > 1.75: no event
    cells, through, hit, st, ev, _ = evidence_ref.mirror(STORED, 1.0, _cfg(sub=1), [BEAMS[:1]], np.eye(4)[None])
    assert cells.tolist() == [[0, -1, 0], [1, 0, 0]] and through.tolist() == [0, 0] and st[0]["n_steps"] == 1
    # two observations add up; an empty map counts nothing
    cells, through, hit, st, ev, _ = evidence_ref.mirror(STORED, 1.0, _cfg(), [BEAMS, BEAMS[:2]], np.stack([np.eye(4)] * 2))
    assert through.tolist() == [0, 4, 2] and hit.tolist() == [1, 0, 0] and [s["n_through_events"] for s in st] == [3, 3]
    cells, through, hit, st, ev, _ = evidence_ref.mirror(np.zeros((0, 3)), 1.0, _cfg(), [BEAMS], np.eye(4)[None])
    assert cells.shape == (0, 3) and through.size == 0 and st[0]["n_end_free"] == 5 and st[0]["n_through_events"] == 0 and st[0]["n_steps"] == 19
    # the rule
    t, h = np.array([2, 3, 3, 4, 8, 7, 0], np.uint32), np.array([0, 0, 1, 1, 2, 2, 0], np.uint32)
    assert evidence_ref.stale_cells(t, h).tolist() == [False, True, False, True, True, False, False]
    assert evidence_ref.stale_cells(np.array([4000000000], np.uint32), np.array([3000000000], np.uint32), 1, 2).tolist() == [False]  # no 32-bit wrap
