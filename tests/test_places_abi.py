"""Place recognition (include/elimaloc_hip.h, "place recognition") on the CPU: the numpy mirror of the contract
(tests/places_ref.py) on bins, shifts, scores and selections worked out by hand; the library's direction table; the quarter turn; the
symbols, the struct layouts, the argument errors without a device and the C++ shim's call lines; the loop's fixed inputs
(tests/places_cases.py) run with the mirror, equal to the committed fixture and meeting the condition the GPU loop test rests on, and
registered with the oracle from their true poses."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import places_cases as cases
import places_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def dirs(L):
    from elimaloc_amd.places import PlaceTables
    return PlaceTables()[2]


def _prev(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


# ---------------------------------------------------------------- the tables
def test_config_defaults_and_tables(L):
    from elimaloc_amd.places import PlaceConfig, PlaceTables
    c = PlaceConfig()
    assert (c.n_rings, c.n_layers, c.r_min_m, c.r_max_m, c.z_min_m, c.z_max_m) == (16, 8, 2.0, 42.0, -3.0, 9.0)
    m = ref.Cfg()
    assert all(getattr(m, k) == getattr(c, k) for k in ("n_rings", "n_layers", "r_min_m", "r_max_m", "z_min_m", "z_max_m"))
    with pytest.raises(AttributeError):
        PlaceConfig(no_such_field=1)
    L.elm_places_config_default(None)
    for kw in (dict(), dict(n_rings=1, n_layers=1), dict(n_rings=32, n_layers=16), dict(n_rings=7, n_layers=3, r_min_m=0.0, r_max_m=33.3, z_min_m=-1.1)):
        c = PlaceConfig(**kw)
        re_, ze, _ = PlaceTables(c)
        mre, mze = ref.edge_tables(ref.Cfg(**{k: getattr(c, k) for k in ("n_rings", "n_layers", "r_min_m", "r_max_m", "z_min_m", "z_max_m")}))
        assert re_.tobytes() == mre.tobytes() and ze.tobytes() == mze.tobytes()  # the mirror re-derives the same bytes
        assert re_[-1] == c.r_max_m * c.r_max_m and ze[-1] == c.z_max_m and re_[0] == c.r_min_m * c.r_min_m and ze[0] == c.z_min_m


def test_direction_table_symmetries_and_values(dirs):
    d = dirs
    assert d.shape == (64, 2) and d[0].tolist() == [1.0, 0.0] and d[16].tolist() == [0.0, 1.0]
    assert d[32].tolist() == [-1.0, 0.0] and d[48].tolist() == [0.0, -1.0]
    assert d[8, 0] == d[8, 1] == math.cos(math.pi / 4.0)
    assert not np.signbit(d[d == 0.0]).any()  # zeros are +0.0
    for k in range(9):
        assert d[16 - k].tolist() == [d[k, 1], d[k, 0]]  # about the diagonal
    for k in range(64):
        assert d[(k + 16) & 63].tolist() == [-d[k, 1], d[k, 0]]  # a quarter turn, exactly (-0.0 == 0.0)
        assert d[(k + 32) & 63].tolist() == [-d[k, 0], -d[k, 1]]
    # numpy's cos / sin of the angle itself.  In float64 the angle 2 pi k / 64 carries a rounding error of up to half an ulp of a number
    # near 6, which cos and sin pass on as up to 4 ulps of a number near 0.1 (measured: 6e-16): the angle is formed in extended
    # precision, so that what is compared to 1 float64 ulp is the table and not the reference's argument
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18
    a = ld(8) * np.arctan(ld(1)) * np.arange(64).astype(ld) / ld(64)
    want = np.stack([np.cos(a), np.sin(a)], axis=1)
    big = np.abs(want) > 1e-9  # (cos(pi / 2) is 1e-20 there, where the table holds the exact 0)
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    assert (np.abs(d.astype(ld) - want)[big] <= ulp[big]).all() and (d[~big] == 0.0).all()


# ---------------------------------------------------------------- the mirror, by hand
def test_bins_at_the_edges(dirs):
    cfg = ref.Cfg()  # rings of 2.5 m from 2 m, layers of 1.5 m from -3 m
    # ring edges 2, 4.5, 7 are float32 values: on the edge the upper ring, its predecessor the lower (none below the first, none at the last)
    pts = np.array([(4.5, 0, 0), (_prev(4.5), 0, 0), (2.0, 0, 0), (_prev(2.0), 0, 0), (42.0, 0, 0), (_prev(42.0), 0, 0)], np.float32)
    ring, layer, sector, n_ok = ref.bins(pts, cfg, dirs)
    assert ring.tolist() == [1, 0, 0, -1, -1, 15] and layer.tolist() == [2] * 6 and sector.tolist() == [0] * 6
    # layer edges -3, -1.5, 0, 9
    pts = np.array([(5, 0, -1.5), (5, 0, _prev(-1.5)), (5, 0, -3.0), (5, 0, _prev(-3.0)), (5, 0, 9.0), (5, 0, _prev(9.0)), (5, 0, 0.0)], np.float32)
    ring, layer, sector, n_ok = ref.bins(pts, cfg, dirs)
    assert layer.tolist() == [1, 0, 0, -1, -1, 7, 2] and ring.tolist() == [1] * 7
    # sector boundaries that float32 holds exactly: the axes and the diagonals.  On the boundary the upper sector, just below it (clockwise)
    # the lower
    pts = np.array([(5, 0, 0), (5, _prev(0.0), 0), (0, 5, 0), (np.nextafter(np.float32(0), np.float32(1)), 5, 0), (-5, 0, 0), (0, -5, 0),
                    (3, 3, 0), (3, _prev(3.0), 0), (-3, -3, 0)], np.float32)
    ring, layer, sector, n_ok = ref.bins(pts, cfg, dirs)
    assert sector.tolist() == [0, 63, 16, 15, 32, 48, 8, 7, 40] and n_ok.tolist() == [1] * 9
    # the origin, a point on the z axis and NaNs have no sector / ring and are dropped
    pts = np.array([(0, 0, 0), (0, 0, 5), (np.nan, 1, 0), (5, np.nan, 0), (5, 0, np.nan), (5, 0, 0)], np.float32)
    words, st = ref.describe(pts, cfg, dirs)
    assert st == dict(n_points=6, n_used=1, n_bits=1) and words[1 * 8 + 2] == 1 and ref.popcount(words) == 1
    # a level moves the point before it is binned: 3 m up puts z = 0 into layer 4, a quarter turn puts +x onto +y
    T = np.eye(4)
    T[2, 3] = 3.0
    T[:2, :2] = [[0, -1], [1, 0]]
    ring, layer, sector, _ = ref.bins(np.array([(5, 0, 0)], np.float32), cfg, dirs, T)
    assert (ring[0], layer[0], sector[0]) == (1, 4, 16)


def test_every_point_has_at_most_one_sector(dirs):
    pts = np.concatenate([cases.sector_boundary_points(dirs), cases.random_scan(20000, 3)])
    _, _, sector, n_ok = ref.bins(pts, ref.Cfg(), dirs)
    assert (n_ok == 1).all() and (sector >= 0).all()


def test_shift_table_of_a_one_bit_descriptor():
    a, b = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    a[2], b[2] = np.uint64(1) << np.uint64(5), np.uint64(1) << np.uint64(60)
    # rotl(b, k) carries bit 60 to bit (60 + k) mod 64: it meets bit 5 at k = 9 only
    assert ref.inter_table(a, b).tolist() == [1 if k == 9 else 0 for k in range(64)]
    m = ref.match_all(a[None], b[None])[0, 0]
    assert (int(m["inter"]), int(m["shift"]), int(m["dice_q16"])) == (1, 9, 65536)
    assert ref.rotl(np.array([1 << 63], np.uint64), 1)[0] == 1 and ref.rotl(np.array([1], np.uint64), 63)[0] == np.uint64(1 << 63)
    b[3] = 1  # a bit in another word never meets it
    assert ref.inter_table(a, b).sum() == 1 and ref.match_all(a[None], b[None])[0, 0]["dice_q16"] == (1 << 17) // 3


def test_dice_at_the_64_bit_edge_and_yaw():
    full = np.full(512, ref.M64, np.uint64)
    m = ref.match_all(full[None], full[None])[0, 0]
    assert int(m["inter"]) == 1 << 15 and int(m["shift"]) == 0 and int(m["dice_q16"]) == 65536  # (2^15 << 17 = 2^32 would wrap a uint32)
    assert ref.dice_q16(1 << 15, 1 << 15, 1 << 15) == 65536 and ref.dice_q16(0, 0, 0) == 0 and ref.dice_q16(3, 4, 5) == (3 << 17) // 9
    assert ref.yaw_of_shift(0) == 0.0 and ref.yaw_of_shift(1) == -2.0 * math.pi / 64.0
    assert ref.yaw_of_shift(32) == math.pi and ref.yaw_of_shift(33) == 2.0 * math.pi * 31.0 / 64.0
    assert all(-math.pi < ref.yaw_of_shift(k) <= math.pi for k in range(64))


def test_selection_order_and_exclusion():
    row = np.zeros(6, ref.MATCH_DTYPE)
    row["dice_q16"] = [500, 900, 900, 100, 900, 500]
    ids = np.array([10, 11, 12, 13, 14, 15])
    assert [c["entry"] for c in ref.select(row, ids, 16)] == [1, 2, 4, 0, 5, 3]  # ties: the smaller entry first
    assert [c["entry"] for c in ref.select(row, ids, 2)] == [1, 2]
    assert [c["entry"] for c in ref.select(row, ids, 16, min_dice_q16=500)] == [1, 2, 4, 0, 5]
    assert [c["entry"] for c in ref.select(row, ids, 16, min_dice_q16=501)] == [1, 2, 4]
    assert ref.select(row, ids, 16, min_dice_q16=901) == []
    # the closed range [12, 14]: 11 and 15 stay, 12 and 14 go
    assert [c["id"] for c in ref.select(row, ids, 16, exclude=(12, 14))] == [11, 10, 15]
    assert [c["id"] for c in ref.select(row, ids, 16, exclude=(11, 11))] == [12, 14, 10, 15, 13]
    assert [c["id"] for c in ref.select(row, ids, 16, exclude=(14, 12))] == [11, 12, 14, 10, 15, 13]  # lo > hi: nothing
    assert ref.select(row, ids, 16, exclude=(-5, 99)) == []


def test_quarter_turn_rotates_the_descriptor_by_16_bits(dirs):
    for cfg in (ref.Cfg(), ref.Cfg(32, 16), ref.Cfg(1, 1)):
        pts = np.concatenate([cases.random_scan(5000, 11), cases.sector_boundary_points(dirs)])
        turned = np.ascontiguousarray(np.stack([-pts[:, 1], pts[:, 0], pts[:, 2]], axis=1))
        a, sa = ref.describe(pts, cfg, dirs)
        b, sb = ref.describe(turned, cfg, dirs)
        assert sa == sb and sa["n_used"] > 1000 and b.tobytes() == ref.rotl(a, 16).tobytes()
        m = ref.match_all(b[None], a[None])[0, 0]
        assert int(m["dice_q16"]) == 65536 and int(m["inter"]) == sa["n_bits"] and (int(m["shift"]) == 16 or cfg.n_words == 1)


# ---------------------------------------------------------------- the ABI
def test_symbols_are_declared_and_exported(L):
    from elimaloc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read(), flags=re.S)
    names = {"elm_places_config_default", "elm_places_tables", "elm_places_create", "elm_places_destroy", "elm_places_reset", "elm_places_size",
             "elm_places_describe", "elm_places_add", "elm_places_add_words", "elm_places_download", "elm_places_match_words", "elm_places_query"}
    assert names == set(re.findall(r"\b(elm_places_[a-z0-9_]+)\s*\(", src)) and names <= set(_lib.EXPORTS)
    for n in names:
        assert hasattr(L, n)
    assert "ELM_PLACES_SECTORS 64" in src and "ELM_PLACES_MAX_TOP_K 16" in src


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "elimaloc_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_places_config), offsetof(elm_places_config, n_rings), offsetof(elm_places_config, n_layers),
         offsetof(elm_places_config, r_min_m), offsetof(elm_places_config, r_max_m), offsetof(elm_places_config, z_min_m),
         offsetof(elm_places_config, z_max_m));
  printf("%zu %zu %zu %zu\n", sizeof(elm_places_stats), offsetof(elm_places_stats, n_points), offsetof(elm_places_stats, n_used),
         offsetof(elm_places_stats, n_bits));
  printf("%zu %zu %zu %zu %zu\n", sizeof(elm_places_query_config), offsetof(elm_places_query_config, top_k),
         offsetof(elm_places_query_config, min_dice_q16), offsetof(elm_places_query_config, exclude_id_lo),
         offsetof(elm_places_query_config, exclude_id_hi));
  printf("%zu %zu %zu %zu\n", sizeof(elm_place_match), offsetof(elm_place_match, dice_q16), offsetof(elm_place_match, inter),
         offsetof(elm_place_match, shift));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(elm_place_candidate), offsetof(elm_place_candidate, entry), offsetof(elm_place_candidate, dice_q16),
         offsetof(elm_place_candidate, id), offsetof(elm_place_candidate, inter), offsetof(elm_place_candidate, shift),
         offsetof(elm_place_candidate, yaw_rad));
  printf("%zu %zu %zu\n", sizeof(elm_evidence_config), sizeof(elm_evidence_stats), sizeof(elm_odometry_config));
  return 0; }
'''
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c, s, q, m, k, old = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    F, S, Q, M, K = _lib.PlacesConfigC, _lib.PlacesStatsC, _lib.PlacesQueryConfigC, _lib.PlaceMatchC, _lib.PlaceCandidateC
    assert c == [C.sizeof(F), F.n_rings.offset, F.n_layers.offset, F.r_min_m.offset, F.r_max_m.offset, F.z_min_m.offset, F.z_max_m.offset]
    assert s == [C.sizeof(S), S.n_points.offset, S.n_used.offset, S.n_bits.offset]
    assert q == [C.sizeof(Q), Q.top_k.offset, Q.min_dice_q16.offset, Q.exclude_id_lo.offset, Q.exclude_id_hi.offset]
    assert m == [C.sizeof(M), M.dice_q16.offset, M.inter.offset, M.shift.offset]
    assert k == [C.sizeof(K), K.entry.offset, K.dice_q16.offset, K.id.offset, K.inter.offset, K.shift.offset, K.yaw_rad.offset]
    assert (c[0], s[0], q[0], m[0], k[0]) == (40, 12, 24, 8, 32) and m[0] == ref.MATCH_DTYPE.itemsize
    assert old == [C.sizeof(_lib.EvidenceConfigC), C.sizeof(_lib.EvidenceStatsC), C.sizeof(_lib.OdometryConfigC)]  # no existing struct moved


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.places import PlaceConfig
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    out = C.c_void_p()
    cfg = PlaceConfig()
    nan, inf = float("nan"), float("inf")
    # create and tables: the config
    assert L.elm_places_create(None, C.byref(cfg), 8, C.byref(out)) == INVALID
    assert L.elm_places_create(one, None, 8, C.byref(out)) == INVALID
    assert L.elm_places_create(one, C.byref(cfg), 8, None) == INVALID
    for cap in (0, -1, 65537):
        assert L.elm_places_create(one, C.byref(cfg), cap, C.byref(out)) == INVALID
    bad = [dict(n_rings=0), dict(n_rings=33), dict(n_layers=0), dict(n_layers=17), dict(r_min_m=nan), dict(r_max_m=inf), dict(z_min_m=nan),
           dict(z_max_m=-inf), dict(r_min_m=42.0), dict(r_min_m=50.0), dict(r_min_m=-1.0), dict(z_min_m=9.0), dict(z_max_m=-4.0),
           dict(r_min_m=1.0, r_max_m=1.0 + 2e-16, n_rings=32)]  # (the last: edges that float64 cannot tell apart)
    dp = C.POINTER(C.c_double)
    buf = np.zeros(128)
    for kw in bad:
        assert L.elm_places_create(one, C.byref(PlaceConfig(**kw)), 8, C.byref(out)) == INVALID, kw
        assert L.elm_places_tables(C.byref(PlaceConfig(**kw)), buf.ctypes.data_as(dp), None, None) == INVALID, kw
    assert L.elm_places_tables(None, None, None, None) == INVALID and L.elm_places_tables(C.byref(cfg), None, None, None) == 0
    L.elm_places_destroy(None)
    assert L.elm_places_reset(None, one) == INVALID and L.elm_places_reset(one, None) == INVALID
    n = C.c_size_t(0)
    assert L.elm_places_size(one, one, None) == INVALID and L.elm_places_size(None, one, C.byref(n)) == INVALID
    assert L.elm_places_size(one, None, C.byref(n)) == INVALID
    # the calls on jobs
    scans = (C.c_void_p * 2)(1, 1)
    words = np.zeros(2 * 128, np.uint64)
    wp = words.ctypes.data_as(C.POINTER(C.c_uint64))
    ids = np.zeros(2, np.int64)
    ip = ids.ctypes.data_as(C.POINTER(C.c_int64))
    st = (_lib.PlacesStatsC * 2)()
    eye = np.tile(np.eye(4).ravel(), 2)
    ep = eye.ctypes.data_as(dp)
    assert L.elm_places_describe(None, one, scans, None, 1, wp, st) == INVALID
    assert L.elm_places_describe(one, None, scans, None, 1, wp, st) == INVALID
    assert L.elm_places_describe(one, one, None, None, 1, wp, st) == INVALID
    assert L.elm_places_describe(one, one, scans, None, 1, None, st) == INVALID
    assert L.elm_places_add(one, one, scans, None, None, 1, st) == INVALID
    assert L.elm_places_add(None, one, scans, None, ip, 1, st) == INVALID
    for nj in (0, -1, 4097):
        assert L.elm_places_describe(one, one, scans, None, nj, wp, st) == INVALID
        assert L.elm_places_add(one, one, scans, None, ip, nj, st) == INVALID
    for v in (nan, inf):
        lv = eye.copy()
        lv[16 + 7] = v  # the second job's level
        assert L.elm_places_describe(one, one, scans, lv.ctypes.data_as(dp), 2, wp, st) == INVALID
        assert L.elm_places_add(one, one, scans, lv.ctypes.data_as(dp), ip, 2, st) == INVALID
    assert L.elm_places_add_words(None, one, wp, ip, 1) == INVALID and L.elm_places_add_words(one, None, wp, ip, 1) == INVALID
    assert L.elm_places_add_words(one, one, None, ip, 1) == INVALID and L.elm_places_add_words(one, one, wp, None, 1) == INVALID
    assert L.elm_places_download(None, one, 0, 0, None, None, None) == INVALID and L.elm_places_download(one, None, 0, 0, None, None, None) == INVALID
    # match and query: the counts and top_k
    qc = (_lib.PlacesQueryConfigC * 2)()
    cands = (_lib.PlaceCandidateC * 32)()
    nc = (C.c_int32 * 2)()

    def both(q_cfgs, nq=2, cd=cands, cnt=nc, w=wp, s=scans, lv=ep):
        return (L.elm_places_match_words(one, one, w, nq, q_cfgs, cd, cnt, None), L.elm_places_query(one, one, s, lv, nq, q_cfgs, cd, cnt, None, None))

    for k0, k1 in ((0, 1), (1, 0), (17, 1), (1, 17), (-1, 1)):
        qc[0].top_k, qc[1].top_k = k0, k1
        assert both(qc) == (INVALID, INVALID), (k0, k1)
    qc[0].top_k = qc[1].top_k = 1
    for nq in (0, -1, 4097):
        assert both(qc, nq=nq) == (INVALID, INVALID)
    assert both(None) == (INVALID, INVALID) and both(qc, cd=None) == (INVALID, INVALID) and both(qc, cnt=None) == (INVALID, INVALID)
    assert both(qc, w=None, s=None) == (INVALID, INVALID)
    assert L.elm_places_match_words(None, one, wp, 2, qc, cands, nc, None) == INVALID
    assert L.elm_places_query(one, None, scans, None, 2, qc, cands, nc, None, None) == INVALID
    lv = eye.copy()
    lv[3] = nan
    assert L.elm_places_query(one, one, scans, lv.ctypes.data_as(dp), 2, qc, cands, nc, None, None) == INVALID


def test_shim_places_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/places_calls.cpp, built as tests/test_map_build_device_abi.py builds build_calls.cpp"""
    exe = tmp_path / "places_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "places_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the loop's inputs
def test_the_loop_inputs_and_the_fixture(dirs):
    """The condition the GPU loop test rests on, met by the mirror alone: every revisit's true entry comes first, with no allowance, and
    the shift is within one sector of round(-yaw 64 / 2 pi) mod 64; the mirror's words and candidates are the committed fixture."""
    Lp = cases.loop_inputs()
    assert len(Lp["entry_scans"]) == 24 and len(Lp["revisit_scans"]) == 12 and all(s.shape == (4096, 3) for s in Lp["entry_scans"])
    for e, T in enumerate(Lp["entry_poses"]):
        assert abs(math.hypot(T[0, 3], T[1, 3]) - 35.0) < 1e-9 and T[2, 3] == 2.1
        assert abs(T[0, 0] * T[0, 3] + T[1, 0] * T[1, 3]) < 1e-9  # facing along the circle
    for i, e in enumerate(Lp["revisit_entry"]):
        d = Lp["revisit_poses"][i][:2, 3] - Lp["entry_poses"][e][:2, 3]
        assert np.abs(d).max() <= 1.0
    g = cases.mirror_loop(dirs)
    gold = np.load(cases.GOLDEN)
    for k in ("entry_words", "revisit_words", "matches", "cand_entry", "cand_dice", "cand_inter", "cand_shift", "revisit_entry", "revisit_yaw"):
        assert np.asarray(g[k]).tobytes() == gold[k].tobytes(), k
    assert g["cand_entry"][:, 0].tolist() == Lp["revisit_entry"].tolist()
    for i in range(12):
        assert (int(g["cand_shift"][i, 0]) - cases.expected_shift(Lp["revisit_yaw"][i])) % 64 in (0, 1, 63)
    assert (g["cand_dice"][:, 0].astype(np.int64) - g["cand_dice"][:, 1].astype(np.int64)).min() > 4000  # (the smallest gap inside one query)


LOOP_WINDOW = 24  # tests/test_places.py::WINDOW: entries e - 24 .. e + 24 clipped at the ends of the log are all 24 entries for every e


def test_the_oracle_registers_every_revisit_from_its_true_pose(oracle):
    """Before any GPU run: on the submap LoopCloser.Submap(entry) builds for each revisit in the GPU loop test -- the kept scans of entries
    max(e - window, 0) .. min(e + window, 23) at their poses, as the mirror of the device build places them, float32(R p + t) -- the
    oracle's registration from the revisit's true pose succeeds for every revisit with the closer's own settings (P2P, up to 50
    iterations, a 2 mm stop) and the shipped gates: the fitness stays below 0.4 against max_fitness_score 0.5, so this loop needs no
    gate opened.  With window 24 the clipped range is 0 .. 23 for every entry, so one map serves all revisits."""
    Lp = cases.loop_inputs()
    ranges = {(max(int(e) - LOOP_WINDOW, 0), min(int(e) + LOOP_WINDOW, 23)) for e in Lp["revisit_entry"]}
    assert ranges == {(0, 23)}
    m = oracle.Map(1.0, 30)
    for k in range(24):
        m.add_points(ref.level(Lp["entry_scans"][k], Lp["entry_poses"][k]).astype(np.float32))
    cfg = oracle.default_config(oracle.P2P, max_iteration=50, icp_termination_threshold_m=0.002)
    for i in range(12):
        r = oracle.register(m, Lp["revisit_scans"][i], Lp["revisit_poses"][i], cfg)
        assert r["is_success"] and r["fitness"] < 0.4, (i, r["gate"], r["fitness"])
