"""The device map build (include/elimaloc_hip.h, device map build) on the CPU: the numpy mirror of AddPoints (tests/build_ref.py) against
the oracle, per voxel and in order, on every input family the GPU module runs (tests/build_cases.py); the two facts the contract rests on
-- the stored points of a map survive their own replay, and an incremental add equals one build -- on the mirror and on the oracle; the
symbols in the header; argument errors without a device; and the C++ shim's BuildOnDevice / Updated / WithoutStale / WithAppeared call
lines compiling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import build_cases  # tests/ is on sys.path via conftest
import build_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def _oracle_map(O, clouds, vs, cap):
    """the oracle's map after one add_points per cloud, in canonical form (voxels by key, insertion order inside)"""
    om = O.Map(vs, cap)
    for c in clouds:
        if len(c):
            om.add_points(c)
    if om.num_points == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
    keys, counts = om.voxels()[:2]
    return build_ref.canonical(om.pointcloud()[0], keys, counts)


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)), (np.shape(x), np.shape(y))


# ---------------------------------------------------------------- the mirror against the oracle
@pytest.mark.parametrize("name", build_cases.NAMES)
def test_the_mirror_is_the_oracle(oracle, name):
    pts, vs, cap = build_cases.case(name)
    mp, mk, mc = build_ref.build(pts, vs, cap)
    assert mp.dtype == np.float64 and mk.dtype == np.int32 and mc.dtype == np.int32
    assert mc.sum() == len(mp) and (mc >= 1).all() and (mc <= cap).all()
    _same(build_ref.canonical(mp, mk, mc), _oracle_map(oracle, [pts], vs, cap))
    # bucket order: the voxels in the order their first point comes in the input
    first = {}
    for i, k in enumerate(map(tuple, build_ref.voxel_keys(pts[:5000], vs).tolist())):
        first.setdefault(k, i)
    assert [tuple(k) for k in mk[:len(first)].tolist()] == sorted(first, key=first.get)  # (the voxels the first 5 000 points open)


def test_the_mirror_on_cases_worked_out_by_hand():
    """voxel 1, cap 4: map_resolution = 0.5 exactly"""
    assert build_ref.resolution(1.0, 4) == 0.5
    kept = lambda name: build_ref.build(*build_cases.case(name))[0].tolist()
    A, B, C_ = [0.125, 0.25, 0.25], [0.5, 0.25, 0.25], [0.75, 0.25, 0.25]
    assert kept("exactly_res_apart") == [[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]]  # `<` is strict
    assert kept("one_ulp_closer") == [[0.25, 0.25, 0.25]]
    assert kept("chain_abc") == [A, C_] and kept("chain_cba") == [C_, A] and kept("chain_bac") == [B]
    assert kept("duplicates") == [[0.25, 0.5, 0.75], [0.75, 0.5, 0.25]]
    # truncation: +-0.5, +-0.999 and -0.0 share voxel 0; a point on a face belongs to the voxel away from zero
    keys = build_ref.voxel_keys(np.array([[0.5, -0.5, 0.999], [-0.999, -0.0, 0.0], [1.0, -1.0, 2.0], [-2.0, 1.5, -1.5]], np.float32), 1.0)
    assert keys.tolist() == [[0, 0, 0], [0, 0, 0], [1, -1, 2], [-2, 1, -1]]
    for cap in build_cases.ONE_VOXEL_CAPS:
        p, k, c = build_ref.build(*build_cases.case("one_voxel_cap%d" % cap))
        assert k.tolist() == [[0, 0, 0]] and c.tolist() == [cap]  # 5 000 points in one voxel reach every one of these caps
    p, k, c = build_ref.build(*build_cases.case("dense3"))
    assert (c == 30).all()
    p, k, c = build_ref.build(*build_cases.case("spacing8"))
    print("spacing8:", len(p), "kept in", len(k), "voxels,", int((c == 30).sum()), "at the cap")
    assert len(p) < 20000 and (c == 30).mean() < 0.01  # almost purely the spacing rule
    assert build_ref.build(*build_cases.case("own_voxel_4097"))[2].tolist() == [1] * 4097
    assert build_ref.build(*build_cases.case("pairs_512"))[2].tolist() == [2] * 512


# ---------------------------------------------------------------- the two facts
@pytest.mark.parametrize("name,vs,cap", [("dense3", 1.0, 30), ("spacing8", 1.0, 30), ("keys_vs03", 0.3, 30), ("one_voxel_cap100", 1.0, 100)])
def test_stored_points_survive_their_own_replay(oracle, name, vs, cap):
    """the stored points in bucket order, fed to AddPoints again: every one is kept, in the same order; and so is any subset"""
    stored = build_ref.build(build_cases.case(name)[0], vs, cap)
    again = build_ref.build(stored[0], vs, cap)
    _same(again, stored)
    _same(_oracle_map(oracle, [stored[0].astype(np.float32)], vs, cap), build_ref.canonical(*stored))
    drop = np.random.default_rng(21).random(len(stored[0])) < 0.3
    rest = stored[0][~drop]
    sub = build_ref.build(rest, vs, cap)
    assert np.array_equal(sub[0], rest) and sub[2].sum() == (~drop).sum()
    _same(_oracle_map(oracle, [rest.astype(np.float32)], vs, cap), build_ref.canonical(*sub))
    # kept points of a voxel are pairwise at least map_resolution apart
    res = build_ref.resolution(vs, cap)
    start = np.concatenate([[0], np.cumsum(stored[2])])
    for v in range(min(len(stored[2]), 50)):
        P = stored[0][start[v]:start[v + 1]]
        d = P[:, None, :] - P[None, :, :]
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        assert (dist[~np.eye(len(P), dtype=bool)] >= res).all()


@pytest.mark.parametrize("vs,cap", [(1.0, 30), (0.5, 30), (1.0, 4)])
def test_an_incremental_add_equals_one_build(oracle, vs, cap):
    """AddPoints(A); AddPoints(B) == AddPoints(stored(A) ++ B), per voxel and in order -- and with the voxel ids of the mirror, whose
    bucket order is first-seen order"""
    a, b = build_cases.dense3(), build_cases.extra5000()
    stored = build_ref.build(a, vs, cap)
    one = build_ref.build(np.concatenate([stored[0].astype(np.float32), b]), vs, cap)
    both = build_ref.build(np.concatenate([a, b]), vs, cap)  # the mirror's "two adds": one pass over A ++ B is the reference's two calls
    _same(one, both)
    assert np.array_equal(one[1][:len(stored[1])], stored[1])  # A's voxels keep their ids
    two_calls = _oracle_map(oracle, [a, b], vs, cap)
    _same(two_calls, build_ref.canonical(*one))
    _same(two_calls, _oracle_map(oracle, [stored[0].astype(np.float32), b], vs, cap))


# ---------------------------------------------------------------- header, arguments, shim
def test_the_symbols_are_in_the_header(L):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+elm_map_build_device\s*\(\s*elm_ctx\*\s*ctx,\s*const elm_map\*\s*base,\s*const uint8_t\*\s*drop,\s*const float\*\s*xyz,"
                     r"\s*size_t n,\s*double voxel_size,\s*int max_points_per_voxel,\s*elm_map\*\*\s*out\)", src)
    assert hasattr(L, "elm_map_build_device") and hasattr(L, "elm_map_build_device_stages")


def test_argument_errors_without_a_device(L):
    out = C.c_void_p(1)
    xyz = np.zeros((4, 3), np.float32)
    fp = xyz.ctypes.data_as(C.POINTER(C.c_float))
    assert L.elm_map_build_device(None, None, None, fp, 4, 1.0, 30, C.byref(out)) == INVALID
    assert out.value is None  # *out is NULL after a refusal
    one = C.c_void_p(1)  # never dereferenced: out is checked first
    assert L.elm_map_build_device(one, None, None, fp, 4, 1.0, 30, None) == INVALID
    ms = (C.c_double * 7)()
    assert L.elm_map_build_device_stages(None, ms) == INVALID


def test_shim_build_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/build_calls.cpp, built as tests/test_growth_objects_abi.py builds objects_calls.cpp"""
    exe = tmp_path / "build_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "build_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
