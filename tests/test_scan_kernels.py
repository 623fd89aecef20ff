"""The scan-side kernels at their edges, through the C ABI: k_deskew (elm_deskew) bit for bit against the oracle, and the device
VoxelDownsample (k_ds_insert / count / offsets / scatter / clear behind elm_deskew_downsample, b_run_deskew = 0 so that the kernels see the
caller's points as they are) ROW FOR ROW, IN INPUT ORDER, against xyz[sort(oracle.voxel_downsample)].

The inputs are the constructed cases of tests/scan_cases.py; tests/test_scan_cases.py (no GPU) asserts what each of them promises and
checks the oracle against two independent numpy mirrors on all of them.  Rotation arguments stay below 120: beyond it the device takes the
float64 library function, which is last-bit accurate only, and csrc/elm_la.hpp states that a deskew rotation never gets there.
"""
import ctypes as C

import numpy as np
import pytest

import scan_cases as S

pytestmark = pytest.mark.gpu

ELM_OK, ELM_ERR_UNSUPPORTED = 0, -5
UNPACKABLE_TEXT = "a voxel key does not fit the packed device table (|coordinate / voxel size| >= 2^20)"
SENTINEL = np.float32(-12345.678)
DESKEW = S.deskew_cases()
DOWNSAMPLE = S.downsample_cases()
FP = C.POINTER(C.c_float)
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    from elimaloc_amd.registration import Context
    c = Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- deskew ------------------------------------------------------------------------------------------------------------------------
def _tables(c, run=1, imu=1, odom=1):
    """A hand-built elm_deskew_tables over the case's own rows (the arrays are returned too: they must outlive the call)."""
    from elimaloc_amd import _lib
    t = np.ascontiguousarray(c["imu_time"], np.float64)
    r = [np.ascontiguousarray(c["imu_rot"][:, k], np.float64) for k in range(3)]
    tab = _lib.DeskewTables()
    tab.d_time_scan_cur, tab.d_time_scan_end = c["scan_cur"], c["scan_end"]
    tab.i_imu_pointer_cur = len(t) - 1
    tab.b_run_deskew, tab.b_is_imu_available, tab.b_is_odom_available = run, imu, odom
    tab.f_odom_incre_x, tab.f_odom_incre_y, tab.f_odom_incre_z = (float(v) for v in c["incre"])
    tab.vec_d_imu_time = t.ctypes.data_as(DP)
    tab.vec_d_imu_rot_x, tab.vec_d_imu_rot_y, tab.vec_d_imu_rot_z = (a.ctypes.data_as(DP) for a in r)
    return tab, (t, r)


def _deskew(ctx, c, **switches):
    """elm_deskew into a buffer filled with a sentinel -> (ok, the buffer)."""
    from elimaloc_amd import _lib
    tab, keep = _tables(c, **switches)
    out = np.full_like(c["xyz"], SENTINEL)
    ok = C.c_int(-1)
    rc = _lib.lib().elm_deskew(ctx._h, c["xyz"].ctypes.data_as(FP), c["rel"].ctypes.data_as(FP), len(c["rel"]), C.byref(tab), out.ctypes.data_as(FP),
                               C.byref(ok))
    _lib.check(rc, ctx._h, "elm_deskew")
    del keep
    return ok.value, out


def _oracle_deskew(oracle, c):
    return oracle.deskew_points(c["xyz"], c["rel"], c["imu_time"], c["imu_rot"], c["scan_cur"], c["scan_end"], c["incre"])


def _assert_same(got, ref, c, what):
    """np.array_equal where the oracle's outputs are all finite, the 32-bit patterns where NaNs occur."""
    if np.isfinite(ref).all():
        same, bad = np.array_equal(got, ref), np.flatnonzero((got != ref).any(axis=1))
    else:
        same, bad = np.array_equal(_bits(got), _bits(ref)), np.flatnonzero((_bits(got) != _bits(ref)).any(axis=1))
    if not same:
        i = int(bad[0])
        ang, _, branch, front = S.np_deskew_angles(c["rel"], c["imu_time"], c["imu_rot"], c["scan_cur"])
        print(f"{what}: {len(bad)} of {len(ref)} points differ, at {bad[:16].tolist()}; first {i} (thread {i % 256} of block {i // 256}, lane {i % 64}): "
              f"point {c['xyz'][i]}, rel {c['rel'][i]!r}, front row {int(front[i])}, branch {int(branch[i])}, (roll, pitch, yaw) {ang[i]}, "
              f"device {got[i]} {[hex(v) for v in _bits(got)[i]]}, oracle {ref[i]} {[hex(v) for v in _bits(ref)[i]]}")
    assert same, f"{what}: {len(bad)} of {len(ref)} deskewed points differ from the oracle's, first at {int(bad[0])}"


@pytest.mark.parametrize("cid,make", DESKEW, ids=[c[0] for c in DESKEW])
def test_deskew_equals_oracle_bit_for_bit(ctx, oracle, cid, make):
    """Every exit of FindRotation (before the first row, after the last, exactly on a row, a repeated row time, one- and two-row tables),
    small and Unix-epoch stamps, every branch of the device's sinf / cosf below 120, the translation path with its division by zero, and
    non-finite inputs: the same 32 bits as the oracle in every output, NaNs included, twice."""
    c = make()
    ref = _oracle_deskew(oracle, c)
    ok, got = _deskew(ctx, c)
    assert ok == 1
    _assert_same(got, ref, c, cid)
    ok2, again = _deskew(ctx, c)
    assert ok2 == 1 and np.array_equal(_bits(again), _bits(got))


def test_deskew_non_finite_points_leave_their_wave_alone(ctx):
    """The points around a NaN / inf point or a NaN time come out exactly as they do in the same scan without the poison."""
    bad = S.deskew_non_finite()
    clean = S.deskew_exact_rows(len(bad["rel"]), 100.0, seed=50)
    others = np.setdiff1d(np.arange(len(bad["rel"])), bad["stats"]["bad"])
    assert np.array_equal(bad["xyz"][others], clean["xyz"][others]) and np.array_equal(bad["rel"][others], clean["rel"][others])
    _, a = _deskew(ctx, bad)
    _, b = _deskew(ctx, clean)
    assert np.array_equal(_bits(a)[others], _bits(b)[others]) and np.isfinite(a[others]).all()
    assert not np.isfinite(a[bad["stats"]["bad"]]).all(axis=1).any()


@pytest.mark.parametrize("make", (lambda: S.deskew_exact_rows(257, 100.0), S.deskew_non_finite), ids=("finite", "nonfinite"))
def test_deskew_switch_paths(ctx, make):
    """b_run_deskew = 0 is a plain copy (pcm.cpp:513-525); without the IMU or the odometry table *ok is 0 and the output buffer is not
    written (pcm.cpp:494-496)."""
    c = make()
    ok, out = _deskew(ctx, c, run=0)
    assert ok == 1 and np.array_equal(_bits(out), _bits(c["xyz"]))
    for sw in (dict(imu=0), dict(odom=0), dict(imu=0, odom=0), dict(run=0, imu=0)):
        ok, out = _deskew(ctx, c, **sw)
        assert ok == 0 and np.all(out == SENTINEL), sw


# ---- device downsample -------------------------------------------------------------------------------------------------------------
def _downsample(ctx, xyz, vs):
    """elm_deskew_downsample with b_run_deskew = 0 -> (status, *ok, kept points or None, whether *scan_out was left null)."""
    from elimaloc_amd import _lib
    L = _lib.lib()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    tab, keep = _tables(dict(imu_time=np.zeros(1), imu_rot=np.zeros((1, 3)), scan_cur=0.0, scan_end=0.1, incre=np.zeros(3, np.float32)), run=0)
    rel = np.zeros(max(n, 1), np.float32)
    scan, ok = C.c_void_p(), C.c_int(-1)
    rc = L.elm_deskew_downsample(ctx._h, xyz.ctypes.data_as(FP), rel.ctypes.data_as(FP), n, C.byref(tab), float(vs), C.byref(scan), C.byref(ok))
    del keep
    if rc != ELM_OK or not scan.value:
        return rc, ok.value, None, not scan.value
    k = int(L.elm_scan_size(scan))
    out = np.empty((k, 3), np.float32)
    try:
        _lib.check(L.elm_scan_download(scan, out.ctypes.data_as(FP), k), ctx._h, "elm_scan_download")
    finally:
        L.elm_scan_destroy(scan)
    return rc, ok.value, out, False


def _explain(xyz, vs, kept, ref_idx):
    """The first row where the device's output leaves the reference: its input index, lane, wave and block, and its home slot."""
    ref = xyz[ref_idx]
    m = min(len(kept), len(ref))
    diff = np.flatnonzero((_bits(kept[:m]) != _bits(ref[:m])).any(axis=1))
    row = int(diff[0]) if len(diff) else m
    msg = f"vs {vs}: device kept {len(kept)}, reference {len(ref)}; first differing output row {row}"
    if row < len(ref):
        i = int(ref_idx[row])
        cap = S.table_cap_log2(len(xyz))
        msg += (f": expected input index {i} (block {i // 1024}, wave {(i % 1024) // 64}, lane {i % 64}; chunk {(i // 1024) // 1024} of the offsets scan), "
                f"point {xyz[i]}, home slot {int(S.ds_slot(xyz[i:i + 1], vs, cap)[0])} of 2^{cap}")
        if row < len(kept):
            src = np.flatnonzero((_bits(xyz) == _bits(kept[row])).all(axis=1))
            msg += f"; device wrote {kept[row]}, which is input index {src[:4].tolist()}"
    return msg


def _check_downsample(ctx, oracle, xyz, vs, twice=True):
    ref_idx = np.sort(oracle.voxel_downsample(xyz, vs))
    rc, ok, kept, _ = _downsample(ctx, xyz, vs)
    assert rc == ELM_OK and ok == 1 and kept is not None, (rc, ok)
    same = kept.shape == (len(ref_idx), 3) and np.array_equal(_bits(kept), _bits(xyz[ref_idx]))
    if not same:
        print(_explain(xyz, vs, kept, ref_idx))
    assert len(kept) == len(ref_idx), _explain(xyz, vs, kept, ref_idx)               # the kept count
    assert np.array_equal(kept, xyz[ref_idx]) and same, _explain(xyz, vs, kept, ref_idx)  # row for row, in input order
    if twice:
        rc2, _, again, _ = _downsample(ctx, xyz, vs)
        assert rc2 == ELM_OK and again.tobytes() == kept.tobytes()
    return ref_idx


@pytest.mark.parametrize("cid,make", DOWNSAMPLE, ids=[c[0] for c in DOWNSAMPLE])
def test_downsample_keeps_first_points_in_input_order(ctx, oracle, cid, make):
    """Wave and block boundaries of n, the extremes of occupancy, first points on the last lane of a wave / block and on lane 0 of the
    next, voxel faces with both signs and -0.0f, the ends of the packable range, and probe chains that wrap through the end of the table."""
    c = make()
    for vs in c["vs"]:
        ref_idx = _check_downsample(ctx, oracle, c["xyz"], vs)
        if "expect" in c["stats"]:
            assert tuple(ref_idx) == c["stats"]["expect"]


@pytest.mark.parametrize("n", S.DS_LARGE_SIZES)
def test_downsample_beyond_one_chunk_of_block_offsets(ctx, oracle, n):
    """More than 1024 blocks of 1024 points: the carry of k_ds_offsets over two and three chunks."""
    c = S.ds_large(n)
    for vs in c["vs"]:
        ref_idx = _check_downsample(ctx, oracle, c["xyz"], vs)
        assert len(ref_idx) > (20_000 if vs == 1.5 else 0.9 * n)
        assert ref_idx[-1] >= 1024 * 1024                                             # kept points behind the first chunk


@pytest.mark.parametrize("vs", (1.5, 0.5))
@pytest.mark.parametrize("kind", S.UNPACKABLE_KINDS)
def test_downsample_unpackable_point_is_unsupported(ctx, oracle, kind, vs):
    """One coordinate with |coordinate / voxel size| >= 2^20 (exactly 2^20, beyond, NaN, inf): ELM_ERR_UNSUPPORTED with the stated text,
    *scan_out null -- and the context takes the next cloud as if nothing had happened."""
    from elimaloc_amd import _lib
    c = S.ds_unpackable(kind, vs)
    for _ in range(2):
        rc, ok, kept, null = _downsample(ctx, c["xyz"], vs)
        assert rc == ELM_ERR_UNSUPPORTED and kept is None and null and ok == 1
        assert _lib.lib().elm_last_error(ctx._h).decode() == UNPACKABLE_TEXT
    good = np.delete(c["xyz"], c["stats"]["bad_index"], axis=0)
    _check_downsample(ctx, oracle, good, vs, twice=False)


def test_downsample_table_is_left_clean_across_sizes_and_errors(oracle):
    """A context of its own (the module's has grown its table for two million points by now: nothing would reallocate), nine calls: the same table capacity reused, a larger one, a smaller one inside the larger allocation, a
    reallocation, a call that ends in ELM_ERR_UNSUPPORTED, and good calls behind it.  Consecutive clouds share most of their voxels: a key
    or a first index left behind by any earlier call shows as a missing or an extra point."""
    from elimaloc_amd.registration import Context
    own = Context(0)
    try:
        for j, c in enumerate(S.ds_clean_sequence()):
            vs = c["vs"][0]
            if "bad_index" in c["stats"]:
                rc, _, kept, null = _downsample(own, c["xyz"], vs)
                assert rc == ELM_ERR_UNSUPPORTED and kept is None and null, j
            else:
                _check_downsample(own, oracle, c["xyz"], vs, twice=False)
    finally:
        own.close()
