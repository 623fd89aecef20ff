"""The constructed inputs of tests/scan_cases.py keep their promises, and the oracle's deskew and downsample agree with the two numpy
mirrors written from the reference's statements.  No GPU: tests/test_scan_kernels.py runs the same cases against the kernels."""
import numpy as np
import pytest

import scan_cases as S

DESKEW = S.deskew_cases()
DOWNSAMPLE = S.downsample_cases()

# the largest |oracle - mirror| over every finite output of every deskew case, measured on the CPU (x86-64, glibc sinf / cosf against
# numpy's float64 sin / cos rounded once): one float32 ulp of a coordinate between 64 m and 128 m, in the large-rotation case; every
# other case agrees bit for bit
MEASURED_MIRROR_DIFF = 7.62939453125e-06
MIRROR_TOL = 2.0 * MEASURED_MIRROR_DIFF


def _oracle_deskew(oracle, c):
    return oracle.deskew_points(c["xyz"], c["rel"], c["imu_time"], c["imu_rot"], c["scan_cur"], c["scan_end"], c["incre"])


# ---- stated properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", S.EPOCHS)
@pytest.mark.parametrize("n", S.DESKEW_SIZES)
def test_exact_row_table_is_what_it_says(n, epoch):
    c = S.deskew_exact_rows(n, epoch)
    t, st = c["imu_time"], c["stats"]
    assert len(t) == 12 and c["xyz"].shape == (n, 3) and c["rel"].shape == (n,) and c["rel"].dtype == np.float32
    assert (np.diff(t) == 0).sum() == 1 and np.all(np.diff(t) >= 0)                     # one repeated row time
    assert np.allclose(np.diff(t)[np.diff(t) > 0], 0.005, rtol=0, atol=1e-6)           # 5 ms spacing (up to the rounding that makes the rows exact)
    pt = np.float64(c["scan_cur"]) + c["rel"].astype(np.float64)
    if n >= 255:
        assert st["before"] >= 50 and st["after"] >= 50 and st["inside"] >= 100
        assert st["rows_hit"] == 12 and all((pt == x).any() for x in t)                 # a point EXACTLY on every row time
        assert c["rel"].min() == 0.0
    else:
        assert st["on_row"] == n
    assert pt.min() >= c["scan_cur"] and pt.max() <= c["scan_end"]


@pytest.mark.parametrize("epoch", S.EPOCHS)
def test_short_tables_are_what_they_say(epoch):
    one, two = S.deskew_short_table(1, 257, epoch), S.deskew_short_table(2, 257, epoch)
    assert len(one["imu_time"]) == 1 and one["stats"]["before"] > 20 and one["stats"]["after"] > 20 and one["stats"]["on_row"] == 1
    assert len(two["imu_time"]) == 2 and min(two["stats"][k] for k in ("before", "after", "inside")) > 20 and two["stats"]["rows_hit"] == 2
    # a one-row table: every point takes row 0, all three rotation arguments are exactly zero
    assert not S.np_deskew_angles(one["rel"], one["imu_time"], one["imu_rot"], one["scan_cur"])[0].any()
    # at the epoch stamp the point times still resolve (2.4e-7 s per step of a double): many distinct ones, not one lump
    assert len(np.unique(np.float64(two["scan_cur"]) + two["rel"].astype(np.float64))) > 200


@pytest.mark.parametrize("epoch", S.EPOCHS)
def test_large_rotation_case_populates_every_class(epoch):
    c = S.deskew_large_rotations(4099, epoch)
    cls = c["stats"]["classes"]
    assert cls["beyond"] == 0                                                           # nothing at or beyond 120: see the constructor
    for ax in range(3):
        for sg in "+-":
            for k in S.ANGLE_CLASSES:
                assert cls[(ax, sg, k)] >= 20, (ax, sg, k, cls[(ax, sg, k)])
    assert c["stats"]["rows_hit"] == len(c["imu_time"]) and c["stats"]["inside"] > 1000


def test_translation_and_non_finite_cases_are_what_they_say():
    for kind in S.TRANSLATION_KINDS:
        c = S.deskew_translation(kind)
        assert c["stats"]["rel_zero"] >= 1 and (c["rel"] > 0).sum() > 200
        if kind.startswith("large"):
            assert abs(c["incre"][0]) == 50.0 and abs(c["incre"][1]) == 50.0 and c["incre"][0] == -c["incre"][1]
        if kind == "zero":
            assert not c["incre"].any()
        assert (c["scan_end"] == c["scan_cur"]) == kind.startswith("end_is_cur")
    c = S.deskew_non_finite()
    bad = c["stats"]["bad"]
    assert np.isnan(c["rel"]).sum() == c["stats"]["nan_time"] >= 3 and (~np.isfinite(c["xyz"])).any(axis=1).sum() == c["stats"]["bad_xyz"] >= 6
    assert np.isnan(c["xyz"]).any() and np.isposinf(c["xyz"]).any() and np.isneginf(c["xyz"]).any()
    waves = {i // 64 for i in bad}
    assert waves == set(range((len(c["rel"]) + 63) // 64))                              # every wave has poisoned lanes AND clean neighbours
    assert {63, 64, 127, 128, 255, 256} <= set(bad)


def test_downsample_sizes_straddle_wave_block_and_chunk():
    assert {63, 64, 65} <= set(S.DS_SIZES) and {1023, 1024, 1025} <= set(S.DS_SIZES) and 1 in S.DS_SIZES and 4097 in S.DS_SIZES
    blocks = [(n + 1023) // 1024 for n in S.DS_LARGE_SIZES]
    assert blocks == [1025, 2049] and [(b + 1023) // 1024 for b in blocks] == [2, 3]     # chunks of the offsets scan


def test_occupancy_cases_are_what_they_say():
    for vs in S.DS_VOXEL_SIZES:
        assert np.array_equal(S.np_first_per_voxel(S.ds_one_voxel()["xyz"], vs), [0])
        c = S.ds_identity()
        assert np.array_equal(S.np_first_per_voxel(c["xyz"], vs), np.arange(len(c["xyz"])))
        c = S.ds_boundary_firsts()
        assert tuple(S.np_first_per_voxel(c["xyz"], vs)) == c["stats"]["expect"] == (0,) + S.BOUNDARY_FIRSTS
    c = S.ds_duplicates()
    pick = c["stats"]["picks"]
    first_seen = np.sort(np.unique(pick, return_index=True)[1])
    assert len(first_seen) < len(pick) / 3                                             # every point several times
    kept = S.np_first_per_voxel(c["xyz"], 0.2)
    assert np.all(np.isin(kept, first_seen))                                           # only first occurrences are ever kept


@pytest.mark.parametrize("vs", (0.5, 1.5, 0.2))
def test_face_case_has_exact_faces_both_signs_and_negative_zero(vs):
    f = S.exact_face_values(vs)
    q = f.astype(np.float64) / np.float64(vs)
    assert f.dtype == np.float32 and len(f) >= 24 and np.all(q == np.floor(q)) and np.all(f > 0)
    st = S.ds_faces(vs)["stats"]
    assert st["on_face"] >= 500 and st["neg_on_face"] >= 200 and st["neg_zero"] >= 10
    # one ulp below a face is the voxel below, on the face and one ulp above are the voxel above -- on both sides of the origin
    for s in (1.0, -1.0):
        v = np.float32(s) * f
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        k = lambda a: S.voxel_coords(np.stack([a, a, a], 1), vs)[:, 0]
        assert np.array_equal(k(lo) + 1, k(v)) and np.array_equal(k(hi), k(v))


@pytest.mark.parametrize("vs", S.DS_VOXEL_SIZES)
def test_pack_edge_values_sit_at_the_ends_of_the_packable_range(vs):
    v = S.pack_edge_values(vs)
    q = v.astype(np.float64) / np.float64(vs)
    assert np.all(np.abs(q) < S.PACK_LIM)
    assert np.floor(q[0]) == S.PACK_LIM - 1 and np.floor(q[1]) in (S.PACK_LIM - 1, S.PACK_LIM - 2)
    assert np.floor(q[2]) == -S.PACK_LIM and abs(q[2] - (-S.PACK_LIM + 0.5)) < 0.1 and np.floor(q[3]) == -S.PACK_LIM
    assert np.float64(np.nextafter(v[0], np.float32(np.inf))) / vs >= S.PACK_LIM      # the very last packable float32 ...
    assert np.float64(np.nextafter(v[3], np.float32(-np.inf))) / vs <= -S.PACK_LIM    # ... at either end
    c = S.ds_pack_edges(vs)
    assert c["vs"] == (vs,) and c["stats"]["max_abs_q"] < S.PACK_LIM and c["stats"]["extreme"] >= 30
    for kind in S.UNPACKABLE_KINDS:
        u = S.ds_unpackable(kind, vs)
        qq = u["xyz"].astype(np.float64) / vs
        assert (~((qq > -S.PACK_LIM) & (qq < S.PACK_LIM))).sum() == 1                   # exactly one coordinate does not pack
    hi, lo = S.ds_unpackable("plus_2^20", vs)["stats"]["quotient"], S.ds_unpackable("minus_2^20", vs)["stats"]["quotient"]
    if vs in (1.5, 0.5):  # 2^20 voxel sizes is a float32 there: the quotient is 2^20 EXACTLY (no float32 has that quotient at 0.2)
        assert hi == S.PACK_LIM and lo == -S.PACK_LIM
    assert S.PACK_LIM <= hi < S.PACK_LIM + 0.1 and -S.PACK_LIM - 0.1 < lo <= -S.PACK_LIM


def test_adversarial_case_collides_in_the_last_eight_slots():
    """If the product's hash or packing ever changes, THIS is the assertion that says the adversarial case needs new keys (the GPU
    comparison of test_scan_kernels.py stays valid regardless)."""
    c = S.ds_adversarial()
    st = c["stats"]
    assert len(c["xyz"]) == 4096 and S.table_cap_log2(4096) == st["cap_log2"] == 13
    assert st["last8_voxels"] >= 512 and st["last8_repeated_voxels"] >= 512
    assert min(st["last8_per_slot"]) > 0 and sum(st["last8_per_slot"]) == st["last8_points"] >= 1024
    assert st["last8_index_span"][0] < 64 and st["last8_index_span"][1] > 4096 - 64     # spread over the whole input
    # 640 voxels whose home is within eight slots of the end: the chain they form is longer than what is left of the table, it wraps
    assert st["last8_voxels"] > 8


def test_clean_sequence_changes_capacity_as_stated():
    seq = S.ds_clean_sequence()
    caps = [S.table_cap_log2(len(c["xyz"])) for c in seq]
    assert caps == [14, 14, 15, 14, 18, 14, 14, 14, 14]
    assert [len(c["xyz"]) for c in seq] == [5000, 6000, 9000, 5000, 70000, 5000, 5000, 5000, 6000]
    assert ["bad_index" in c["stats"] for c in seq] == [False] * 6 + [True] + [False] * 2
    vox = [set(map(tuple, S.voxel_coords(c["xyz"][np.isfinite(c["xyz"]).all(axis=1)], 0.5))) for c in seq]
    for a, b, c in zip(vox, vox[1:], seq[1:]):
        assert len(a & b) > 1000 and len(a ^ b) > 500                                   # many voxels in common, and not the same cloud
    assert len({c["xyz"].tobytes() for c in seq}) == len(seq)


# ---- the mirrors against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,make", DOWNSAMPLE, ids=[c[0] for c in DOWNSAMPLE])
def test_downsample_mirror_equals_oracle(oracle, cid, make):
    c = make()
    for vs in c["vs"]:
        assert np.array_equal(S.np_first_per_voxel(c["xyz"], vs), np.sort(oracle.voxel_downsample(c["xyz"], vs))), (cid, vs)


def test_downsample_mirror_equals_oracle_clean_sequence_and_large(oracle):
    clouds = [c for c in S.ds_clean_sequence() if "bad_index" not in c["stats"]] + [S.ds_large(S.DS_LARGE_SIZES[0])]
    for c in clouds:
        for vs in c["vs"]:
            ref = np.sort(oracle.voxel_downsample(c["xyz"], vs))
            assert np.array_equal(S.np_first_per_voxel(c["xyz"], vs), ref), (len(c["xyz"]), vs)
    big = S.ds_large(S.DS_LARGE_SIZES[0])
    assert 20_000 < len(S.np_first_per_voxel(big["xyz"], 1.5)) < 100_000                # tens of thousands of 1.5 m voxels
    assert len(S.np_first_per_voxel(big["xyz"], 0.2)) > 0.9 * len(big["xyz"])           # most points kept at 0.2 m


def test_deskew_mirror_agrees_with_oracle(oracle):
    """oracle.deskew_points against np_deskew on every deskew case.

    Measured on the CPU: the largest absolute difference over all finite outputs of all cases is 7.62939453125e-06 m (one float32 ulp
    of a coordinate between 64 m and 128 m), reached in the large-rotation case; every other case agrees bit for bit.  The bound is
    twice that, 1.52587890625e-05 m: the only legitimate difference is the last-bit rounding of sinf / cosf against float64 sin / cos,
    carried through nine products with coordinates up to 80 m.  Non-finite outputs must be non-finite on both sides, in the same places
    and of the same kind (NaN, +inf, -inf)."""
    worst = 0.0
    for cid, make in DESKEW:
        c = make()
        a = _oracle_deskew(oracle, c)
        b = S.np_deskew(c["xyz"], c["rel"], c["imu_time"], c["imu_rot"], c["scan_cur"], c["scan_end"], c["incre"])
        assert a.shape == b.shape == c["xyz"].shape
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), cid
        fin = np.isfinite(a)
        d = float(np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64)).max()) if fin.any() else 0.0
        print(f"{cid}: max |oracle - mirror| = {d:.6g} m over {int(fin.sum())} finite outputs")
        worst = max(worst, d)
        assert d <= MIRROR_TOL, (cid, d)
    print(f"worst: {worst!r}")
    assert worst > 0.0  # the mirror is NOT the oracle's own arithmetic: somewhere sinf differs from the rounded float64 sine
