"""Constructed inputs for the scan-side kernels (tests/test_scan_cases.py on the CPU, tests/test_scan_kernels.py on the GPU): k_deskew and
the k_ds_* family of csrc/elm_k_scan.hip.  Plain numpy, no GPU.

Two things live here:

* two mirrors written from the reference's statements, not from the kernels: `np_deskew` (DeskewPoint / FindRotation / FindPosition,
  pcm_matching.cpp:731-824, with pcl::getTransformation's float32 products) and `np_first_per_voxel` (VoxelDownsample, voxel_hash_map.hpp:
  260-283, with PointToVoxel's float64 quotient and floor).  The oracle is checked against them on every case below, so that the oracle
  and a kernel cannot be wrong in the same way;
* constructors.  Every one returns a dict with the arrays a call needs and, under "stats", the numbers it promises (so many point times
  before the first table row, so many voxels hashing into the last eight slots, ...): tests/test_scan_cases.py asserts those numbers.

A deskew case: xyz (n, 3) float32, rel (n,) float32, imu_time (k,) float64, imu_rot (k, 3) float64, scan_cur, scan_end (float), incre (3,) float32.
A downsample case: xyz (n, 3) float32 and vs, the voxel sizes it runs at.
"""
import numpy as np

F32, F64 = np.float32, np.float64
DS_VOXEL_SIZES = (1.5, 0.2, 0.5)
DESKEW_SIZES = (1, 255, 256, 257, 4099)
DS_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
DS_LARGE_SIZES = (1_048_577, 2_097_157)  # 1025 and 2049 blocks of 1024 points: two and three 1024-block chunks of the offsets scan
EPOCHS = (100.0, 1.7e9)                  # a small stamp; a Unix-epoch stamp (a double resolves 2.4e-7 s there)
PACK_LIM = 1 << 20                       # the device packs three 21-bit voxel coordinates: |coordinate / voxel size| < 2^20
HASH_MUL = 0x9E3779B97F4A7C15            # restated from k_ds_insert / elm_glue.cpp ONLY to choose the adversarial input
TINY, QUARTER_PI = 2.0 ** -12, float(F32(np.pi / 4))
ANGLE_CLASSES = ("tiny", "small", "q0", "q1", "q2", "q3")


# ---------------------------------------------------------------------------------------------------------------------------------
# mirrors
# ---------------------------------------------------------------------------------------------------------------------------------
def np_deskew_angles(rel, imu_time, imu_rot, scan_cur):
    """FindRotation (pcm.cpp:731-762) for every point and the differences DeskewPoint feeds to pcl::getTransformation:
    (roll, pitch, yaw) float32 (n, 3), the float32 rotation at the point time (n, 3), and the branch taken per point
    (0 = the row `front` as it is, 1 = interpolated) with `front`."""
    imu_time = np.asarray(imu_time, F64)
    imu_rot = np.asarray(imu_rot, F64).reshape(-1, 3)
    cur = len(imu_time) - 1
    pt = F64(scan_cur) + np.asarray(rel, F32).astype(F64)                    # pcm.cpp:783, double
    lt = pt[:, None] < imu_time[None, :cur]                                   # the while loop: the first row the point is before
    front = np.where(lt.any(axis=1), lt.argmax(axis=1), cur) if cur > 0 else np.zeros(len(pt), np.int64)
    direct = (pt > imu_time[front]) | (front == 0)
    back = np.maximum(front - 1, 0)
    with np.errstate(all="ignore"):
        tf, tb = imu_time[front], imu_time[back]
        rf = (pt - tb) / (tf - tb)
        rb = (tf - pt) / (tf - tb)
        inter = imu_rot[front] * rf[:, None] + imu_rot[back] * rb[:, None]    # double, then the store into float* rounds once
    rot = np.where(direct[:, None], imu_rot[front], inter).astype(F32)
    end = imu_rot[cur].astype(F32)                                            # pcm.cpp:786-788: float
    with np.errstate(all="ignore"):
        ang = rot - end[None, :]                                              # float32 - float32
    return ang, rot, np.where(direct, 0, 1), front


def np_deskew(xyz, rel, imu_time, imu_rot, scan_cur, scan_end, incre, odom_available=True):
    """DeskewPoint (pcm.cpp:780-824) for every point: float32 where the reference has float, float64 where it has double, sin / cos from
    numpy's float64 functions rounded once to float32 (NOT bit-exact against sinf / cosf: last-bit differences are expected)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    rel = np.asarray(rel, F32)
    incre = np.asarray(incre, F32)
    ang, rot, _, _ = np_deskew_angles(rel, imu_time, imu_rot, scan_cur)
    with np.errstate(all="ignore"):
        px = py = np.zeros(len(rel), F32)
        if odom_available:                                                    # FindPosition (pcm.cpp:764-778)
            ratio = (rel.astype(F64) / (F64(scan_end) - F64(scan_cur))).astype(F32)
            px, py = ratio * incre[0], ratio * incre[1]
        tx, ty = px - incre[0], py - incre[1]
        tz = rot[:, 2] - incre[2]                                             # pcm.cpp:804: the rotation about z, not a position
        sc = lambda a, f: f(a.astype(F64)).astype(F32)
        roll, pitch, yaw = ang[:, 0], ang[:, 1], ang[:, 2]
        A, B, Cc, D, E, F = sc(yaw, np.cos), sc(yaw, np.sin), sc(pitch, np.cos), sc(pitch, np.sin), sc(roll, np.cos), sc(roll, np.sin)
        DE, DF = D * E, D * F                                                 # pcl::getTransformation, Scalar = float
        t00, t01, t02 = A * Cc, A * DF - B * E, B * F + A * DE
        t10, t11, t12 = B * Cc, A * E + B * DF, B * DE - A * F
        t20, t21, t22 = -D, Cc * F, Cc * E
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        out = np.stack([t00 * x + t01 * y + t02 * z + tx, t10 * x + t11 * y + t12 * z + ty, t20 * x + t21 * y + t22 * z + tz], axis=1)
    assert out.dtype == F32
    return out


def voxel_coords(xyz, vs):
    """PointToVoxel (vhm.hpp:176-180) of finite points: floor of the float64 quotient, int64 (n, 3)."""
    q = np.asarray(xyz, F32).reshape(-1, 3).astype(F64) / F64(vs)
    return np.floor(q).astype(np.int64)


def np_first_per_voxel(xyz, vs):
    """VoxelDownsample (vhm.hpp:260-283): the ascending indices of the first point of every floor-keyed voxel.  Finite points only."""
    k = voxel_coords(xyz, vs)
    if len(k) == 0:
        return np.zeros(0, np.int64)
    k = k - k.min(axis=0)
    ext = [int(e) for e in k.max(axis=0) + 1]
    if ext[0] * ext[1] * ext[2] < 2 ** 62:  # one integer per voxel
        lin = (k[:, 0] * ext[1] + k[:, 1]) * ext[2] + k[:, 2]
        _, first = np.unique(lin, return_index=True)
    else:
        _, first = np.unique(k, axis=0, return_index=True)
    return np.sort(first).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# deskew cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _points(rng, n, half=80.0):
    """Sensor-frame points with coordinates up to `half` metres (z within a tenth of that)."""
    p = rng.uniform(-half, half, size=(n, 3))
    p[:, 2] *= 0.1
    return p.astype(F32)


def _case(xyz, rel, imu_time, imu_rot, scan_cur, scan_end, incre, **stats):
    return dict(xyz=np.ascontiguousarray(xyz, F32), rel=np.ascontiguousarray(rel, F32), imu_time=np.ascontiguousarray(imu_time, F64),
                imu_rot=np.ascontiguousarray(imu_rot, F64), scan_cur=float(scan_cur), scan_end=float(scan_end),
                incre=np.asarray(incre, F32), stats=stats)


def _time_stats(case):
    pt = F64(case["scan_cur"]) + case["rel"].astype(F64)
    t = case["imu_time"]
    return dict(before=int((pt < t[0]).sum()), after=int((pt > t[-1]).sum()), on_row=int(np.isin(pt, t).sum()),
                rows_hit=int(np.isin(t, pt).sum()), inside=int(((pt > t[0]) & (pt < t[-1]) & ~np.isin(pt, t)).sum()))


def deskew_exact_rows(n, epoch, seed=0, incre=(0.5, -0.2, 0.01)):
    """A 12-row table at 5 ms spacing with ONE REPEATED row time (rows 5 and 6) under a scan of 0.1 s that is wider than the table: point
    times before row 0, after the last row, exactly on every row time, and inside.  The row times are DEFINED as
    fl(scan_cur + (double)rel_j) for float32 rel_j, so that a point with that rel_j meets its row exactly (asserted below), at a small stamp
    as at a Unix-epoch one."""
    rng = np.random.default_rng(7100 + seed + n)
    scan_cur = F64(epoch) + F64(0.0123)
    step = np.array([0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 10], F64)
    rel_rows = (0.02 + 0.005 * step).astype(F32)
    imu_time = scan_cur + rel_rows.astype(F64)
    assert np.all(np.diff(imu_time)[np.diff(step) > 0] > 0) and imu_time[5] == imu_time[6]
    imu_rot = np.cumsum(rng.normal(0.0, 0.004, size=(12, 3)), axis=0)
    imu_rot[0] = 0.0
    n_row = min(12, n)
    n_out = min(60, (n - n_row) // 3)
    n_in = n - n_row - 2 * n_out
    before = rng.uniform(0.0, float(rel_rows[0]) - 1e-4, n_out).astype(F32)
    before[:1] = 0.0  # the scan's first point: the time every other one is relative to
    rel = np.concatenate([rel_rows[rng.permutation(12)[:n_row]] if n_row < 12 else rel_rows, before,
                          rng.uniform(float(rel_rows[-1]) + 1e-4, 0.1, n_out).astype(F32),
                          rng.uniform(float(rel_rows[0]) + 1e-4, float(rel_rows[-1]) - 1e-4, n_in).astype(F32)])
    rel = rel[rng.permutation(n)]
    c = _case(_points(rng, n), rel, imu_time, imu_rot, scan_cur, scan_cur + 0.1, incre)
    c["stats"] = _time_stats(c)
    pt = scan_cur + rel.astype(F64)
    assert c["stats"]["on_row"] >= n_row
    if n >= 255:
        assert all((pt == t).any() for t in imu_time), "a row time without its point"
    return c


def deskew_short_table(rows, n, epoch, seed=0):
    """A one-row table (i_imu_pointer_cur = 0: every point takes row 0) or a two-row one (before / between / after / on a row)."""
    rng = np.random.default_rng(7200 + seed + 10 * rows + n)
    scan_cur = F64(epoch) + F64(0.5)
    rel_rows = np.array([0.03, 0.06][:rows], F32)
    imu_time = scan_cur + rel_rows.astype(F64)
    imu_rot = np.array([[0.011, -0.007, 0.02], [0.03, 0.004, -0.05]][:rows], F64)
    rel = rng.uniform(0.0, 0.1, n).astype(F32)
    rel[: min(rows, n)] = rel_rows[: min(rows, n)]
    rel = rel[rng.permutation(n)]
    c = _case(_points(rng, n), rel, imu_time, imu_rot, scan_cur, scan_cur + 0.1, (0.3, 0.1, -0.02))
    c["stats"] = _time_stats(c)
    return c


def angle_class_counts(ang):
    """How many of the float32 rotation arguments fall in every (axis, sign, class): |y| < 2^-12 (sinf returns y, cosf 1), the plain
    polynomial below pi / 4, and the range reduction below 120 by quadrant n & 3, n = round(y / (pi / 2))."""
    out = {}
    a = np.abs(ang.astype(F64))
    n = np.rint(ang.astype(F64) / (np.pi / 2)).astype(np.int64)
    for ax in range(3):
        for sg, sel in (("+", ang[:, ax] > 0), ("-", ang[:, ax] < 0)):
            v = a[:, ax]
            out[(ax, sg, "tiny")] = int((sel & (v < TINY)).sum())
            out[(ax, sg, "small")] = int((sel & (v >= TINY) & (v < QUARTER_PI)).sum())
            for q in range(4):
                out[(ax, sg, f"q{q}")] = int((sel & (v >= QUARTER_PI) & (v < 120.0) & ((n[:, ax] & 3) == q)).sum())
    out["beyond"] = int((a >= 120.0).sum())
    return out


def deskew_large_rotations(n=4099, epoch=100.0, seed=0):
    """Table rotations drawn so that roll, pitch and yaw -- the arguments of sinf / cosf -- cover, on every axis and with both signs,
    |y| < 2^-12, 2^-12 <= |y| < pi / 4 and pi / 4 <= |y| < 120 with every quadrant of the range reduction.  The last row's rotation is
    exactly representable in float32, so a row's difference is what was drawn up to one rounding.  Two of three points sit on a row time
    (they take that row's value through the interpolation branch with ratios 0 and 1), the rest interpolate between neighbouring rows: a
    convex combination, so nothing reaches 120.  (Beyond 120 the device takes the float64 library function, which is last-bit accurate
    only; elm_la.hpp states that a deskew rotation never gets there, and this case leaves it out.)"""
    rng = np.random.default_rng(7300 + seed)
    rows = 96
    scan_cur = F64(epoch) + F64(0.25)
    rel_rows = (0.001 * np.arange(1, rows + 1)).astype(F32)
    imu_time = scan_cur + rel_rows.astype(F64)
    assert np.all(np.diff(imu_time) > 0)
    end = np.array([0.25, -0.5, 1.0])
    cls = rng.integers(0, 3, size=(rows, 3))
    mag = np.where(cls == 0, 10.0 ** rng.uniform(-7.0, np.log10(TINY * 0.9), size=(rows, 3)),
                   np.where(cls == 1, rng.uniform(TINY * 1.1, QUARTER_PI * 0.98, size=(rows, 3)),
                            10.0 ** rng.uniform(np.log10(0.8), np.log10(119.0), size=(rows, 3))))
    imu_rot = end[None, :] + mag * rng.choice([-1.0, 1.0], size=(rows, 3))
    imu_rot[-1] = end
    n_row = (2 * n) // 3
    rel = np.concatenate([rel_rows[rng.integers(0, rows, n_row)], rng.uniform(0.0, 0.1, n - n_row).astype(F32)])
    rel = rel[rng.permutation(n)]
    c = _case(_points(rng, n), rel, imu_time, imu_rot, scan_cur, scan_cur + 0.1, (0.4, -0.3, 0.05))
    ang = np_deskew_angles(c["rel"], imu_time, imu_rot, scan_cur)[0]
    c["stats"] = dict(classes=angle_class_counts(ang), **_time_stats(c))
    return c


def deskew_translation(kind, n=257, epoch=100.0):
    """FindPosition's path: a large odometry increment (+-50 m), a zero one, and time_scan_end == time_scan_cur (the ratio is a division
    by zero: inf for a positive point time, NaN for the scan's first point at 0; whatever the reference's arithmetic gives is the contract)."""
    c = deskew_exact_rows(n, epoch, seed=40)
    if kind == "large":
        c["incre"] = np.array([50.0, -50.0, 0.75], F32)
    elif kind == "large_neg":
        c["incre"] = np.array([-50.0, 50.0, -0.75], F32)
    elif kind == "zero":
        c["incre"] = np.zeros(3, F32)
    elif kind == "end_is_cur":
        c["scan_end"] = c["scan_cur"]
        c["incre"] = np.array([2.0, -1.0, 0.1], F32)
    elif kind == "end_is_cur_zero_incre":
        c["scan_end"] = c["scan_cur"]
        c["incre"] = np.array([0.0, -1.0, 0.1], F32)
    else:
        raise ValueError(kind)
    c["stats"]["rel_zero"] = int((c["rel"] == 0).sum())
    return c


TRANSLATION_KINDS = ("large", "large_neg", "zero", "end_is_cur", "end_is_cur_zero_incre")


def deskew_non_finite(n=257, epoch=100.0):
    """A few points with a NaN or an infinite coordinate and a few with a NaN time, spread over waves whose other lanes are ordinary
    points.  stats: the indices of the poisoned points."""
    c = deskew_exact_rows(n, epoch, seed=50)
    bad_xyz = {3: (np.nan, 1.0, 2.0), 64: (1.0, np.nan, 2.0), 65: (1.0, 2.0, np.nan), 127: (np.inf, 1.0, 2.0), 128: (-np.inf, 1.0, 2.0),
               130: (1.0, np.inf, 2.0), 131: (1.0, 2.0, -np.inf), 200: (np.inf, np.inf, -np.inf), 255: (np.nan, np.nan, np.nan)}
    for i, p in bad_xyz.items():
        c["xyz"][i] = p
    bad_t = (5, 63, 129, 256)
    for i in bad_t:
        c["rel"][i] = np.nan
    c["stats"] = dict(bad=sorted(set(bad_xyz) | set(bad_t)), nan_time=len(bad_t), bad_xyz=len(bad_xyz))
    return c


def deskew_cases():
    """(id, constructor) of every deskew case the oracle is compared with the mirror (CPU) and the kernel (GPU) on."""
    out = []
    for ep in EPOCHS:
        for n in DESKEW_SIZES:
            out.append((f"rows-n{n}-t{ep:g}", lambda n=n, ep=ep: deskew_exact_rows(n, ep)))
        for rows in (1, 2):
            for n in (1, 257):
                out.append((f"table{rows}-n{n}-t{ep:g}", lambda rows=rows, n=n, ep=ep: deskew_short_table(rows, n, ep)))
        out.append((f"rot-t{ep:g}", lambda ep=ep: deskew_large_rotations(4099, ep)))
    for kind in TRANSLATION_KINDS:
        out.append((f"incre-{kind}", lambda kind=kind: deskew_translation(kind)))
    out.append(("nonfinite", deskew_non_finite))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# downsample cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _ds(xyz, vs=DS_VOXEL_SIZES, **stats):
    return dict(xyz=np.ascontiguousarray(xyz, F32).reshape(-1, 3), vs=tuple(vs), stats=stats)


def ds_random(n, seed, half=3.0, half_z=1.0):
    """Uniform points over +-half (z: +-half_z).  The default box holds 4 x 4 x 2 voxels of 1.5 m and 30 x 30 x 10 of 0.2 m."""
    rng = np.random.default_rng(8000 + seed)
    p = rng.uniform(-1.0, 1.0, size=(n, 3)) * np.array([half, half, half_z])
    return _ds(p)


def ds_large(n):
    """The chunk loop of the offsets scan: points over +-100 m (z: -2 .. 2.5 m; the last 3000 shifted 300 m along x), tens of thousands of 1.5 m voxels, most points kept at 0.2 m."""
    rng = np.random.default_rng(8100 + n % 1000)
    p = np.empty((n, 3), F32)
    p[:, :2] = rng.uniform(-100.0, 100.0, size=(n, 2))
    p[:, 2] = rng.uniform(-2.0, 2.5, size=n)
    p[-3000:, 0] += 300.0  # the end of the input opens voxels of its own: first points in the LAST chunk at 1.5 m too
    return _ds(p, vs=(1.5, 0.2))


def ds_one_voxel(n=3000):
    """Every point inside (0.01, 0.19)^3: one voxel at every size, index 0 kept."""
    return _ds(np.random.default_rng(8201).uniform(0.01, 0.19, size=(n, 3)))


def ds_identity(n=2500):
    """Points on a 2 m lattice (jitter below 0.1 m) in shuffled order: every point alone in its voxel at every size up to 1.5 m."""
    rng = np.random.default_rng(8202)
    g = np.stack(np.meshgrid(np.arange(-10, 10), np.arange(-10, 10), np.arange(-4, 4), indexing="ij"), -1).reshape(-1, 3)
    p = g[rng.permutation(len(g))[:n]] * 2.0 + 0.3 + rng.uniform(0.0, 0.1, size=(n, 3))
    return _ds(p)


def ds_duplicates(n=3000, distinct=700):
    """`distinct` points, each repeated bit for bit at random places of the input: the first occurrence wins."""
    rng = np.random.default_rng(8203)
    base = rng.uniform(-6.0, 6.0, size=(distinct, 3)).astype(F32)
    pick = rng.integers(0, distinct, n)
    return _ds(base[pick], picks=pick)


BOUNDARY_FIRSTS = (63, 64, 127, 128, 1023, 1024, 2047, 2048)


def ds_boundary_firsts(n=2200):
    """One crowded voxel (first point: index 0) and eight more voxels whose FIRST point is the last lane of a wave (63, 127), of a block
    (1023, 2047) and lane 0 of the next (64, 128, 1024, 2048); each of them comes back later in the input."""
    rng = np.random.default_rng(8204)
    p = rng.uniform(0.01, 0.19, size=(n, 3))
    for j, i in enumerate(BOUNDARY_FIRSTS):
        c = np.array([3.0 * (j + 1), -3.0 * (j + 1), 3.0]) + rng.uniform(0.01, 0.19, size=3)
        p[i] = c
        for later in rng.integers(i + 1, n, 3):
            if int(later) not in BOUNDARY_FIRSTS:
                p[later] = c + rng.uniform(-0.005, 0.005, size=3)
    return _ds(p, expect=(0,) + BOUNDARY_FIRSTS)


def exact_face_values(vs, count=24):
    """float32 values v > 0 whose FLOAT64 quotient (double)v / vs is an integer exactly (for 0.2, which no float32 multiple of equals in the
    reals, these are the values whose quotient ROUNDS onto the face)."""
    out = []
    for k in range(1, 4000):
        c = F32(k * vs)
        for v in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
            q = F64(v) / F64(vs)
            if q == np.floor(q) and float(v) not in out:
                out.append(float(v))
        if len(out) >= count:
            break
    assert len(out) >= count, (vs, len(out))
    return np.array(out, F32)


def ds_faces(vs, n=2400):
    """Coordinates exactly on a voxel face of size vs (float64 quotient integral), one float32 ulp either side, +-0.0, and all of it
    mirrored to negative coordinates; on one, two or three axes of a point, the other axes random.  Runs at every voxel size."""
    rng = np.random.default_rng(8300 + int(vs * 10))
    f = exact_face_values(vs)
    pos = np.concatenate([f, np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf)), np.array([0.0, np.nextafter(F32(0), F32(1))], F32)])
    special = np.concatenate([pos, -pos])                                      # (-0.0f is in here)
    p = rng.uniform(-float(f.max()), float(f.max()), size=(n, 3)).astype(F32)
    on = rng.random(size=(n, 3)) < 0.5
    p[on] = special[rng.integers(0, len(special), int(on.sum()))]
    p[:6] = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [f[0], -f[0], 0.0], [-f[0], f[0], -0.0]], F32)
    q = p.astype(F64) / F64(vs)
    return _ds(p, on_face=int((q == np.floor(q)).sum()), neg_zero=int((np.signbit(p) & (p == 0)).sum()),
               neg_on_face=int(((q == np.floor(q)) & (p < 0)).sum()))


def pack_edge_values(vs):
    """float32 coordinates at the ends of the packable range of voxel size vs: the largest with v / vs < 2^20, one with v / vs about
    2^20 - 1, one with v / vs about -2^20 + 0.5 (its cell is -2^20, the lowest), the smallest with v / vs > -2^20 and one about -(2^20 - 1)."""
    def quot(v):
        return F64(F32(v)) / F64(vs)
    top = F32(vs * PACK_LIM)
    while quot(top) >= PACK_LIM:
        top = np.nextafter(top, F32(-np.inf))
    bot = F32(-vs * PACK_LIM)
    while quot(bot) <= -PACK_LIM:
        bot = np.nextafter(bot, F32(np.inf))
    vals = np.array([top, F32(vs * (PACK_LIM - 1)), F32(vs * (-PACK_LIM + 0.5)), bot, F32(-vs * (PACK_LIM - 1))], F32)
    q = vals.astype(F64) / F64(vs)
    assert np.all((q > -PACK_LIM) & (q < PACK_LIM)), (vs, q)
    assert np.floor(q[0]) == PACK_LIM - 1 and np.floor(q[2]) == -PACK_LIM and np.floor(q[3]) == -PACK_LIM
    return vals


def ds_pack_edges(vs, n=600):
    """Random points plus, on every axis, points at the ends of the packable range -- each twice (the second a little off on the other
    axes, same voxel) so that "kept correctly" includes "the later one dropped".  Runs at its own voxel size only."""
    rng = np.random.default_rng(8400 + int(vs * 10))
    p = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(F32)
    vals = pack_edge_values(vs)
    rows = []
    for ax in range(3):
        for v in vals:
            a = rng.uniform(0.3, 0.4, size=3) * vs
            a[ax] = v
            b = a + 0.05 * vs
            b[ax] = v
            rows += [a, b]
    rows.append(np.array([vals[0], vals[3], vals[0]]))  # three extreme fields in one key
    rows.append(np.array([vals[3], vals[0], vals[3]]))
    where = rng.permutation(n)[: len(rows)]
    p[where] = np.array(rows, F32)
    return _ds(p, vs=(vs,), extreme=len(rows), max_abs_q=float(np.abs(p.astype(F64) / vs).max()))


UNPACKABLE_KINDS = ("plus_2^20", "minus_2^20", "beyond", "nan", "plus_inf", "minus_inf")


def ds_unpackable(kind, vs=1.5, n=5000, seed=0, at=None):
    """A cloud with ONE point the device cannot pack (coordinate / vs = +-2^20 exactly, beyond, NaN, inf): ELM_ERR_UNSUPPORTED."""
    c = ds_random(n, 60 + seed, half=10.0)
    v = {"plus_2^20": vs * PACK_LIM, "minus_2^20": -vs * PACK_LIM, "beyond": 1.0e7, "nan": np.nan, "plus_inf": np.inf, "minus_inf": -np.inf}[kind]
    i = n // 2 if at is None else at
    c["xyz"][i, 1] = v
    q = F64(c["xyz"][i, 1]) / F64(vs)
    assert not (q > -PACK_LIM and q < PACK_LIM)
    c["vs"] = (vs,)
    c["stats"] = dict(bad_index=i, quotient=float(q))
    return c


def ds_slot(xyz, vs, cap_log2):
    """The home slot of every point's voxel in a table of 2^cap_log2 entries: the packing of ds_key (three 21-bit fields, cell + 2^20) and
    the multiplicative hash of k_ds_insert, restated to choose and to audit the adversarial input."""
    k = voxel_coords(xyz, vs) + PACK_LIM
    key = (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)
    with np.errstate(over="ignore"):
        return ((key * np.uint64(HASH_MUL)) >> np.uint64(64 - cap_log2)).astype(np.int64)


def ds_adversarial(n=4096, vs=1.5, colliding=640, repeats=3):
    """n = 4096 points (a table of 2^13 slots): `colliding` voxels whose home slot is one of the LAST EIGHT, so that their probe chains
    run through the end of the table and wrap into slot 0 and on for hundreds of slots; each of them `repeats` times at indices spread
    over the whole input, the rest random."""
    cap_log2 = 13
    rng = np.random.default_rng(8500)
    g = np.stack(np.meshgrid(np.arange(-160, 160), np.arange(-160, 160), np.arange(-10, 10), indexing="ij"), -1).reshape(-1, 3)
    centre = ((g + 0.5) * vs).astype(F32)
    assert np.array_equal(voxel_coords(centre, vs), g)
    home = ds_slot(centre, vs, cap_log2)
    hit = np.flatnonzero(home >= (1 << cap_log2) - 8)
    assert len(hit) >= colliding, len(hit)
    hit = hit[rng.permutation(len(hit))[:colliding]]
    pts = np.repeat(centre[hit].astype(F64), repeats, axis=0) + rng.uniform(-0.3, 0.3, size=(colliding * repeats, 3)) * vs
    rest = rng.uniform(-1.0, 1.0, size=(n - len(pts), 3)) * np.array([240.0, 240.0, 15.0])
    p = np.concatenate([pts, rest]).astype(F32)[rng.permutation(n)]
    home = ds_slot(p, vs, cap_log2)
    last8 = home >= (1 << cap_log2) - 8
    vox = voxel_coords(p, vs)
    uniq, cnt = np.unique(vox[last8], axis=0, return_counts=True)
    idx = np.flatnonzero(last8)
    return _ds(p, cap_log2=cap_log2, last8_voxels=len(uniq), last8_repeated_voxels=int((cnt >= 2).sum()), last8_points=int(last8.sum()),
               last8_index_span=(int(idx.min()), int(idx.max())), last8_per_slot=np.bincount(home[last8] - ((1 << cap_log2) - 8), minlength=8).tolist())


CLEAN_SEQUENCE = (5000, 6000, 9000, 5000, 70000, 5000, "unpackable", 5000, 6000)


def ds_clean_sequence():
    """The calls of the clean-table sequence on ONE context: the same capacity twice (2^14 slots for 5000 and 6000 points),
    9000 -> 2^15, back to 2^14 inside the larger allocation, 70 000 -> 2^18 (a reallocation), back, a call that ends in
    ELM_ERR_UNSUPPORTED, and two more good ones.  Every cloud has its own seed and fills the same 20 m x 20 m x 2 m box, so consecutive calls
    share most of their voxels: a key or a first index left behind by an earlier call shows as a missing or an extra point."""
    out = []
    for j, n in enumerate(CLEAN_SEQUENCE):
        if n == "unpackable":
            out.append(ds_unpackable("beyond", vs=0.5, n=5000, seed=100 + j, at=1234))
        else:
            c = ds_random(n, 100 + j, half=10.0)
            c["vs"] = (0.5,)
            out.append(c)
    return out


def table_cap_log2(n):
    """The table size downsample_enqueue picks (restated for the sequence's own audit: which calls share a capacity)."""
    c = 6
    while (1 << c) < 2 * max(n, 1):
        c += 1
    return c


def downsample_cases():
    """(id, constructor) of every packable downsample case except the two million-point ones (those: ds_large)."""
    out = [(f"n{n}", lambda n=n: ds_random(n, n)) for n in DS_SIZES]
    out += [("one_voxel", ds_one_voxel), ("identity", ds_identity), ("duplicates", ds_duplicates), ("boundary_firsts", ds_boundary_firsts)]
    out += [(f"faces{vs}", lambda vs=vs: ds_faces(vs)) for vs in (0.5, 1.5, 0.2)]
    out += [(f"pack{vs}", lambda vs=vs: ds_pack_edges(vs)) for vs in DS_VOXEL_SIZES]
    out += [("adversarial", ds_adversarial)]
    return out
