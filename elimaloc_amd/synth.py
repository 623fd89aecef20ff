"""Seeded synthetic worlds / scans / initial guesses for tests and bench.

World: jittered 0.2 m lattices on a ground plane (z ~ 0.3 m) plus a grid of 6 m high vertical walls in both
axis directions every 22 m, 3-axis uniform jitter +-0.004 m, float32-exact, centred on the origin so that
negative coordinates (the trunc-vs-floor voxel key quirk, vhm.cpp:275 vs vhm.hpp:176-180) are exercised.
Everything here is plain numpy on the host; nothing in this module is on the measured path.
"""
import math

import numpy as np

PITCH = 0.2
JITTER = 0.004
WALL_SPACING = 22.0
WALL_ROWS = 30  # 30 rows * 0.2 m = 6 m
PTS_PER_M2 = 25.0 + 2 * (WALL_ROWS / PITCH / WALL_SPACING) * 0.93  # rough density used to size the extent


def make_world(n_points, seed=1001):
    """Return (n_points, 3) float32 map points in a fixed, spatially coherent order."""
    rng = np.random.default_rng(seed)
    L = 0.5 * math.sqrt(n_points * 1.08 / PTS_PER_M2) + 2.0
    L = math.ceil(L / WALL_SPACING * 2) * WALL_SPACING / 2 + 1.0  # keep whole wall cells around the origin
    n_side = int(round(2 * L / PITCH))
    lat = (np.arange(n_side, dtype=np.float64) + 0.5) * PITCH - L

    parts = []
    # ground plane, row-major (x outer, y inner)
    gx, gy = np.meshgrid(lat, lat, indexing="ij")
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.3)], axis=1)
    parts.append(ground)
    del gx, gy
    # vertical walls: z rows 1.1 .. 6.9 (voxel layers 1..6, never sharing a voxel with the ground layer)
    zrow = 1.0 + (np.arange(WALL_ROWS, dtype=np.float64) + 0.5) * PITCH
    kmax = int(math.floor(L / WALL_SPACING)) + 1
    for k in range(-kmax, kmax + 1):
        xw = k * WALL_SPACING + 0.5
        if abs(xw) < L:
            wy, wz = np.meshgrid(lat, zrow, indexing="ij")
            parts.append(np.stack([np.full(wy.size, xw), wy.ravel(), wz.ravel()], axis=1))
    for k in range(-kmax, kmax + 1):
        yw = k * WALL_SPACING + 11.5
        if abs(yw) < L:
            # leave a 1.6 m gap either side of every x-wall so wall voxels never hold two lattices
            d = np.abs((lat - 0.5 + WALL_SPACING / 2) % WALL_SPACING - WALL_SPACING / 2)
            lx = lat[d >= 1.6]
            wx, wz = np.meshgrid(lx, zrow, indexing="ij")
            parts.append(np.stack([wx.ravel(), np.full(wx.size, yw), wz.ravel()], axis=1))
    pts = np.concatenate(parts, axis=0)
    del parts
    if pts.shape[0] < n_points:
        raise RuntimeError(f"world extent too small: {pts.shape[0]} < {n_points}")
    # keep the n_points closest to the origin in the Chebyshev sense, in generation order
    r = np.maximum(np.abs(pts[:, 0]), np.abs(pts[:, 1]))
    idx = np.argpartition(r, n_points - 1)[:n_points]
    idx.sort()
    pts = pts[idx]
    pts += rng.uniform(-JITTER, JITTER, size=pts.shape)
    return np.ascontiguousarray(pts.astype(np.float32))


def collinear_triples(base, n_triples, seed, z=(1.2, 1.8), spacing=0.25):
    """3 n points: n isolated triples (c - s d, c, c + s d) along random directions d, centres over the central half of `base`'s extent at
    heights `z` (clear of the ground lattice and of each other's 0.4 m neighbourhoods with overwhelming probability).  A collinear
    neighbourhood has a rank-1 sample covariance: the reference's JacobiSVD regularisation U diag(1, 1, 1e-3) V^T (vhm.hpp:141-146,
    241-247) then returns U != V for most of them and the stored "covariance" is NOT symmetric -- what thin poles, wires and edges do to a
    real map.  Used by the tests and by `bench.py --asym-triples` to put such records into an otherwise ordinary world."""
    rng = np.random.default_rng(seed)
    ext = 0.5 * np.abs(base[:, :2]).max(axis=0).astype(np.float64)
    c = np.column_stack([rng.uniform(-ext[0], ext[0], n_triples), rng.uniform(-ext[1], ext[1], n_triples), rng.uniform(z[0], z[1], n_triples)])
    d = rng.normal(size=(n_triples, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(np.concatenate([c - spacing * d, c, c + spacing * d]).astype(np.float32))


def make_field_world(n_points, seed=1001):
    """A second, less regular world (bench.py --world field; VERDICT r4 item 3: are the kernels tuned to the jittered planes?).

    Poisson-sampled height-field terrain whose density falls with the distance from the centre (40 -> 12 points per square metre:
    voxels from the 30-point cap down to a handful, most insertions deciding by the 0.1826 m spacing rule, vhm.hpp:106-113), yawed
    boxes with densely sampled walls and roofs (30-point voxels), vegetation-like Gaussian clutter blobs, one patch of EXACT
    voxel-centre lattice (a voxel-filtered PCD map: coplanar, rank-deficient neighbourhoods) and slanted poles (collinear
    neighbourhoods: asymmetric regularised covariances, layout bits 7 / 8).  Centred on the origin (negative coordinates: the
    trunc-vs-floor key quirk).  Returns ~n_points float32 points in a spatially coherent order (x strips), deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    dens0, dens1, r0 = 40.0, 12.0, 150.0
    # extent from the mean ground density; ~80 % of the points are ground, the rest structures
    L = 0.5 * math.sqrt(0.8 * n_points / (0.5 * (dens0 + dens1))) + 5.0
    n_ground = int(0.8 * n_points)
    # rejection sampling of the radial density profile
    xy = rng.uniform(-L, L, size=(int(n_ground * 1.9), 2))
    r = np.hypot(xy[:, 0], xy[:, 1])
    keep = rng.uniform(0.0, dens0, size=xy.shape[0]) < dens1 + (dens0 - dens1) * np.exp(-r / r0)
    xy = xy[keep][:n_ground]

    def height(x, y):
        return 0.3 + 0.8 * np.sin(x / 17.0) * np.cos(y / 23.0) + 0.3 * np.sin(x / 5.1 + 1.0) * np.sin(y / 6.3)

    ground = np.column_stack([xy, height(xy[:, 0], xy[:, 1]) + rng.normal(0.0, 0.01, xy.shape[0])])
    parts = [ground]
    # boxes: walls + roof, ~12 % of the points
    n_box_pts = int(0.12 * n_points)
    n_boxes = max(4, n_box_pts // 30000)  # ~80 points per square metre of wall: voxels at the 30-point cap
    for _ in range(n_boxes):
        c = rng.uniform(-0.9 * L, 0.9 * L, 2)
        sx, sy, hgt = rng.uniform(5.0, 20.0), rng.uniform(5.0, 20.0), rng.uniform(3.0, 10.0)
        yaw = rng.uniform(0.0, math.pi)
        area_w = 2.0 * (sx + sy) * hgt
        per_box = max(64, min(int(80.0 * (area_w + 0.3 * sx * sy)), 2 * (n_box_pts // n_boxes)))
        n_w = int(per_box * area_w / (area_w + 0.3 * sx * sy))
        u = rng.uniform(0.0, 2.0 * (sx + sy), n_w)
        z = rng.uniform(0.0, hgt, n_w)
        px = np.where(u < sx, u - sx / 2, np.where(u < sx + sy, sx / 2, np.where(u < 2 * sx + sy, sx / 2 - (u - sx - sy), -sx / 2)))
        py = np.where(u < sx, -sy / 2, np.where(u < sx + sy, u - sx - sy / 2, np.where(u < 2 * sx + sy, sy / 2, sy / 2 - (u - 2 * sx - sy))))
        n_r = per_box - n_w
        rx, ry = rng.uniform(-sx / 2, sx / 2, n_r), rng.uniform(-sy / 2, sy / 2, n_r)
        bx = np.concatenate([px, rx])
        by = np.concatenate([py, ry])
        bz = np.concatenate([z, np.full(n_r, hgt)])
        cy_, sy_ = math.cos(yaw), math.sin(yaw)
        g0 = float(height(c[0], c[1]))
        parts.append(np.column_stack([c[0] + cy_ * bx - sy_ * by, c[1] + sy_ * bx + cy_ * by, g0 + bz + rng.normal(0.0, 0.01, bx.size)]))
    # clutter: Gaussian blobs 0.5 .. 3 m above the ground, ~7 %
    n_cl = int(0.07 * n_points)
    n_blobs = max(8, n_cl // 40)
    bc = rng.uniform(-L, L, size=(n_blobs, 2))
    bz = height(bc[:, 0], bc[:, 1]) + rng.uniform(0.5, 3.0, n_blobs)
    which = rng.integers(0, n_blobs, n_cl)
    parts.append(np.column_stack([bc[which], bz[which]]) + rng.normal(0.0, 0.4, size=(n_cl, 3)))
    # a 40 m x 40 m patch of exact voxel-centre lattice (0.25 m pitch, float32-exact) on a flat plate 4 m above the terrain's mean
    g = (np.arange(160, dtype=np.float64) + 0.5) * 0.25
    lx, ly = np.meshgrid(g + 60.0, g - 100.0, indexing="ij")
    parts.append(np.column_stack([lx.ravel(), ly.ravel(), np.full(lx.size, 4.625)]))
    # slanted poles: 8 points 0.15 m apart along near-vertical random directions
    n_poles = max(16, int(0.0005 * n_points / 8))
    pc = rng.uniform(-0.8 * L, 0.8 * L, size=(n_poles, 2))
    pdir = np.column_stack([rng.normal(0.0, 0.15, n_poles), rng.normal(0.0, 0.15, n_poles), np.ones(n_poles)])
    pdir /= np.linalg.norm(pdir, axis=1)[:, None]
    base = np.column_stack([pc, height(pc[:, 0], pc[:, 1]) + 1.2])
    parts.append((base[:, None, :] + (np.arange(8) * 0.15)[None, :, None] * pdir[:, None, :]).reshape(-1, 3))
    pts = np.concatenate(parts, axis=0)
    # spatially coherent order: 8 m strips along x, y inside a strip (a map file written tile by tile)
    pts = pts.astype(np.float32)
    order = np.argsort(np.floor(pts[:, 0] / 8.0).astype(np.float64) * 65536.0 + pts[:, 1].astype(np.float64), kind="stable")
    return np.ascontiguousarray(pts[order])


def rot_zyx(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def rotvec_to_matrix(v):
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def rows_times(d, R):
    """d @ R for an (n,3) array and a 3x3 matrix as explicit column arithmetic (no BLAS call).

    OpenBLAS's threaded dgemm is not safe to call from several Python threads at once on this image (rows came back
    corrupted when scans were generated in a thread pool); this form is also bit-reproducible across BLAS builds."""
    d = np.asarray(d, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    out = np.empty((d.shape[0], 3), dtype=np.float64)
    for j in range(3):
        out[:, j] = (d[:, 0] * R[0, j] + d[:, 1] * R[1, j]) + d[:, 2] * R[2, j]
    return out


_EXTENT_CACHE = {}


def _array_key(a):
    """Identity of a world array for the per-array caches: address + size + a content fingerprint (first / middle / last rows), so that a
    world freed and another of the same length allocated at the same address does not inherit the old one's cache entry."""
    n = a.shape[0]
    fp = tuple(np.asarray(a[[0, n // 2, n - 1]], dtype=np.float64).ravel().tolist()) if n else ()
    return (a.ctypes.data, n, fp)


def _xy_extent(map_xyz):
    """max |x|, |y| over the map (cached per array: 10 M points cost 0.1-0.2 s, once per scan before)."""
    key = _array_key(map_xyz)
    ext = _EXTENT_CACHE.get(key)
    if ext is None:
        ext = float(np.max(np.abs(map_xyz[:, :2])))
        _EXTENT_CACHE.clear()
        _EXTENT_CACHE[key] = ext
    return ext


def make_pose(map_xyz, seed):
    """Sensor pose T_true: translation uniform in the central half of the map, yaw uniform, roll/pitch +-2 deg."""
    rng = np.random.default_rng(seed)
    ext = _xy_extent(map_xyz)
    t = np.array([rng.uniform(-ext / 2, ext / 2), rng.uniform(-ext / 2, ext / 2), 0.3 + 1.8])
    roll, pitch = np.deg2rad(rng.uniform(-2, 2, size=2))
    yaw = rng.uniform(-math.pi, math.pi)
    T = np.eye(4)
    T[:3, :3] = rot_zyx(roll, pitch, yaw)
    T[:3, 3] = t
    return T


_TILE_CACHE = {}


def _near_indices(map_xyz, centre, max_range, tile=32.0):
    """Ascending indices of the map points within max_range of centre -- the same set and order as the brute-force mask
    over the whole map, but through a cached x/y tile index for large maps (many scans are cut from one 10 M-point world)."""
    n = map_xyz.shape[0]
    if n < 2_000_000:
        d = map_xyz.astype(np.float64) - centre
        return np.flatnonzero(np.einsum("ij,ij->i", d, d) < max_range * max_range)
    key = _array_key(map_xyz)
    idx = _TILE_CACHE.get(key)
    if idx is None:
        tx = np.floor(map_xyz[:, 0] / tile).astype(np.int64)
        ty = np.floor(map_xyz[:, 1] / tile).astype(np.int64)
        x0, y0 = int(tx.min()), int(ty.min())
        ny = int(ty.max()) - y0 + 1
        code = (tx - x0) * ny + (ty - y0)
        order = np.argsort(code, kind="stable")
        starts = np.searchsorted(code[order], np.arange(int(code.max()) + 2))
        idx = (order, starts, x0, y0, ny, int(tx.max()) - x0 + 1)
        _TILE_CACHE.clear()
        _TILE_CACHE[key] = idx
    order, starts, x0, y0, ny, nx = idx
    ax0 = max(int(math.floor((centre[0] - max_range) / tile)) - x0, 0)
    ax1 = min(int(math.floor((centre[0] + max_range) / tile)) - x0, nx - 1)
    ay0 = max(int(math.floor((centre[1] - max_range) / tile)) - y0, 0)
    ay1 = min(int(math.floor((centre[1] + max_range) / tile)) - y0, ny - 1)
    parts = [order[starts[ix * ny + ay0]:starts[ix * ny + ay1 + 1]] for ix in range(ax0, ax1 + 1)]
    cand = np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
    d = map_xyz[cand].astype(np.float64) - centre
    return cand[np.einsum("ij,ij->i", d, d) < max_range * max_range]


def make_scan(map_xyz, n_scan, seed, T_true=None, max_range=60.0, noise=0.01):
    """Draw n_scan map points within max_range of the sensor, add N(0, noise), express in the sensor frame.

    Returns (scan_xyz float32 (n,3) sensor frame, T_true 4x4 float64)."""
    if T_true is None:
        T_true = make_pose(map_xyz, seed)
    rng = np.random.default_rng(seed + 7919)
    near = _near_indices(map_xyz, T_true[:3, 3], max_range)
    if near.size >= n_scan:
        pick = rng.choice(near, size=n_scan, replace=False)
    else:  # small worlds: sample with replacement, the noise makes the points distinct
        pick = rng.choice(near, size=n_scan, replace=True)
    pick.sort()
    world = map_xyz[pick].astype(np.float64) + rng.normal(0.0, noise, size=(n_scan, 3))
    local = rows_times(world - T_true[:3, 3], T_true[:3, :3])  # R^T (w - t), BLAS-free (deterministic, thread-safe)
    return np.ascontiguousarray(local.astype(np.float32)), T_true


def lidar_beams(rings=32, azimuths=512, elevation_min_deg=-25.0, elevation_max_deg=15.0):
    """Unit vectors of a spinning LiDAR in the sensor frame: `rings` elevations evenly spaced over [elevation_min_deg, elevation_max_deg]
    (one ring: their mean) x `azimuths` evenly spaced over the full turn from 0 -> float32 [rings * azimuths, 3], ring-major.  The beam
    model of VoxelHashMap.RayCast / RenderScan: one return per beam, unlike make_scan's draw of map points."""
    el = np.deg2rad(np.linspace(elevation_min_deg, elevation_max_deg, rings) if rings > 1 else np.array([0.5 * (elevation_min_deg + elevation_max_deg)]))
    az = 2.0 * math.pi * np.arange(azimuths, dtype=np.float64) / azimuths
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    v = np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], se * np.ones_like(az)[None, :]], 2).reshape(-1, 3)
    return np.ascontiguousarray(v.astype(np.float32))


def perturb(T_true, seed, max_trans=0.15, max_rot_deg=0.5):
    """Initial guess T0 = T_true * delta; delta translation uniform in a ball, rotation angle uniform <= max."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=3)
    v /= np.linalg.norm(v)
    t = v * max_trans * rng.uniform() ** (1.0 / 3.0)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    ang = np.deg2rad(max_rot_deg) * rng.uniform()
    D = np.eye(4)
    D[:3, :3] = rotvec_to_matrix(a * ang)
    D[:3, 3] = t
    return T_true @ D


def pose_error(Ta, Tb):
    """(translation error m, rotation angle rad) of Ta^-1 Tb."""
    D = np.linalg.inv(Ta) @ Tb
    dt = float(np.linalg.norm(D[:3, 3]))
    c = (np.trace(D[:3, :3]) - 1.0) / 2.0
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return dt, float(math.atan2(s, c))


def make_deskew_stream(n_points, seed, scan_period=0.1, imu_hz=200.0, odom_hz=100.0, yaw_rate=0.3, speed=10.0,
                       stamp=1000.0):
    """Raw scan with per-point time + IMU/odom samples around it (config 5).

    lidar_scan_time_end semantics: point times are a linear ramp -scan_period..0 in azimuth order and the
    message stamp is the scan END (loc.ini:5).  Returns dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    az = np.sort(rng.uniform(-math.pi, math.pi, n_points))
    rngs = rng.uniform(2.0, 80.0, n_points)
    el = np.deg2rad(rng.uniform(-15, 15, n_points))
    xyz = np.stack([rngs * np.cos(el) * np.cos(az), rngs * np.cos(el) * np.sin(az), rngs * np.sin(el)], axis=1)
    t = (-scan_period + scan_period * (np.arange(n_points) + 0.5) / n_points).astype(np.float32)
    t[-1] = 0.0
    imu_t = stamp - scan_period - 0.05 + np.arange(int((scan_period + 0.1) * imu_hz) + 1) / imu_hz
    imu_w = np.stack([rng.normal(0, 0.01, imu_t.size), rng.normal(0, 0.01, imu_t.size),
                      yaw_rate + rng.normal(0, 0.01, imu_t.size)], axis=1)
    od_t = stamp - scan_period - 0.095 + np.arange(int((scan_period + 0.2) * odom_hz) + 1) / odom_hz
    odom = np.zeros((od_t.size, 14))
    yaw = yaw_rate * (od_t - od_t[0])
    odom[:, 0] = od_t
    odom[:, 1] = speed * (od_t - od_t[0]) * np.cos(0.1)
    odom[:, 2] = speed * (od_t - od_t[0]) * np.sin(0.1)
    odom[:, 3] = 0.02 * (od_t - od_t[0])
    odom[:, 6] = np.sin(yaw / 2)
    odom[:, 7] = np.cos(yaw / 2)
    odom[:, 8] = speed
    odom[:, 13] = yaw_rate
    return dict(xyz=np.ascontiguousarray(xyz.astype(np.float32)), time=t, stamp=stamp, imu_t=imu_t, imu_w=imu_w,
                odom=odom)


class Drive:
    """Ground-truth ego trajectory for the config-5 stream: parked for `t_park` s (the PCM-init warm-up blocks prediction),
    then accelerating to `speed` with a slow sinusoidal yaw rate.  Planar (roll = pitch = 0, constant z)."""

    def __init__(self, start_xy=(3.0, -2.0), z=0.3, yaw0=0.4, t_park=1.5, accel=2.0, speed=8.0, yaw_amp=0.25, t_total=30.0):
        self.dt = 5e-4
        n = int(t_total / self.dt) + 2
        self.t = np.arange(n) * self.dt
        tm = np.clip(self.t - t_park, 0.0, None)
        self.v = np.minimum(accel * tm, speed)
        self.a = np.where((tm > 0) & (accel * tm < speed), accel, 0.0)
        self.w = yaw_amp * np.sin(0.7 * tm) * (tm > 0)
        self.yaw = yaw0 + np.concatenate([[0.0], np.cumsum(0.5 * (self.w[1:] + self.w[:-1]) * self.dt)])
        vx, vy = self.v * np.cos(self.yaw), self.v * np.sin(self.yaw)
        self.x = start_xy[0] + np.concatenate([[0.0], np.cumsum(0.5 * (vx[1:] + vx[:-1]) * self.dt)])
        self.y = start_xy[1] + np.concatenate([[0.0], np.cumsum(0.5 * (vy[1:] + vy[:-1]) * self.dt)])
        self.z = z

    def at(self, t):
        """-> x, y, yaw, speed, yaw_rate, accel at time(s) t (linear interpolation of the 2 kHz integration)."""
        f = lambda arr: np.interp(t, self.t, arr)
        return f(self.x), f(self.y), f(self.yaw), f(self.v), f(self.w), f(self.a)

    def ego_pose(self, t):
        x, y, yaw, *_ = self.at(float(t))
        T = np.eye(4)
        T[:3, :3] = rot_zyx(0.0, 0.0, float(yaw))
        T[:3, 3] = [x, y, self.z]
        return T

    def imu(self, t, rng=None, gyro_noise=1e-3, acc_noise=1e-2, gravity=9.81):
        """Ego-frame gyro and specific force at time t."""
        _, _, _, v, w, a = self.at(float(t))
        g = np.array([0.0, 0.0, float(w)])
        f = np.array([float(a), float(v * w), gravity])
        if rng is not None:
            g = g + rng.normal(0, gyro_noise, 3)
            f = f + rng.normal(0, acc_noise, 3)
        return g, f

    def scan(self, world, n_points, t_end, tf_ego_to_lidar, seed, period=0.1, max_range=40.0, noise=0.01):
        """Raw (skewed) scan: point i is observed at its own time t_end - period .. t_end from the lidar pose of that instant.
        Returns xyz float32 [n,3] in the lidar frame and the PointXYZIT `time` field (ramp -period .. 0, scan_time_end)."""
        rng = np.random.default_rng(seed)
        end = self.ego_pose(t_end) @ tf_ego_to_lidar
        near = world[np.linalg.norm(world - end[:3, 3].astype(np.float32), axis=1) < max_range]
        pick = near[rng.choice(len(near), n_points, replace=len(near) < n_points)].astype(np.float64)
        rel = -period + period * (np.arange(n_points) + 0.5) / n_points
        rel[-1] = 0.0
        x, y, yaw, *_ = self.at(t_end + rel)
        d = pick - np.stack([x, y, np.full_like(x, self.z)], 1)
        c, s = np.cos(yaw), np.sin(yaw)
        ego = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], d[:, 2]], 1)      # R_z(yaw)^T d
        Rl, tl = tf_ego_to_lidar[:3, :3], tf_ego_to_lidar[:3, 3]
        lidar = rows_times(ego - tl, Rl) + rng.normal(0, noise, (n_points, 3))                             # Rl^T (ego - tl)
        return np.ascontiguousarray(lidar.astype(np.float32)), rel.astype(np.float32)
