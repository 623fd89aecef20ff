"""Scenes for the registration information, shared by the CPU and the GPU tests: a closed room, and a corridor
whose planes are exact in float32 so that its free direction is exactly free.

The room stands away from the origin (the reference's default target there is reachable from an empty neighbourhood).  The corridor runs
along x: two walls at y = +-2 and a floor at z = -1 -- powers of two, so that the mean of equal coordinates, their deviations and with them
a whole row of every neighbourhood covariance are exactly zero, and every plane normal has an x component of exactly 0.  The floor ends
0.5 m short of the walls and the walls start 0.5 m above it: no neighbourhood of 0.4 m radius mixes two planes."""
import numpy as np

import reginfo_ref as ref

ROOM_CENTRE = np.array([20.0, 10.0, 0.0])
ROOM_HALF = np.array([4.0, 3.0, 1.5])
CORRIDOR_AXIS = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0])  # in the tangent [v; w] of a pose whose rotation is about x


def _plane(u, v, fixed_axis, fixed, rng, jitter):
    """points on the plane x[fixed_axis] = fixed over the grids u x v of the two other axes, jittered inside the plane"""
    U, V = np.meshgrid(u, v, indexing="ij")
    p = np.empty((U.size, 3))
    axes = [a for a in range(3) if a != fixed_axis]
    p[:, axes[0]] = U.ravel() + rng.uniform(-jitter, jitter, U.size)
    p[:, axes[1]] = V.ravel() + rng.uniform(-jitter, jitter, U.size)
    p[:, fixed_axis] = fixed
    return p


def room_points(seed=5, step=0.15, roughness=0.01):
    """About 8 000 float32 map points on the six faces of an 8 x 6 x 3 m room around ROOM_CENTRE, each face a little rough."""
    rng = np.random.default_rng(seed)
    h = ROOM_HALF
    g = [np.arange(-h[a] + step / 2, h[a], step) for a in range(3)]
    faces = []
    for axis in range(3):
        o = [a for a in range(3) if a != axis]
        for side in (-1.0, 1.0):
            f = _plane(g[o[0]], g[o[1]], axis, side * h[axis], rng, 0.04)
            f[:, axis] += rng.normal(0.0, roughness, len(f))
            faces.append(f)
    return (np.concatenate(faces) + ROOM_CENTRE).astype(np.float32)


def corridor_points(seed=6, step=0.25, length=20.0):
    """About 2 500 float32 map points: walls y = +-2 over z in [-0.5, 2], floor z = -1 over y in [-1.5, 1.5], x in [-length / 2, length / 2].
    The step keeps every voxel under the map's cap of 30 points: a capped voxel keeps the first points it was given, which can leave a
    point with a collinear neighbourhood, whose plane normal is then decided by rounding and may point along the corridor."""
    rng = np.random.default_rng(seed)
    x = np.arange(-length / 2 + step / 2, length / 2, step)
    zw = np.arange(-0.5 + step / 2, 2.0, step)
    yf = np.arange(-1.5 + step / 2, 1.5, step)
    parts = [_plane(x, zw, 1, 2.0, rng, 0.04), _plane(x, zw, 1, -2.0, rng, 0.04), _plane(x, yf, 2, -1.0, rng, 0.04)]
    return np.concatenate(parts).astype(np.float32)


def rot_x(a):
    """rotation about x with exact zeros and an exact one: R^T n keeps an x component of exactly 0"""
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def general_rotation(seed, max_deg=180.0):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    return ref.exp_so3(ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(0.3 * max_deg, max_deg)))


def scan_of(world, T, n, seed, noise=0.02, within=None):
    """n float32 scan points in the frame of T: map points drawn without replacement (all of them if n exceeds them; `within`: only those
    within that distance of T's origin), plus N(0, noise)"""
    rng = np.random.default_rng(seed)
    w = np.asarray(world, dtype=np.float64)
    if within is not None:
        w = w[np.linalg.norm(w - T[:3, 3], axis=1) < within]
    sel = rng.choice(len(w), min(n, len(w)), replace=False)
    g = w[sel] + rng.normal(0.0, noise, (len(sel), 3))
    return ((g - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


def corridor_pairs(T, n=400, seed=7, noise=0.01):
    """The corridor as pairs built by hand for the CPU: scan points near the three planes, each paired with its foot on its plane and that
    plane's normal -> (points float32 [n, 3], pairs as reginfo_ref.job takes them)"""
    rng = np.random.default_rng(seed)
    g = np.empty((n, 3))
    normals = np.empty((n, 3))
    k = rng.integers(0, 3, n)
    g[:, 0] = rng.uniform(-8.0, 8.0, n)
    for i in range(n):
        if k[i] == 2:
            g[i, 1], g[i, 2], normals[i] = rng.uniform(-1.5, 1.5), -1.0, (0.0, 0.0, 1.0)
        else:
            g[i, 1], g[i, 2], normals[i] = (2.0 if k[i] else -2.0), rng.uniform(-0.5, 2.0), (0.0, 1.0, 0.0)
    mu = g.copy()
    pts = (((g + rng.normal(0.0, noise, g.shape)) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return pts, [(i, mu[i], None, normals[i], False) for i in range(n)]


def room_pairs(T, n=400, seed=8, noise=0.01):
    """The closed room as pairs built by hand: points near the six faces with their feet and normals"""
    rng = np.random.default_rng(seed)
    g = ROOM_CENTRE + rng.uniform(-1.0, 1.0, (n, 3)) * ROOM_HALF
    normals = np.zeros((n, 3))
    face = rng.integers(0, 6, n)
    for i in range(n):
        a, side = face[i] // 2, 1.0 if face[i] % 2 else -1.0
        g[i, a] = ROOM_CENTRE[a] + side * ROOM_HALF[a]
        normals[i, a] = 1.0
    mu = g.copy()
    pts = (((g + rng.normal(0.0, noise, g.shape)) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return pts, [(i, mu[i], None, normals[i], False) for i in range(n)]
