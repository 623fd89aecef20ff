"""The numpy mirror of the map build, written from the reference's VoxelHashMap::AddPoints (vhm.cpp:270-285) and
VoxelBlock::AddPointWithSpacing (vhm.hpp:106-113), not from the library's host build:

    map_resolution = sqrt(voxel_size * voxel_size / max_points_per_voxel)                        vhm.cpp:272
    for every point, in input order:
        voxel = (pose / voxel_size).cast<int>()               truncation toward zero             vhm.cpp:275
        a voxel seen for the first time takes the point as it is                                 vhm.cpp:282
        otherwise the point is kept iff the voxel holds fewer than max_points_per_voxel points and
        none of them is nearer than map_resolution: (kept.pose - pose).norm() < map_resolution   vhm.hpp:107-112

pose is float64 filled from float32 coordinates; the norm is taken as sqrt((dx * dx + dy * dy) + dz * dz).  A voxel's points never depend
on another voxel's, so the mirror groups the input per voxel (stable) and replays every voxel on its own.  The result is in BUCKET order:
voxels in first-seen order, insertion order inside a voxel (the reference's own unordered_map has no order to mirror).

build(points, voxel_size, cap) -> (points float64 [m, 3], keys int32 [v, 3], counts int32 [v]).  Keys must lie inside (-2^20, 2^20).
"""
import numpy as np


def resolution(voxel_size, cap):
    return np.sqrt(np.float64(voxel_size) * np.float64(voxel_size) / np.float64(cap))


def voxel_keys(points, voxel_size):
    """(pose / voxel_size).cast<int>() of float32 points: int64 [n, 3]"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    return np.trunc(p / np.float64(voxel_size)).astype(np.int64)


def replay(P, cap, res):
    """the indices of the points of ONE voxel (float64 [k, 3], input order) that AddPointWithSpacing keeps"""
    kept = [0]
    for j in range(1, len(P)):
        if len(kept) >= cap:
            break
        d = P[kept] - P[j]
        if not (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < res).any():
            kept.append(j)
    return kept


def build(points, voxel_size, cap):
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    if n == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
    res = resolution(voxel_size, cap)
    keys = voxel_keys(pts, voxel_size)
    assert np.abs(keys).max() < (1 << 20)
    code = ((keys[:, 0] + (1 << 20)) << 42) | ((keys[:, 1] + (1 << 20)) << 21) | (keys[:, 2] + (1 << 20))
    _, first, inv = np.unique(code, return_index=True, return_inverse=True)
    by_first = np.argsort(first)                      # voxels in first-seen order
    vid = np.empty(len(first), np.int64)
    vid[by_first] = np.arange(len(first))
    vid = vid[inv.reshape(-1)]
    order = np.argsort(vid, kind="stable")            # the input grouped per voxel, input order inside a group
    raw = np.bincount(vid, minlength=len(first))
    start = np.concatenate([[0], np.cumsum(raw)])
    P = pts.astype(np.float64)
    keep = np.zeros(n, bool)
    keep[order[start[:-1]]] = True                    # the first point of a voxel
    for v in np.nonzero(raw > 1)[0]:
        idx = order[start[v]:start[v + 1]]
        keep[idx[replay(P[idx], cap, res)]] = True
    kept_order = order[keep[order]]
    counts = np.bincount(vid[keep], minlength=len(first)).astype(np.int32)
    return P[kept_order], keys[first[by_first]].astype(np.int32), counts


def canonical(points, keys, counts):
    """a map's read-back with its voxels in ascending key order and the order inside every voxel kept: what two maps with different voxel
    orders (the reference's hash map has its own) are compared by"""
    points, keys, counts = np.asarray(points), np.asarray(keys), np.asarray(counts, dtype=np.int64)
    by_key = np.lexsort(keys.T[::-1]) if len(keys) else np.zeros(0, np.int64)
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    c = counts[by_key]
    src = np.repeat(start[by_key] - np.concatenate([[0], np.cumsum(c)])[:-1], c) + np.arange(int(c.sum()))
    return points[src], keys[by_key], c
