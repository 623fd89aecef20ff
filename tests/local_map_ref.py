"""The numpy mirror of the device producers of elm_map_build_device_from and of the odometry's host rules, written from the contract in
include/elimaloc_hip.h ("device map build from resident sources", "LiDAR odometry on a rolling local map"), not from the C++:

    drop[i] = 0  iff  keep is None, or ((dx dx + dy dy) + dz dz) <= r2, d = float64(stored float32 point) - centre, r2 = radius * radius
    xyz          = for every job in order, every point of its scan in resident order: float32(((R_r0 x + R_r1 y) + R_r2 z) + t_r)

numpy's elementwise float64 multiply, add and subtract are single IEEE operations (no fused multiply-add), and astype(float32) rounds to
nearest even: the expressions below are the contract's, operation for operation.  tests/build_ref.py then gives the map.

    keyframe     insert iff sqrt((dx dx + dy dy) + dz dz) >= key_min_trans_m or (((R00 + R11) + R22) - 1) / 2 <= cos(key_min_rot_rad),
                 d = t_new - t_key, R_ii = (K_0i N_0i + K_1i N_1i) + K_2i N_2i
    prediction   T_{k-1} (T_{k-2}^-1 T_{k-1}) with the rigid inverse [R^T, -R^T t]
"""
import math

import numpy as np

import build_ref


def keep_flags(base_points, keep):
    """drop uint8 [n] for stored points [n, 3] (float32 values) and keep = None or (centre [3], radius)"""
    p = np.asarray(base_points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    if keep is None:
        return np.zeros(len(p), np.uint8)
    c = np.asarray(keep[0], dtype=np.float64).reshape(3)
    r2 = np.float64(keep[1]) * np.float64(keep[1])
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    return (~(((dx * dx + dy * dy) + dz * dz) <= r2)).astype(np.uint8)


def transform(points, T):
    """float32 [n, 3]: float32(R p + t) of float32 points under the 4 x 4 pose T, the contract's association"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
        return np.ascontiguousarray(q.astype(np.float32))


def sources(base_points, keep, scans, poses):
    """(drop uint8 [n_base], xyz float32 [sum of the scans, 3]) -- what elm_map_build_device takes to build the same map.  scans: the
    resident points of every job (Scan.points()), poses: one 4 x 4 per job."""
    drop = keep_flags(base_points, keep)
    parts = [transform(s, T) for s, T in zip(scans, poses)]
    xyz = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    return drop, np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)


def input_points(base_points, keep, scans, poses):
    """P: the kept stored points followed by the transformed scan points, float32 [n, 3]"""
    drop, xyz = sources(base_points, keep, scans, poses)
    base = np.asarray(base_points, dtype=np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([base[drop == 0], xyz])), drop, xyz


def build(base_points, keep, scans, poses, voxel_size, cap):
    """the mirror map (points float64, keys int32, counts int32) and the stats dict elm_map_build_device_from reports"""
    P, drop, xyz = input_points(base_points, keep, scans, poses)
    m = build_ref.build(P, voxel_size, cap)
    stats = dict(n_base_kept=int((drop == 0).sum()), n_base_dropped=int((drop != 0).sum()), n_scan_points=len(xyz), n_points=len(m[0]),
                 n_voxels=len(m[1]))
    return m, stats


def is_keyframe(T_key, T_new, key_min_trans_m, key_min_rot_rad):
    K, N = np.asarray(T_key, dtype=np.float64), np.asarray(T_new, dtype=np.float64)
    dx, dy, dz = N[0, 3] - K[0, 3], N[1, 3] - K[1, 3], N[2, 3] - K[2, 3]
    if math.sqrt((dx * dx + dy * dy) + dz * dz) >= key_min_trans_m:
        return True
    R = [(K[0, i] * N[0, i] + K[1, i] * N[1, i]) + K[2, i] * N[2, i] for i in range(3)]
    return (((R[0] + R[1]) + R[2]) - 1.0) / 2.0 <= math.cos(key_min_rot_rad)


def rigid_inverse(T):
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def predict(history):
    """the constant-velocity guess from the poses of the steps that succeeded so far"""
    if not history:
        return np.eye(4)
    if len(history) == 1:
        return np.array(history[-1], dtype=np.float64)
    return history[-1] @ (rigid_inverse(history[-2]) @ history[-1])


def oracle_loop(O, method, poses, scans, guesses, voxel_size, cap, max_range, key_min_trans_m=0.0, key_min_rot_rad=0.0, **reg):
    """The odometry loop with the oracle's registration on mirror-built maps: per step a dict (T, registered, is_success, inserted,
    iterations), and the stored points of the last map; reg: fields of the oracle's config.  The oracle's map of a step is add_points of the mirror map's stored points (they
    survive their own replay), with the covariances the method reads."""
    cfg = O.default_config(method, **reg)
    stored = np.zeros((0, 3))
    history, steps, T_key = [], [], None
    for k, scan in enumerate(scans):
        guess = np.asarray(guesses[k], dtype=np.float64) if guesses is not None else predict(history)
        st = dict(T=guess, registered=False, is_success=True, inserted=False, iterations=0)
        if T_key is not None:
            om = O.Map(voxel_size, cap)
            om.add_points(stored.astype(np.float32))
            if method == O.GICP:
                om.cal_point_cov_all(cfg.gicp_cov_search_dist)
            elif method in (O.VGICP, O.AVGICP):
                om.cal_voxel_cov_all()
            r = O.register(om, scan, guess, cfg)
            st.update(T=r["T"], registered=True, is_success=bool(r["is_success"]), iterations=int(r["iterations"]))
        if st["is_success"]:
            if T_key is None or is_keyframe(T_key, st["T"], key_min_trans_m, key_min_rot_rad):
                (stored, _, _), _ = build(stored, (st["T"][:3, 3], max_range) if T_key is not None else None, [scan], [st["T"]], voxel_size, cap)
                T_key = st["T"]
                st["inserted"] = True
            history.append(st["T"])
        steps.append(st)
    return steps, stored
