"""Cost of a local-map insert on one GPU, device producers against host primitives: prints ONE JSON line and writes it to
profiles/local_map_rate.json (--out).

The insert of the odometry: from a resident local map of about 300 000 stored points, forget what lies farther than
--range metres from the new pose and add one resident 16 384-point scan at that pose.  Per step, wall clock (each call ends in its own
synchronise) of
    device   elm_map_build_device_from: the sphere and the scan's transform run on the device, only the job table crosses the bus; its
             stages come from hipEvents on the context's stream (elm_map_build_device_stages), what is left of the wall clock is the
             host's share (scratch allocation, slot table, transfers of keys and ranges)
    host     the same insert from the host primitives of the same commit: Pointcloud() download, the flags and the transform in numpy,
             elm_map_build_device with host arrays
and, for the device path, what an odometry step adds on top: the covariance recompute over the whole new map (CalPointCovAll(0.4) for
GICP, CalVoxelCovAll for VGICP; each followed by a synchronise).  Then one whole-log build: --log scans x 16 384 points at as many poses, no base, one call, against numpy
transforms + elm_map_build_device.  The two maps' read-backs (points, keys, counts, info) are asserted equal before anything is reported.

    python tools/local_map_rate.py [--steps 8] [--log 256] [--range 55] [--out profiles/local_map_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("input", "insert", "voxel_ids", "raw_counts", "grouping", "replay", "emit")
SCAN_POINTS = 16384


def read(vm):
    mi = vm.info()
    keys, counts = vm.Voxels()[:2]
    return vm.Pointcloud(), keys, counts, (mi.n_input_points, mi.n_points, mi.n_voxels, mi.hash_capacity, mi.voxel_size, mi.max_points_per_voxel)


def same(a, b):
    return a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def drop_flags(stored, centre, radius):
    """the contract's flags: ((dx dx + dy dy) + dz dz) <= r2 keeps"""
    dx, dy, dz = stored[:, 0] - centre[0], stored[:, 1] - centre[1], stored[:, 2] - centre[2]
    return (~(((dx * dx + dy * dy) + dz * dz) <= np.float64(radius) * np.float64(radius))).astype(np.uint8)


def transform(points, T):
    """the contract's points: float32(((R_r0 x + R_r1 y) + R_r2 z) + t_r)"""
    p = points.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.ascontiguousarray(np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(np.float32))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(steps, n_log, max_range):
    from elimaloc_amd import _lib, synth
    from elimaloc_amd.registration import Context, Scan, VoxelHashMap
    ctx = Context(0)
    L = _lib.lib()

    def stages():
        ms = (C.c_double * len(STAGES))()
        assert L.elm_map_build_device_stages(ctx._h, ms) == 0
        return {k: round(v, 3) for k, v in zip(STAGES, ms)}

    def pose(k, step_m=0.5, step_deg=2.0):
        T = np.eye(4)
        T[:3, :3] = synth.rot_zyx(0.0, 0.0, np.deg2rad(step_deg) * k)
        T[:3, 3] = (step_m * k, 0.0, 2.1)
        return T

    world = synth.make_world(2_000_000, seed=1001)
    d = world.astype(np.float64) - pose(0)[:3, 3]
    start = world[np.einsum("ij,ij->i", d, d) <= max_range * max_range]
    dev = VoxelHashMap(1.0, 30, ctx, device_build=True)
    dev.AddPoints(start)
    dev._handle()
    host = dev
    out = dict(scan_points=SCAN_POINTS, max_range_m=max_range, start_points=int(dev.info().n_points), steps=[])
    for k in range(1, steps + 2):  # (the first step warms both paths up and is not reported)
        T = pose(k)
        scan = Scan(ctx, synth.make_scan(world, SCAN_POINTS, 500 + k, T_true=T, max_range=max_range)[0])
        centre = T[:3, 3]
        dev_ms, (new_dev, st) = wall(lambda: dev.UpdatedFromScans([scan], T[None], keep_center=centre, keep_radius=max_range, stats=True))
        stage = stages()

        def host_path():
            stored = host.Pointcloud()
            return host._derive(drop_flags(stored, centre, max_range), transform(scan.points(), T))

        host_ms, new_host = wall(host_path)
        assert same(read(new_dev), read(new_host)), k
        ctx.synchronize()
        gicp_ms, _ = wall(lambda: (new_dev.CalPointCovAll(0.4), ctx.synchronize()))
        vgicp_ms, _ = wall(lambda: (new_dev.CalVoxelCovAll(), ctx.synchronize()))
        if k > 1:
            out["steps"].append(dict(points=st["n_points"], base_kept=st["n_base_kept"], base_dropped=st["n_base_dropped"], device_ms=round(dev_ms, 3),
                                     device_stage_ms=stage, device_host_share_ms=round(dev_ms - sum(stage.values()), 3), host_path_ms=round(host_ms, 3),
                                     host_over_device=round(host_ms / dev_ms, 2), point_cov_ms=round(gicp_ms, 3), voxel_cov_ms=round(vgicp_ms, 3)))
        dev, host = new_dev, new_host
        scan.close()
    med = lambda key: round(float(np.median([s[key] for s in out["steps"]])), 3)
    out["median"] = dict(device_ms=med("device_ms"), host_path_ms=med("host_path_ms"), device_host_share_ms=med("device_host_share_ms"),
                         point_cov_ms=med("point_cov_ms"), voxel_cov_ms=med("voxel_cov_ms"),
                         device_kernels_ms=round(float(np.median([sum(s["device_stage_ms"].values()) for s in out["steps"]])), 3))
    # the whole log in one call
    poses = np.stack([pose(k, 0.25, 1.0) for k in range(n_log)])
    scans = [Scan(ctx, synth.make_scan(world, SCAN_POINTS, 2000 + k, T_true=poses[k], max_range=max_range)[0]) for k in range(n_log)]
    empty = VoxelHashMap(1.0, 30, ctx, device_build=True)
    empty.UpdatedFromScans(scans[:2], poses[:2])  # warm-up
    log_ms, (log_dev, st) = wall(lambda: empty.UpdatedFromScans(scans, poses, stats=True))
    stage = stages()

    def log_host():
        xyz = np.concatenate([transform(s.points(), T) for s, T in zip(scans, poses)])
        return empty._derive(None, xyz)

    log_host_ms, log_h = wall(log_host)
    assert same(read(log_dev), read(log_h))
    out["whole_log"] = dict(scans=n_log, input_points=st["n_scan_points"], points=st["n_points"], voxels=st["n_voxels"], device_ms=round(log_ms, 3),
                            device_stage_ms=stage, host_path_ms=round(log_host_ms, 3), host_over_device=round(log_host_ms / log_ms, 2))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--log", type=int, default=256)
    ap.add_argument("--range", type=float, default=55.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_rate.json"))
    a = ap.parse_args()
    line = json.dumps(dict(tool="local_map_rate", **measure(a.steps, a.log, a.range)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
