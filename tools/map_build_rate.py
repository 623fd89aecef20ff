"""Map build cost on one GPU, host build against device build: prints ONE JSON line and writes it to profiles/map_build_rate.json (--out).

In one process, wall-clock medians of --reps runs (each ends in the call's own synchronise) of elm_map_build and of elm_map_build_device on
the same input: the lattice world (synth.make_world) at 1 M and 10 M points and the 1 M field world (synth.make_field_world), voxel 1.0,
cap 30.  The device build's stages are timed inside the call with hipEvents on the context's stream (elm_map_build_device_stages); what
is left of its wall clock is the host's share (the slot table, the transfers).  On the two 1 M worlds, two edits, today's path (download
the stored points, edit them in numpy, the host build of everything) against the device path (only the flags / the new points cross the
bus): prune 1 % of the stored points, add 10 000 points.  The two maps' read-backs (points, keys, counts, info) are asserted equal
before anything is reported.  The yardstick is the host path of the same commit: it is the definition of the result.

    python tools/map_build_rate.py [--reps 9] [--big 10000000] [--out profiles/map_build_rate.json]
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


def timed(fn, reps):
    """median wall-clock ms of fn() over reps runs, after one warm-up; the last result"""
    out = fn()
    ts = []
    for _ in range(reps):
        del out
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def read(vm):
    mi = vm.info()
    keys, counts = vm.Voxels()[:2]
    return vm.Pointcloud(), keys, counts, (mi.n_input_points, mi.n_points, mi.n_voxels, mi.hash_capacity, mi.voxel_size, mi.max_points_per_voxel)


def same(a, b):
    return a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def measure(reps, big):
    from elimaloc_amd import _lib, synth
    from elimaloc_amd.registration import Context, VoxelHashMap
    ctx = Context(0)
    L = _lib.lib()

    def build(pts, device):
        vm = VoxelHashMap(1.0, 30, ctx, device_build=device)
        vm.AddPoints(pts)
        vm._handle()
        return vm

    def stages():
        ms = (C.c_double * len(STAGES))()
        assert L.elm_map_build_device_stages(ctx._h, ms) == 0
        return {k: round(v, 3) for k, v in zip(STAGES, ms)}

    out = dict(reps=reps, scenes={})
    scenes = [("lattice_1M", lambda: synth.make_world(1_000_000, seed=1001), True), ("field_1M", lambda: synth.make_field_world(1_000_000, seed=1001), True),
              ("lattice_big", lambda: synth.make_world(big, seed=1001), False)]
    for name, make, edits in scenes:
        world = make()
        host_ms, host = timed(lambda: build(world, False), reps)
        dev_ms, dev = timed(lambda: build(world, True), reps)
        st = stages()
        assert same(read(dev), read(host)), name
        mi = host.info()
        r = dict(input_points=int(len(world)), points=int(mi.n_points), voxels=int(mi.n_voxels), host_build_ms=round(host_ms, 2),
                 device_build_ms=round(dev_ms, 2), device_stage_ms=st, device_host_share_ms=round(dev_ms - sum(st.values()), 2),
                 host_over_device=round(host_ms / dev_ms, 2))
        if edits:
            n = int(mi.n_points)
            drop = np.zeros(n, np.uint8)
            drop[np.random.default_rng(3).choice(n, n // 100, replace=False)] = 1
            extra = (world[np.random.default_rng(4).choice(len(world), 10_000, replace=False)] + np.float32(0.21)).astype(np.float32)

            def prune_host():
                return build(host.Pointcloud()[drop == 0].astype(np.float32), False)

            def add_host():
                return build(np.concatenate([host.Pointcloud().astype(np.float32), extra]), False)

            for edit, today, device in (("prune_1pct", prune_host, lambda: host._derive(drop, np.zeros((0, 3), np.float32))),
                                        ("add_10000", add_host, lambda: host.Updated(extra))):
                t_ms, t_map = timed(today, reps)
                d_ms, d_map = timed(device, reps)
                assert same(read(d_map), read(t_map)), (name, edit)
                r[edit] = dict(host_path_ms=round(t_ms, 2), device_path_ms=round(d_ms, 2), device_stage_ms=stages(), points=int(d_map.info().n_points),
                               host_over_device=round(t_ms / d_ms, 2))
                del t_map, d_map
        out["scenes"][name] = r
        del host, dev
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_build_rate.json"))
    a = ap.parse_args()
    line = json.dumps(dict(tool="map_build_rate", **measure(a.reps, a.big)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
