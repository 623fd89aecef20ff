"""Free-space check cost on one GPU: prints ONE JSON line.

The 10 M-point make_field_world map (voxel 1.0), a 16 384-point scan 1.8 m over the ground, the default FreeSpaceConfig (0.25 m fine cells,
0.125 m steps), 1 and 16 poses around the truth.  Reported: the fine table's build (host ms, device bytes, coarse cells are the table's
keys), samples per call, wall-clock ms of one CheckFreeSpace call (pose upload, k_free_rays + k_free_sum, download) with and without the
per-ray array, the samples per second that implies, and the same with ELM_CHECK=free_wave (a wave per ray: the lane-balancing A/B) when
--form both runs it in a child process.
Kernel-only times: run under `rocprofv3 --kernel-trace --stats` (k_free_rays<FORM> / k_free_sum).

    python tools/free_space_rate.py [--points 10000000] [--reps 9] [--form lane|wave|both]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def measure(points, reps):
    from elimaloc_amd import synth
    from elimaloc_amd.registration import Context, FreeSpaceConfig, Scan, VoxelHashMap
    ctx = Context(0)
    world = synth.make_field_world(points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    scan, _ = synth.make_scan(world, 16384, seed=8, T_true=T)
    rng = np.random.default_rng(1)
    poses = np.tile(T, (16, 1, 1))
    for h in range(1, 16):
        poses[h][:3, :3] = synth.rot_zyx(0.0, 0.0, rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:2, 3] += rng.uniform(-5.0, 5.0, 2)
    cfg = FreeSpaceConfig()
    sc = Scan(ctx, scan)
    t0 = time.perf_counter()
    first = vm.CheckFreeSpace(sc, poses[:1], cfg)  # builds the fine table
    first_ms = (time.perf_counter() - t0) * 1e3
    out = dict(form=os.environ.get("ELM_CHECK", "") or "lane", map_points=points, stored_points=int(vm.info().n_points), scan_points=int(scan.shape[0]),
               fine_cells=int(len(vm.FineCells(4))), first_call_ms=round(first_ms, 2), truth=first[0])
    for n in (1, 16):
        vm.CheckFreeSpace(sc, poses[:n], cfg, hits=True)
        ms = median_ms(lambda: vm.CheckFreeSpace(sc, poses[:n], cfg), reps)
        ms_h = median_ms(lambda: vm.CheckFreeSpace(sc, poses[:n], cfg, hits=True), reps)
        st = vm.CheckFreeSpace(sc, poses[:n], cfg)
        samples = sum(s["n_samples"] for s in st)
        out[f"poses_{n}"] = dict(call_ms=round(ms, 4), call_with_hits_ms=round(ms_h, 4), samples=samples,
                                 samples_per_s=round(samples / (ms * 1e-3), 1), pierced_share=[round(s["pierced_share"], 3) for s in st])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--form", choices=("lane", "wave", "both"), default="lane")
    a = ap.parse_args()
    if a.form == "both":  # each form in a fresh child process (the switch is read per call, the table build is paid per process)
        res = {}
        for form in ("lane", "wave"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--points", str(a.points), "--reps", str(a.reps), "--form", form],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                sys.exit(r.returncode)
            res[form] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(dict(tool="free_space_rate", **res)))
        return
    if a.form == "wave":
        os.environ["ELM_CHECK"] = "free_wave"
    else:
        os.environ.pop("ELM_CHECK", None)
    print(json.dumps(dict(tool="free_space_rate", **measure(a.points, a.reps))))


if __name__ == "__main__":
    main()
