"""Ray-casting cost on one GPU: prints ONE JSON line.

The 10 M-point make_field_world map (voxel 1.0), a 32 x 512 = 16 384-beam synth.lidar_beams model 1.8 m over the ground, the default
RayCastConfig (0.25 m fine cells, walks of 1 .. 100 m), 1 and 16 poses around the truth.  Reported: the first call (fine-table build),
steps per call, wall-clock ms of one RayCast call (pose upload, k_ray_cast + k_ray_sum, download) with and without the per-beam arrays, the
steps per second that implies, the same for every pose block of the sweep (ELM_CHECK=ray_poses=N, read per call), and beside it the
free-space check's samples per second on the scan rendered from the same beams (RenderScan), so that the two can be compared per metre of
ray.
Kernel-only times: run under `rocprofv3 --kernel-trace --stats` (k_ray_cast / k_ray_sum), e.g. with --blocks 1 for one pose block.

    python tools/raycast_rate.py [--points 10000000] [--reps 9] [--blocks 1,4,16]
"""
import argparse
import json
import math
import os
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


def measure(points, reps, blocks):
    from elimaloc_amd import synth
    from elimaloc_amd.registration import Context, FreeSpaceConfig, RayCastConfig, Scan, VoxelHashMap
    ctx = Context(0)
    world = synth.make_field_world(points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    beams = synth.lidar_beams(32, 512)
    rng = np.random.default_rng(1)
    poses = np.tile(T, (16, 1, 1))
    for h in range(1, 16):
        poses[h][:3, :3] = synth.rot_zyx(0.0, 0.0, rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:2, 3] += rng.uniform(-5.0, 5.0, 2)
    cfg = RayCastConfig()
    sc = Scan(ctx, beams)
    os.environ.pop("ELM_CHECK", None)
    t0 = time.perf_counter()
    first = vm.RayCast(sc, poses[:1], cfg)  # builds the fine table
    first_ms = (time.perf_counter() - t0) * 1e3
    out = dict(map_points=points, stored_points=int(vm.info().n_points), beams=int(beams.shape[0]), fine_cells=int(len(vm.FineCells(4))),
               first_call_ms=round(first_ms, 2), truth=first[0])
    base = None
    for blk in ["shipped"] + list(blocks):
        if blk == "shipped":
            os.environ.pop("ELM_CHECK", None)
        else:
            os.environ["ELM_CHECK"] = f"ray_poses={blk}"
        res = {}
        for n in (1, 16):
            full = vm.RayCast(sc, poses[:n], cfg, ranges=True, cells=True, flags=True)
            if n == 16:
                if base is None:
                    base = full
                else:  # the same outputs for every pose block
                    assert full[0] == base[0] and all(np.array_equal(full[1][k], base[1][k]) for k in base[1]), blk
            ms = median_ms(lambda: vm.RayCast(sc, poses[:n], cfg), reps)
            ms_a = median_ms(lambda: vm.RayCast(sc, poses[:n], cfg, ranges=True, cells=True, flags=True), reps)
            st = vm.RayCast(sc, poses[:n], cfg)
            steps = sum(s["n_steps"] for s in st)
            res[f"poses_{n}"] = dict(call_ms=round(ms, 4), call_with_arrays_ms=round(ms_a, 4), steps=steps,
                                     steps_per_s=round(steps / (ms * 1e-3), 1), hit_share=[round(s["n_hit"] / max(s["n_cast"], 1), 3) for s in st])
        out[f"block_{blk}"] = res
    os.environ.pop("ELM_CHECK", None)
    # metres of ray walked up to the hit / the end of the walk at the truth, and the free-space check on the scan these beams render
    _, arr = vm.RayCast(sc, poses[:1], cfg, ranges=True, flags=True)
    walked = np.where(arr["flag"][0] == 1, arr["range_in"][0], cfg.max_range_m) - cfg.min_range_m
    out["metres_walked_truth"] = round(float(walked.sum()), 1)
    rendered = vm.RenderScan(T, beams, cfg, noise=0.01, seed=3)
    fs = FreeSpaceConfig()
    rs = Scan(ctx, rendered)
    fst = vm.CheckFreeSpace(rs, poses, fs)
    f = {}
    for n in (1, 16):
        ms = median_ms(lambda: vm.CheckFreeSpace(rs, poses[:n], fs), reps)
        samples = sum(s["n_samples"] for s in fst[:n])
        f[f"poses_{n}"] = dict(call_ms=round(ms, 4), samples=samples, samples_per_s=round(samples / (ms * 1e-3), 1))
    step = 0.125
    out["free_space_on_rendered_scan"] = dict(points=int(rendered.shape[0]), sample_step_m=step, truth=fst[0], **f,
                                              metres_sampled_truth=round(fst[0]["n_samples"] * step, 1))
    rc = vm.RayCast(rs, poses[:1], cfg)[0]
    out["raycast_of_rendered_scan_truth"] = rc
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--blocks", default="1,4,16")
    a = ap.parse_args()
    blocks = [int(b) for b in a.blocks.split(",") if b]
    print(json.dumps(dict(tool="raycast_rate", **measure(a.points, a.reps, blocks))))


if __name__ == "__main__":
    main()
