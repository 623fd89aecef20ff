"""Map-evidence cost on one GPU: prints ONE JSON line.

The 10 M-point make_field_world map (voxel 1.0), the scan that a 32 x 512 = 16 384-beam synth.lidar_beams model 1.8 m over the ground
renders on it (RenderScan), the default EvidenceConfig (0.25 m fine cells, walks from 1 m to a margin before the end point).  Reported:
elm_evidence_create (the counter prefix built from the fine table), one observation (wall-clock ms of one Accumulate call: job upload,
k_evid_walk + k_evid_sum, stats download; with and without the per-beam events), a batch of 64 observations (the same scan at 64 poses
around the truth), the steps per second both imply, the download of the counters and the stale-point flags, and beside them k_ray_cast at
one pose on the same beams as the yardstick for steps per second.
Kernel-only times: run under a kernel trace (k_evid_walk / k_evid_sum / k_ray_cast), e.g. with --reps 1.

    python tools/evidence_rate.py [--points 10000000] [--reps 9] [--batch 64]
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


def measure(points, reps, batch):
    from elimaloc_amd import synth
    from elimaloc_amd.registration import Context, EvidenceConfig, RayCastConfig, Scan, VoxelHashMap
    ctx = Context(0)
    world = synth.make_field_world(points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    beams = synth.lidar_beams(32, 512)
    rc = RayCastConfig()
    rendered = vm.RenderScan(T, beams, rc, noise=0.01, seed=3)  # (builds the fine table)
    rng = np.random.default_rng(1)
    poses = np.tile(T, (batch, 1, 1))
    for h in range(1, batch):
        poses[h][:3, :3] = synth.rot_zyx(0.0, 0.0, rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:2, 3] += rng.uniform(-5.0, 5.0, 2)
    cfg = EvidenceConfig()
    sc = Scan(ctx, rendered)
    t0 = time.perf_counter()
    ev = vm.Evidence()
    create_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    first = ev.Accumulate(sc, T, cfg)
    first_ms = (time.perf_counter() - t0) * 1e3
    out = dict(map_points=points, stored_points=int(vm.info().n_points), fine_cells=int(len(vm.FineCells(4))), scan_points=int(rendered.shape[0]),
               create_ms=round(create_ms, 2), first_accumulate_ms=round(first_ms, 3), truth=first)
    ms = median_ms(lambda: ev.Accumulate(sc, T, cfg), reps)
    ms_e = median_ms(lambda: ev.Accumulate(sc, T, cfg, events=True), reps)
    out["one_observation"] = dict(call_ms=round(ms, 4), call_with_events_ms=round(ms_e, 4), steps=first["n_steps"],
                                  steps_per_s=round(first["n_steps"] / (ms * 1e-3), 1))
    jobs = [sc] * batch
    st = ev.Accumulate(jobs, poses, cfg)
    steps = sum(s["n_steps"] for s in st)
    ms_b = median_ms(lambda: ev.Accumulate(jobs, poses, cfg), reps)
    out[f"batch_{batch}"] = dict(call_ms=round(ms_b, 4), steps=steps, steps_per_s=round(steps / (ms_b * 1e-3), 1),
                                 through_events=sum(s["n_through_events"] for s in st), end_hit=sum(s["n_end_hit"] for s in st),
                                 observing=sum(s["n_observing"] for s in st))
    out["counts_download_ms"] = round(median_ms(ev.Counts, 3), 2)
    out["stale_points_ms"] = round(median_ms(ev.StalePoints, 3), 2)
    t, h = ev.Counts()
    out["cells_counted"] = int(((t > 0) | (h > 0)).sum())
    out["stale_points"] = int(ev.StalePoints().sum())
    # the yardstick: the ray cast of the model's beams at the truth (walks to 100 m), and of the rendered scan itself
    for name, b in (("raycast_beams", Scan(ctx, beams)), ("raycast_rendered_scan", sc)):
        r = vm.RayCast(b, T[None], rc)[0]
        ms_r = median_ms(lambda: vm.RayCast(b, T[None], rc), reps)
        out[name] = dict(call_ms=round(ms_r, 4), steps=r["n_steps"], steps_per_s=round(r["n_steps"] / (ms_r * 1e-3), 1))
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    print(json.dumps(dict(tool="evidence_rate", **measure(a.points, a.reps, a.batch))))


if __name__ == "__main__":
    main()
