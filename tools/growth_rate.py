"""Map-growth cost on one GPU: prints ONE JSON line.

The 10 M-point make_field_world map (voxel 1.0), the scan that a 32 x 512 = 16 384-beam synth.lidar_beams model 1.8 m over the ground
renders on it (RenderScan, 5 cm of noise so that end points leave the mapped cells), the default GrowthConfig (0.25 m fine cells, clearance
1).  Reported: elm_growth_create (the tables allocated and cleared), one observation (wall-clock ms of one Accumulate call: job upload,
k_grow_end + k_grow_walk + k_grow_sum, stats and count download; with and without the per-beam events), a batch of 64 observations (the
same scan at 64 poses around the truth, one call), the steps per second both imply, the download of the cells and the appeared points, and
beside them the map evidence's k_evid_walk on the same jobs as the yardstick for steps per second (the same walk against the map's own
table).
Kernel-only times: run under a kernel trace (k_grow_end / k_grow_walk / k_grow_sum / k_evid_walk), e.g. with --reps 1.

    python tools/growth_rate.py [--points 10000000] [--reps 9] [--batch 64]
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
    from elimaloc_amd.registration import Context, EvidenceConfig, GrowthConfig, RayCastConfig, Scan, VoxelHashMap
    ctx = Context(0)
    world = synth.make_field_world(points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    beams = synth.lidar_beams(32, 512)
    rendered = vm.RenderScan(T, beams, RayCastConfig(), noise=0.05, seed=3)  # (builds the fine table)
    rng = np.random.default_rng(1)
    poses = np.tile(T, (batch, 1, 1))
    for h in range(1, batch):
        poses[h][:3, :3] = synth.rot_zyx(0.0, 0.0, rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:2, 3] += rng.uniform(-5.0, 5.0, 2)
    cfg = GrowthConfig()
    sc = Scan(ctx, rendered)
    n = int(rendered.shape[0])
    capacity = n * (batch + 2)  # a call needs room for one candidate per beam; the table is reset between the timed calls
    t0 = time.perf_counter()
    g = vm.Growth(capacity)
    create_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    first = g.Accumulate(sc, T, cfg)
    first_ms = (time.perf_counter() - t0) * 1e3
    out = dict(map_points=points, stored_points=int(vm.info().n_points), scan_points=n, capacity=capacity, create_ms=round(create_ms, 2),
               first_accumulate_ms=round(first_ms, 3), truth=first, candidates_after_one=g.Count())

    def timed(call):  # the candidate count grows with every call and the guard counts beams: reset outside the clock
        ts = []
        for _ in range(reps):
            g.Reset()
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    ms = timed(lambda: g.Accumulate(sc, T, cfg))
    ms_e = timed(lambda: g.Accumulate(sc, T, cfg, events=True))
    out["one_observation"] = dict(call_ms=round(ms, 4), call_with_events_ms=round(ms_e, 4), steps=first["n_steps"],
                                  steps_per_s=round(first["n_steps"] / (ms * 1e-3), 1))
    jobs = [sc] * batch
    g.Reset()
    st = g.Accumulate(jobs, poses, cfg)
    steps = sum(s["n_steps"] for s in st)
    ms_b = timed(lambda: g.Accumulate(jobs, poses, cfg))
    out[f"batch_{batch}"] = dict(call_ms=round(ms_b, 4), steps=steps, steps_per_s=round(steps / (ms_b * 1e-3), 1),
                                 through_events=sum(s["n_through_events"] for s in st), end_hit=sum(s["n_end_hit"] for s in st),
                                 end_near=sum(s["n_end_near"] for s in st), end_new=sum(s["n_end_new"] for s in st),
                                 dropped=sum(s["n_dropped"] for s in st), observing=sum(s["n_observing"] for s in st), candidates=g.Count())
    out["cells_download_ms"] = round(median_ms(g.Cells, 3), 2)
    out["appeared_points_ms"] = round(median_ms(g.AppearedPoints, 3), 2)
    out["appeared_cells"] = int(len(g.AppearedPoints()))
    # the yardstick: the map evidence's walk on the same jobs
    ev = vm.Evidence()
    ec = EvidenceConfig()
    e1 = ev.Accumulate(sc, T, ec)
    ms_1 = median_ms(lambda: ev.Accumulate(sc, T, ec), reps)
    eb = ev.Accumulate(jobs, poses, ec)
    ms_eb = median_ms(lambda: ev.Accumulate(jobs, poses, ec), reps)
    esteps = sum(s["n_steps"] for s in eb)
    out["evidence_one_observation"] = dict(call_ms=round(ms_1, 4), steps=e1["n_steps"], steps_per_s=round(e1["n_steps"] / (ms_1 * 1e-3), 1))
    out[f"evidence_batch_{batch}"] = dict(call_ms=round(ms_eb, 4), steps=esteps, steps_per_s=round(esteps / (ms_eb * 1e-3), 1))
    out["walk_steps_per_s_vs_evidence"] = round(out[f"batch_{batch}"]["steps_per_s"] / out[f"evidence_batch_{batch}"]["steps_per_s"], 3)
    ev.close()
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    print(json.dumps(dict(tool="growth_rate", **measure(a.points, a.reps, a.batch))))


if __name__ == "__main__":
    main()
