"""Growth-objects cost on one GPU: prints ONE JSON line and writes it to profiles/objects_rate.json (--out).

The table that tools/growth_rate.py fills: the 10 M-point make_field_world map (voxel 1.0), the scan that a 32 x 512-beam model 1.8 m over
the ground renders on it (5 cm of noise), accumulated at 64 poses around the truth in one call -- about 156 k candidate cells.  For two
rules, the default one (the appeared cells: a few thousand members) and {1, 0, 26, 1} (every candidate is a member), the wall-clock median
of --reps runs of: elm_growth_find_objects (the labelling on the device, the listed records down, their ranks up), the objects download,
elm_growth_cell_objects, elm_growth_beam_objects for one scan; and, in the same run, what a caller pays today for the same answer:
elm_growth_cells plus the labelling of the numpy mirror (tests/objects_ref.py) on the host.  The device result is checked against the
mirror's on the way.

    python tools/objects_rate.py [--points 10000000] [--reps 9] [--batch 64] [--out profiles/objects_rate.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the mirror lives with the tests


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def measure(points, reps, batch):
    import objects_ref
    from elimaloc_amd import synth
    from elimaloc_amd.registration import Context, GrowthConfig, GrowthObjectRule, RayCastConfig, Scan, VoxelHashMap
    ctx = Context(0)
    world = synth.make_field_world(points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    rendered = vm.RenderScan(T, synth.lidar_beams(32, 512), RayCastConfig(), noise=0.05, seed=3)
    rng = np.random.default_rng(1)
    poses = np.tile(T, (batch, 1, 1))
    for h in range(1, batch):
        poses[h][:3, :3] = synth.rot_zyx(0.0, 0.0, rng.uniform(-math.pi, math.pi)) @ T[:3, :3]
        poses[h][:2, 3] += rng.uniform(-5.0, 5.0, 2)
    cfg = GrowthConfig()
    sc = Scan(ctx, rendered)
    n = int(rendered.shape[0])
    g = vm.Growth(n * (batch + 2))
    g.Accumulate([sc] * batch, poses, cfg)
    out = dict(map_points=points, scan_points=n, capacity=g.capacity, candidates=g.Count())
    for name, kw in (("default_rule", {}), ("every_candidate", dict(min_hit=1, hit_per_through=0, connectivity=26, min_cells=1))):
        rule = GrowthObjectRule(**kw)
        t0 = time.perf_counter()
        st = g.FindObjects(rule)
        first_ms = (time.perf_counter() - t0) * 1e3  # (the first call of all allocates the object state)
        r = dict(stats=st, first_find_objects_ms=round(first_ms, 3), find_objects_ms=round(median_ms(lambda: g.FindObjects(rule), reps), 4),
                 objects_ms=round(median_ms(g.Objects, reps), 4), cell_objects_ms=round(median_ms(g.CellObjects, reps), 3),
                 beam_objects_ms=round(median_ms(lambda: g.BeamObjects(sc, poses[1], cfg), reps), 4))
        # today's way: the whole table down, then the labelling on the host
        host = {}

        def today():
            cells, hit, through, _ = g.Cells()
            host["m"] = objects_ref.Objects(cells, hit, through, objects_ref.Rule(**kw))

        r["cells_plus_host_labelling_ms"] = round(median_ms(today, max(reps // 3, 1)), 2)
        r["cells_download_ms"] = round(median_ms(g.Cells, max(reps // 3, 1)), 2)
        m, objs = host["m"], g.Objects()
        same = st == m.stats and all(np.array_equal(objs[f], m.objects[f]) for f in objects_ref.OBJECT_FIELDS)
        same = same and np.array_equal(g.CellObjects(), m.cell_map) and np.array_equal(g.BeamObjects(sc, poses[1], cfg), m.beams(cfg, 0.25, sc.points(), poses[1]))
        r["equals_mirror"] = bool(same)
        r["beams_on_objects"] = int((g.BeamObjects(sc, poses[1], cfg) >= 0).sum())
        r["host_over_device"] = round(r["cells_plus_host_labelling_ms"] / (r["find_objects_ms"] + r["objects_ms"]), 1)
        out[name] = r
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_rate.json"))
    a = ap.parse_args()
    line = json.dumps(dict(tool="objects_rate", **measure(a.points, a.reps, a.batch)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
