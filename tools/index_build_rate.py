"""Cell-grid build cost on one GPU, host producer against device producer: prints ONE JSON line and writes it to
profiles/index_build_rate.json (--out).

In one process, per scene -- the lattice world (synth.make_world) and the field world (synth.make_field_world) at 1 M points, the lattice
world at 10 M; voxel 1.0, cap 30 -- wall-clock medians of --reps runs after one warm-up of elm_map_build_neighbourhoods on a fresh map
(built on the device, outside the timed span) with the host index build and with the device index build (elm_map_set_index_build); each
call ends in its own synchronise.  The device producer's stages are timed inside the call with hipEvents (elm_map_index_build_stages);
what is left of its wall clock is the host's share (allocations, the words that come down, the statistics box, the commit).  On the two
1 M worlds the end-to-end edit: prune 1 % of the stored points / add 10 000 points through the device map build, then the first P2P
registration against the new map (which builds its index), with the device index build against the host index build.  The two grids'
read-backs (descriptor, block starts, blocks, slot points, tiles) are asserted equal before any figure is reported.  The yardstick is
the host producer of the same commit, which this feature does not alter.

    python tools/index_build_rate.py [--reps 9] [--big 10000000] [--out profiles/index_build_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("box", "entries_counts", "sort", "block_starts", "pad_fill")


def timed(setup, fn, reps):
    """median wall-clock ms of fn(setup()) over reps runs, after one warm-up (setup is outside the timed span); the last result"""
    ts, out = [], None
    for k in range(reps + 1):
        out = None
        arg = setup()
        t0 = time.perf_counter()
        out = fn(arg)
        if k:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def same_grids(a, b):
    return a["desc"] == b["desc"] and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("start", "blocks", "slot_point", "tiles"))


def measure(reps, big):
    from elimaloc_amd import synth
    from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig, VoxelHashMap
    ctx = Context(0)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)

    def fresh(world, device_index):
        def make():
            vm = VoxelHashMap(1.0, 30, ctx, device_build=True, device_index=device_index)
            vm.AddPoints(world)
            vm._handle()
            ctx.synchronize()
            return vm
        return make

    def index(vm):
        vm.BuildNeighbourhoods()
        return vm

    out = dict(reps=reps, scenes={})
    scenes = [("lattice_1M", lambda: synth.make_world(1_000_000, seed=1001), True), ("field_1M", lambda: synth.make_field_world(1_000_000, seed=1001), True),
              ("lattice_big", lambda: synth.make_world(big, seed=1001), False)]
    for name, make, edits in scenes:
        world = make()
        host_ms, host = timed(fresh(world, False), index, reps)
        dev_ms, dev = timed(fresh(world, True), index, reps)
        assert dev.info().layout_flags & 512 and not host.info().layout_flags & 512, name
        assert same_grids(host.CellGrid(), dev.CellGrid()), name
        st = {k: round(float(v), 3) for k, v in zip(STAGES, dev.IndexBuildStages())}
        mi = host.info()
        r = dict(input_points=int(len(world)), points=int(mi.n_points), cells=int(host.CellGrid()["desc"]["n_start_words"]) - 4,
                 tiled=bool(mi.layout_flags & 4), host_index_ms=round(host_ms, 2), device_index_ms=round(dev_ms, 2), device_stage_ms=st,
                 device_host_share_ms=round(dev_ms - sum(st.values()), 2), host_over_device=round(host_ms / dev_ms, 2))
        if edits:
            n = int(mi.n_points)
            drop = np.zeros(n, np.uint8)
            drop[np.random.default_rng(3).choice(n, n // 100, replace=False)] = 1
            extra = (world[np.random.default_rng(4).choice(len(world), 10_000, replace=False)] + np.float32(0.21)).astype(np.float32)
            scan, T = synth.make_scan(world, 4000, seed=7)
            T0 = np.array(T)
            T0[:3, 3] += (0.2, -0.1, 0.05)

            def edit_and_register(base, what):
                new = base._derive(drop, np.zeros((0, 3), np.float32)) if what == "prune_1pct" else base.Updated(extra)
                pose = reg.RunRegister(scan, new, T0)[0]
                return new, pose

            for what in ("prune_1pct", "add_10000"):
                h_ms, (h_map, h_pose) = timed(lambda: host, lambda b: edit_and_register(b, what), reps)
                d_ms, (d_map, d_pose) = timed(lambda: dev, lambda b: edit_and_register(b, what), reps)
                assert d_map.info().layout_flags & 512 and not h_map.info().layout_flags & 512, (name, what)
                assert same_grids(h_map.CellGrid(), d_map.CellGrid()) and h_pose.tobytes() == d_pose.tobytes(), (name, what)
                r[what + "_to_first_p2p"] = dict(host_index_ms=round(h_ms, 2), device_index_ms=round(d_ms, 2), points=int(d_map.info().n_points),
                                                 host_over_device=round(h_ms / d_ms, 2))
                del h_map, d_map
        out["scenes"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        del host, dev
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build_rate.json"))
    a = ap.parse_args()
    line = json.dumps(dict(tool="index_build_rate", **measure(a.reps, a.big)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
