"""Place-recognition cost on one GPU: prints ONE JSON line and writes it to profiles/places_rate.json.

The default PlaceConfig (16 rings x 8 layers = 128 words).  Reported, as medians over --reps calls: describing 64 scans of 16 384 points
in one elm_places_describe call (job table up, k_pl_describe + k_pl_bits, words and stats down), and one query descriptor against
databases of 1 000 and 10 000 random entries (elm_places_match_words: words up, k_pl_bits + k_pl_match + k_pl_topk, 16 candidates
down).  Each as the wall clock of the call and as the time between two events recorded on the context's stream around it (the span the
device saw, without the call's own host work before its first and after its last operation).
Kernel-only times: run under a kernel trace (k_pl_describe / k_pl_bits / k_pl_match / k_pl_topk), e.g. with --reps 1.

    python tools/places_rate.py [--reps 21] [--scans 64] [--points 16384] [--out profiles/places_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, fn, reps):
    """(median wall ms, median event ms) of fn() over reps calls, after one warm-up call"""
    import torch
    stream = torch.cuda.ExternalStream(ctx.stream)
    fn()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        e1.record(stream)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    return round(float(np.median(wall)), 4), round(float(np.median(dev)), 4)


def random_words(n, W, density, seed):
    rng = np.random.default_rng(seed)
    bits = (rng.random((n, W, 64)) < density).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little").view(np.uint64).reshape(n, W))


def measure(reps, n_scans, n_points):
    from elimaloc_amd.places import PlaceConfig, PlaceDatabase
    from elimaloc_amd.registration import Context, Scan
    ctx = Context(0)
    rng = np.random.default_rng(1)
    scans = []
    for _ in range(n_scans):
        az, r = rng.uniform(-np.pi, np.pi, n_points), rng.uniform(0.0, 50.0, n_points)
        scans.append(Scan(ctx, np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-4.0, 10.0, n_points)], axis=1).astype(np.float32)))
    db = PlaceDatabase(PlaceConfig(), 10000, ctx)
    words, st = db.Describe(scans)
    wall, dev = timed(ctx, lambda: db.Describe(scans), reps)
    out = dict(n_words=db.n_words, describe=dict(scans=n_scans, points_per_scan=n_points, call_ms=wall, event_ms=dev,
                                                 points_per_s=round(n_scans * n_points / (wall * 1e-3), 1),
                                                 mean_used=float(np.mean([s["n_used"] for s in st])), mean_bits=float(np.mean([s["n_bits"] for s in st]))))
    entries = random_words(10000, db.n_words, 0.2, 2)
    for n in (1000, 10000):
        db.Reset()
        db.AddDescriptors(entries[:n], np.arange(n))
        q = entries[n // 2]
        got = db.Match(q, top_k=16)
        assert got[0]["entry"] == n // 2 and got[0]["dice_q16"] == 65536
        wall, dev = timed(ctx, lambda: db.Match(q, top_k=16), reps)
        out[f"query_{n}"] = dict(entries=n, top_k=16, call_ms=wall, event_ms=dev, popcounts=n * 64 * db.n_words * 2)
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "places_rate.json"))
    a = ap.parse_args()
    line = json.dumps(dict(tool="places_rate", **measure(a.reps, a.scans, a.points)))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
