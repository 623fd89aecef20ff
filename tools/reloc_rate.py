"""Relocalization cost on one GPU: prints ONE JSON line.

The 10 M-point make_field_world map (voxel 1.0, GICP covariances), a 16 384-point scan, a guess 4 m and 90 deg of yaw off, the default
RelocConfig (21 x 21 xy offsets x 180 yaws = 79 380 hypotheses, 8 192 score points).  Reported: hypotheses, scored points, the lookup form
and bitmap bytes (the library's host rule, mirrored here), wall-clock ms of one ScorePoses call (Python marshalling of the poses, their
upload, bitmap + score kernels, download) and the point-evaluations per second that implies, elm_relocalize in total with its split (one
elm_register_batch over the kept hypotheses, measured on its own / the rest: hypotheses, scores, NMS, scan upload), and the score call at
lds_budget_bytes = 0 / 16 / 32 / 64 KiB and without a bitmap (hash probes only).
Kernel-only times: run under `rocprofv3 --kernel-trace --stats` (k_reloc_bitmap / k_reloc_score<FORM> / k_reloc_sum).

    python tools/reloc_rate.py [--points 10000000] [--reps 7]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elimaloc_amd import synth  # noqa: E402
from elimaloc_amd.registration import (Context, MakeHypotheses, Registration, RegistrationConfig, RelocConfig, Scan,  # noqa: E402
                                       VoxelHashMap)

LDS_BITMAP_MAX = 65536 - 32 * 4 * 4  # elm_reloc.cpp: kLdsBitmapMax


def form_of(S, poses, vs, cfg):
    """The library's choice (elm_reloc.cpp score_impl): key box of the transformed AABB of S over all poses, one key of margin per side."""
    lo, hi = S.min(0).astype(np.float64), S.max(0).astype(np.float64)
    R = poses[:, :3, :3]
    t = poses[:, :3, 3]
    qlo = np.einsum("nrc,nrc->nr", R, np.where(R >= 0, lo, hi)) + t
    qhi = np.einsum("nrc,nrc->nr", R, np.where(R >= 0, hi, lo)) + t
    kmin, kmax = np.trunc(qlo / vs).min(0), np.trunc(qhi / vs).max(0)
    cells = int(np.prod(kmax - kmin + 3))
    nbytes = (cells + 63) // 64 * 8
    form = "lds" if nbytes <= min(cfg.lds_budget_bytes, LDS_BITMAP_MAX) else ("global" if nbytes <= cfg.bitmap_max_bytes else "probe")
    return form, nbytes, [int(x) for x in kmax - kmin + 3]


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = Context(0)
    t0 = time.perf_counter()
    world = synth.make_field_world(a.points, seed=1001)
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(world)
    vm.CalPointCovAll(0.4)
    setup_s = time.perf_counter() - t0
    T = synth.make_pose(world, 7)
    found, gz = vm.FindGroundHeight(T[:2, 3])
    T[2, 3] = gz + 1.8
    scan, _ = synth.make_scan(world, 16384, seed=8, T_true=T)
    G = np.eye(4)
    G[:3, :3] = synth.rot_zyx(0.0, 0.0, math.radians(90.0)) @ T[:3, :3]
    G[:2, 3] = T[:2, 3] + [4.0 / math.sqrt(2.0), -4.0 / math.sqrt(2.0)]
    G[2, 3] = T[2, 3]
    cfg = RelocConfig()
    H = MakeHypotheses(G, cfg)
    stride = -(-scan.shape[0] // cfg.max_score_points)
    sub = scan[::stride]
    d2 = np.einsum("ij,ij->i", sub.astype(np.float64), sub.astype(np.float64))
    S = sub[d2 <= cfg.score_max_range_m ** 2]
    form, nbytes, box = form_of(S, H, 1.0, cfg)
    sc = Scan(ctx, S)
    vm.ScorePoses(sc, H, cfg)  # warm-up (scratch allocation)
    score_ms = median_ms(lambda: vm.ScorePoses(sc, H, cfg), a.reps)
    sweep = {}
    for name, kw in [("lds_0KiB", dict(lds_budget_bytes=0)), ("lds_16KiB", dict(lds_budget_bytes=16 << 10)),
                     ("lds_32KiB", dict(lds_budget_bytes=32 << 10)), ("lds_64KiB", dict(lds_budget_bytes=64 << 10)),
                     ("no_bitmap", dict(lds_budget_bytes=0, bitmap_max_bytes=0))]:
        c = RelocConfig(**kw)
        vm.ScorePoses(sc, H, c)
        sweep[name] = dict(form=form_of(S, H, 1.0, c)[0], score_call_ms=round(median_ms(lambda: vm.ScorePoses(sc, H, c), a.reps), 4))
    reg = Registration(RegistrationConfig(), ctx)
    out = {}

    def reloc():
        out["r"] = reg.Relocalize(scan, vm, G, cfg)
    reloc()
    total_ms = median_ms(reloc, a.reps)
    pose, ok, fit, cov, cands = out["r"]
    scans = [Scan(ctx, scan)] * len(cands)
    T0s = [c["T0"] for c in cands]
    reg.RunRegisterBatch(scans, vm, T0s)
    refine_ms = median_ms(lambda: reg.RunRegisterBatch(scans, vm, T0s), a.reps)
    ref, ok_ref, _, _ = reg.RunRegister(scan, vm, T)
    dt, dr = synth.pose_error(ref, pose)
    evals = float(H.shape[0]) * S.shape[0]
    print(json.dumps(dict(
        tool="reloc_rate", map_points=a.points, map_voxels=int(vm.info().n_voxels), scan_points=int(scan.shape[0]),
        hypotheses=int(H.shape[0]), scored_points=int(S.shape[0]), form=form, bitmap_bytes=int(nbytes), box_keys=box,
        score_call_ms=round(score_ms, 4), point_evals=evals, point_evals_per_s=round(evals / (score_ms * 1e-3), 1),
        relocalize_ms=round(total_ms, 4), split_ms=dict(refine=round(refine_ms, 4), hypotheses_score_nms_upload=round(total_ms - refine_ms, 4)),
        lds_sweep=sweep, kept=len(cands), success=bool(ok), iterations=int(reg.last_relocalize_["iterations"]),
        err_vs_icp_from_truth=dict(m=dt, deg=math.degrees(dr)), best_score=int(cands[0]["score"]) if cands else 0,
        setup_s=round(setup_s, 1))))


if __name__ == "__main__":
    main()
