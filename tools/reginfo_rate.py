#!/usr/bin/env python3
"""Developer tool (MI355X): what the registration information costs and how well calibrated it is.
  rate         milliseconds per elm_register_information call for 1, 16 and 64 jobs of 131 072-point scans on the 10 M-point bench map,
               per method, beside one RunRegisterBatch of the same jobs in the same process;
  consistency  on the synthetic room of tests/reginfo_cases.py, 200 registrations of independently noised scans from one pose: the mean
               of eps^T Omega eps of the estimate's error eps = Log(T_true^-1 T_est) in the tangent [v; w] under the call's information
               Omega at the estimate, per method and metric.  6 for a calibrated Omega; above 6 the information is overconfident.
Writes profiles/reginfo_rate.json.
    python tools/reginfo_rate.py [--points 10000000] [--scan 131072] [--trials 200] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reginfo_cases as cases  # noqa: E402
from elimaloc_amd import synth  # noqa: E402
from elimaloc_amd.registration import Context, IcpMethod, RegInfoConfig, Registration, RegistrationConfig, Scan, VoxelHashMap  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=10_000_000)
ap.add_argument("--scan", type=int, default=131072)
ap.add_argument("--trials", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None, help="where to write the json (default: profiles/reginfo_rate.json)")
args = ap.parse_args()
METHODS = (IcpMethod.P2P, IcpMethod.GICP, IcpMethod.VGICP, IcpMethod.AVGICP)


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def log_so3(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = float(np.arccos(c))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * w if th < 1e-9 else w * (th / (2.0 * np.sin(th)))


ctx = Context(0)
out = {"tool": "tools/reginfo_rate.py", "map_points": args.points, "scan_points": args.scan, "rate": [], "consistency": []}

# ---- rate
world = synth.make_world(args.points, seed=1001)
vm = VoxelHashMap(1.0, 30, ctx)
vm.AddPoints(world)
vm.CalVoxelCovAll()
vm.CalPointCovAll(0.4)
drawn = []  # eight scans, each at eight different guesses
for k in range(8):
    scan, Tt = synth.make_scan(world, args.scan, seed=2002 + k)
    drawn.append((Scan(ctx, scan), Tt))
jobs = [(drawn[k % 8][0], synth.perturb(drawn[k % 8][1], seed=3003 + k)) for k in range(64)]
for method in METHODS:
    reg = Registration(RegistrationConfig(icp_method=method), ctx)
    for n in (1, 16, 64):
        scans, poses = [j[0] for j in jobs[:n]], np.stack([j[1] for j in jobs[:n]])
        ms_info = median_ms(lambda: reg.Information(scans, vm, poses, raw=True), args.reps)
        ms_reg = median_ms(lambda: reg.RunRegisterBatch(scans, vm, poses), args.reps)
        r = reg.Information(scans, vm, poses)[0]
        row = dict(method=method.name, jobs=n, information_ms=ms_info, register_batch_ms=ms_reg, n_pairs_job0=r["n_pairs"], rank_job0=r["rank"])
        out["rate"].append(row)
        print(row, flush=True)
del jobs, vm

# ---- consistency
room = cases.room_points()
rm = VoxelHashMap(1.0, 30, ctx)
rm.AddPoints(room)
rm.CalVoxelCovAll()
rm.CalPointCovAll(0.4)
T_true = cases.pose(cases.general_rotation(3, 60.0), cases.ROOM_CENTRE + [0.4, -0.3, 0.1])
NOISE = 0.02
scans = [Scan(ctx, cases.scan_of(room, T_true, 700, 9000 + k, noise=NOISE)) for k in range(args.trials)]
guess = np.stack([T_true] * args.trials)
for method in METHODS:
    reg = Registration(RegistrationConfig(icp_method=method, max_iteration=50, icp_termination_threshold_m=1e-4), ctx)
    res = reg.RunRegisterBatch(scans, rm, guess)
    est = np.stack([r["T"] for r in res])
    eps = []
    for T in est:
        d = np.linalg.inv(T_true) @ T
        eps.append(np.concatenate([d[:3, 3], log_so3(d[:3, :3])]))
    eps = np.array(eps)
    for metric in ((0, 1) if method in (IcpMethod.P2P, IcpMethod.GICP) else (0,)):
        info = reg.Information(scans, rm, est, RegInfoConfig(metric=metric))
        nees = np.array([e @ r["information"] @ e for e, r in zip(eps, info)])
        row = dict(method=method.name, metric="plane" if metric else "method", trials=args.trials, noise_m=NOISE, mean_nees=float(nees.mean()),
                   median_nees=float(np.median(nees)), expected=6.0, overconfidence=float(nees.mean() / 6.0),
                   mean_sigma2=float(np.mean([r["sigma2"] for r in info])), rms_trans_m=float(np.sqrt((eps[:, :3] ** 2).sum(1).mean())),
                   rms_rot_rad=float(np.sqrt((eps[:, 3:] ** 2).sum(1).mean())), converged=int(sum(r["is_success"] for r in res)))
        out["consistency"].append(row)
        print(row, flush=True)

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
dest = args.out or os.path.join(ROOT, "profiles", "reginfo_rate.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", dest)
ctx.close()
