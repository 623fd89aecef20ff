"""The covariance model of the loop-consistency check beside the scalar one, on one GPU: prints ONE JSON line and writes it to
profiles/loop_covariance_rate.json.

The fixture of tools/loop_consistency_rate.py (4 096 poses on four laps, L loops of which half are true, L in 256, 2 048 and 16 384), at
that tool's own odometry noise (0.01 m, 1e-4 rad per step) and at the drift its text names as the scalar model's limit (0.02 m, 0.002 rad
per step).  Per noise and L three calls on the same loops: elm_loops_consistency with its shipped q (q_t = 0.05^2, q_r = 0.002^2),
elm_loops_consistency with the honest q (the step's own variances), and elm_loopcov_consistency with the honest Q = diag(sigma_t^2 x 3,
sigma_r^2 x 3) and Sigma = diag(0.03^2 x 3, 0.003^2 x 3), all at gamma = 16.81.  Reported per call: the true and the false loops among the
members, the clique's size and steps, and the device times of its parts (the calls' own stream events, median of --reps).  Nothing here
is a requirement; the figures are recorded.

    python tools/loop_covariance_rate.py [--reps 3] [--sizes 256,2048,16384] [--out profiles/loop_covariance_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import loop_consistency_rate as scalar_tool  # noqa: E402

GAMMA = 16.81
LOOP_SIGMA_T, LOOP_SIGMA_R = 0.03, 0.003
NOISES = dict(shipped=(0.01, 1e-4), drift=(0.02, 0.002))  # name -> (sigma_t m, sigma_r rad) per step


def _row(res, is_true, wall, parts):
    kept = res["members"]
    row = dict(size=res["size"], steps=res["steps"], adjacent_pairs=res["adjacent_pairs"], true_kept=int(is_true[kept].sum()),
               false_kept=int((~is_true[kept]).sum()), call_ms=float(np.median(wall)))
    row.update({k: float(np.median(v)) for k, v in parts.items()})
    if "non_finite_pairs" in res:
        row["non_finite_pairs"] = res["non_finite_pairs"]
    return row


def _timed(call, reps, keys):
    call()  # warm-up
    wall, parts = [], {k: [] for k in keys}
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        for k in keys:
            parts[k].append(res[k])
    return res, wall, parts


def measure(sizes, reps):
    from elimaloc_amd.loops import LoopConsistency, LoopConsistencyConfig, LoopConsistencyCov
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    out = {}
    Sigma = np.diag([LOOP_SIGMA_T ** 2] * 3 + [LOOP_SIGMA_R ** 2] * 3)
    for name, (sigma_t, sigma_r) in NOISES.items():
        Q = np.diag([sigma_t ** 2] * 3 + [sigma_r ** 2] * 3)
        for L in sizes:
            poses, a, b, Z, is_true = scalar_tool.fixture(L, sigma_r=sigma_r, sigma_t=sigma_t)
            rows = dict(loops=L, poses=scalar_tool.N_POSES, sigma_t=sigma_t, sigma_r=sigma_r, true_loops=int(is_true.sum()))
            for key, cfg in (("scalar_shipped_q", LoopConsistencyConfig(**scalar_tool.CFG)),
                             ("scalar_honest_q", LoopConsistencyConfig(q_t=sigma_t ** 2, q_r=sigma_r ** 2, gamma=GAMMA))):
                res, wall, parts = _timed(lambda: LoopConsistency(poses, a, b, Z, scalar_tool.VAR_T, scalar_tool.VAR_R, cfg, ctx), reps,
                                          ("adjacency_ms", "greedy_ms"))
                rows[key] = _row(res, is_true, wall, parts)
            res, wall, parts = _timed(lambda: LoopConsistencyCov(poses, a, b, Z, Sigma, Q, LoopConsistencyConfig(gamma=GAMMA), ctx), reps,
                                      ("chain_ms", "adjacency_ms", "greedy_ms"))
            rows["covariance"] = _row(res, is_true, wall, parts)
            rows["covariance"]["adjacency_ns_per_pair"] = 1e6 * rows["covariance"]["adjacency_ms"] / (L * L)
            out[f"{name}_loops_{L}"] = rows
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="256,2048,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_covariance_rate.json"))
    a = ap.parse_args()
    rows = measure([int(s) for s in a.sizes.split(",")], a.reps)
    line = json.dumps(dict(tool="loop_covariance_rate", reps=a.reps, gamma=GAMMA, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
