"""Cost of the pose graph's covariance columns on one GPU: prints ONE JSON line and writes it to profiles/posegraph_cov_rate.json.

The rings of tools/posegraph_rate.py (1 000 and 10 000 nodes; odometry, a loop edge every 100 nodes, the closing edge, identity
informations, node 0 fixed), linearized at the drifted start.  Per ring and preconditioner: one elm_posegraph_solve at lambda = 0 and the
covariance call's tolerance (its iterations and the call's wall-clock ms, median of --reps), then elm_posegraph_covariance for 1, 10 and
100 nodes spread evenly over the ring (6, 60 and 600 columns: 1, 1 and 10 groups of 64 lanes): the columns' iterations, the call's
ms_device (stream events around the device work) and wall-clock ms, the ms per column, and the figure of interest: ms per column over
ms per Solve (one Solve is what one column would cost if the columns were chained through elm_posegraph_solve), under block Jacobi
and under the chain preconditioner.

    python tools/posegraph_cov_rate.py [--reps 3] [--sizes 1000,10000] [--requests 1,10,100] [--tol 1e-10] [--pcg-max 20000]
                                       [--out profiles/posegraph_cov_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posegraph_rate import ring, wall_ms  # noqa: E402


def measure(sizes, requests, reps, tol, pcg_max):
    from elimaloc_amd._lib import ElmError
    from elimaloc_amd.posegraph import PoseGraph, PoseGraphCovConfig
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    out = {}
    cfg = PoseGraphCovConfig(pcg_rel_tol=tol, pcg_max_iterations=pcg_max)
    for N in sizes:
        truth, start, i, j, Z = ring(N)
        fixed = np.zeros(N, bool)
        fixed[0] = True
        pg = PoseGraph(N, len(i), ctx)
        pg.AddNodes(start, fixed)
        pg.AddEdges(i, j, Z)
        pg.Linearize()
        row = dict(nodes=N, edges=len(i))
        for kind in ("block_jacobi", "chain"):
            pg.SetPreconditioner(kind)
            pg.Solve(0.0, tol, pcg_max)
            solve_ms, (_, ss) = wall_ms(lambda: pg.Solve(0.0, tol, pcg_max), reps)
            rec = dict(solve=dict(iterations=ss["iterations"], converged=ss["converged"], call_ms=solve_ms,
                                  ms_per_iteration=round(solve_ms / max(ss["iterations"], 1), 5)))
            for m in requests:
                nodes = (1 + (np.arange(m) * (N - 1)) // m).astype(np.int32)  # never the fixed node 0
                try:
                    pg.Covariance(nodes, None, cfg)
                    call_ms, (_, _, info) = wall_ms(lambda: pg.Covariance(nodes, None, cfg), reps)
                except ElmError as e:
                    rec[f"request_{m}"] = dict(refused=str(e))
                    continue
                its = info["iterations"]
                rec[f"request_{m}"] = dict(columns=info["n_columns"], converged=info["n_converged"], passes=info["passes"],
                                           iterations_min=int(its.min()), iterations_max=int(its.max()), ms_device=round(info["ms_device"], 4),
                                           call_ms=call_ms, scratch_bytes=info["scratch_bytes"],
                                           ms_per_column=round(info["ms_device"] / info["n_columns"], 5),
                                           ms_per_iteration=round(info["ms_device"] / max(int(its.max()), 1), 5),
                                           column_over_solve=round(info["ms_device"] / info["n_columns"] / solve_ms, 5))
            row[kind] = rec
        out[f"ring_{N}"] = row
        pg.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--requests", default="1,10,100")
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--pcg-max", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_cov_rate.json"))
    a = ap.parse_args()
    rows = measure([int(s) for s in a.sizes.split(",")], [int(s) for s in a.requests.split(",")], a.reps, a.tol, a.pcg_max)
    line = json.dumps(dict(tool="posegraph_cov_rate", tol=a.tol, pcg_max=a.pcg_max, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
