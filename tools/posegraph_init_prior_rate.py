"""What the pose graph's initialization with priors gives on one GPU: prints ONE JSON line and writes it to
profiles/posegraph_init_prior_rate.json.

The "priors" rings of tools/posegraph_prior_rate.py (N in 1 000, 10 000 and 65 536: no fixed node, the drifted start, the chain
preconditioner), once with a position prior from the truth on every 8th node at the antenna (0.5, -0.2, 1.2) and once with pose priors
on the same nodes.  Reported per ring and kind:
  init_ms            wall clock of one elm_posegraph_initialize_priors from the drifted start, median of --reps
  iterations         of the rotation solve, the gauge-fixed translation solve and the last translation solve
  aligned / deficient / min_align_ratio, applied, cost_before, cost_after
  error_after_init_m the largest position error against the truth after the call; error_after_optimize_m after Optimize as well (the
                     configuration of tools/posegraph_prior_rate.py), with its solves, stop reason and ms
  optimize_alone     Optimize alone from the drifted start, same configuration, on this build; per ring optimize_alone_prior_rate is
                     the row "priors" of profiles/posegraph_prior_rate.json (position priors), when that file is there

    python tools/posegraph_init_prior_rate.py [--reps 5] [--sizes 1000,10000,65536] [--pcg-max 20000]
                                              [--out profiles/posegraph_init_prior_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from posegraph_prior_rate import EVERY, LEVER  # noqa: E402
from posegraph_rate import ring, wall_ms  # noqa: E402


def row_of(pg, truth, start, reps, pcg_max):
    from elimaloc_amd.posegraph import PoseGraphConfig
    worst = lambda poses: float(np.linalg.norm(poses[:, :3, 3] - truth[:, :3, 3], axis=1).max())
    pg.SetPreconditioner("chain")

    def init():
        pg.SetPoses(start)
        return pg.InitializeWithPriors()

    def set_poses():
        pg.SetPoses(start)

    cfg = PoseGraphConfig(pcg_rel_tol=1e-6, pcg_max_iterations=pcg_max, max_iterations=20, step_tol=1e-7)
    set_poses()
    alone_ms, alone = wall_ms(lambda: pg.Optimize(cfg), 1)  # Optimize alone from the drifted start, on this build
    alone_error = worst(pg.Poses())
    init()
    set_ms, _ = wall_ms(set_poses, reps)
    ms, res = wall_ms(init, reps)  # (the last of them leaves its poses in the object)
    after_init = worst(pg.Poses())
    opt_ms, opt = wall_ms(lambda: pg.Optimize(cfg), 1)
    return dict(init_ms=round(ms - set_ms, 4), iterations=[res["rot_iterations"], res["pre_iterations"], res["trans_iterations"]],
                aligned=res["aligned_components"], deficient=res["rank_deficient_components"], min_align_ratio=res["min_align_ratio"],
                applied=res["applied"], cost_before=res["cost_before"], cost_after=res["cost_after"], start_error_m=worst(start),
                error_after_init_m=after_init, error_after_optimize_m=worst(pg.Poses()),
                optimize=dict(solves=opt["solves"], accepted=opt["accepted"], stop_reason=opt["stop_reason"], cost_final=opt["cost_final"],
                              pcg_iterations_total=opt["pcg_iterations_total"], total_ms=opt_ms),
                optimize_alone=dict(solves=alone["solves"], accepted=alone["accepted"], stop_reason=alone["stop_reason"], cost_final=alone["cost_final"],
                                    pcg_iterations_total=alone["pcg_iterations_total"], total_ms=alone_ms, end_error_m=alone_error))


def measure(sizes, reps, pcg_max):
    from elimaloc_amd.posegraph import PoseGraph
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    alone = {}
    parent = os.path.join(ROOT, "profiles", "posegraph_prior_rate.json")
    if os.path.exists(parent):
        alone = json.loads(open(parent).readline())
    out = {}
    for N in sizes:
        truth, start, i, j, Z = ring(N)
        node = np.arange(0, N, EVERY)
        row = dict(nodes=N, edges=len(i), n_priors=len(node))
        for kind in ("position", "pose"):
            pg = PoseGraph(N, len(i), ctx, prior_capacity=len(node))
            pg.AddNodes(start)
            pg.AddEdges(i, j, Z)
            if kind == "position":
                pg.AddPositionPriors(node, truth[node, :3, 3] + truth[node, :3, :3] @ np.array(LEVER), lever=LEVER)
            else:
                pg.AddPriors(node, truth[node])
            row[kind] = row_of(pg, truth, start, reps, pcg_max)
            pg.close()
        if f"ring_{N}" in alone and "priors" in alone[f"ring_{N}"]:
            row["optimize_alone_prior_rate"] = alone[f"ring_{N}"]["priors"]["optimize"]
        out[f"ring_{N}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,65536")
    ap.add_argument("--pcg-max", type=int, default=20000)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_init_prior_rate.json"))
    a = ap.parse_args()
    rows = measure([int(s) for s in a.sizes.split(",")], a.reps, a.pcg_max)
    line = json.dumps(dict(tool="posegraph_init_prior_rate", pcg_max=a.pcg_max, preconditioner="chain", note=a.note, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
