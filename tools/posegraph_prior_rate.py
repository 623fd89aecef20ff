"""What the pose graph's priors cost on one GPU: prints ONE JSON line and writes it to profiles/posegraph_prior_rate.json.

The rings of tools/posegraph_rate.py (N in 1 000, 10 000 and 65 536: odometry edges, a loop edge every 100 nodes, one edge closing the
ring, the start drifted by 0.2 rad and 5 m over the ring), the chain preconditioner.  Per N two graphs on the same edges:
  "fixed"   node 0 fixed and no prior: the loop-closing row of tools/posegraph_rate.py.  It calls nothing that the priors added, so the
            same rows can be taken on a build from before them (--fixed-only) and compared;
  "priors"  no fixed node; a position prior from the truth on every 8th node at the antenna (0.5, -0.2, 1.2), information the identity.
Reported per graph, as wall clock of the calls (median of --reps):
  linearize_ms   one elm_posegraph_linearize: the linearization, the assembly, one cost evaluation and the read-back of its record
  one_solve_ms   one elm_posegraph_optimize cut to one solve of one PCG iteration: one linearization and assembly, one iteration, one
                 retraction and TWO cost evaluations
  optimize       elm_posegraph_optimize from the drifted start (pcg_rel_tol 1e-6, step_tol 1e-7, at most 20 solves): solves, PCG
                 iterations, stop reason, costs, total ms, the largest position error against the truth before and after
A cost evaluation has no call of its own, so it is not timed alone: one_solve_ms less linearize_ms is one iteration, one retraction and
one cost evaluation (and one more read-back), and the difference of THAT between the two graphs is the priors' share of a cost
evaluation; likewise the difference of linearize_ms is their share of a linearization with its cost.
Kernel-only times: run under a kernel trace (k_pgp_*), e.g. with --sizes 1000.

    python tools/posegraph_prior_rate.py [--reps 5] [--sizes 1000,10000,65536] [--pcg-max 20000] [--fixed-only]
                                         [--out profiles/posegraph_prior_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from posegraph_rate import ring, wall_ms  # noqa: E402

EVERY, LEVER = 8, (0.5, -0.2, 1.2)


def rows_of(pg, truth, start, reps, pcg_max):
    from elimaloc_amd.posegraph import PoseGraphConfig
    worst = lambda poses: float(np.linalg.norm(poses[:, :3, 3] - truth[:, :3, 3], axis=1).max())
    pg.SetPreconditioner("chain")
    pg.SetPoses(start)
    pg.Linearize()
    lin_ms, st = wall_ms(lambda: pg.Linearize(), reps)
    one = PoseGraphConfig(max_iterations=1, pcg_max_iterations=1, pcg_rel_tol=0.0)

    def one_solve():
        pg.SetPoses(start)
        return pg.Optimize(one)

    def set_poses():
        pg.SetPoses(start)

    one_solve()
    one_ms, _ = wall_ms(one_solve, reps)
    set_ms, _ = wall_ms(set_poses, reps)
    pg.SetPoses(start)
    cfg = PoseGraphConfig(pcg_rel_tol=1e-6, pcg_max_iterations=pcg_max, max_iterations=20, step_tol=1e-7)
    opt_ms, res = wall_ms(lambda: pg.Optimize(cfg), 1)
    return dict(linearize_ms=lin_ms, one_solve_ms=round(one_ms - set_ms, 4), cost_at_start=st["cost"],
                optimize=dict(solves=res["solves"], accepted=res["accepted"], rejected=res["rejected"],
                              pcg_iterations_total=res["pcg_iterations_total"], pcg_iterations_per_solve=[t["pcg_iterations"] for t in res["trace"]],
                              stop_reason=res["stop_reason"], cost_initial=res["cost_initial"], cost_final=res["cost_final"], total_ms=opt_ms,
                              start_error_m=worst(start), end_error_m=worst(pg.Poses())))


def measure(sizes, reps, pcg_max, fixed_only):
    from elimaloc_amd.posegraph import PoseGraph
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    out = {}
    for N in sizes:
        truth, start, i, j, Z = ring(N)
        fixed = np.zeros(N, bool)
        fixed[0] = True
        pg = PoseGraph(N, len(i), ctx)
        pg.AddNodes(start, fixed)
        pg.AddEdges(i, j, Z)
        row = dict(nodes=N, edges=len(i), fixed=rows_of(pg, truth, start, reps, pcg_max))
        pg.close()
        if not fixed_only:
            node = np.arange(0, N, EVERY)
            pos = truth[node, :3, 3] + truth[node, :3, :3] @ np.array(LEVER)
            pg = PoseGraph(N, len(i), ctx, prior_capacity=len(node))
            pg.AddNodes(start)
            pg.AddEdges(i, j, Z)
            pg.AddPositionPriors(node, pos, lever=LEVER)
            row["priors"] = dict(n_priors=len(node), **rows_of(pg, truth, start, reps, pcg_max))
            pg.close()
        out[f"ring_{N}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,65536")
    ap.add_argument("--pcg-max", type=int, default=20000)
    ap.add_argument("--fixed-only", action="store_true", help="the rows without priors alone (they run on a build from before the priors too)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_prior_rate.json"))
    a = ap.parse_args()
    rows = measure([int(s) for s in a.sizes.split(",")], a.reps, a.pcg_max, a.fixed_only)
    line = json.dumps(dict(tool="posegraph_prior_rate", pcg_max=a.pcg_max, preconditioner="chain", fixed_only=a.fixed_only, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
