"""Pose-graph cost on one GPU: prints ONE JSON line and writes it to profiles/posegraph_rate.json (and a second line, the
initialization's rows, described below).

A ring of N nodes, N in 1 000, 10 000 and 65 536: the truth runs along a circle with 1 m between neighbours; odometry edges k -> k + 1
without noise, a loop edge k -> k + 100 for every k that is a multiple of 100, and one edge closing the ring (N - 1 -> 0), all from the
truth with the identity as information; the start is the odometry integrated with a fixed drift per step (0.2 rad of yaw and 5 m in all
over the whole ring, whatever N), node 0 fixed.  Reported per N, as wall clock of the calls: one elm_posegraph_linearize (median of --reps), one
elm_posegraph_solve at lambda 1e-4 and pcg_rel_tol 1e-6 (its iterations, whether it met the tolerance within --pcg-max, and the ms per
iteration), and one elm_posegraph_optimize from the drifted start with the same PCG settings (solves, PCG iterations in all, stop
reason, costs, total ms, and the largest pose error against the truth).
--preconditioner block_jacobi | chain | both (the default): with both, the block-Jacobi figures stay where they were and the chain
preconditioner's go under "chain" of the same N, with the factor's ms and the apply's ms per iteration.  Those two are wall clock too:
a solve without a stop test is timed at 32 and at 288 iterations under either preconditioner; the difference over 256 is the ms per
iteration, the rest of the 32-iteration call its fixed part; the apply is the chain's ms per iteration less block Jacobi's (whose own
z = M^-1 r is a 6 x 6 product inside k_pg_update<true>), the factor the chain's fixed part less block Jacobi's and less one apply (the z0
of the start).
The linear initialization (elm_posegraph_initialize, rotations first and then translations) has rows of its own, per N and
preconditioner, in a second JSON line written to profiles/posegraph_init_rate.json: from the same drifted start one Initialize with its
defaults (1e-8, at most 50 000 iterations per stage) -- the call's ms, the PCG iterations of both stages, whether it was applied, the
costs and the largest pose error after the initialization alone -- and then the same Optimize as above run after it.  The first line
and its file are what they were.
Kernel-only times: run under a kernel trace (k_pg_*, k_pgc_*, k_pgi_*), e.g. with --sizes 1000.

    python tools/posegraph_rate.py [--reps 5] [--sizes 1000,10000,65536] [--pcg-max 20000] [--preconditioner both]
                                   [--out profiles/posegraph_rate.json] [--init-out profiles/posegraph_init_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rz(a):
    T = np.tile(np.eye(4), (len(a), 1, 1))
    c, s = np.cos(a), np.sin(a)
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1] = c, -s, s, c
    return T


def ring(N):
    a = 2.0 * np.pi * np.arange(N) / N
    radius = N / (2.0 * np.pi)
    truth = rz(a + np.pi / 2.0)
    truth[:, 0, 3], truth[:, 1, 3], truth[:, 2, 3] = radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(3.0 * a)
    k = np.arange(0, N - 100, 100)
    i = np.concatenate([np.arange(N - 1), k, [N - 1]])
    j = np.concatenate([np.arange(1, N), k + 100, [0]])
    Z = np.linalg.inv(truth[i]) @ truth[j]
    D = rz(np.array([0.2 / N]))[0]
    D[:3, 3] = np.array([4.0, -2.5, 1.5]) / N
    start = np.empty_like(truth)
    start[0] = truth[0]
    for n in range(N - 1):
        start[n + 1] = start[n] @ Z[n] @ D
    return truth, start, i, j, Z


def wall_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4), out


def solve_and_optimize(pg, truth, start, pcg_max):
    """the solve and the optimize of the current preconditioner, from the drifted start -> their two records"""
    pg.SetPoses(start)
    pg.Linearize()
    solve_ms, (_, ss) = wall_ms(lambda: pg.Solve(1e-4, 1e-6, pcg_max), 1)
    from elimaloc_amd.posegraph import PoseGraphConfig
    cfg = PoseGraphConfig(pcg_rel_tol=1e-6, pcg_max_iterations=pcg_max, max_iterations=20, step_tol=1e-7)
    opt_ms, res = wall_ms(lambda: pg.Optimize(cfg), 1)
    poses = pg.Poses()
    err = float(np.linalg.norm(poses[:, :3, 3] - truth[:, :3, 3], axis=1).max())
    err0 = float(np.linalg.norm(start[:, :3, 3] - truth[:, :3, 3], axis=1).max())
    return dict(solve=dict(lambda_=1e-4, pcg_rel_tol=1e-6, iterations=ss["iterations"], converged=ss["converged"],
                           rel_residual=ss["rel_residual"], call_ms=solve_ms, ms_per_iteration=round(solve_ms / max(ss["iterations"], 1), 5)),
                optimize=dict(solves=res["solves"], accepted=res["accepted"], rejected=res["rejected"],
                              pcg_iterations_total=res["pcg_iterations_total"],
                              pcg_iterations_per_solve=[t["pcg_iterations"] for t in res["trace"]],
                              stop_reason=res["stop_reason"], cost_initial=res["cost_initial"], cost_final=res["cost_final"],
                              total_ms=opt_ms, start_error_m=err0, end_error_m=err))


def initialize_and_optimize(pg, truth, start, pcg_max):
    """Initialize from the drifted start with the current preconditioner, then the optimize of solve_and_optimize -> one record"""
    from elimaloc_amd.posegraph import PoseGraphConfig
    worst = lambda poses: float(np.linalg.norm(poses[:, :3, 3] - truth[:, :3, 3], axis=1).max())
    pg.SetPoses(start)
    init_ms, init = wall_ms(lambda: pg.Initialize(), 1)
    after_init = worst(pg.Poses())
    cfg = PoseGraphConfig(pcg_rel_tol=1e-6, pcg_max_iterations=pcg_max, max_iterations=20, step_tol=1e-7)
    opt_ms, res = wall_ms(lambda: pg.Optimize(cfg), 1)
    return dict(initialize=dict(call_ms=init_ms, rot_iterations=init["rot_iterations"], trans_iterations=init["trans_iterations"],
                                rot_converged=init["rot_converged"], trans_converged=init["trans_converged"], applied=init["applied"],
                                degenerate_nodes=init["degenerate_nodes"], cost_before=init["cost_before"], cost_after=init["cost_after"],
                                start_error_m=worst(start), error_after_m=after_init),
                optimize=dict(solves=res["solves"], accepted=res["accepted"], rejected=res["rejected"],
                              pcg_iterations_total=res["pcg_iterations_total"], stop_reason=res["stop_reason"],
                              cost_initial=res["cost_initial"], cost_final=res["cost_final"], total_ms=opt_ms, end_error_m=worst(pg.Poses())))


def iteration_and_fixed_ms(pg, start, reps):
    """(ms per iteration, fixed ms of a solve call) of the current preconditioner: solves without a stop test at 32 and 288 iterations"""
    pg.SetPoses(start)
    pg.Linearize()
    pg.Solve(1e-4, 0.0, 32)
    short, _ = wall_ms(lambda: pg.Solve(1e-4, 0.0, 32), reps)
    long_, _ = wall_ms(lambda: pg.Solve(1e-4, 0.0, 288), reps)
    per = (long_ - short) / 256.0
    return per, short - 32.0 * per


def measure(sizes, reps, pcg_max, kinds=("block_jacobi", "chain")):
    from elimaloc_amd.posegraph import PoseGraph
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    out, init_out = {}, {}
    for N in sizes:
        truth, start, i, j, Z = ring(N)
        fixed = np.zeros(N, bool)
        fixed[0] = True
        pg = PoseGraph(N, len(i), ctx)
        pg.AddNodes(start, fixed)
        pg.AddEdges(i, j, Z)
        pg.Linearize()
        lin_ms, st = wall_ms(lambda: pg.Linearize(), reps)
        row = dict(nodes=N, edges=len(i), linearize_ms=lin_ms, cost_at_start=st["cost"])
        if "block_jacobi" in kinds:
            pg.SetPreconditioner("block_jacobi")
            row.update(solve_and_optimize(pg, truth, start, pcg_max))
        if "chain" in kinds:
            pg.SetPreconditioner("chain")
            row["chain"] = solve_and_optimize(pg, truth, start, pcg_max)
            per_c, fixed_c = iteration_and_fixed_ms(pg, start, reps)
            pg.SetPreconditioner("block_jacobi")
            per_b, fixed_b = iteration_and_fixed_ms(pg, start, reps)
            apply_ms = per_c - per_b
            row["chain"].update(iteration_ms=round(per_c, 5), block_jacobi_iteration_ms=round(per_b, 5), apply_ms_per_iteration=round(apply_ms, 5),
                                factor_ms=round(fixed_c - fixed_b - apply_ms, 4))
        out[f"ring_{N}"] = row
        init_out[f"ring_{N}"] = dict(nodes=N, edges=len(i))
        for kind in kinds:  # after every figure of the first line has been taken
            pg.SetPreconditioner(kind)
            init_out[f"ring_{N}"][kind] = initialize_and_optimize(pg, truth, start, pcg_max)
        pg.close()
    return out, init_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,10000,65536")
    ap.add_argument("--pcg-max", type=int, default=20000)
    ap.add_argument("--preconditioner", default="both", choices=("both", "block_jacobi", "chain"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_rate.json"))
    ap.add_argument("--init-out", default=os.path.join(ROOT, "profiles", "posegraph_init_rate.json"))
    a = ap.parse_args()
    kinds = ("block_jacobi", "chain") if a.preconditioner == "both" else (a.preconditioner,)
    rows, init_rows = measure([int(s) for s in a.sizes.split(",")], a.reps, a.pcg_max, kinds)
    line = json.dumps(dict(tool="posegraph_rate", pcg_max=a.pcg_max, preconditioner=a.preconditioner, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    init_line = json.dumps(dict(tool="posegraph_rate", rows="initialize", pcg_max=a.pcg_max, preconditioner=a.preconditioner, **init_rows))
    print(init_line)
    with open(a.init_out, "w") as f:
        f.write(init_line + "\n")


if __name__ == "__main__":
    main()
