"""Global relocalization cost on one GPU: prints ONE JSON line and writes it to profiles/reloc_global_rate.json (--out).

The 10 M-point make_field_world map (voxel 1.0, GICP covariances), a 16 384-point scan at 1.8 m above the ground, the default
GlobalRelocConfig (the map's rectangle, 0.5 m x 2 deg).  Reported: lattice size and valid leaves, per-level nodes bounded / kept, leaves
scored, point-evaluations against the exhaustive count (counted points x valid leaves), ms of ground field / search / refinement, the final
pose error against ICP from the truth, the exhaustive scoring of the SAME lattice through ScorePoses (every valid pose, one yaw row per call,
the same counted points: wall-clock ms), and a min-height sweep (--min-heights) of the search.

Kernel times come from separate runs under the kernel trace, one per mode (the modes run only their own part, once, without warm-up):
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o search -- python tools/reloc_global_rate.py --mode search
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o exhaustive -- python tools/reloc_global_rate.py --mode exhaustive

    python tools/reloc_global_rate.py [--points 10000000] [--min-heights 0.5,-inf] [--mode all|search|exhaustive]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from elimaloc_amd import _lib, synth  # noqa: E402
from elimaloc_amd.registration import (Context, GlobalRelocConfig, IcpMethod, Registration, RegistrationConfig, RelocConfig,  # noqa: E402
                                       Scan, VoxelHashMap)


def counted(scan, cfg, T_tilt):
    stride = -(-scan.shape[0] // cfg.max_score_points)
    p = scan[::stride]
    q = p.astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    keep = (x * x + y * y) + z * z <= cfg.score_max_range_m ** 2
    R = T_tilt[:3, :3]
    keep &= ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + T_tilt[2, 3] >= cfg.score_min_height_m
    return p[keep]


def lattice_size(ctx, vm, T_tilt, cfg):
    n = C.c_size_t(0)
    T = np.ascontiguousarray(T_tilt.T).ravel()
    rc = _lib.lib().elm_reloc_global_hypotheses(ctx._h, vm._handle(), T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cfg), None, None, 0,
                                                C.byref(n))
    assert rc == 0, rc
    return n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--mode", choices=("all", "search", "exhaustive"), default="all")
    ap.add_argument("--min-heights", default="0.5,-inf")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "reloc_global_rate.json"))
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
    yaw = math.atan2(T[1, 0], T[0, 0])
    T_tilt = np.eye(4)
    T_tilt[:3, :3] = synth.rot_zyx(0.0, 0.0, -yaw) @ T[:3, :3]
    T_tilt[2, 3] = 1.8
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.GICP), ctx)
    cfg = GlobalRelocConfig()
    out = dict(points=world.shape[0], setup_s=round(setup_s, 1), n_scan=scan.shape[0], mode=a.mode)
    if a.mode == "all":
        reg.RelocalizeGlobal(scan, vm, T_tilt, cfg)  # warm-up: the ground index, scratch
    if a.mode in ("all", "search"):
        t1 = time.perf_counter()
        pose, ok, fit, _, cands, st = reg.RelocalizeGlobal(scan, vm, T_tilt, cfg)
        total_ms = (time.perf_counter() - t1) * 1e3
        ref, ok_ref, _, _ = reg.RunRegister(scan, vm, T)
        dt, dr = synth.pose_error(ref, pose)
        dt0, dr0 = synth.pose_error(T, cands[0]["T0"]) if cands else (None, None)
        out.update(config=dict(step_xy_m=cfg.step_xy_m, step_yaw_deg=cfg.step_yaw_deg, score_min_height_m=cfg.score_min_height_m,
                               top_k=cfg.top_k, pool_min=cfg.pool_min),
                   lattice_poses=st["lattice_poses"], nx=st["nx"], ny=st["ny"], n_yaw=st["n_yaw"], valid_leaves=st["valid_leaves"],
                   n_counted=st["n_counted"], levels=st["levels"], passes=st["passes"], tau=st["tau"],
                   nodes_bounded=st["nodes_bounded"], nodes_kept=st["nodes_kept"], leaves_scored=st["leaves_scored"],
                   leaves_scored_ratio=st["leaves_scored"] / max(st["valid_leaves"], 1), point_evals=st["point_evals"],
                   exhaustive_point_evals=st["n_counted"] * st["valid_leaves"],
                   point_evals_ratio=st["point_evals"] / max(st["n_counted"] * st["valid_leaves"], 1),
                   ms_ground=round(st["ms_ground"], 1), ms_search=round(st["ms_search"], 1), ms_refine=round(st["ms_refine"], 1),
                   total_ms=round(total_ms, 1), is_success=ok, ok_ref=ok_ref, err_vs_icp_from_truth_m=float(dt),
                   err_vs_icp_from_truth_deg=math.degrees(dr), top_candidate_err_m=dt0,
                   top_candidate_err_deg=math.degrees(dr0) if cands else None)
    if a.mode in ("all", "exhaustive"):
        # every valid pose of the lattice through ScorePoses, one yaw row per call: row k = row 0 with R = Rz(k step) R0 (the host's
        # arithmetic), the same counted points
        S = counted(scan, cfg, T_tilt)
        n_yaw = int(math.ceil(360.0 / cfg.step_yaw_deg - 1e-9))
        n = lattice_size(ctx, vm, T_tilt, cfg)
        H0, valid0 = vm.GlobalHypotheses(T_tilt, cfg, max_poses=n // n_yaw)
        H0 = H0[valid0]
        R0 = T_tilt[:3, :3]
        sc = Scan(ctx, S)
        rc = RelocConfig(score_max_range_m=cfg.score_max_range_m)
        vm.ScorePoses(sc, H0[:1024], rc)
        best = 0
        t2 = time.perf_counter()
        for k in range(n_yaw):
            ang = (k * cfg.step_yaw_deg) * (math.pi / 180.0)
            ca, sa = math.cos(ang), math.sin(ang)
            H0[:, 0, :3] = ca * R0[0] - sa * R0[1]
            H0[:, 1, :3] = sa * R0[0] + ca * R0[1]
            best = max(best, int(vm.ScorePoses(sc, H0, rc).max()))
        ex_ms = (time.perf_counter() - t2) * 1e3
        out.update(exhaustive_poses=int(H0.shape[0]) * n_yaw, exhaustive_n_counted=int(S.shape[0]), exhaustive_calls=n_yaw,
                   exhaustive_wall_ms=round(ex_ms, 1), exhaustive_best_score=best)
    if a.mode == "all":
        sweep = {}
        for mh in [float(v) for v in a.min_heights.split(",") if v]:
            c = GlobalRelocConfig(score_min_height_m=mh)
            t3 = time.perf_counter()
            _, ok2, _, _, c2, s2 = reg.RelocalizeGlobal(scan, vm, T_tilt, c)
            e = synth.pose_error(T, c2[0]["T0"]) if c2 else (None, None)
            sweep[str(mh)] = dict(total_ms=round((time.perf_counter() - t3) * 1e3, 1), search_ms=round(s2["ms_search"], 1),
                                  n_counted=s2["n_counted"], leaves_scored=s2["leaves_scored"], passes=s2["passes"], tau=s2["tau"],
                                  ok=ok2, top_err_m=round(float(e[0]), 3) if c2 else None,
                                  top_err_deg=round(math.degrees(e[1]), 3) if c2 else None)
        out.update(min_height_sweep=sweep)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
