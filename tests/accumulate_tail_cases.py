"""The registrations of tests/test_accumulate_tail.py, shared with tools/record_tail_golden.py (which runs them on the PARENT's
library and writes tests/golden/accumulate_tail_parent.npz).  Everything is seeded; nothing here asserts.

The cases aim at the parts of an accumulate workgroup that carry no arithmetic of their own -- the head (block -> scan, the two
early exits), the queue of undecided points with its stage-2 results, the block reduction's DPP steps, the expansion of the 18
reduced P2P values into the packed record -- so that a change of those parts can be held to "not one bit moved"."""
import numpy as np

from elimaloc_amd import synth

P2P, GICP, VGICP = 0, 1, 2
P2P_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)  # one lane; wavefront and workgroup edges; a second / fourth workgroup, the last one partial
WORLD_POINTS = 30000
PATCH_Z = 10.02      # the sparse patch: a horizontal sheet just above a cell face (cells of 0.5 m)
LIFT = 0.37          # the lifted scan: 0.37 m above the sheet
QUEUE_MIN = 65       # more undecided points than one pass of stage 2 serves (64 groups of four lanes per workgroup)


def world():
    return synth.make_world(WORLD_POINTS, seed=4101)


def sparse_patch():
    """About six points per square metre on one sheet, well inside positive coordinates (stored and queried voxel keys agree there)."""
    rng = np.random.default_rng(4102)
    xy = rng.uniform(20.0, 28.0, size=(384, 2))
    z = PATCH_Z + rng.normal(0.0, 0.004, size=384)
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


def lifted_scan():
    """256 points (one workgroup) LIFT above the sheet: the nearest map point of most of them lies beyond the distance to an open face
    of their 2 x 2 x 2 block of cells, so stage 1 cannot certify it and the point is queued for stage 2."""
    rng = np.random.default_rng(4103)
    xy = rng.uniform(21.0, 27.0, size=(256, 2))
    return np.concatenate([xy, np.full((256, 1), PATCH_Z + LIFT)], axis=1).astype(np.float32)


def rho(g, voxel_size=1.0):
    """Distance from g to the nearest open face of the two-cell span it leans into, per point (cells of voxel_size / 2; the spans of
    these points are never clipped: positive coordinates, away from the map's border)."""
    h = 0.5 * voxel_size
    t = np.asarray(g, np.float64) / h
    fr = t - np.floor(t)
    lean_up = fr >= 0.5
    dlo = np.where(lean_up, fr, 1.0 + fr)
    dhi = np.where(lean_up, 2.0 - fr, 1.0 - fr)
    return (np.minimum(dlo, dhi) * h).min(axis=1)


def surely_undecided(om, g, th=5.0):
    """Points whose nearest neighbour (the CPU oracle's) lies beyond rho by a clear margin: whatever stage 1 finds in the block is at least
    that far, i.e. beyond rho -- undecided.  (Points with a runner-up inside the margin are undecided as well; they only add to the count.)"""
    acc, tgt, _ = om.nearest_points(np.asarray(g, np.float64), th)
    d = np.linalg.norm(tgt - np.asarray(g, np.float64), axis=1)
    return np.asarray(acc, bool) & (d > rho(g) + 1e-3)


def _maps(ctx, oracle, pts, method, cov_dist=0.4):
    from elimaloc_amd.registration import VoxelHashMap
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(pts)
    om = None
    if oracle is not None:
        om = oracle.Map(1.0, 30)
        om.add_points(pts)
    if method == VGICP:
        vm.CalVoxelCovAll()
    if method == GICP:
        vm.CalPointCovAll(cov_dist)
        if om is not None:
            om.cal_point_cov_all(cov_dist)
    return vm, om


def _record(det):
    """The compared fields of one traced registration, as float64 / int64 arrays."""
    its = det["iters"]
    return {
        "JTJ": np.array([i["JTJ"] for i in its], np.float64).reshape(len(its), 6, 6),
        "JTr": np.array([i["JTr"] for i in its], np.float64).reshape(len(its), 6),
        "residual_sum": np.array([i["residual_sum"] for i in its], np.float64),
        "n_corr": np.array([i["n_corr"] for i in its], np.float64),
        "T": np.array(det["T"], np.float64),
        "iterations": np.array([det["iterations"]], np.int64),
        "fitness_score": np.array([det["fitness_score"]], np.float64),
        "local_cov": np.array(det["local_cov"], np.float64),
    }


FIELDS = ("JTJ", "JTr", "residual_sum", "n_corr", "T", "iterations", "fitness_score", "local_cov")


def _register(ctx, vm, scan, T0, method, **cfg):
    from elimaloc_amd.registration import Registration, RegistrationConfig, IcpMethod
    reg = Registration(RegistrationConfig(icp_method=IcpMethod(method), **cfg), ctx)
    return reg.RunRegister(scan, vm, T0, trace=True)[-1]


def run_all(ctx, counters_ctx):
    """Every registration of the file -> {case name: {field: array}} plus the work counters of the queue cases.  ctx runs the production
    kernels, counters_ctx (elm_ctx_set_work_counters on) the instrumented ones."""
    out, counters = {}, {}
    w = world()
    vm, _ = _maps(ctx, None, w, P2P)
    for n in P2P_SIZES:
        scan, T_true = synth.make_scan(w, n, seed=4200 + n)
        out[f"p2p_n{n}"] = _record(_register(ctx, vm, scan, synth.perturb(T_true, seed=4300 + n), P2P))
    # every point outside the search radius: no neighbour bucket at all and 500 m from the origin / winners beyond a 0.3 m radius
    scan, T_true = synth.make_scan(w, 256, seed=4400)
    far = T_true.copy()
    far[:3, 3] += [500.0, 0.0, 0.0]
    out["p2p_far"] = _record(_register(ctx, vm, scan, far, P2P))
    patch, lifted = sparse_patch(), lifted_scan()
    vmp, _ = _maps(ctx, None, patch, P2P)
    out["p2p_beyond_radius"] = _record(_register(ctx, vmp, lifted, np.eye(4), P2P, max_search_dist=0.3))
    # one workgroup whose queue takes two passes of stage 2, production and instrumented kernels
    for name, method in (("p2p", P2P), ("gicp", GICP)):
        for c, tag in ((ctx, ""), (counters_ctx, "_counters")):
            vmq, _ = _maps(c, None, patch, method)
            out[f"{name}_queue{tag}"] = _record(_register(c, vmq, lifted, np.eye(4), method, max_iteration=4, min_overlap_ratio=0.0))
            if tag:
                first = _register(c, vmq, lifted, np.eye(4), method, max_iteration=1, min_overlap_ratio=0.0)
                counters[name] = float(first["fallback_blocks"])
    vmv, _ = _maps(ctx, None, w, VGICP)
    scan, T_true = synth.make_scan(w, 257, seed=4500)
    out["vgicp_n257"] = _record(_register(ctx, vmv, scan, synth.perturb(T_true, seed=4501), VGICP))
    return out, counters
