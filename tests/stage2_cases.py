"""The scans, maps and calls of tests/test_stage2_groups.py, shared with tools/record_stage2_golden.py (which runs them on the PARENT's
library and writes tests/golden/stage2_parent.npz).  Everything is seeded; nothing here asserts.

The cases aim at stage 2 of k_accumulate_grid -- the queue of undecided points of a workgroup, one 64-record segment per wavefront, and
the lane groups that walk their balls -- at every queue length where a lane group sized to the queue would change its width (16 lanes up
to 4 points, 8 up to 8, 4 beyond) or where the 4-lane groups need another pass (64 points per pass), with the undecided points at seeded
random places of the thread order so that the four segments fill unevenly (none at all, one record, all 64), so that a change of who
walks which column or of where a record lies can be held to "not one bit, not one pair moved"."""
import numpy as np

import accumulate_tail_cases as tc
from accumulate_tail_cases import FIELDS, GICP, P2P, _maps, _record, _register  # noqa: F401

QUEUE_K = (0, 1, 4, 5, 8, 9, 16, 17, 64, 65, 256)  # undecided points of the one workgroup: every group-width and pass boundary
MIXED_K = (3, 7, 12, 40)                           # the 1 000-point scan: four workgroups (the last one of 232 points) in one launch
SEED_K = (3, 20)                                   # lifted past a whole cell: stage 1 finds an empty block, stage 2 seeds first
SEED_LIFT = 1.2
SEED_RADIUS = 2.0
FORM_K = (5, 65)                                   # repeated on the two-level grid and with GICP
QUERY_K = 5
NEAR = 0.02        # an on-sheet scan point lies within NEAR (per axis) of a map point ...
CLEAR = 0.30       # ... whose nearest other map point is at least CLEAR away: stage 1 decides it
UNDECIDED_BY = 5e-3  # a lifted point's nearest neighbour lies this far beyond the open faces of its block: stage 1 cannot decide it


def _nn(patch, g):
    """Brute-force distances (float64) of g's points to the patch: nearest, second nearest."""
    d = np.sqrt(((g[:, None, :] - patch[None, :, :].astype(np.float64)) ** 2).sum(axis=2))
    d.sort(axis=1)
    return d[:, 0], d[:, 1]


def _lifted_pool(lift, seed):
    """Points `lift` above the sheet at random places whose nearest map point is surely beyond the open faces of their block."""
    patch = tc.sparse_patch()
    rng = np.random.default_rng(seed)
    xy = rng.uniform(21.0, 27.0, size=(4096, 2))
    g = np.concatenate([xy, np.full((len(xy), 1), tc.PATCH_Z + lift)], axis=1).astype(np.float32)
    d1, _ = _nn(patch, g.astype(np.float64))
    return g[d1 > tc.rho(g.astype(np.float64)) + UNDECIDED_BY]


def _sheet_pool(seed):
    """Points on the sheet next to an isolated map point: the winner is within 0.04 m, the runner-up a quarter metre behind, and every
    open face of the block is at least 0.25 m - NEAR away."""
    patch = tc.sparse_patch()
    rng = np.random.default_rng(seed)
    _, d2 = _nn(patch, patch.astype(np.float64))  # (the nearest is the point itself)
    lone = patch[(d2 > CLEAR) & (patch[:, 0] > 21.0) & (patch[:, 0] < 27.0) & (patch[:, 1] > 21.0) & (patch[:, 1] < 27.0)]
    base = lone[rng.integers(0, len(lone), size=2048)]
    g = base.copy()
    g[:, :2] += rng.uniform(-NEAR, NEAR, size=(len(g), 2)).astype(np.float32)
    g[:, 2] = tc.PATCH_Z
    return g.astype(np.float32)


def workgroup_scan(k, n=256, lift=tc.LIFT, seed=0):
    """n points: k lifted (undecided), n - k on the sheet (decided by stage 1), the lifted ones at seeded random places of the thread order."""
    lifted, sheet = _lifted_pool(lift, 5100 + seed), _sheet_pool(5200 + seed)
    rng = np.random.default_rng(5300 + 7 * seed + k)
    pts = sheet[rng.permutation(len(sheet))[: n]].copy()
    where = np.sort(rng.permutation(n)[:k])
    pts[where] = lifted[rng.permutation(len(lifted))[:k]]
    return pts


def mixed_scan():
    """1 000 points: workgroups with 3, 7, 12 and 40 undecided points side by side in one launch."""
    sizes = (256, 256, 256, 232)
    return np.concatenate([workgroup_scan(k, n, seed=10 + i) for i, (k, n) in enumerate(zip(MIXED_K, sizes))])


def seed_scan(k):
    return workgroup_scan(k, lift=SEED_LIFT, seed=20)


# ---- exact float64 ties: a lattice whose midpoints are equidistant from two or four map points -------------------------------------
LATTICE_N = (14, 14, 2)
LATTICE_0 = (20.125, 20.125, 10.125)  # every coordinate a multiple of 1/8: float32-exact, squared distances exact in float64
TIE_RUNS = ((4, 9), (8, 4), (40, 1))  # (ties per 256-query workgroup, calls): 16-lane, 8-lane and 4-lane groups; >= 32 ties each


def lattice_map():
    ii = np.stack(np.meshgrid(*[np.arange(n) for n in LATTICE_N], indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.asarray(LATTICE_0) + 0.5 * ii
    return pts[np.random.default_rng(6100).permutation(len(pts))].astype(np.float32)


def tie_queries(k, call):
    """256 queries: k exact midpoints (alternately between two and between four lattice points, along / across every axis pair) at seeded
    places among 256 - k points 0.03 m beside a lattice point."""
    rng = np.random.default_rng(6200 + 100 * k + call)
    shifts = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))
    hi = np.asarray(LATTICE_N) - 1
    q = np.empty((256, 3))
    base = np.stack([rng.integers(1, n - 1, size=256) if n > 2 else rng.integers(0, n, size=256) for n in LATTICE_N], axis=1)
    q[:] = np.asarray(LATTICE_0) + 0.5 * base + rng.choice([-0.03125, 0.03125], size=(256, 3))
    where = np.sort(rng.permutation(256)[:k])
    for j, w in enumerate(where):
        s = np.asarray(shifts[(j + call) % 6])
        b = np.minimum(base[w], hi - s)
        q[w] = np.asarray(LATTICE_0) + 0.5 * b + 0.25 * s
    return q, where


def exact_ties(q):
    """Per query: how many of the lattice's points lie at exactly the smallest float64 distance."""
    pts = lattice_map().astype(np.float64)
    d2 = ((q[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    return (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)


# ---- the recorded runs ------------------------------------------------------------------------------------------------------------------
def _run_queue(ctx, cctx, maps, scan, method, out, counters, name, **cfg):
    """One traced registration on the production kernels, and the work counters of its first iteration on the instrumented ones."""
    if method not in maps:
        maps[method] = (_maps(ctx, None, tc.sparse_patch(), method)[0], _maps(cctx, None, tc.sparse_patch(), method)[0])
    vm, vmc = maps[method]
    out[name] = _record(_register(ctx, vm, scan, np.eye(4), method, max_iteration=4, min_overlap_ratio=0.0, **cfg))
    out[name + "_counters"] = _record(_register(cctx, vmc, scan, np.eye(4), method, max_iteration=4, min_overlap_ratio=0.0, **cfg))
    first = _register(cctx, vmc, scan, np.eye(4), method, max_iteration=1, min_overlap_ratio=0.0, **cfg)
    counters[name] = (float(first["fallback_blocks"]), float(first["n_tested_total"]))


def run_dense(ctx, cctx):
    """Every registration on the default (dense) grid -> ({case: {field: array}}, {case: (points served by stage 2, candidates tested)})."""
    out, counters, maps = {}, {}, {}
    for k in QUEUE_K:
        _run_queue(ctx, cctx, maps, workgroup_scan(k), P2P, out, counters, f"p2p_k{k}")
    _run_queue(ctx, cctx, maps, mixed_scan(), P2P, out, counters, "p2p_mixed")
    for k in SEED_K:
        _run_queue(ctx, cctx, maps, seed_scan(k), P2P, out, counters, f"p2p_seed_k{k}", max_search_dist=SEED_RADIUS)
    for k in FORM_K:
        _run_queue(ctx, cctx, maps, workgroup_scan(k), GICP, out, counters, f"gicp_k{k}")
    return out, counters


def run_tiled():
    """The k = 5 and k = 65 workgroups on the two-level grid, in contexts of their own (ELM_GRID is read when the index is built)."""
    from elimaloc_amd.registration import Context
    from index_form_cases import form_env
    out, counters, maps = {}, {}, {}
    with form_env("tiled"):
        ctx, cctx = Context(0), Context(0)
        cctx.set_work_counters(True)
        try:
            for k in FORM_K:
                _run_queue(ctx, cctx, maps, workgroup_scan(k), P2P, out, counters, f"tiled_p2p_k{k}")
        finally:
            cctx.close()
            ctx.close()
    return out, counters


def run_all(ctx, cctx):
    out, counters = run_dense(ctx, cctx)
    o2, c2 = run_tiled()
    out.update(o2)
    counters.update(c2)
    return out, counters


CASES = tuple(f"p2p_k{k}" for k in QUEUE_K) + ("p2p_mixed",) + tuple(f"p2p_seed_k{k}" for k in SEED_K) + tuple(f"gicp_k{k}" for k in FORM_K) \
    + tuple(f"tiled_p2p_k{k}" for k in FORM_K)
