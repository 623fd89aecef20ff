"""The maps, index forms and calls of tests/test_index_forms.py, shared with tools/record_index_golden.py (which runs them on the PARENT's
library and writes tests/golden/index_forms_parent.npz).  Everything is seeded; nothing here asserts.

The cases aim at the HOST side of the search indices -- which index a map gets, its byte accounting, and the order of the points inside a
cell, which decides every tie -- so that a change of the index builders can be held to "not one pair, not one bit moved"."""
import contextlib
import hashlib
import os

import numpy as np

from accumulate_tail_cases import FIELDS, _record  # noqa: F401  (the compared fields of a traced registration)

P2P, GICP, VGICP, AVGICP = 0, 1, 2, 3
METHODS = (("p2p", P2P), ("gicp", GICP), ("vgicp", VGICP), ("avgicp", AVGICP))
COV_DIST = 0.6
TH = 2.0
N_QUERY, N_TIES = 2000, 300

# one fresh context each: ELM_KERNEL is read when the context is created, ELM_GRID when the index is built.  The boxes of the `single` and
# `crowded` maps hold at most 1000 cells, so on those two maps the two small_budget forms refuse nothing and repeat `default`: the lists
# in place of a refused grid and the voxel-mean lists without their dense table are pinned by `straddle` and `sheet`, the unsorted lists
# past 1024 entries by `crowded` under `lists`.
FORMS = {
    "default": {},
    "tiled": {"ELM_GRID": "tiled"},
    "wide": {"ELM_GRID": "max_block_bytes=48"},
    "wide_tiled": {"ELM_GRID": "max_block_bytes=48,tiled"},
    "lists": {"ELM_KERNEL": "lists"},
    "small_budget": {"ELM_GRID": "max_cells=1000"},           # the voxel-mean lists without their dense table
    "small_budget_dense": {"ELM_GRID": "max_cells=1000,dense"},  # no grid at all: the neighbourhood lists
}
MAPS = ("straddle", "single", "crowded", "sheet")

HOLE = (-3.05, 1.05)   # straddle: no point with x AND y inside (one whole tile of 8 x 8 half-metre columns, see tiles_of)
FLAT = 1.2             # straddle: beyond x, y > FLAT every point lies in ONE layer of cells


def tie_pairs():
    """N_TIES pairs of map points half a metre apart along one axis, every coordinate a multiple of 0.25: the point midway is exactly
    0.25 m from both."""
    rng = np.random.default_rng(7101)
    a = rng.integers(-22, 22, size=(4 * N_TIES, 3)).astype(np.float64) * 0.25
    a[:, 2] = rng.integers(-5, 5, size=len(a)) * 0.25
    inside = (a[:, 0] >= HOLE[0] - 0.5) & (a[:, 0] < HOLE[1] + 0.5) & (a[:, 1] >= HOLE[0] - 0.5) & (a[:, 1] < HOLE[1] + 0.5)
    a = np.unique(a[~inside], axis=0)
    a = a[rng.permutation(len(a))][:N_TIES]
    axis = rng.integers(0, 3, size=len(a))
    b = a.copy()
    b[np.arange(len(a)), axis] += 0.5
    return a, b


def straddle_map():
    """About 3000 points over 12 m x 12 m x 3 m around the origin (negative coordinates: truncated stored keys against floored query
    keys).  The lattice pairs of tie_pairs come first, so AddPoints keeps them all; one tile-sized hole; one flat corner."""
    rng = np.random.default_rng(7102)
    a, b = tie_pairs()
    p = rng.uniform([-6.0, -6.0, -1.5], [6.0, 6.0, 1.5], size=(3400, 3))
    hole = (p[:, 0] >= HOLE[0]) & (p[:, 0] < HOLE[1]) & (p[:, 1] >= HOLE[0]) & (p[:, 1] < HOLE[1])
    p = p[~hole][:2550]
    flat = (p[:, 0] > FLAT) & (p[:, 1] > FLAT)
    p[flat, 2] = rng.uniform(0.05, 0.45, size=int(flat.sum()))
    lattice = np.concatenate([a, b])
    lattice = lattice[~((lattice[:, 0] > FLAT - 0.5) & (lattice[:, 1] > FLAT - 0.5))]  # (the flat corner keeps its one layer)
    anchors = np.array([[-5.9, -5.9, -1.4], [5.9, 5.9, 0.3]])
    return np.concatenate([lattice, anchors, p]).astype(np.float32)


def tiles_of(points, voxel_size=1.0):
    """{(tile x, tile y): (lowest, highest) cell z} of the two-level grid over `points`: half-voxel cells, the box starts two cells below
    the lowest cell, tiles of 8 x 8 columns.  (floor is the grid's own cell rule away from cell faces, where these points are.)"""
    c = np.floor(np.asarray(points, np.float64) / (0.5 * voxel_size)).astype(np.int64)
    c -= c.min(axis=0) - 2
    out = {}
    for tx, ty, cz in zip(c[:, 0] >> 3, c[:, 1] >> 3, c[:, 2]):
        lo, hi = out.get((tx, ty), (cz, cz))
        out[(int(tx), int(ty))] = (min(lo, cz), max(hi, cz))
    return out


def single_map():
    return np.array([[-0.3, 0.4, 0.2]], np.float32)


def crowded_map():
    """27 voxels of 64 lattice points each, a quarter metre apart (max_points_per_voxel = 50 keeps the first 50): the middle voxel's
    neighbourhood list holds 27 x 50 = 1350 entries, more than the 1024 a cell-sorted list may have."""
    g = 0.125 + 0.25 * np.arange(4)
    cell = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(7103)
    vox = np.stack(np.meshgrid(*[np.arange(10, 13)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([v + cell[rng.permutation(64)] for v in vox]).astype(np.float32)


def sheet_map():
    """Two or three points per voxel, all on one slightly tilted sheet: every voxel covariance is rank-deficient (flagged)."""
    rng = np.random.default_rng(7104)
    out = []
    for vx in range(-5, 5):
        for vy in range(-5, 5):
            k = 2 + (vx + vy) % 2
            xy = np.array([vx, vy]) + rng.uniform(0.1, 0.9, size=(k, 2))
            out.append(np.concatenate([xy, 0.3 + 0.01 * xy[:, :1]], axis=1))
    return np.concatenate(out).astype(np.float32)


MAP_POINTS = {"straddle": straddle_map, "single": single_map, "crowded": crowded_map, "sheet": sheet_map}
MAP_MAX_POINTS = {"straddle": 30, "single": 30, "crowded": 50, "sheet": 30}


def queries(name):
    """About N_QUERY points: noisy copies of map points, points around the map's box (some without any neighbour), and for the straddle
    map the N_TIES midpoints of its lattice pairs."""
    pts = MAP_POINTS[name]().astype(np.float64)
    rng = np.random.default_rng(7200 + MAPS.index(name))
    lo, hi = pts.min(axis=0) - 2.5, pts.max(axis=0) + 2.5
    ties = np.zeros((0, 3))
    if name == "straddle":
        a, b = tie_pairs()
        ties = 0.5 * (a + b)
    n_near = (N_QUERY - len(ties)) * 3 // 4
    near = pts[rng.integers(0, len(pts), n_near)] + rng.normal(0.0, 0.15, size=(n_near, 3))
    box = rng.uniform(lo, hi, size=(N_QUERY - len(ties) - n_near, 3))
    q = np.concatenate([ties, near, box])
    return q[rng.permutation(len(q))]


def exact_ties(name):
    """How many queries have two or more of the map's INPUT points at exactly the smallest distance (float64; exact for the lattice)."""
    pts, q = MAP_POINTS[name]().astype(np.float64), queries(name)
    d2 = ((q[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    return int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())


def scan_of(name):
    """A scan of the map: up to 400 of its points with 2 cm of noise, seen from a pose near the identity; and the initial guess."""
    pts = MAP_POINTS[name]().astype(np.float64)
    rng = np.random.default_rng(7300 + MAPS.index(name))
    sel = pts[rng.permutation(len(pts))[:400]] + rng.normal(0.0, 0.02, size=(min(len(pts), 400), 3))
    yaw = 0.02
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = [0.08, -0.05, 0.03]
    local = (sel - T[:3, 3]) @ T[:3, :3]
    T0 = T.copy()
    T0[:3, 3] += [0.05, 0.04, -0.02]
    return local.astype(np.float32), T0


@contextlib.contextmanager
def form_env(form):
    """The environment of one index form, for the life of one context."""
    keys = ("ELM_GRID", "ELM_KERNEL")
    before = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(FORMS[form])
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if before[k] is not None:
                os.environ[k] = before[k]


def _info(vm):
    mi = vm.info()
    return np.array([mi.layout_flags, mi.device_bytes, mi.n_query_voxels, mi.nbr_entries, mi.index_bytes, *mi.index_part_bytes, mi.n_list_voxels],
                    np.int64)


def run_case(name, form):
    """One map on one index form, in a context of its own -> {field: array}: the map's info once the search index is built and again
    after every call, the pairs of the three correspondence calls, one traced registration per method."""
    from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig, VoxelHashMap
    out = {}
    with form_env(form):
        ctx = Context(0)
        vm = VoxelHashMap(1.0, MAP_MAX_POINTS[name], ctx)
        try:
            vm.AddPoints(MAP_POINTS[name]())
            vm.CalVoxelCovAll()
            vm.CalPointCovAll(COV_DIST)
            vm.BuildNeighbourhoods()
            out["info_index"] = _info(vm)
            q = queries(name)
            for call in ("GetCorrespondencePoints", "GetCorrespondencesCov", "GetCorrespondencesAllCov"):
                res = getattr(vm, call)(q, TH, indices=True)
                out[f"{call}/src"] = np.asarray(res[-2], np.int32)
                out[f"{call}/tgt"] = np.asarray(res[-1], np.int32)
            scan, T0 = scan_of(name)
            for mname, method in METHODS:
                reg = Registration(RegistrationConfig(icp_method=IcpMethod(method), max_iteration=4, min_overlap_ratio=0.0), ctx)
                for field, arr in _record(reg.RunRegister(scan, vm, T0, trace=True)[-1]).items():
                    out[f"{mname}/{field}"] = arr
            out["info_end"] = _info(vm)
        finally:
            vm.Clear()
            ctx.close()
    return out


def digest(arr):
    a = np.ascontiguousarray(arr)
    return hashlib.sha1(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()
