"""Hand-built inputs for the relocalization kernels' edges (tests/test_reloc_cases.py on the CPU, tests/test_reloc_edges.py on the GPU).
Plain numpy, no GPU, no library call.  Every coordinate is a float32 value; maps hold a few hundred to a few thousand points.

A global case is a world and a scan built around it:

* the ground is a coarse sheet of points (pitch 2 m: some twenty points within 5 m of a lattice node, so the node stands on ground), tilted
  or terraced where a node's z range must be several keys wide, with holes (wider than 5 m) where leaves must be invalid;
* the scan is a set of sensor-frame points; the structure of the map is that scan placed at a few lattice poses ("echoes", each a
  prefix of the scan, so the leaf scores have peaks of chosen heights), plus clutter and the explicit voxels a case is about;
* the rectangle, steps, voxel size and config name the edge: the level the search starts at, the window widths, the z words of a
  bitmap column, the z cap, the box edges, the key band around the origin, the pruning pressure.

`global_case(name)` builds (and caches) a case; `mirror(name)` its reloc_ref.Mirror over the numpy lattice.  A score case (for
ScorePoses) carries map, scan, poses, r_max and the indices of the points that sit exactly on an edge.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import reloc_ref as rr

INF = math.inf


def config(**kw):
    """elm_reloc_global_config's fields with its defaults, as a plain namespace (no library needed)"""
    c = dict(x_min=math.nan, x_max=math.nan, y_min=math.nan, y_max=math.nan, step_xy_m=0.5, step_yaw_deg=2.0, score_max_range_m=50.0,
             score_min_height_m=1.0, max_score_points=8192, top_k=16, nms_xy_m=1.0, nms_yaw_deg=6.0, pool_min=64, max_kz_span=64,
             bitmap_max_bytes=256 << 20)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    return SimpleNamespace(**c)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3).astype(np.float32))


def _sheet(x0, x1, y0, y1, pitch, zfun, holes=()):
    gx, gy = np.meshgrid(np.arange(x0, x1 + 1e-9, pitch), np.arange(y0, y1 + 1e-9, pitch), indexing="ij")
    x, y = gx.ravel(), gy.ravel()
    keep = np.ones(x.size, bool)
    for (cx, cy, r) in holes:
        keep &= np.hypot(x - cx, y - cy) >= r
    x, y = x[keep], y[keep]
    return np.column_stack([x, y, np.round(zfun(x, y) * 64.0) / 64.0])


def _scan(seed, n, r_xy, z_lo, z_hi, q=16.0):
    """n sensor-frame points on the 1 / q grid: xy within r_xy, z in [z_lo, z_hi]"""
    rng = np.random.default_rng(seed)
    p = np.column_stack([rng.uniform(-r_xy, r_xy, n), rng.uniform(-r_xy, r_xy, n), rng.uniform(z_lo, z_hi, n)])
    return np.round(p * q) / q


def _build(name, edge, *, vs, x_min, y_min, NX, NY, step, yaw_step, ground, zfun=lambda x, y: 0.0 * x, holes=(), pitch=2.0, scan, echoes,
           h=1.5, tilt=None, clutter=0, clutter_box=None, extra_map=(), extra_scan=(), targets=(), seed=1, **cfg_kw):
    """ground: (x0, x1, y0, y1) of the sheet.  echoes: [(k, i, j, n)]: the first n scan points placed at lattice pose (k, i, j)."""
    cfg = config(x_min=x_min, x_max=x_min + (NX - 1) * step + 0.25 * step, y_min=y_min, y_max=y_min + (NY - 1) * step + 0.25 * step, step_xy_m=step,
                 step_yaw_deg=yaw_step, **({"score_min_height_m": -INF, "score_max_range_m": 200.0} | cfg_kw))
    T_tilt = np.eye(4)
    if tilt is not None:
        T_tilt[:3, :3] = tilt
    T_tilt[2, 3] = h
    sheet = _f32(_sheet(*ground, pitch, zfun, holes))
    scan = _f32(np.concatenate([np.asarray(scan, dtype=np.float64).reshape(-1, 3), np.asarray(extra_scan, dtype=np.float64).reshape(-1, 3)]))
    low = np.concatenate([sheet, _f32(extra_map)]) if len(extra_map) else sheet  # what the ground field reads (echoes and clutter lie higher)
    H, valid = rr.lattice(low, T_tilt, cfg)
    parts = [sheet]
    s64 = scan.astype(np.float64)
    for (k, i, j, n) in echoes:
        hyp = (k * NX + i) * NY + j
        assert valid[hyp], (name, k, i, j)
        parts.append(_f32(s64[:n] @ H[hyp][:3, :3].T + H[hyp][:3, 3]))
    if clutter:
        rng = np.random.default_rng(seed + 77)
        lo, hi = np.array(clutter_box[0]), np.array(clutter_box[1])
        parts.append(_f32((np.floor(rng.uniform(lo, hi, (clutter, 3)) / vs) + 0.5) * vs))
    for (cx, cy, r) in holes:  # a hole is empty at every height: any stored point counts as ground
        parts = [p[np.hypot(p[:, 0].astype(np.float64) - cx, p[:, 1].astype(np.float64) - cy) >= r] for p in parts]
    if len(extra_map):
        parts.append(_f32(extra_map))
    world = np.concatenate(parts)
    return SimpleNamespace(name=name, edge=edge, map=world, scan=scan, T_tilt=T_tilt, vs=vs, cap=30, cfg=cfg, targets=tuple(targets),
                           dims=(rr.n_yaw(cfg), NX, NY))


def _quarter_probes(n):
    """sensor-frame points with integer xy: under the quarter-turn yaws a + x_lo lands within rounding of a key face, the only place where a
    key range over a node can reach the window width"""
    rng = np.random.default_rng(5)
    return np.column_stack([rng.integers(-9, 10, n), rng.integers(-9, 10, n), np.round(rng.uniform(1.0, 9.0, n) * 16.0) / 16.0]).astype(np.float64)


def _corner_voxels(vs, kx, ky, kz):
    """one point in each of the eight corner voxels of the key box kx x ky x kz (inclusive key ranges, non-negative keys)"""
    return [((a + 0.5) * vs, (b + 0.5) * vs, (c + 0.5) * vs) for a in kx for b in ky for c in kz]


GLOBAL = {}


def _case(fn):
    GLOBAL[fn.__name__] = fn
    return fn


# ---------------------------------------------------------------------------------------------------------------- levels
@_case
def top1_k4_9x7():
    return _build("top1_k4_9x7", "top = 1, ragged 9 x 7 lattice, quarter-turn yaws", vs=0.5, x_min=2.0, y_min=3.0, NX=9, NY=7, step=0.5,
                  yaw_step=90.0, ground=(-10.0, 18.0, -10.0, 18.0), scan=_scan(11, 120, 8.0, 0.5, 12.0),
                  echoes=[(1, 4, 3, 120), (0, 1, 5, 90), (3, 7, 1, 70), (2, 2, 2, 50), (1, 8, 6, 40)], clutter=300,
                  clutter_box=((-8.0, -8.0, 2.0), (16.0, 16.0, 14.0)), pool_min=4, top_k=8, nms_xy_m=0.0, nms_yaw_deg=0.0, targets=("w1",))


@_case
def top2_33x33():
    return _build("top2_33x33", "top = 2 (36 x 17 x 17 > 4096 >= 36 x 9 x 9), holes in the ground", vs=0.5, x_min=1.0, y_min=1.0, NX=33, NY=33,
                  step=0.5, yaw_step=10.0, ground=(-8.0, 26.0, -8.0, 26.0), holes=((2.0, 2.0, 6.5), (4.0, 14.0, 6.0)),
                  scan=_scan(12, 100, 7.0, 0.5, 14.0), echoes=[(5, 20, 20, 100), (17, 30, 9, 80), (30, 27, 30, 60), (2, 18, 31, 45)],
                  clutter=100, clutter_box=((-6.0, -6.0, 2.0), (24.0, 24.0, 16.0)), pool_min=1, top_k=6, targets=("w1",))


@_case
def top3_33x33():
    return _build("top3_33x33", "top = 3 (72 x 9 x 9 > 4096 >= 72 x 5 x 5), tilted ground", vs=0.5, x_min=1.0, y_min=1.0, NX=33, NY=33,
                  step=0.5, yaw_step=5.0, ground=(-8.0, 26.0, -8.0, 26.0), zfun=lambda x, y: 0.25 * x + 0.125 * y + 3.0,
                  scan=_scan(13, 90, 7.0, 0.5, 14.0), echoes=[(9, 12, 22, 90), (40, 29, 4, 75), (63, 3, 3, 60), (20, 25, 27, 50)],
                  clutter=200, clutter_box=((-6.0, -6.0, 3.0), (24.0, 24.0, 24.0)), pool_min=4, top_k=6, targets=("w1", "w2"))


@_case
def nx1_line():
    return _build("nx1_line", "NX = 1: a lattice one node wide", vs=0.5, x_min=4.0, y_min=1.0, NX=1, NY=13, step=0.5, yaw_step=45.0,
                  ground=(-8.0, 16.0, -8.0, 16.0), scan=_scan(14, 80, 6.0, 0.5, 8.0), echoes=[(3, 0, 7, 80), (6, 0, 2, 60), (1, 0, 12, 30)],
                  clutter=150, clutter_box=((-4.0, -6.0, 2.0), (12.0, 14.0, 10.0)), pool_min=4, top_k=4, targets=("w1",))


# ---------------------------------------------------------------------------------------------------------------- window width
def _width(name, edge, step, vs, NX=12, NY=10, yaw_step=90.0, **kw):
    ext = max(NX, NY) * step
    return _build(name, edge, vs=vs, x_min=2.0, y_min=3.0, NX=NX, NY=NY, step=step, yaw_step=yaw_step,
                  ground=(-10.0, 12.0 + ext, -10.0, 12.0 + ext), **({"pool_min": 4, "top_k": 8, "nms_xy_m": 0.0, "nms_yaw_deg": 0.0} | kw))


@_case
def width_05_05():
    return _width("width_05_05", "(2^l - 1) step / vs an exact integer; key ranges of exactly w - 1 keys", 0.5, 0.5,
                  scan=np.concatenate([_scan(21, 60, 6.0, 0.5, 9.0, q=2.0), _scan(22, 60, 6.0, 0.5, 9.0)]),
                  echoes=[(2, 6, 4, 120), (0, 2, 8, 90), (1, 10, 1, 70), (3, 4, 4, 50)], clutter=200,
                  clutter_box=((-6.0, -6.0, 2.0), (14.0, 14.0, 11.0)), targets=("w1",))


@_case
def width_025_05():
    return _width("width_025_05", "step half a voxel: w_1 = 2", 0.25, 0.5, scan=np.concatenate([_scan(23, 60, 6.0, 0.5, 9.0, q=4.0), _scan(24, 60, 6.0, 0.5, 9.0)]),
                  echoes=[(2, 6, 4, 120), (0, 2, 8, 90), (1, 10, 1, 70), (3, 4, 4, 50)], clutter=200,
                  clutter_box=((-6.0, -6.0, 2.0), (12.0, 12.0, 11.0)), targets=("w1",))


@_case
def width_075_05():
    return _width("width_075_05", "(2^l - 1) step / vs not an integer", 0.75, 0.5, scan=np.concatenate([_scan(25, 60, 6.0, 0.5, 9.0, q=4.0), _scan(26, 60, 6.0, 0.5, 9.0)]),
                  echoes=[(2, 6, 4, 120), (0, 2, 8, 90), (1, 10, 1, 70), (3, 4, 4, 50)], clutter=200,
                  clutter_box=((-6.0, -6.0, 2.0), (18.0, 18.0, 11.0)), targets=("w1",))


@_case
def width_w2_eq_w1():
    return _width("width_w2_eq_w1", "w_2 == w_1 == 2 (step 0.1, vs 1.0): the window pass with a single offset; pool_min 64", 0.1, 1.0, NX=17, NY=17,
                  yaw_step=5.0, scan=_scan(27, 100, 7.0, 0.5, 9.0), echoes=[(30, 8, 8, 100), (51, 2, 13, 80), (7, 15, 3, 60)], clutter=300,
                  clutter_box=((-6.0, -6.0, 2.0), (12.0, 12.0, 11.0)), pool_min=64, top_k=16, nms_xy_m=0.25, nms_yaw_deg=6.0, targets=("w1",))


@_case
def width_vs03():
    return _width("width_vs03", "vs = 0.3: keys by division, not by the exact reciprocal", 0.5, 0.3,
                  scan=np.concatenate([_scan(28, 60, 6.0, 0.5, 9.0, q=1.0 / 0.3), _scan(29, 60, 6.0, 0.5, 9.0)]),
                  echoes=[(2, 6, 4, 120), (0, 2, 8, 90), (1, 10, 1, 70), (3, 4, 4, 50)], clutter=200,
                  clutter_box=((-6.0, -6.0, 2.0), (14.0, 14.0, 11.0)), targets=("w1",))


@_case
def width_floor_under():
    """step 0.6 / vs 0.2: 0.6 / 0.2 rounds to 2.9999999999999996, so w_1 = 4 where the ratio is 3, and a point within rounding of a key face
    has a key range of 4 = w_1 over a level-1 node: the wide rule, the only thing that keeps such a point in the bound."""
    pr = np.concatenate([_scan(30, 60, 6.0, 0.5, 9.0), _quarter_probes(60)])
    return _build("width_floor_under", "the floor of w_l under-estimates: key ranges of exactly w keys (the wide rule)", vs=0.2, x_min=1.2, y_min=2.4,
                  NX=12, NY=10, step=0.6, yaw_step=90.0, ground=(-12.0, 20.0, -12.0, 20.0), scan=pr,
                  echoes=[(2, 6, 4, 120), (0, 2, 8, 100), (1, 10, 1, 80), (3, 4, 4, 60)], clutter=200, clutter_box=((-8.0, -8.0, 2.0), (18.0, 18.0, 11.0)),
                  pool_min=4, top_k=8, nms_xy_m=0.0, nms_yaw_deg=0.0, targets=("wide",))


# ---------------------------------------------------------------------------------------------------------------- z words and the cap
def _zwords(cap):
    """vs 0.25, a box of nz = 128.  The ground is a plain 10 m up, rising by a key over the lattice's y range, with one pit: six columns of structure voxels, half a metre across, at
    column bits 0, 31, 32, 63, 64 and 127.  Their bit-0 points are the lowest within 5 m of them, so the ground field drops by 10 m (40
    keys) across the rim of that disk, within one lattice step: the nodes on the rim have z ranges of some 40 keys -- lookups over three
    words, or the cap.  Scan points 50..99 aim at the 31|32 and 63|64 seams (z = 8 and 16) from the plain's sensor heights (12.0 .. 12.3); the
    first three look straight up at a three-key ceiling (bits 119 .. 121) over the plain, so every pose on the plain scores at least 3.  The
    best-bounded nodes are the rim's (under a small cap every point counts there), so four echoes stand on the plain side of the first four rim
    nodes: the first threshold is then an echo's score, and with top_k = 40 and no NMS it drops pass by pass through the range where the
    points that the cap adds to a bound decide whether a node is kept."""
    vs = 0.25
    cols = [(-1.125 + 0.25 * a, 5.125 + 0.25 * b) for a in range(3) for b in range(2)]
    extra_map = [(x, y, (bit + 0.5) * vs) for (x, y) in cols for bit in (0, 31, 32, 63, 64, 127)]
    extra_map += [(x, y, z) for x in np.arange(1.375, 12.626, 0.25) for y in np.arange(2.375, 7.626, 0.25) for z in (29.875, 30.125, 30.375)]
    up = [(0.0, 0.0, 18.0), (0.5, 0.25, 18.0), (-0.25, 0.5, 18.0)]
    rng = np.random.default_rng(31)
    seam = []
    for face in (8.0, 16.0):
        for d in np.arange(-0.75, 0.76, 0.0625):
            seam.append((rng.integers(-40, 41) / 8.0, rng.integers(-16, 17) / 8.0, face - 12.125 + d))
    return _build(f"zwords_cap{cap}", f"z words of a column (nz = 128), seams 31|32 and 63|64, max_kz_span = {cap}", vs=vs, x_min=2.0, y_min=3.0,
                  NX=21, NY=9, step=0.5, yaw_step=90.0, ground=(-8.0, 20.0, -8.0, 16.0), zfun=lambda x, y: 10.125 + 0.0625 * (y + 8.0),
                  scan=np.concatenate([up, _scan(32, 47, 5.0, 0.5, 12.0)]), extra_scan=seam,
                  echoes=[(0, 5, 1, 50), (0, 5, 3, 45), (0, 5, 5, 40), (0, 5, 7, 35), (1, 13, 2, 50), (3, 18, 4, 42)], extra_map=extra_map, clutter=150,
                  clutter_box=((-4.0, -4.0, 13.0), (16.0, 12.0, 29.0)), pool_min=4, top_k=40, nms_xy_m=0.0, nms_yaw_deg=0.0, max_kz_span=cap,
                  targets={1: ("zcap", "w1"), 2: ("zcap", "w2"), 33: ("zcap", "w2"), 64: ("w3", "w2")}[cap])


for _c in (1, 2, 33, 64):
    GLOBAL[f"zwords_cap{_c}"] = functools.partial(_zwords, _c)


# ---------------------------------------------------------------------------------------------------------------- box edges, origin
@_case
def box_overhang():
    kx, ky = (4, 27), (6, 25)
    return _build("box_overhang", "the rectangle overhangs the map's key box on all four sides; voxels at the box's eight corners", vs=0.5, x_min=-2.0,
                  y_min=-1.0, NX=37, NY=33, step=0.5, yaw_step=90.0, ground=(2.0, 13.75, 3.0, 12.75), pitch=1.0, scan=_scan(41, 110, 3.0, 0.5, 9.0),
                  echoes=[(1, 16, 16, 110), (0, 22, 18, 90), (3, 18, 20, 70), (2, 24, 15, 50)],
                  extra_map=_corner_voxels(0.5, kx, ky, (0, 40)), pool_min=4, top_k=8, nms_xy_m=0.0, nms_yaw_deg=0.0,
                  targets=("clamp", "past", "out"))


@_case
def thin_y():
    line = [(x, y, 0.125) for x in np.arange(-6.0, 18.1, 0.5) for y in (4.125, 4.625)]
    return _build("thin_y", "a map two keys thick in y", vs=0.5, x_min=2.0, y_min=2.0, NX=17, NY=9, step=0.5, yaw_step=90.0,
                  ground=(0.0, 0.0, 4.125, 4.125), scan=[(x, 0.0625 * (q % 5), 0.5 + 0.5 * (q % 7)) for q, x in enumerate(np.arange(-6.0, 6.01, 0.125))],
                  extra_map=line + [(x, 4.125 + 0.5 * (q % 2), 2.125 + 0.5 * (q % 7)) for q, x in enumerate(np.arange(-4.0, 16.0, 0.375))], echoes=[],
                  pool_min=4, top_k=8, nms_xy_m=0.0, nms_yaw_deg=0.0, targets=("clamp", "past", "out"))


@_case
def origin_band():
    return _build("origin_band", "map and lattice straddle 0 on x, y and z: keys -1, 0, +1 and the two-voxel-wide key 0", vs=0.5, x_min=-2.5, y_min=-2.0,
                  NX=11, NY=9, step=0.5, yaw_step=90.0, ground=(-12.0, 12.0, -12.0, 12.0), zfun=lambda x, y: -1.75 + 0.03125 * x, h=1.0,
                  scan=np.concatenate([_scan(51, 60, 4.0, -0.5, 2.5, q=4.0), _scan(52, 60, 2.0, -0.25, 1.5, q=8.0)]),
                  echoes=[(2, 5, 4, 120), (0, 3, 6, 90), (1, 8, 2, 70), (3, 4, 4, 50)], clutter=250, clutter_box=((-6.0, -6.0, -1.5), (6.0, 6.0, 2.5)),
                  pool_min=4, top_k=8, nms_xy_m=0.0, nms_yaw_deg=0.0, targets=("w1",))


# ---------------------------------------------------------------------------------------------------------------- pruning pressure
def _pressure(name, edge, **kw):
    return _build(name, edge, vs=0.5, x_min=1.0, y_min=1.0, NX=19, NY=14, step=0.5, yaw_step=30.0, ground=(-8.0, 20.0, -8.0, 18.0),
                  scan=_scan(61, 110, 7.0, 0.5, 10.0),
                  echoes=[(4, 9, 7, 110), (0, 2, 11, 95), (7, 16, 3, 80), (10, 5, 4, 65), (2, 13, 12, 50), (9, 11, 1, 40)], clutter=250,
                  clutter_box=((-6.0, -6.0, 2.0), (18.0, 16.0, 12.0)), targets=("w1",), **kw)


@_case
def pool_1():
    return _pressure("pool_1", "pool_min = 1: the first threshold is the best leaf of one descent", pool_min=1, top_k=4, nms_xy_m=0.0, nms_yaw_deg=0.0)


@_case
def pool_64_topk_1024():
    return _pressure("pool_64_topk_1024", "pool_min = 64, top_k = 1024 without NMS: every leaf with score >= tau is output", pool_min=64, top_k=1024,
                     nms_xy_m=0.0, nms_yaw_deg=0.0)


@_case
def nms_wide_passes():
    return _pressure("nms_wide_passes", "a large NMS radius leaves fewer than top_k: the threshold drops and the pass repeats", pool_min=4, top_k=6,
                     nms_xy_m=3.0, nms_yaw_deg=180.0)


GLOBAL_NAMES = tuple(GLOBAL)
MULTI_LEVEL = ("top2_33x33", "top3_33x33", "width_w2_eq_w1")


@functools.lru_cache(maxsize=None)
def global_case(name):
    return GLOBAL[name]()


@functools.lru_cache(maxsize=None)
def mirror(name):
    """the case's Mirror over the lattice built in numpy from the documented formulas"""
    c = global_case(name)
    H, valid = rr.lattice(rr.stored_points(c.map, c.vs, c.cap), c.T_tilt, c.cfg)
    return rr.Mirror(rr.voxel_keys(c.map, c.vs), c.vs, rr.counted(c.scan, c.cfg, c.T_tilt), H, valid, c.cfg)


@functools.lru_cache(maxsize=None)
def searched(name):
    return mirror(name).search()


# ================================================================================================================ score cases (ScorePoses)
def _inside(keys, vs):
    """a point well inside every voxel of `keys` (truncation keys: key 0 spans (-vs, vs), a negative key k spans ((k - 1) vs, k vs])"""
    k = np.asarray(keys, dtype=np.float64)
    return _f32(np.where(k > 0, k + 0.5, np.where(k < 0, k - 0.5, 0.0)) * vs)


def _rz_exact(n):
    """the n-th quarter turn about z with exact 0 / +-1 entries"""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][n % 4]
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _quarter_poses(vs):
    """identity, exact quarter turns and the quarter turns of cos / sin (entries of 6e-17 where the exact ones have 0), at translations that
    are multiples of the voxel size: a point on a key face lands on a key face"""
    P = [_pose(np.eye(3), (0.0, 0.0, 0.0)), _pose(np.eye(3), (vs, -2 * vs, 3 * vs))]
    for n in (1, 2, 3):
        P.append(_pose(_rz_exact(n), (2 * vs * n, -vs, vs * n)))
        a = n * 90.0 * (math.pi / 180.0)
        P.append(_pose(np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]), (-vs * n, 3 * vs, 0.0)))
    return np.array(P)


def _score_case(name, edge, vs, scan, poses, hit, r_max=50.0, extra_keys=(), edge_points=(), **kw):
    """the map holds the voxels that the scan points `hit` (indices) read under every pose, plus extra_keys"""
    scan = _f32(scan)
    keys = rr.pose_keys(scan[np.asarray(hit, dtype=np.int64)], poses, vs).reshape(-1, 3) if len(hit) else np.zeros((0, 3), np.int64)
    if len(extra_keys):
        keys = np.concatenate([keys, np.asarray(extra_keys, dtype=np.int64).reshape(-1, 3)])
    return SimpleNamespace(name=name, edge=edge, vs=vs, map=_inside(np.unique(keys, axis=0), vs), scan=scan, poses=np.asarray(poses, dtype=np.float64),
                           r_max=r_max, edge_points=tuple(edge_points), **kw)


SCORE = {}


def _faces(vs):
    """every coordinate a float32 multiple of the voxel size (for 0.3: the float32 next to it): each point lies on three key faces"""
    rng = np.random.default_rng(int(vs * 100))
    scan = _f32(rng.integers(-9, 10, (96, 3)).astype(np.float64) * vs)
    return _score_case(f"faces_vs{vs}", f"points exactly on voxel faces, identity and quarter-turn poses, vs = {vs}", vs, scan, _quarter_poses(vs),
                       hit=np.arange(0, 96, 2), edge_points=range(0, 96, 2))


for _vs in (0.5, 0.25, 0.3):
    SCORE[f"faces_vs{_vs}"] = functools.partial(_faces, _vs)


def _band():
    """coordinates in (-2 vs, 2 vs) on the quarter-voxel grid: keys -1, 0, +1, with key 0 two voxels wide and the faces at +-vs"""
    vs = 0.5
    g = np.arange(-7, 8) * 0.125
    rng = np.random.default_rng(7)
    scan = rng.choice(g, (120, 3))
    poses = np.array([_pose(np.eye(3), (0.0, 0.0, 0.0)), _pose(_rz_exact(1), (0.0, 0.0, 0.0)), _pose(_rz_exact(2), (0.125, -0.125, 0.0)),
                      _pose(_rz_exact(3), (0.0, 0.5, -0.5)), _pose(np.eye(3), (-0.5, 0.0, 0.5))])
    on_face = [i for i in range(120) if np.any(np.abs(scan[i]) == 0.5)][:40]
    r = np.arange(-2, 3)
    board = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    board = board[board.sum(axis=1) % 2 == 0]  # a checkerboard of voxels: crossing any one face changes the answer
    return _score_case("band_vs0.5", "keys in the -1 / 0 / +1 band, where truncation makes key 0 two voxels wide", vs, scan, poses,
                       hit=[], extra_keys=board, edge_points=on_face)


SCORE["band_vs0.5"] = _band


def _tight_box():
    """A pose set whose key box is tight around the scan, and one far pose.  Under pose 0 the scan spans keys 2 .. 9 on x, so the box starts
    at key 1 (the margin); occupied voxels sit at the scan's outermost keys, in the margin (key 1 and its like) and one key outside the box
    (key 0): none of the last two may count.  The far pose stretches the box on x only; 50 x 10 x 7 cells is no multiple of 64."""
    vs = 0.5
    rng = np.random.default_rng(9)
    scan = np.round(rng.uniform((1.0, 1.0, 1.0), (4.74, 4.74, 3.24), (150, 3)) * 16.0) / 16.0
    scan[:6] = [(1.0, 1.0, 1.0), (4.75, 4.75, 3.25), (1.0, 4.75, 1.0), (4.75, 1.0, 3.25), (1.0, 1.0, 3.25), (4.75, 4.75, 1.0)]
    poses = np.array([_pose(np.eye(3), (0.0, 0.0, 0.0)), _pose(np.eye(3), (20.0, 0.0, 0.0)), _pose(np.eye(3), (0.0625, 0.0, 0.0))])
    margin = [(1, 2, 2), (1, 1, 1), (10, 10, 7), (5, 1, 3), (5, 10, 3), (5, 5, 1), (5, 5, 7), (50, 10, 7)]
    outside = [(0, 2, 2), (0, 0, 0), (5, 0, 3), (5, 11, 3), (5, 5, 0), (5, 5, 8), (51, 5, 3), (60, 5, 3)]
    return _score_case("tight_box", "occupied voxels in the hypothesis box's one-key margin and one key outside it; a far pose in the set", vs, scan,
                       poses, hit=np.arange(0, 150, 2), extra_keys=margin + outside, margin=margin, outside=outside)


SCORE["tight_box"] = _tight_box


def _rmax():
    """(30, 40, 0) lies at exactly 50 m and counts; the next float32 above 30 does not (float64 sum of squares against 2500)"""
    up = float(np.nextafter(np.float32(30.0), np.float32(np.inf)))
    dn = float(np.nextafter(np.float32(30.0), np.float32(0.0)))
    scan = [(30.0, 40.0, 0.0), (up, 40.0, 0.0), (dn, 40.0, 0.0), (40.0, 30.0, 0.0), (0.0, 30.0, 40.0), (0.0, up, 40.0), (0.0, 0.0, 50.0),
            (0.0, 0.0, float(np.nextafter(np.float32(50.0), np.float32(np.inf)))), (3.0, 4.0, 0.0), (-30.0, -40.0, 0.0), (-up, -40.0, 0.0)]
    poses = np.array([_pose(np.eye(3), (0.0, 0.0, 0.0)), _pose(_rz_exact(1), (1.0, 0.0, 0.0)), _pose(_rz_exact(2), (0.0, 0.5, 0.0))])
    return _score_case("r_max", "a point at exactly r_max = 50 m and the next float32 beyond it", 1.0, scan, poses, hit=np.arange(len(scan)),
                       edge_points=(0, 3, 4, 6, 9), sphere=True)


SCORE["r_max"] = _rmax

N_COUNTED = (1, 255, 256, 257, 2047, 2048, 2049)
N_POSES = (1, 31, 32, 33)


def _blocks(n, p):
    """n counted points (a chunk is 2048, a wave 64, a workgroup pass 256) x p poses (a workgroup takes 32): every point reads a voxel of its own
    under pose 0 and under the last pose, so a point or a pose dropped at a block edge shows in the score"""
    rng = np.random.default_rng(1000 * p + n)
    scan = np.round(rng.uniform(-12.0, 12.0, (n, 3)) * 8.0) / 8.0
    # three points beyond r_max among them: the counted points are not a prefix of the scan
    scan = np.insert(scan, [min(1, n), n // 2, n], [(80.0, 0.0, 0.0), (0.0, -70.0, 1.0), (0.0, 0.0, 90.0)], axis=0)
    poses = [_pose(np.eye(3), (0.25, 0.0, 0.5))]
    for q in range(1, p):
        a = rng.uniform(-math.pi, math.pi)
        poses.append(_pose(np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]), rng.uniform(-2.0, 2.0, 3)))
    if p > 1:
        poses[-1] = _pose(_rz_exact(1), (0.0, 0.25, -0.5))
    poses = np.array(poses)
    near = np.flatnonzero(np.abs(scan).max(axis=1) < 50.0)
    keys = rr.pose_keys(_f32(scan)[near], poses[[0, -1]], 0.5).reshape(-1, 3)
    return SimpleNamespace(name=f"blocks_n{n}_p{p}", edge="chunk, wave and hypothesis-block edges", vs=0.5, map=_inside(np.unique(keys, axis=0), 0.5),
                           scan=_f32(scan), poses=poses, r_max=50.0, edge_points=(), n_counted=n)


for _n in N_COUNTED:
    for _p in N_POSES:
        SCORE[f"blocks_n{_n}_p{_p}"] = functools.partial(_blocks, _n, _p)

SCORE_NAMES = tuple(SCORE)


@functools.lru_cache(maxsize=None)
def score_case(name):
    return SCORE[name]()


@functools.lru_cache(maxsize=None)
def score_ref(name):
    c = score_case(name)
    return rr.mirror_scores(c.map, c.vs, c.scan, c.poses, c.r_max)
