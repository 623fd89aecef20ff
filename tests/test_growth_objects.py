"""Growth objects on the GPU (elm_growth_find_objects / _objects / _cell_objects / _beam_objects): the object records, the stats, the cell
map and the beam map against the numpy mirror of the contract (tests/objects_ref.py), exactly.  Exact cell sets are built the way
tests/test_growth.py builds contended cells: a growth object on an empty map, clearance 0, scans whose points are cell centres, repeated
to set hit, at the identity or a translated pose; no beam walks (end_margin_frac 1), so through is 0 and the members are chosen by hit
alone.  The mirror runs on the cell set as it was constructed, after the table's download is checked against it.  In the scenes the
candidates are whatever the scans make them (tests/test_growth.py checks those against the growth mirror); there the objects mirror
runs on the downloaded cells and counters."""
import ctypes as C

import numpy as np
import pytest

import growth_ref
import objects_ref
import ray_ref  # tests/ is on sys.path via conftest
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import (Context, GrowthConfig, GrowthObjectRule, IcpMethod, Registration, RegistrationConfig, Scan,
                                        VoxelHashMap)
from test_growth import _noisy, box_cells, box_scene

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
CELL = 0.25  # voxel 1.0, sub 4
ORIGIN = (2.0 ** -7, 2.0 ** -6, 2.0 ** -5)  # float32 values, and no cell centre
M = (1 << 20) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def empty(ctx):
    return VoxelHashMap(1.0, 20, ctx)


@pytest.fixture(scope="module")
def field300k():
    return synth.make_field_world(300_000, seed=4242)


@pytest.fixture(scope="module")
def field_map(ctx, field300k):
    vm = VoxelHashMap(1.0, 20, ctx)
    vm.AddPoints(field300k)
    return vm, vm.Pointcloud()


def _cfg(**kw):
    """every end point observes and is new, no beam walks"""
    c = dict(clearance_cells=0, obs_min_range_m=0.0, obs_max_range_m=1e7, end_margin_frac=1.0, origin=ORIGIN)
    c.update(kw)
    return GrowthConfig(**c)


def _rules(**kw):
    return GrowthObjectRule(**kw), objects_ref.Rule(**kw)


def _pose(shift=(0, 0, 0)):
    T = np.eye(4)
    T[:3, 3] = np.asarray(shift, dtype=np.float64) * CELL  # a translation on the cell lattice: q = p + t is exact
    return T


def _centres(cells, shift=(0, 0, 0)):
    """the float32 centres of `cells` as seen from a sensor translated by `shift` cells"""
    return ((np.asarray(cells, dtype=np.int64).reshape(-1, 3) - np.asarray(shift) + 0.5) * CELL).astype(np.float32)


def _sorted(cells, hit):
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    hit = np.broadcast_to(np.asarray(hit, dtype=np.int64), (len(cells),))
    order = np.lexsort(cells.T[::-1])
    assert len(np.unique(cells, axis=0)) == len(cells)
    return cells[order], hit[order]


def _feed(g, cells, hit, shift=(0, 0, 0), per_call=None):
    """hit[i] beams into cell i, in calls that the capacity guard admits (count + beams <= capacity)"""
    pts = _centres(np.repeat(np.asarray(cells, dtype=np.int64).reshape(-1, 3), np.broadcast_to(hit, (len(cells),)), axis=0), shift)
    a = 0
    while a < len(pts):
        room = g.capacity - g.Count()
        assert room > 0
        b = min(len(pts), a + (room if per_call is None else min(room, per_call)))
        g.Accumulate(pts[a:b], _pose(shift), _cfg())
        a = b


def _made(g, cells, hit):
    """the table holds exactly the constructed set"""
    cells, hit = _sorted(cells, hit)
    got, h, t, _ = g.Cells()
    assert np.array_equal(got, cells) and np.array_equal(h, hit) and not t.any()
    return cells, hit


def _same(g, m, rule, beams=()):
    """one labelling on the device against the mirror's: stats, object records, cell map and, per (scan, pose, cfg), the beam map"""
    st = g.FindObjects(rule)
    assert st == m.stats, (st, m.stats)
    objs = g.Objects()
    assert tuple(objs) == objects_ref.OBJECT_FIELDS
    for f in objects_ref.OBJECT_FIELDS:
        assert objs[f].dtype == m.objects[f].dtype and np.array_equal(objs[f], m.objects[f]), (f, objs[f], m.objects[f])
    cm = g.CellObjects()
    assert cm.dtype == np.int32 and np.array_equal(cm, m.cell_map), int(np.count_nonzero(cm != m.cell_map))
    out = []
    for sc, T, cfg in beams:
        sc = sc if isinstance(sc, Scan) else Scan(g.ctx, sc)
        bm = g.BeamObjects(sc, T, cfg)
        want = m.beams(cfg, CELL, sc.points(), T)
        assert bm.dtype == np.int32 and np.array_equal(bm, want), int(np.count_nonzero(bm != want))
        out.append(bm)
    return st, objs, cm, out


def _in_order(sc, pts, values):
    """values (one per resident point of sc) in the order of pts, the distinct points sc was made from"""
    key = np.dtype((np.void, 12))
    res = np.ascontiguousarray(sc.points()).view(key).ravel()
    own = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3).view(key).ravel()
    order = np.argsort(res, kind="stable")
    at = order[np.searchsorted(res[order], own)]
    assert np.array_equal(res[at], own)
    return values[at]


def _exact(empty, cells, hit, beams_cells=None, capacity=None, shift=(0, 0, 0), **rule_kw):
    """the constructed set on a fresh growth object, labelled under the rule, GPU == mirror on everything; the beam map of one beam per
    cell of beams_cells (default: the set's own cells), returned in that order"""
    n_beams = int(np.broadcast_to(hit, (len(cells),)).sum())
    g = empty.Growth(capacity if capacity is not None else max(n_beams, 1))
    _feed(g, cells, hit, shift)
    cells_s, hit_s = _made(g, cells, hit)
    rule, mrule = _rules(**rule_kw)
    m = objects_ref.Objects(cells_s, hit_s, np.zeros(len(hit_s)), mrule)
    look = cells_s if beams_cells is None else np.asarray(beams_cells, dtype=np.int64).reshape(-1, 3)
    sc = Scan(g.ctx, _centres(look, shift))
    st, objs, cm, (bm,) = _same(g, m, rule, [(sc, _pose(shift), _cfg())])
    g.close()
    return st, objs, cm, _in_order(sc, _centres(look, shift), bm), cells_s


OFFSETS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
LIMIT = {6: 1, 18: 2, 26: 3}


# ---------------------------------------------------------------- 1. connectivity
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_every_offset_under_every_connectivity(empty, connectivity):
    """The 26 two-cell cases {c, c + d} in one table, 10 cells apart along x (so across x = 0 and across many coarse-cell faces): pair k is
    one object exactly when |d|_1 <= 1 / 2 / 3."""
    base = np.array([(10 * k - 130, 2 * (k % 5) - 4, 3 - k % 7) for k in range(26)])
    cells = np.concatenate([base, base + np.array(OFFSETS)])
    st, objs, cm, bm, cells_s = _exact(empty, cells, 3, connectivity=connectivity)
    at = lambda c: cm[np.searchsorted(ray_ref.codes(cells_s), ray_ref.codes(c))]
    joined = np.array([sum(abs(x) for x in d) <= LIMIT[connectivity] for d in OFFSETS])
    assert np.array_equal(at(base) == at(base + np.array(OFFSETS)), joined)
    assert st == dict(n_members=52, n_objects=52 - int(joined.sum()), n_small=0, n_small_cells=0, max_cells=2)
    assert int(joined.sum()) == connectivity


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_a_cell_and_its_neighbours(empty, connectivity):
    c = np.array((-1, 3, 4))  # the 3 x 3 x 3 block around it spans x = -2 .. 0, y = 2 .. 4 and z = 3 .. 5: 0 and a coarse face on every axis
    off = np.array(OFFSETS)
    l1 = np.abs(off).sum(axis=1)
    # the centre with all 26 neighbours is a full block: its cells hang together by faces alone, one object under every connectivity
    st, objs, _, _, _ = _exact(empty, np.concatenate([c[None], c + off]), 3, connectivity=connectivity)
    assert st["n_objects"] == 1 and objs["n_cells"].tolist() == [27] and objs["lo"].tolist() == [[-2, 2, 3]] and objs["hi"].tolist() == [[0, 4, 5]]
    # the centre with its 8 corner neighbours: |d|_1 = 3, and two corners are 2 apart: one object under 26, nine otherwise
    st, _, _, _, _ = _exact(empty, np.concatenate([c[None], c + off[l1 == 3]]), 3, connectivity=connectivity)
    assert st["n_objects"] == (1 if connectivity == 26 else 9)
    # the centre with its 12 edge neighbours: |d|_1 = 2, and no two of them share a face: one object under 18 and 26, thirteen under 6
    st, _, _, _, _ = _exact(empty, np.concatenate([c[None], c + off[l1 == 2]]), 3, connectivity=connectivity)
    assert st["n_objects"] == (13 if connectivity == 6 else 1)


# ---------------------------------------------------------------- 2. members
def test_a_cell_that_is_no_member_connects_nothing(empty):
    blob = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    bridge = np.array([(2, 0, 0)])
    cells = np.concatenate([blob, bridge, blob + (3, 0, 0)])
    hit = np.array([3] * 8 + [1] + [3] * 8)
    st, objs, cm, bm, cells_s = _exact(empty, cells, hit)  # min_hit 3: the bridge has hit 1
    i = int(np.flatnonzero((cells_s == bridge[0]).all(axis=1))[0])
    assert st == dict(n_members=16, n_objects=2, n_small=0, n_small_cells=0, max_cells=8) and cm[i] == -1 and bm[i] == -1
    assert objs["label"].tolist() == [[0, 0, 0], [3, 0, 0]] and objs["hit"].tolist() == [24, 24]
    st, objs, cm, bm, _ = _exact(empty, cells, hit, min_hit=1)
    assert st == dict(n_members=17, n_objects=1, n_small=0, n_small_cells=0, max_cells=17) and cm[i] == 0 and bm[i] == 0
    assert objs["hit"].tolist() == [49] and objs["lo"].tolist() == [[0, 0, 0]] and objs["hi"].tolist() == [[4, 1, 1]]


# ---------------------------------------------------------------- 3. min_cells
def test_min_cells_at_the_threshold(ctx, empty):
    three, four = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)]), np.array([(0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0)])  # two lines, a free line between
    cells = np.concatenate([three, four])
    st, objs, cm, bm, _ = _exact(empty, cells, 3, connectivity=26, min_cells=4)
    assert st == dict(n_members=7, n_objects=1, n_small=1, n_small_cells=3, max_cells=4)
    assert cm.tolist() == [-2, 0, -2, 0, -2, 0, 0] and bm.tolist() == cm.tolist() and objs["label"].tolist() == [[0, 2, 0]]
    st, objs, cm, bm, _ = _exact(empty, cells, 3, connectivity=26, min_cells=3)
    assert st == dict(n_members=7, n_objects=2, n_small=0, n_small_cells=0, max_cells=4) and cm.tolist() == [0, 1, 0, 1, 0, 1, 1]
    st, objs, cm, bm, _ = _exact(empty, cells, 3, connectivity=26, min_cells=5)
    assert st == dict(n_members=7, n_objects=0, n_small=2, n_small_cells=7, max_cells=4) and (cm == -2).all() and (bm == -2).all()
    assert objs["label"].shape == (0, 3)
    g = empty.Growth(16)
    with pytest.raises(ElmError):
        g.FindObjects(GrowthObjectRule(min_cells=0))
    g.close()


# ---------------------------------------------------------------- 4. where the union-find can go wrong
def serpentine(nx, ny, nz, n):
    """the first n cells of a face-connected path: rows along x at even y and even z, joined at alternating ends by one cell in y, the
    layers by one cell in z.  Two cells of it share a face only where the path runs from one to the next."""
    path, x_up, y_up = [], True, True
    for k in range(nz):
        ys = range(ny) if y_up else range(ny - 1, -1, -1)
        for jj, j in enumerate(ys):
            path += [(x, 2 * j, 2 * k) for x in (range(nx) if x_up else range(nx - 1, -1, -1))]
            if jj < ny - 1:
                path.append((path[-1][0], 2 * j + (1 if y_up else -1), 2 * k))
            x_up = not x_up
        if k < nz - 1:
            path.append((path[-1][0], path[-1][1], 2 * k + 1))
        y_up = not y_up
    return np.array(path[:n])


def _contacts(a, b, connectivity):
    ca = np.sort(ray_ref.codes(a))
    return sum(int(ray_ref.is_in(ca, ray_ref.codes(b + d)).sum()) for d in objects_ref.offsets(connectivity))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_two_serpentines_one_diagonal_apart(empty, connectivity):
    """2 000 cells folded in 3-D (20 x 10 rows x 10 layers), and its mirror image in y and z moved to y, z <= -1: the first rows of the two
    run along each other at d = (0, 1, 1) and nowhere do the two share a face."""
    s1 = serpentine(20, 10, 10, 2000)
    s2 = s1 * (1, -1, -1) + (0, -1, -1)
    assert len(np.unique(np.concatenate([s1, s2]), axis=0)) == 4000 and _contacts(s1, s2, 6) == 0 and _contacts(s1, s2, 26) >= 20
    st, objs, cm, _, _ = _exact(empty, np.concatenate([s1, s2]), 1, min_hit=1, connectivity=connectivity)
    if connectivity == 6:
        assert st == dict(n_members=4000, n_objects=2, n_small=0, n_small_cells=0, max_cells=2000) and objs["n_cells"].tolist() == [2000, 2000]
    else:
        assert st == dict(n_members=4000, n_objects=1, n_small=0, n_small_cells=0, max_cells=4000)


def test_ring_pairs_block_and_blobs(empty):
    # a closed ring of 40 cells in a plane: the last union joins what is joined already
    r = np.arange(11)
    ring = np.unique(np.concatenate([np.stack([r, 0 * r], 1), np.stack([r, 0 * r + 10], 1), np.stack([0 * r, r], 1), np.stack([0 * r + 10, r], 1)]), axis=0)
    ring = np.concatenate([ring, np.full((len(ring), 1), -1)], 1) - (5, 5, 0)
    st, objs, _, _, _ = _exact(empty, ring, 1, min_hit=1, connectivity=6)
    assert len(ring) == 40 and st["n_objects"] == 1 and objs["n_cells"].tolist() == [40]
    # 512 two-cell components in one launch, 3 cells apart
    i, j = np.meshgrid(np.arange(32), np.arange(16), indexing="ij")
    first = np.stack([3 * i.ravel() - 40, 3 * j.ravel() - 20, 0 * i.ravel() + 2], 1)
    st, objs, cm, _, _ = _exact(empty, np.concatenate([first, first + (1, 0, 0)]), 1, min_hit=1)
    assert st == dict(n_members=1024, n_objects=512, n_small=0, n_small_cells=0, max_cells=2) and (objs["n_cells"] == 2).all()
    assert np.array_equal(np.bincount(cm), np.full(512, 2))
    # a dense 16 x 16 x 16 block across the origin: 4 096 members, one root under contention
    a = np.arange(16) - 7
    block = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    st, objs, cm, _, _ = _exact(empty, block, 1, min_hit=1, connectivity=26)
    assert st == dict(n_members=4096, n_objects=1, n_small=0, n_small_cells=0, max_cells=4096) and objs["label"].tolist() == [[-7, -7, -7]]
    assert objs["cell_sum"].tolist() == [[4096 * (1 << 20) + 4096 // 16 * int(a.sum())] * 3] and objs["hit"].tolist() == [4096]
    # two blobs of 512 cells that touch through one single cell
    b = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    st, objs, _, _, _ = _exact(empty, np.concatenate([b, [(8, 3, 3)], b + (9, 0, 0)]), 1, min_hit=1, connectivity=6)
    assert st["n_objects"] == 1 and objs["n_cells"].tolist() == [1025]
    st, objs, _, _, _ = _exact(empty, np.concatenate([b, b + (9, 0, 0)]), 1, min_hit=1, connectivity=26)
    assert st["n_objects"] == 2 and objs["n_cells"].tolist() == [512, 512]


# ---------------------------------------------------------------- 5. placement
def test_placement_across_zero_coarse_faces_and_the_key_range(ctx, empty):
    two = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    # 2 x 2 x 2 blocks across e_r = -1 | 0 and across coarse-cell faces (e_r = 3 | 4, 7 | 8, -5 | -4) on every axis at once, 8 apart
    cells = np.concatenate([two + (-1, -1, -1), two + (3, 3, 3) + (8, 0, 0), two + (7, 7, 7) + (16, 0, 0), two + (-5, -5, -5) - (8, 0, 0)])
    st, objs, _, _, _ = _exact(empty, cells, 3, connectivity=6)
    assert st["n_objects"] == 4 and objs["n_cells"].tolist() == [8] * 4
    assert objs["label"].tolist() == [[-13, -5, -5], [-1, -1, -1], [11, 3, 3], [23, 7, 7]]
    # members at e_r = 2^20 - 1 and -(2^20 - 1), reached through translated poses: the neighbours beyond the range are never looked up
    g = empty.Growth(64)
    top = np.array([(M, M, M), (M - 1, M, M), (M, M - 1, M - 1)])        # a face and an edge neighbour of the corner cell
    bottom = np.array([(-M, -M, -M), (-M + 1, -M + 1, -M + 1), (-M, 5, -M)])  # a corner neighbour, and a cell on its own on two range faces
    _feed(g, top, 3, shift=(M - 2, M - 2, M - 2))
    _feed(g, bottom, 3, shift=(-M + 2, -M + 2, -M + 2))
    cells_s, hit_s = _made(g, np.concatenate([top, bottom]), 3)
    beams = [(_centres(top, (M - 2,) * 3), _pose((M - 2,) * 3), _cfg()), (_centres(bottom, (-M + 2,) * 3), _pose((-M + 2,) * 3), _cfg()),
             (_centres(top, (M - 2,) * 3), _pose((M - 1,) * 3), _cfg())]  # the last: one cell further on every axis, beyond the range for some
    for connectivity, want in ((6, [1, 1, 1, 1, 2]), (18, [1, 1, 1, 3]), (26, [1, 2, 3])):
        rule, mrule = _rules(connectivity=connectivity)
        st, objs, cm, bm = _same(g, objects_ref.Objects(cells_s, hit_s, np.zeros(6), mrule), rule, beams)
        assert sorted(objs["n_cells"].tolist()) == want
        assert (bm[0] >= 0).all() and (bm[1] >= 0).all() and (bm[2] == -1).all()
    assert objs["cell_sum"].tolist()[0] == [3, 3, 3] and objs["hi"].tolist()[-1] == [M, M, M]
    g.close()


# ---------------------------------------------------------------- 6. layout and order
def test_independent_of_capacity_order_and_probe_chains(ctx, empty):
    rng = np.random.default_rng(17)
    cells = np.unique(np.cumsum(rng.integers(-1, 2, (400, 3)), axis=0)[::3] + rng.integers(-1, 2, (134, 3)), axis=0)[:60]  # a loose trail: several components
    assert len(cells) == 60
    rule, mrule = _rules(min_hit=1, connectivity=18, min_cells=2)
    cs, hs = _sorted(cells, 1)
    m = objects_ref.Objects(cs, hs, np.zeros(60), mrule)
    assert m.stats["n_objects"] >= 2 and m.stats["n_small"] >= 1
    look = Scan(ctx, _centres(np.concatenate([cells, cells + (1, 0, 0)])))
    results = []

    def done(g):
        _made(g, cells, 1)
        st, objs, cm, (bm,) = _same(g, m, rule, [(look, _pose(), _cfg())])
        results.append(b"".join(objs[f].tobytes() for f in objects_ref.OBJECT_FIELDS) + cm.tobytes() + bm.tobytes())
        g.close()

    for capacity, per_call in ((64, None), (4096, None), (64, 4)):  # 60 cells in 128 slots (at once, and 4 beams a call), and in 8 192
        g = empty.Growth(capacity)
        _feed(g, cells, 1, per_call=per_call)
        done(g)
    mixed = rng.permutation(cells)
    jobs = [_centres(mixed[a:b]) for a, b in ((0, 7), (7, 8), (8, 40), (40, 60))]
    for order in (slice(None), slice(None, None, -1)):  # one batch, and the reversed batch
        g = empty.Growth(4096)
        g.Accumulate(jobs[order], np.stack([_pose()] * 4), _cfg())
        done(g)
    assert len(results) == 5 and all(r == results[0] for r in results)


# ---------------------------------------------------------------- 7. the beam map
def test_beam_map_sizes_and_edge_beams(ctx, empty):
    """Objects 12 .. 16 m from the origin, a candidate that is no member (hit 1), a single cell (small under min_cells 2) and two members at
    70 m, outside the default observing window.  Scans of random picks among beams that end anywhere in those cells, in cells that are no
    candidates, at NaN / inf, at the origin itself and outside the window."""
    blob = np.stack(np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    objs_cells = np.concatenate([blob + (50, 0, 0), blob + (50, 8, 1), blob + (-60, 3, 3)])
    weak, single, far = np.array([(53, 0, 0)]), np.array([(40, 40, 2)]), np.array([(280, 0, 0), (281, 0, 0)])
    cells = np.concatenate([objs_cells, weak, single, far])
    hit = np.array([3] * len(objs_cells) + [1, 3, 3, 3])
    g = empty.Growth(4096)
    _feed(g, cells, hit)
    cells_s, hit_s = _made(g, cells, hit)
    rule, mrule = _rules(min_cells=2)
    m = objects_ref.Objects(cells_s, hit_s, np.zeros(len(hit_s)), mrule)
    rng = np.random.default_rng(23)
    nan, inf = float("nan"), float("inf")
    bad = np.array([(nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 2.0, -inf), ORIGIN, (nan, nan, nan), (0.3, 0.1, 0.2), (0.0, 0.0, 60.0)], np.float32)

    def scan(n):
        pick = np.concatenate([cells, cells + (0, 0, 4), cells + (1, 1, 0)])[rng.integers(0, 3 * len(cells), n)]
        p = ((pick + rng.uniform(0.05, 0.95, (n, 3))) * CELL).astype(np.float32)
        k = rng.integers(0, n, max(n // 8, 1) if n > 1 else 0)
        p[k] = bad[rng.integers(0, len(bad), len(k))]
        return p

    narrow = GrowthConfig(clearance_cells=0, origin=ORIGIN)  # the default window: 2 .. 50 m
    seen = set()
    for n in (1, 255, 256, 257, 3001):
        sc = Scan(ctx, scan(n))
        _, _, _, (wide, near) = _same(g, m, rule, [(sc, _pose(), _cfg()), (sc, _pose(), narrow)])
        assert wide.shape == (n,)
        seen |= set(wide.tolist())
        res = sc.points()
        ends_far = (np.floor(res.astype(np.float64) / CELL) == far[0]).all(axis=1)
        assert (near[ends_far] == -1).all() and (wide[ends_far] == 3).all()
    assert seen == {-2, -1, 0, 1, 2, 3}
    # the categories one by one, in a scan of their own: object, no candidate, weak candidate, small, outside the window, NaN, inf, zero length
    one = np.concatenate([_centres([(50, 0, 0), (50, 0, 9), weak[0], single[0], far[0]]), bad[[0, 1, 3]]])
    sc = Scan(ctx, one)
    _, _, _, (wide, near) = _same(g, m, rule, [(sc, _pose(), _cfg()), (sc, _pose(), narrow)])
    at = lambda p: int(np.flatnonzero((sc.points().view(np.uint32) == np.asarray(p, np.float32).view(np.uint32)).all(axis=1))[0])
    assert [int(wide[at(p)]) for p in one[:5]] == [1, -1, -1, -2, 3] and [int(near[at(p)]) for p in one[:5]] == [1, -1, -1, -2, -1]
    assert all(wide[at(p)] == -1 for p in one[6:]) and (wide[~np.isfinite(sc.points()).all(axis=1)] == -1).all()
    # an empty scan
    assert g.BeamObjects(np.zeros((0, 3), np.float32), _pose(), _cfg()).shape == (0,)
    g.close()


# ---------------------------------------------------------------- 8. state and misuse
def test_state_misuse_and_the_context_stays_usable(ctx, empty):
    L = _lib.lib()
    cells = np.array([(0, 0, 0), (1, 0, 0), (5, 5, 5)])
    g = empty.Growth(64)
    _feed(g, cells, 3)
    sc = Scan(ctx, _centres(cells))
    cfg = _cfg()
    T16 = np.ascontiguousarray(np.eye(4)).ravel()
    dp = T16.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_size_t(0)
    out = (C.c_int32 * 8)()
    rule, mrule = _rules()

    def reads(c=ctx, h=g, s=sc, pose=dp, cf=cfg):
        return (L.elm_growth_objects(c._h, h._h, None, 0, C.byref(n)), L.elm_growth_cell_objects(c._h, h._h, None, 0, C.byref(n)),
                L.elm_growth_beam_objects(c._h, h._h, s._h, pose, C.byref(cf), out))

    def refused():
        assert reads() == (INVALID,) * 3 and "no objects are held" in L.elm_last_error(ctx._h).decode()
        for call in (g.Objects, g.CellObjects, lambda: g.BeamObjects(sc, np.eye(4), cfg)):
            with pytest.raises(ElmError):
                call()

    refused()  # before any find
    m = objects_ref.Objects(*_sorted(cells, 3), np.zeros(3), mrule)
    _same(g, m, rule, [(sc, np.eye(4), cfg)])
    assert reads() == (0, 0, 0) and n.value == 3
    # min(cap, count) written, *n = count
    objs = (_lib.GrowthObjectC * 2)()
    objs[1].n_cells = 77
    assert L.elm_growth_objects(ctx._h, g._h, objs, 1, C.byref(n)) == 0 and n.value == 2 and objs[0].n_cells == 2 and objs[1].n_cells == 77
    cm = (C.c_int32 * 3)(9, 9, 9)
    assert L.elm_growth_cell_objects(ctx._h, g._h, cm, 2, C.byref(n)) == 0 and n.value == 3 and list(cm) == [0, 0, 9]
    # a second find with another rule replaces the first
    rule2, mrule2 = _rules(min_cells=2, connectivity=6)
    st, _, cm2, _ = _same(g, objects_ref.Objects(*_sorted(cells, 3), np.zeros(3), mrule2), rule2, [(sc, np.eye(4), cfg)])
    assert st["n_objects"] == 1 and st["n_small"] == 1 and cm2.tolist() == [0, 0, -2]
    # misuse: every refusal leaves the result held
    assert L.elm_growth_find_objects(ctx._h, g._h, C.byref(GrowthObjectRule(connectivity=7)), None) == INVALID
    assert L.elm_growth_find_objects(ctx._h, g._h, C.byref(GrowthObjectRule(min_cells=0)), None) == INVALID
    assert reads(cf=_cfg(sub=2))[2] == INVALID
    for bad in (float("nan"), float("inf")):
        B16 = T16.copy()
        B16[13] = bad
        assert reads(pose=B16.ctypes.data_as(C.POINTER(C.c_double)))[2] == INVALID
    other = Context(0)
    osc = Scan(other, _centres(cells))
    assert reads(c=other) == (INVALID,) * 3 and reads(s=osc)[2] == INVALID
    assert L.elm_growth_find_objects(other._h, g._h, C.byref(rule), None) == INVALID
    other.set_allreduce_hook(lambda p, n_, s: 0)
    assert L.elm_growth_find_objects(other._h, g._h, C.byref(rule), None) == UNSUPPORTED and "one rank" in L.elm_last_error(other._h).decode()
    assert reads(c=other) == (UNSUPPORTED,) * 3
    other.set_allreduce_hook(None)
    del osc
    other.close()
    grp = Context.multi([0, 0])
    assert L.elm_growth_find_objects(grp._h, g._h, C.byref(rule), None) == UNSUPPORTED and "one rank" in L.elm_last_error(grp._h).decode()
    grp.close()
    world = synth.make_world(30_000, seed=11)
    small = VoxelHashMap(1.0, 30, ctx)
    small.AddPoints(world)
    scan, T = synth.make_scan(world, 512, seed=12)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx=ctx)
    reg.EnqueueBatch([Scan(ctx, scan)], small, T[None])
    assert L.elm_growth_find_objects(ctx._h, g._h, C.byref(rule), None) == INVALID and reads() == (INVALID,) * 3  # a batch in flight
    reg.FinishBatch()
    assert reads() == (0, 0, 0) and np.array_equal(g.CellObjects(), cm2)
    # Accumulate and Reset drop the result
    g.Accumulate(_centres([(1, 1, 0)] * 3), np.eye(4), cfg)
    refused()
    cells4 = np.concatenate([cells, [(1, 1, 0)]])
    st, _, _, _ = _same(g, objects_ref.Objects(*_sorted(cells4, 3), np.zeros(4), mrule), rule, [(sc, np.eye(4), cfg)])
    assert st["n_objects"] == 2 and st["max_cells"] == 3
    g.Accumulate([_centres([(9, 9, 9)])], np.eye(4)[None], cfg)  # a batch drops it too
    refused()
    g.FindObjects()
    g.Reset()
    refused()
    # the empty object
    m0 = objects_ref.Objects(np.zeros((0, 3)), np.zeros(0), np.zeros(0), mrule)
    st, objs, cm, (bm,) = _same(g, m0, rule, [(sc, np.eye(4), cfg)])
    assert st == dict.fromkeys(objects_ref.STAT_FIELDS, 0) and objs["label"].shape == (0, 3) and cm.shape == (0,) and (bm == -1).all()
    fresh = empty.Growth(16)
    assert fresh.FindObjects() == st and fresh.Objects()["hit"].shape == (0,)
    fresh.close()
    # the Python layer refuses a rebuilt map and a closed object
    tmp = VoxelHashMap(1.0, 30, ctx)
    tmp.AddPoints(world[:1000])
    tg = tmp.Growth(64)
    tg.FindObjects()
    tmp.AddPoints(world[1000:2000])
    for call in (tg.FindObjects, tg.Objects, tg.CellObjects, lambda: tg.BeamObjects(sc, np.eye(4))):
        with pytest.raises(ElmError):
            call()
    tg.close()
    with pytest.raises(ElmError):
        tg.FindObjects()
    # the context and the object are usable afterwards, with the answer of the mirror
    _feed(g, cells, 3)
    _same(g, m, rule, [(sc, np.eye(4), cfg)])
    g.close()


# ---------------------------------------------------------------- 9. scenes
def _scene_same(g, rule_kw, beams):
    """the mirror on the table as the scans made it (its cells and counters are test_growth.py's subject), then GPU == mirror"""
    cells, hit, through, _ = g.Cells()
    rule, mrule = _rules(**rule_kw)
    m = objects_ref.Objects(cells, hit, through, mrule)
    st, objs, cm, bms = _same(g, m, rule, beams)
    return cells, hit, through, st, objs, cm, bms


def _figures(name, st, objs, n_appeared):
    largest = int(objs["n_cells"].max()) if st["n_objects"] else 0
    print(name, "appeared cells", n_appeared, "objects", st["n_objects"], "largest", largest, "share", round(largest / max(n_appeared, 1), 4), st)


@pytest.fixture(scope="module")
def box1(ctx, field300k, field_map):
    """the box scene of tests/test_growth.py, seed 1: the twelve rendered scans, their poses and the box's cells"""
    vm_a, stored_a = field_map
    box, poses = box_scene(vm_a, 1)
    vm_b = VoxelHashMap(1.0, 20, ctx)
    vm_b.AddPoints(np.concatenate([field300k, box]))
    beams = synth.lidar_beams(32, 512)
    scans = [Scan(ctx, vm_b.RenderScan(P, beams)) for P in poses]
    return scans, poses, box_cells(stored_a, vm_b.Pointcloud())


def test_scene_one_box(ctx, field_map, box1):
    vm_a, _ = field_map
    scans, poses, bx = box1
    cfg = GrowthConfig()
    g = vm_a.Growth(sum(s.n for s in scans))
    g.Accumulate(scans, poses, cfg)
    cells, hit, through, st, objs, cm, _ = _scene_same(g, {}, [(scans[0], poses[0], cfg), (scans[7], poses[7], cfg)])
    appeared = growth_ref.appeared_cells(hit, through)
    assert st["n_objects"] >= 1 and appeared.sum() > 100
    # DESIGN.md section 16 records that this scene has no candidate outside the box: every object lies inside the box's cells' bounding box
    assert (objs["lo"] >= bx.min(axis=0)).all() and (objs["hi"] <= bx.max(axis=0)).all()
    assert int(objs["n_cells"].sum()) + st["n_small_cells"] == int(appeared.sum()) == st["n_members"]
    _figures("one box (seed 1, 12 scans)", st, objs, int(appeared.sum()))
    st5 = g.FindObjects(GrowthObjectRule(min_cells=5))
    print("  min_cells 5:", st5)
    g.close()


def test_scene_two_boxes(ctx, field300k, field_map):
    vm_a, stored_a = field_map
    (b1, p1), (b2, p2) = box_scene(vm_a, 1), box_scene(vm_a, 2)
    vm_b = VoxelHashMap(1.0, 20, ctx)
    vm_b.AddPoints(np.concatenate([field300k, b1, b2]))
    bx = box_cells(stored_a, vm_b.Pointcloud())
    # the box's cells, told apart by the box whose footprint (grown by a cell) they stand in
    inside = lambda b: ((bx[:, :2] >= np.floor(b[:, :2].min(axis=0) / CELL) - 1) & (bx[:, :2] <= np.floor(b[:, :2].max(axis=0) / CELL) + 1)).all(axis=1)
    in1, in2 = inside(b1), inside(b2)
    assert (in1 ^ in2).all() and in1.sum() > 200 and in2.sum() > 200
    s1, s2 = bx[in1], bx[in2]
    gap = np.maximum(s1.min(axis=0) - s2.max(axis=0), s2.min(axis=0) - s1.max(axis=0)).max()
    assert gap >= 2  # at least 2 cells apart in the Chebyshev sense: no connectivity joins them
    beams = synth.lidar_beams(32, 512)
    poses = np.concatenate([p1[::2], p2[::2]])
    scans = [Scan(ctx, vm_b.RenderScan(P, beams)) for P in poses]
    cfg = GrowthConfig()
    g = vm_a.Growth(sum(s.n for s in scans))
    g.Accumulate(scans, poses, cfg)
    cells, hit, through, st, objs, cm, _ = _scene_same(g, {}, [(scans[0], poses[0], cfg), (scans[6], poses[6], cfg)])
    appeared = growth_ref.appeared_cells(hit, through)
    assert st["n_objects"] >= 2
    c1, c2 = np.sort(ray_ref.codes(s1)), np.sort(ray_ref.codes(s2))
    of1, of2 = ray_ref.is_in(c1, ray_ref.codes(cells)), ray_ref.is_in(c2, ray_ref.codes(cells))
    k1, k2 = set(cm[of1 & (cm >= 0)].tolist()), set(cm[of2 & (cm >= 0)].tolist())
    assert k1 and k2 and not (k1 & k2)  # no object has member cells in both boxes
    _figures("two boxes (seeds 1 and 2, 6 + 6 scans)", st, objs, int(appeared.sum()))
    g.close()


def _foreground(vm, sc, T):
    """a fresh object fed one scan, the rule {1, 0, 26, 1}: the objects are the scan's returns that the map does not explain"""
    cfg = GrowthConfig()
    g = vm.Growth(max(sc.n, 1))
    acc = g.Accumulate(sc, T, cfg)
    cells, hit, through, st, objs, cm, (bm,) = _scene_same(g, dict(min_hit=1, hit_per_through=0, connectivity=26, min_cells=1), [(sc, T, cfg)])
    assert acc["n_end_new"] > 0 and int((bm >= 0).sum()) == acc["n_end_new"] and int(objs["hit"].sum()) == acc["n_end_new"]
    assert st["n_members"] == len(cells) and st["n_small"] == 0 and not (bm == -2).any()
    g.close()
    return acc, st, objs


def test_scene_foreground_of_one_scan(field_map, box1):
    vm_a, _ = field_map
    scans, poses, _ = box1
    acc, st, objs = _foreground(vm_a, scans[0], poses[0])
    _figures("foreground of one scan (END-NEW beams %d)" % acc["n_end_new"], st, objs, st["n_members"])


# ---------------------------------------------------------------- 10. index forms
@pytest.mark.parametrize("env", [("ELM_KERNEL", "lists"), ("ELM_GRID", "tiled")])
def test_same_result_under_every_index_form(monkeypatch, field300k, env):
    monkeypatch.setenv(*env)
    c = Context(0)
    scan, T = synth.make_scan(field300k, 3000, seed=31)
    vm = VoxelHashMap(1.0, 20, c)
    vm.AddPoints(field300k)
    vm.BuildNeighbourhoods()
    acc, st, objs = _foreground(vm, Scan(c, _noisy(scan, seed=32)), T)
    assert acc["n_end_new"] > 300 and st["n_objects"] > 10
    del vm
    c.close()
