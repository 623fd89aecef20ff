"""A numpy mirror of the growth-objects contract (include/elimaloc_hip.h, "map growth: objects"), written from the header's text; shared by
tests/test_growth_objects.py (GPU against it) and tests/test_growth_objects_abi.py (it against cases worked out by hand and against
scipy.ndimage.label).  Its input is a growth mirror (growth_ref.Growth) or any sorted cell set with counters.  Components come from label
propagation over the sorted codes: every member's label is the index of the smallest member it is known to be connected to, and "label =
min over self and adjacent members" is iterated to its fixed point (with a jump label = label[label] per round, which changes the number
of rounds and not the fixed point).  No union-find."""
import math

import numpy as np

import growth_ref
from ray_ref import codes, rays

LIM = growth_ref.LIM
STAT_FIELDS = ("n_members", "n_objects", "n_small", "n_small_cells", "max_cells")
OBJECT_FIELDS = ("label", "n_cells", "lo", "hi", "hit", "through", "cell_sum")


class Rule:
    """a plain object with elm_growth_object_rule's fields and defaults"""

    def __init__(self, **kw):
        self.min_hit, self.hit_per_through, self.connectivity, self.min_cells = 3, 4, 26, 1
        self.__dict__.update(kw)


def offsets(connectivity):
    """every d != 0 with max |d_r| <= 1 and |d_x| + |d_y| + |d_z| <= 1 / 2 / 3 for connectivity 6 / 18 / 26"""
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    r = (-1, 0, 1)
    return np.array([(x, y, z) for x in r for y in r for z in r if 0 < abs(x) + abs(y) + abs(z) <= limit], np.int64)


def components(cells, connectivity):
    """cells int [m, 3], distinct, ascending (x, y, z), every |c_r| < 2^20 -> int64 [m]: for every cell the index of the smallest cell of
    its component"""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    m = len(cells)
    lab = np.arange(m, dtype=np.int64)
    if m == 0:
        return lab
    code = codes(cells)
    assert (np.diff(code) > 0).all()
    nbr = []  # per offset: (the cells that have that neighbour, the neighbour's index)
    for d in offsets(connectivity):
        c = cells + d
        ok = np.flatnonzero((np.abs(c) < LIM).all(axis=1))  # a cell beyond the key range is no cell
        k = codes(c[ok])
        i = np.minimum(np.searchsorted(code, k), m - 1)
        hit = code[i] == k
        nbr.append((ok[hit], i[hit]))
    while True:
        new = lab.copy()
        for a, b in nbr:
            np.minimum.at(new, a, lab[b])
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


class Objects:
    """The result of one labelling: stats (dict of STAT_FIELDS), objects (dict of OBJECT_FIELDS arrays, ascending label), cell_map int32
    [count] in the growth mirror's cell order."""

    def __init__(self, cells, hit, through, rule):
        assert rule.connectivity in (6, 18, 26) and rule.min_cells >= 1
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
        self.code = codes(cells)
        member = growth_ref.appeared_cells(hit, through, rule.min_hit, rule.hit_per_through)
        idx = np.flatnonzero(member)
        mc = cells[idx]
        lab = components(mc, rule.connectivity)
        roots, inv, n_cells = np.unique(lab, return_inverse=True, return_counts=True)  # ascending root index = ascending label
        listed = n_cells >= rule.min_cells
        rank = np.where(listed, np.cumsum(listed) - 1, -2)
        k = len(roots)
        h64, t64 = np.asarray(hit, dtype=np.uint64)[idx], np.asarray(through, dtype=np.uint64)[idx]
        def osum(v):  # per component, the sum of the members' rows of v (uint64)
            out = np.zeros((k,) + v.shape[1:], np.uint64)
            np.add.at(out, inv, v)
            return out

        lo, hi = np.full((k, 3), LIM, np.int64), np.full((k, 3), -LIM, np.int64)
        np.minimum.at(lo, inv, mc)
        np.maximum.at(hi, inv, mc)
        full = dict(label=mc[roots].astype(np.int32).reshape(-1, 3), n_cells=n_cells.astype(np.uint32), lo=lo.astype(np.int32), hi=hi.astype(np.int32),
                    hit=osum(h64), through=osum(t64), cell_sum=osum((mc + LIM).astype(np.uint64)))
        self.objects = {f: np.ascontiguousarray(full[f][listed]) for f in OBJECT_FIELDS}
        self.stats = dict(n_members=int(len(idx)), n_objects=int(listed.sum()), n_small=int((~listed).sum()),
                          n_small_cells=int(n_cells[~listed].sum()), max_cells=int(n_cells.max()) if k else 0)
        self.cell_map = np.full(len(cells), -1, np.int32)
        self.cell_map[idx] = rank[inv]

    def beams(self, cfg, cell, beams, T):
        """one int32 per beam: the object of its end cell (cell: the fine cell's edge in metres; beams float32 [n, 3]; T [4, 4])"""
        p = np.asarray(beams, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        out = np.full(len(p), -1, np.int32)
        L2, _, cast, _, _ = rays(cfg, beams, T)
        T = np.asarray(T, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            obs = cast & (L2 >= cfg.obs_min_range_m * cfg.obs_min_range_m) & (L2 <= cfg.obs_max_range_m * cfg.obs_max_range_m)
        o = np.flatnonzero(obs)
        q = np.stack([((T[r, 0] * p[o, 0] + T[r, 1] * p[o, 1]) + T[r, 2] * p[o, 2]) + T[r, 3] for r in range(3)], 1).reshape(-1, 3)
        v = q * (1.0 / cell) if math.frexp(cell)[0] == 0.5 else q / cell  # q / cell formed as the fine occupancy forms it
        e = np.floor(v)
        ok = (np.abs(e) < LIM).all(axis=1)  # (on the floats: a far end point does not fit an integer)
        o, e = o[ok], e[ok].astype(np.int64)
        if len(o) and self.code.size:
            k = codes(e)
            i = np.minimum(np.searchsorted(self.code, k), self.code.size - 1)
            found = self.code[i] == k
            out[o[found]] = self.cell_map[i[found]]
        return out


def find(growth, rule=None):
    """the objects of a growth mirror (growth_ref.Growth)"""
    cells, hit, through, _ = growth.cells()
    return Objects(cells, hit, through, rule if rule is not None else Rule())
