"""A numpy mirror of the map-growth contract (include/elimaloc_hip.h, "map growth"), written from the header's text, float64, one statement
of the contract per line; shared by tests/test_growth.py (GPU against it) and tests/test_growth_abi.py (it against a map worked out by
hand).  A Growth object is fed call by call; every call runs the two phases of the contract: the end points of ALL its jobs are recorded
first, then every job walks against the candidates that exist by then.  Vectorised over the beams, one loop iteration per step of the
walk."""
import math

import numpy as np

from ray_ref import cell_of, codes, is_in, occupancy, rays

FIELDS = ("n_cast", "n_observing", "n_walked", "n_truncated", "n_end_hit", "n_end_near", "n_end_new", "n_end_out", "n_through_beams",
          "n_dropped", "n_through_events", "n_steps")
LIM = 1 << 20  # a cell packs into one key when every |e_r| < 2^20


class Cfg:
    """a plain object with elm_growth_config's fields and defaults: the mirror needs no library"""

    def __init__(self, **kw):
        self.sub, self.max_steps, self.clearance_cells = 4, 4096, 1
        self.min_range_m, self.obs_min_range_m, self.obs_max_range_m = 1.0, 2.0, 50.0
        self.end_margin_m, self.end_margin_frac, self.origin = 1.0, 0.2, (0.0, 0.0, 0.0)
        self.__dict__.update(kw)


def _in_range(c):
    return (np.abs(c) < LIM).all(axis=1)


def _occupied(occ, c):
    """is the integer cell c [n, 3] one of the sorted codes occ?  (a cell beyond the key range is in no table)"""
    ok = _in_range(c)
    out = np.zeros(len(c), bool)
    out[ok] = is_in(occ, codes(c[ok]))
    return out


def _lookup(tab, c):
    """index into tab (sorted codes) of every cell of c [n, 3], -1 where absent"""
    out = np.full(len(c), -1, np.int64)
    ok = np.flatnonzero(_in_range(c))
    if tab.size and ok.size:
        k = codes(c[ok])
        i = np.minimum(np.searchsorted(tab, k), tab.size - 1)
        out[ok] = np.where(tab[i] == k, i, -1)
    return out


class Growth:
    """The growth object of one (map, sub): the candidate cells (ascending codes = ascending (x, y, z)) with hit, through and the three
    fixed-point sums."""

    def __init__(self, stored, voxel_size, sub=4):
        self.sub, self.cell = sub, voxel_size / sub
        self.occ = occupancy(stored, self.cell)
        self.reset()

    def reset(self):
        self.code = np.zeros(0, np.int64)
        self.hit, self.through, self.sums = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64)

    # ---- phase 1
    def _ends(self, cfg, beams, T):
        """the end class of every beam of one job -> (stats part, cells [m, 3] and k [m, 3] of its END-NEW beams)"""
        p = np.asarray(beams, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        L2, L, cast, s, w = rays(cfg, beams, T)
        T = np.asarray(T, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            obs = cast & (L2 >= cfg.obs_min_range_m * cfg.obs_min_range_m) & (L2 <= cfg.obs_max_range_m * cfg.obs_max_range_m)
        o = np.flatnonzero(obs)
        q = np.stack([((T[r, 0] * p[o, 0] + T[r, 1] * p[o, 1]) + T[r, 2] * p[o, 2]) + T[r, 3] for r in range(3)], 1).reshape(-1, 3)
        v = q * (1.0 / self.cell) if _pow2(self.cell) else q / self.cell  # q / cell formed as fine_of forms it
        fl = np.floor(v)
        e = fl.astype(np.int64)
        end_hit = _occupied(self.occ, e)
        end_out = ~end_hit & ~_in_range(e)
        near = np.zeros(len(e), bool)
        C = int(cfg.clearance_cells)
        rest = ~end_hit & ~end_out
        if C > 0:
            r = np.arange(-C, C + 1)
            for off in np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3):
                near |= rest & _occupied(self.occ, e + off)
        new = rest & ~near
        k = np.minimum(65535, np.floor((v - fl) * 65536.0)).astype(np.int64)
        st = dict(n_cast=int(cast.sum()), n_observing=int(obs.sum()), n_end_hit=int(end_hit.sum()), n_end_near=int(near.sum()),
                  n_end_new=int(new.sum()), n_end_out=int(end_out.sum()), n_dropped=0)
        return st, e[new], k[new]

    def _record(self, e, k):
        """END-NEW beams: e becomes a candidate if it is not one yet, hit[e] += 1, sum_r[e] += k_r"""
        if not len(e):
            return
        c = codes(e)
        allc = np.union1d(self.code, c)
        hit, through, sums = np.zeros(allc.size, np.int64), np.zeros(allc.size, np.int64), np.zeros((allc.size, 3), np.int64)
        old = np.searchsorted(allc, self.code)
        hit[old], through[old], sums[old] = self.hit, self.through, self.sums
        i = np.searchsorted(allc, c)
        np.add.at(hit, i, 1)
        np.add.at(sums, i, k)
        self.code, self.hit, self.through, self.sums = allc, hit, through, sums

    # ---- phase 2
    def _walk(self, cfg, beams, T, trace):
        """the evidence walk of one job against the candidates -> (stats part, events int64 [n], left)"""
        n = np.asarray(beams).reshape(-1, 3).shape[0]
        cell = self.cell
        L2, L, cast, s, w = rays(cfg, beams, T)
        with np.errstate(invalid="ignore"):
            obs = cast & (L2 >= cfg.obs_min_range_m * cfg.obs_min_range_m) & (L2 <= cfg.obs_max_range_m * cfg.obs_max_range_m)
            reach = L - np.fmax(cfg.end_margin_m, cfg.end_margin_frac * L)
            walks = obs & (reach > cfg.min_range_m)
        t_min, max_steps = float(cfg.min_range_m), int(cfg.max_steps)
        t_in = np.full(n, t_min)
        with np.errstate(invalid="ignore"):
            c = np.nan_to_num(cell_of(s + w * t_min, cell)).astype(np.int64)
            sg = np.where(w > 0.0, 1, np.where(w < 0.0, -1, 0)).astype(np.int64)
        up = (sg > 0).astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tx = np.where(sg != 0, ((c + up).astype(np.float64) * cell - s) / w, np.inf)
        steps, events = np.zeros(n, np.int64), np.zeros(n, np.int64)
        trunc = np.zeros(n, bool)
        left = [[] for _ in range(n)] if trace else None
        act = np.flatnonzero(walks)
        while act.size:
            ax = np.argmin(tx[act], axis=1)  # the axis with the smallest exit parameter, x before y before z on ties
            t_next = np.fmax(t_in[act], tx[act, ax])
            by_reach = t_next > reach[act]
            by_steps = ~by_reach & (steps[act] >= max_steps)
            trunc[act[by_steps]] = True
            go = ~(by_reach | by_steps)
            g, a = act[go], ax[go]
            # the current cell is left by this step: a through event when it is a candidate
            k = _lookup(self.code, c[g])
            np.add.at(self.through, k[k >= 0], 1)
            events[g[k >= 0]] += 1
            if trace:
                for b in g:
                    left[b].append(tuple(int(x) for x in c[b]))
            t_in[g] = t_next[go]
            c[g, a] += sg[g, a]
            tx[g, a] = ((c[g, a] + up[g, a]).astype(np.float64) * cell - s[a]) / w[g, a]
            steps[g] += 1
            act = g
        st = dict(n_walked=int(walks.sum()), n_truncated=int(trunc.sum()), n_through_beams=int((events > 0).sum()),
                  n_through_events=int(events.sum()), n_steps=int(steps.sum()))
        return st, events, left

    def call(self, cfg, scans, poses, trace=False):
        """One accumulate call (a batch of len(scans) jobs; accumulate is a batch of one) -> (stats: one dict of FIELDS per job, events:
        one uint16 [n_j] (saturated) per job, left: per job the traced walks or None)."""
        assert cfg.sub == self.sub
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        assert len(poses) == len(scans)
        ends = [self._ends(cfg, b, T) for b, T in zip(scans, poses)]
        for _, e, k in ends:  # phase 1 of every job before phase 2 of any
            self._record(e, k)
        stats, events, lefts = [], [], []
        for (st, _, _), b, T in zip(ends, scans, poses):
            w, ev, left = self._walk(cfg, b, T, trace)
            st = dict(st, **w)
            stats.append({f: st[f] for f in FIELDS})
            events.append(np.minimum(ev, 65535).astype(np.uint16))
            lefts.append(left)
        return stats, events, lefts

    def cells(self):
        """-> (cells int32 [m, 3] ascending (x, y, z), hit uint32 [m], through uint32 [m], sums uint64 [m, 3])"""
        c = self.code
        k = np.stack([(c >> 42), (c >> 21) & ((1 << 21) - 1), c & ((1 << 21) - 1)], 1) - LIM
        return k.astype(np.int32).reshape(-1, 3), self.hit.astype(np.uint32), self.through.astype(np.uint32), self.sums.astype(np.uint64).reshape(-1, 3)

    def appeared(self, min_hit=3, hit_per_through=4):
        """the cells that the rule calls appeared, as a mask over cells()"""
        return appeared_cells(self.hit, self.through, min_hit, hit_per_through)

    def appeared_points(self, min_hit=3, hit_per_through=4):
        """one float64 point per appeared cell, in cell order: m_r = ((double)e_r + ((double)sum_r / (double)hit + 0.5) / 65536.0) cell"""
        cells, hit, _, sums = self.cells()
        a = self.appeared(min_hit, hit_per_through)
        return (cells[a].astype(np.float64) + (sums[a].astype(np.float64) / hit[a].astype(np.float64)[:, None] + 0.5) / 65536.0) * self.cell


def _pow2(x):
    return math.frexp(x)[0] == 0.5


def appeared_cells(hit, through, min_hit=3, hit_per_through=4):
    """the rule of elm_growth_rule on counters: hit >= min_hit and hit >= hit_per_through * through (64-bit product)"""
    h, t = np.asarray(hit).astype(np.uint64), np.asarray(through).astype(np.uint64)
    return (h >= np.uint64(min_hit)) & (h >= np.uint64(hit_per_through) * t)
