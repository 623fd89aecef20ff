"""A numpy mirror of the map-evidence contract (include/elimaloc_hip.h, "map evidence"), written from the header's text, float64, one
statement of the contract per line; shared by tests/test_evidence.py (GPU against it) and tests/test_evidence_abi.py (it against a map
worked out by hand).  Vectorised over the beams, one loop iteration per step of the walk."""
import numpy as np

from ray_ref import cell_of, codes, occupancy, rays

FIELDS = ("n_cast", "n_observing", "n_walked", "n_truncated", "n_through_beams", "n_end_hit", "n_end_free", "n_through_events", "n_steps")


class Cfg:
    """a plain object with elm_evidence_config's fields and defaults: the mirror needs no library"""

    def __init__(self, **kw):
        self.sub, self.max_steps = 4, 4096
        self.min_range_m, self.obs_min_range_m, self.obs_max_range_m = 1.0, 2.0, 50.0
        self.end_margin_m, self.end_margin_frac, self.origin = 1.0, 0.2, (0.0, 0.0, 0.0)
        self.__dict__.update(kw)


def _lookup(occ, c):
    """index into occ (sorted codes) of every code in c, -1 where absent"""
    if occ.size == 0:
        return np.full(c.shape, -1, np.int64)
    i = np.minimum(np.searchsorted(occ, c), occ.size - 1)
    return np.where(occ[i] == c, i, -1)


def observe(occ, cell, cfg, beams, T, through, hit, trace=False):
    """One observation added to through / hit (int64 [len(occ)], aligned with occ = the ascending codes of the occupied cells, which is
    elm_map_fine_cells' ascending (x, y, z) order).  -> (stats dict of FIELDS, events int64 [n] (not saturated), left: with trace the list
    of the cells every beam left by a step, in walk order, else None)."""
    p = np.asarray(beams, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    L2, L, cast, s, w = rays(cfg, beams, T)
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        obs = cast & (L2 >= cfg.obs_min_range_m * cfg.obs_min_range_m) & (L2 <= cfg.obs_max_range_m * cfg.obs_max_range_m)
    o = np.flatnonzero(obs)
    # end point
    q = np.stack([((T[r, 0] * p[o, 0] + T[r, 1] * p[o, 1]) + T[r, 2] * p[o, 2]) + T[r, 3] for r in range(3)], 1)
    e = _lookup(occ, codes(cell_of(q, cell)))
    np.add.at(hit, e[e >= 0], 1)
    n_end_hit = int((e >= 0).sum())
    # reach and walk
    with np.errstate(invalid="ignore"):
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
        # step: the axis with the smallest exit parameter, x before y before z on ties
        ax = np.argmin(tx[act], axis=1)
        t_next = np.fmax(t_in[act], tx[act, ax])
        by_reach = t_next > reach[act]
        by_steps = ~by_reach & (steps[act] >= max_steps)
        trunc[act[by_steps]] = True
        go = ~(by_reach | by_steps)
        g, a = act[go], ax[go]
        # the current cell is left by this step: seen through when occupied
        k = _lookup(occ, codes(c[g]))
        np.add.at(through, k[k >= 0], 1)
        events[g[k >= 0]] += 1
        if trace:
            for b in g:
                left[b].append(tuple(int(v) for v in c[b]))
        t_in[g] = t_next[go]
        c[g, a] += sg[g, a]
        tx[g, a] = ((c[g, a] + up[g, a]).astype(np.float64) * cell - s[a]) / w[g, a]
        steps[g] += 1
        act = g
    st = dict(n_cast=int(cast.sum()), n_observing=int(obs.sum()), n_walked=int(walks.sum()), n_truncated=int(trunc.sum()),
              n_through_beams=int((events > 0).sum()), n_end_hit=n_end_hit, n_end_free=int(obs.sum()) - n_end_hit,
              n_through_events=int(events.sum()), n_steps=int(steps.sum()))
    return st, events, left


def mirror(stored, voxel_size, cfg, scans, poses, trace=False):
    """Observations (scans[j] at poses[j]) accumulated from zero -> (cells int64 [m, 3] ascending (x, y, z), through uint32 [m], hit uint32
    [m], stats: one dict per observation, events: one uint16 [n_j] (saturated) per observation, left: per observation the traced walks)."""
    cell = voxel_size / cfg.sub
    occ = occupancy(stored, cell)
    through, hit = np.zeros(occ.size, np.int64), np.zeros(occ.size, np.int64)
    stats, events, lefts = [], [], []
    for beams, T in zip(scans, np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)):
        st, ev, left = observe(occ, cell, cfg, beams, T, through, hit, trace)
        stats.append(st)
        events.append(np.minimum(ev, 65535).astype(np.uint16))
        lefts.append(left)
    k = np.stack([(occ >> 42), (occ >> 21) & ((1 << 21) - 1), occ & ((1 << 21) - 1)], 1) - (1 << 20)
    return k, through.astype(np.uint32), hit.astype(np.uint32), stats, events, lefts


def stale_cells(through, hit, min_through=3, through_per_hit=4):
    """the rule of elm_evidence_rule on counters: through >= min_through and through >= through_per_hit * hit (64-bit product)"""
    t, h = through.astype(np.uint64), hit.astype(np.uint64)
    return (t >= np.uint64(min_through)) & (t >= np.uint64(through_per_hit) * h)
