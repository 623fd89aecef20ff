"""A numpy mirror of the ray-casting contract (include/elimaloc_hip.h, "ray casting"), written from the header's text, float64, one
statement of the contract per line; shared by tests/test_raycast.py (GPU against it) and tests/test_raycast_abi.py (it against a map
worked out by hand).  Vectorised over the beams, one loop iteration per cell test."""
import math

import numpy as np

FIELDS = ("n_cast", "n_hit", "n_miss", "n_truncated", "n_compared", "n_match", "n_through", "n_front", "n_steps")


def codes(k):
    """One int64 per integer cell triple (|k| < 2^20 per axis)."""
    k = np.asarray(k, dtype=np.int64).reshape(-1, 3) + (1 << 20)
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def is_in(occ, c):
    if occ.size == 0:
        return np.zeros(c.shape, bool)
    i = np.searchsorted(occ, c)
    return occ[np.minimum(i, occ.size - 1)] == c


def occupancy(stored, cell):
    """The sorted codes of the fine cells of the stored points: floor(q / cell)."""
    stored = np.asarray(stored, dtype=np.float64).reshape(-1, 3)
    return np.unique(codes(np.floor(stored / cell)))


def cell_of(q, cell):
    """floor(q / cell) of world coordinates, q / cell formed as q * (1 / cell) where cell is a power of two (the same bits)."""
    return np.floor(q * (1.0 / cell) if math.frexp(cell)[0] == 0.5 else q / cell)


def rays(cfg, beams, T):
    """d, L2, L, u, cast of the beams and the world origin s [3] / directions w [n, 3] at pose T."""
    p = np.asarray(beams, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    o = np.array(list(cfg.origin), dtype=np.float64)
    d = p - o
    L2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.sqrt(L2)
        u = d / L[:, None]
    cast = (L2 > 0.0) & np.isfinite(L2)
    T = np.asarray(T, dtype=np.float64)
    s = np.array([((T[r, 0] * o[0] + T[r, 1] * o[1]) + T[r, 2] * o[2]) + T[r, 3] for r in range(3)])
    with np.errstate(invalid="ignore"):
        w = np.stack([(T[r, 0] * u[:, 0] + T[r, 1] * u[:, 1]) + T[r, 2] * u[:, 2] for r in range(3)], 1)
    return L2, L, cast, s, w


def mirror(stored, voxel_size, cfg, beams, poses, trace=False):
    """-> (stats: one dict of FIELDS per pose, arrays: range_in / range_out float64 [n_poses, n], cell int32 [n_poses, n, 3], flag uint8
    [n_poses, n], visited).  visited (trace=True): per pose a list with one (beam indices, cells [k, 3]) entry per test of the walk's
    search phase -- every cell tested up to and including the hit cell, in walk order; else None."""
    cell = voxel_size / cfg.sub
    occ = occupancy(stored, cell)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    n = np.asarray(beams).reshape(-1, 3).shape[0]
    t_min, t_max, max_steps = float(cfg.min_range_m), float(cfg.max_range_m), int(cfg.max_steps)
    stats = []
    RIN, ROUT = np.full((len(poses), n), -1.0), np.full((len(poses), n), -1.0)
    CELL, FLAG = np.zeros((len(poses), n, 3), np.int32), np.zeros((len(poses), n), np.uint8)
    visited = [] if trace else None
    for h, T in enumerate(poses):
        L2, L, cast, s, w = rays(cfg, beams, T)
        t_in = np.full(n, t_min)
        with np.errstate(invalid="ignore"):
            c = np.nan_to_num(cell_of(s + w * t_min, cell)).astype(np.int64)
            sg = np.where(w > 0.0, 1, np.where(w < 0.0, -1, 0)).astype(np.int64)
        up = (sg > 0).astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tx = np.where(sg != 0, ((c + up).astype(np.float64) * cell - s) / w, np.inf)
        in_run = np.zeros(n, bool)
        flag = np.zeros(n, np.uint8)
        rin, rout = np.full(n, -1.0), np.full(n, -1.0)
        hc = np.zeros((n, 3), np.int64)
        steps, steps_hit = np.zeros(n, np.int64), np.zeros(n, np.int64)
        act = np.flatnonzero(cast)
        seen = []
        while act.size:
            # test the current cell
            occ_here = is_in(occ, codes(c[act]))
            if trace:
                srch = ~in_run[act]
                seen.append((act[srch].copy(), c[act[srch]].copy()))
            new_hit = act[~in_run[act] & occ_here]
            run_end = in_run[act] & ~occ_here  # (a beam that has just hit is not in the run yet: evaluated before the update)
            flag[new_hit] = 1
            rin[new_hit] = t_in[new_hit]
            hc[new_hit] = c[new_hit]
            steps_hit[new_hit] = steps[new_hit]
            rout[act[run_end]] = t_in[act[run_end]]
            in_run[new_hit] = True
            act = act[~run_end]
            if not act.size:
                break
            # step: the axis with the smallest exit parameter, x before y before z on ties
            ax = np.argmin(tx[act], axis=1)
            t_next = np.fmax(t_in[act], tx[act, ax])
            by_range = t_next > t_max
            by_steps = ~by_range & (steps[act] >= max_steps)
            for ended, fl, out in ((act[by_range], 2, None), (act[by_steps], 3, t_in)):
                r, m = ended[in_run[ended]], ended[~in_run[ended]]
                rout[r] = t_max if out is None else out[r]
                flag[m] = fl
                steps_hit[m] = steps[m]
            go = ~(by_range | by_steps)
            g, a = act[go], ax[go]
            t_in[g] = t_next[go]
            c[g, a] += sg[g, a]
            tx[g, a] = ((c[g, a] + up[g, a]).astype(np.float64) * cell - s[a]) / w[g, a]
            steps[g] += 1
            act = g
        hit = flag == 1
        compared = cast & (L2 >= cfg.cmp_min_range_m * cfg.cmp_min_range_m) & (L2 <= cfg.cmp_max_range_m * cfg.cmp_max_range_m)
        with np.errstate(invalid="ignore"):
            tol = np.fmax(cfg.tol_m, cfg.tol_frac * L)
            match = compared & hit & (rin - tol <= L) & (L <= rout + tol)
            through = compared & hit & (L > rout + tol)
        front = compared & ~match & ~through
        stats.append(dict(n_cast=int(cast.sum()), n_hit=int(hit.sum()), n_miss=int((flag == 2).sum()), n_truncated=int((flag == 3).sum()),
                          n_compared=int(compared.sum()), n_match=int(match.sum()), n_through=int(through.sum()), n_front=int(front.sum()),
                          n_steps=int(steps_hit.sum())))
        RIN[h], ROUT[h], CELL[h], FLAG[h] = rin, rout, hc.astype(np.int32), flag
        if trace:
            visited.append(seen)
    return stats, dict(range_in=RIN, range_out=ROUT, cell=CELL, flag=FLAG), visited


def render_pick(stored, voxel_size, cfg, beams, T, cells, flags):
    """RenderScan's pick, beam by beam in plain loops: for every beam with flag 1 the stored point of its hit cell nearest to the beam
    (e = q - s, a = (e_x w_x + e_y w_y) + e_z w_z, r = e - w a, smallest (r_x r_x + r_y r_y) + r_z r_z, lowest index on a tie).
    -> (beam indices, stored indices)."""
    cell = voxel_size / cfg.sub
    stored = np.asarray(stored, dtype=np.float64)
    pc = codes(np.floor(stored / cell))
    order = np.argsort(pc, kind="stable")
    spc = pc[order]
    _, _, _, s, w = rays(cfg, beams, T)
    bi, si = [], []
    for i in np.flatnonzero(flags == 1):
        code = codes(cells[i][None])[0]
        cand = np.sort(order[np.searchsorted(spc, code, "left"):np.searchsorted(spc, code, "right")])
        best, best_d = -1, math.inf
        for k in cand:
            e = stored[k] - s
            a = (e[0] * w[i, 0] + e[1] * w[i, 1]) + e[2] * w[i, 2]
            r = e - w[i] * a
            d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
            if d2 < best_d:
                best, best_d = int(k), d2
        bi.append(int(i))
        si.append(best)
    return np.array(bi, dtype=np.int64), np.array(si, dtype=np.int64)
