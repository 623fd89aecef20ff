"""Relocalization in numpy float64, written from the contract (include/elimaloc_hip.h; DESIGN.md sections 11 and 12) and independent of
the library's scoring.  Plain numpy, no GPU, no library call.

* `voxel_keys` / `counted` / `scores`: the occupancy score.  The key is always trunc(q / vs) with q = ((R0 x + R1 y) + R2 z) + t.
* `lattice`: the global form's poses and their validity from the documented formulas (the ground field by brute force over the stored
  points), for the CPU checks of the cases; a GPU test takes them from GlobalHypotheses instead.
* `Mirror`: one global search problem.  `bounds` gives DESIGN.md section 12's three rules for the nodes of a level (`bound` for one node),
  with the rule each point took; the box and the level windows are derived from the key SET (a key k marks every window start in
  (k - w, k]), not from the kernel's word and mask loops.  `search` is the driver: the choice of the top level, the first threshold by
  greedy descents, the passes and the greedy non-maximum suppression.  Leaf scores are `scores()`, never ScorePoses.
"""
import math
from types import SimpleNamespace

import numpy as np

# the rule a (point, node) pair took in bounds(): exactly one of WIDE / ZCAP / W1 / W2 / W3 / OUT, and with a window lookup (W1..W3)
# CLAMP (the start lay below the box on x or y and was clamped) and / or PAST (the window runs past the box's high x or y edge)
WIDE, ZCAP, W1, W2, W3, CLAMP, PAST, OUT = 1, 2, 4, 8, 16, 32, 64, 128
TAGS = dict(wide=WIDE, zcap=ZCAP, w1=W1, w2=W2, w3=W3, clamp=CLAMP, past=PAST, out=OUT)


def _codes(k):
    k = np.asarray(k, dtype=np.int64) + (1 << 20)
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


def voxel_keys(map_xyz, vs):
    """the voxel set: the unique truncated keys of ALL map points, int64 [n, 3]"""
    c = np.unique(_codes(np.trunc(np.asarray(map_xyz).astype(np.float64) / vs)))
    return np.stack([c >> 42, (c >> 21) & ((1 << 21) - 1), c & ((1 << 21) - 1)], -1) - (1 << 20)


def in_range(scan, r_max):
    """the points with ((x*x + y*y) + z*z) <= r_max^2 in float64"""
    p = scan.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return scan[(x * x + y * y) + z * z <= r_max * r_max]


def counted(scan, cfg, T_tilt):
    """the global form's counted points: every stride-th point of the scan (stride = ceil(n / max_score_points)), within r_max, then
    (R0 p)_z + h >= score_min_height_m (float64, the contract's association)."""
    n = scan.shape[0]
    cap = int(getattr(cfg, "max_score_points", 0)) or n
    scan = scan[::max(1, -(-n // cap))] if n else scan
    scan = in_range(scan, cfg.score_max_range_m)
    p = scan.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    R = T_tilt[:3, :3]
    return scan[((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + T_tilt[2, 3] >= cfg.score_min_height_m]


def pose_keys(S, poses, vs):
    """the keys of the points S [n, 3] under the poses [m, 4, 4]: int64 [m, n, 3]"""
    p = np.asarray(S).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    T = np.asarray(poses, dtype=np.float64)
    q = [((T[:, r, 0, None] * x + T[:, r, 1, None] * y) + T[:, r, 2, None] * z) + T[:, r, 3, None] for r in range(3)]
    return np.trunc(np.stack(q, -1) / vs).astype(np.int64)


def scores(vox, vs, S, poses):
    """score(T) of every pose: the number of points of S (already the counted ones) whose key under T is in the key set vox"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    out = np.zeros(len(poses), np.uint32)
    if len(vox) == 0 or len(S) == 0:
        return out
    code = np.unique(_codes(vox))
    step = max(1, 2_000_000 // len(S))
    for o in range(0, len(poses), step):
        c = _codes(pose_keys(S, poses[o:o + step], vs))
        i = np.minimum(np.searchsorted(code, c), code.size - 1)
        out[o:o + step] = np.count_nonzero(code[i] == c, axis=1)
    return out


def mirror_scores(map_xyz, vs, scan, poses, r_max):
    """score(T) by the contract: the voxel set = unique truncated keys of ALL map points; counted points within r_max (float64); the
    transform in the contract's association; truncated keys by division."""
    return scores(voxel_keys(map_xyz, vs), vs, in_range(scan, r_max), poses)


def wrap_deg(d):
    d = math.fmod(d, 360.0)
    return d - 360.0 if d > 180.0 else (d + 360.0 if d < -180.0 else d)


def greedy_nms(order, pos, top_k, nms_xy, nms_yaw):
    """greedy non-maximum suppression over the hypotheses `order` (rank order); pos(h) -> (x, y, yaw_deg).  A hypothesis within nms_xy in xy
    AND nms_yaw in wrapped yaw of a kept one is suppressed; at most top_k are kept."""
    kept, at = [], []
    for h in order:
        if len(kept) >= top_k:
            break
        x, y, yaw = pos(int(h))
        if any(math.hypot(x - kx, y - ky) <= nms_xy and abs(wrap_deg(yaw - kyaw)) <= nms_yaw for (kx, ky, kyaw) in at):
            continue
        kept.append(int(h))
        at.append((x, y, yaw))
    return kept


def n_yaw(cfg):
    return max(1, int(math.ceil(360.0 / cfg.step_yaw_deg - 1e-9)))


def stored_points(map_xyz, vs, cap):
    """the points a map keeps of map_xyz (VoxelHashMap::AddPoints): the first point of a voxel (truncation key) always; a later one while the
    voxel holds fewer than cap and none of its points lies closer than sqrt(vs^2 / cap)"""
    p32 = np.asarray(map_xyz, dtype=np.float32)
    p = p32.astype(np.float64)
    res = math.sqrt(vs * vs / cap)
    buckets, keep = {}, []
    for i, k in enumerate(map(tuple, np.trunc(p / vs).astype(np.int64).tolist())):
        b = buckets.setdefault(k, [])
        if b and (len(b) >= cap or any(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < res for d in (p[j] - p[i] for j in b))):
            continue
        b.append(i)
        keep.append(i)
    return p32[keep]


def ground_heights(stored, xy):
    """elm_map_find_ground_height by brute force: the stored points with dx*dx + dy*dy <= 25 (float64), the (up to) 5 lowest z summed in
    ascending order from 0.0, divided by their number; found with more than 3 points"""
    p = np.asarray(stored, dtype=np.float32).astype(np.float64)
    found, z = np.zeros(len(xy), bool), np.zeros(len(xy))
    for q, (x, y) in enumerate(np.asarray(xy, dtype=np.float64)):
        dx, dy = p[:, 0] - x, p[:, 1] - y
        zs = np.sort(p[dx * dx + dy * dy <= 25.0, 2])
        if zs.size > 3:
            s = 0.0
            for v in zs[:5]:
                s += float(v)
            found[q], z[q] = True, s / min(5, zs.size)
    return found, z


def lattice(stored, T_tilt, cfg):
    """the lattice of DESIGN.md section 12 from its formulas -> (H [K NX NY, 4, 4], valid): x_i = x_min + i step, y_j likewise,
    R_k = Rz(k step_yaw) R0 with the host's cos / sin, z = fl(g + h) on ground and h off it; hyp = (k NX + i) NY + j."""
    NX = int(math.floor((cfg.x_max - cfg.x_min) / cfg.step_xy_m + 1e-9)) + 1
    NY = int(math.floor((cfg.y_max - cfg.y_min) / cfg.step_xy_m + 1e-9)) + 1
    K = n_yaw(cfg)
    xs = cfg.x_min + np.arange(NX, dtype=np.float64) * cfg.step_xy_m
    ys = cfg.y_min + np.arange(NY, dtype=np.float64) * cfg.step_xy_m
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    found, g = ground_heights(stored, np.column_stack([gx.ravel(), gy.ravel()]))
    h = float(T_tilt[2, 3])
    R0 = np.asarray(T_tilt, dtype=np.float64)[:3, :3]
    H = np.zeros((K, NX * NY, 4, 4))
    for k in range(K):
        a = (k * cfg.step_yaw_deg) * (math.pi / 180.0)
        ca, sa = math.cos(a), math.sin(a)
        H[k, :, 0, :3] = ca * R0[0] - sa * R0[1]
        H[k, :, 1, :3] = sa * R0[0] + ca * R0[1]
        H[k, :, 2, :3] = R0[2]
        H[k, :, 0, 3], H[k, :, 1, 3] = gx.ravel(), gy.ravel()
        H[k, :, 2, 3] = np.where(found, g + h, h)
        H[k, :, 3, 3] = 1.0
    return H.reshape(-1, 4, 4), np.tile(found, K)


class Mirror:
    """One global search: the voxel keys `vox` of the map, the counted points S, the lattice (H, valid) and the config.  Everything else
    (node ranges, the key box, the level windows) is derived here."""

    def __init__(self, vox, vs, S, H, valid, cfg):
        self.vox, self.vs, self.S, self.H, self.valid_flat, self.cfg = np.asarray(vox, np.int64), float(vs), S, H, np.asarray(valid, bool), cfg
        self.K = n_yaw(cfg)
        nxy = H.shape[0] // self.K
        ys = H[:nxy, 1, 3]
        self.NY = int(np.argmax(H[:nxy, 0, 3] != H[0, 0, 3])) if np.any(H[:nxy, 0, 3] != H[0, 0, 3]) else nxy
        self.NX = nxy // self.NY
        self.xs, self.ys = H[:nxy:self.NY, 0, 3].copy(), ys[:self.NY].copy()
        self.rot = H[::nxy, :3, :3].copy()  # [K, 3, 3]
        self.gz = H[:nxy, 2, 3].reshape(self.NX, self.NY)
        self.valid = self.valid_flat[:nxy].reshape(self.NX, self.NY)
        self.step = float(cfg.step_xy_m)
        self.nS = len(S)
        top = 0
        while (1 << top) < max(self.NX, self.NY):
            top += 1
        while top > 1 and self.K * self.nI(top - 1) * self.nJ(top - 1) <= 4096:
            top -= 1
        self.top = top
        self.w = [1] + [int(math.floor(((1 << l) - 1) * self.step / self.vs)) + 2 for l in range(1, top + 1)]
        # z range of fl(g + h) over the valid leaves of every node, per level
        zmin, zmax = np.where(self.valid, self.gz, np.inf), np.where(self.valid, self.gz, -np.inf)
        self.zmin, self.zmax = [zmin], [zmax]
        for l in range(1, top + 1):
            self.zmin.append(self._pool(self.zmin[0], l, np.minimum, np.inf))
            self.zmax.append(self._pool(self.zmax[0], l, np.maximum, -np.inf))
        # the map's key box, z padded up to a multiple of 64 keys from z0
        if len(self.vox):
            self.k0 = self.vox.min(axis=0)
            self.dims = self.vox.max(axis=0) - self.k0 + 1
            self.dims[2] = (self.dims[2] + 63) // 64 * 64
        self._win, self._rp, self._leaf = {}, None, None

    def nI(self, l):
        return (self.NX + (1 << l) - 1) >> l

    def nJ(self, l):
        return (self.NY + (1 << l) - 1) >> l

    def _pool(self, a, l, op, fill):
        s = 1 << l
        p = np.full((self.nI(l) * s, self.nJ(l) * s), fill)
        p[:a.shape[0], :a.shape[1]] = a
        return op.reduce(op.reduce(p.reshape(self.nI(l), s, self.nJ(l), s), axis=3), axis=1)

    # ------------------------------------------------------------------ leaves
    def leaf_scores(self):
        """the exact score of every lattice pose (valid or not), by scores()"""
        if self._leaf is None:
            self._leaf = scores(self.vox, self.vs, self.S, self.H).astype(np.int64)
        return self._leaf

    def leaf_max(self, l):
        """the greatest leaf score under every level-l node, [K, nI, nJ]; -1 for a node without a valid leaf"""
        s = np.where(self.valid_flat, self.leaf_scores(), -1).reshape(self.K, self.NX, self.NY)
        return np.stack([self._pool(s[k], l, np.maximum, -1) for k in range(self.K)])

    def pos(self, h):
        return float(self.H[h, 0, 3]), float(self.H[h, 1, 3]), float(h // (self.NX * self.NY)) * self.cfg.step_yaw_deg

    # ------------------------------------------------------------------ bounds
    def window(self, l):
        """W[cx, cy, cz] = some key of the map in [x0 + cx, x0 + cx + w_l) x [y0 + cy, y0 + cy + w_l) at z0 + cz, as running counts along
        z: the entry [cx, cy, c] counts the occupied cells below c.  From the key set: key k marks the starts k - w + 1 .. k."""
        if l not in self._win:
            w, d = self.w[l], self.dims
            W = np.zeros((d[0], d[1], d[2]), bool)
            r = self.vox - self.k0
            for dx in range(w):
                for dy in range(w):
                    ok = (r[:, 0] >= dx) & (r[:, 1] >= dy)
                    W[r[ok, 0] - dx, r[ok, 1] - dy, r[ok, 2]] = True
            cs = np.zeros((d[0], d[1], d[2] + 1), np.int32)
            np.cumsum(W, axis=2, out=cs[:, :, 1:])
            self._win[l] = cs
        return self._win[l]

    def node_ranges(self, l, nodes):
        """xlo, xhi, ylo, yhi, zlo, zhi of the nodes [n, 3] = (k, I, J) of level l: the translations of the first and last leaves"""
        I, J = nodes[:, 1], nodes[:, 2]
        i1 = np.minimum((I + 1) << l, self.NX) - 1
        j1 = np.minimum((J + 1) << l, self.NY) - 1
        return self.xs[I << l], self.xs[i1], self.ys[J << l], self.ys[j1], self.zmin[l][I, J], self.zmax[l][I, J]

    def _key(self, q):
        return np.trunc(q / self.vs).astype(np.int64)

    def key_ranges(self, l, nodes):
        """kx0, kx1, ky0, ky1, kz0, kz1 [n, nS] of every counted point over the level-l nodes [n, 3] = (k, I, J): the keys of a + t at the
        two ends of the node's t range, a = R_k p in the score's association"""
        nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 3)
        if self._rp is None:
            p = np.asarray(self.S).astype(np.float64)
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            R = self.rot
            self._rp = np.stack([(R[:, r, 0, None] * x + R[:, r, 1, None] * y) + R[:, r, 2, None] * z for r in range(3)], -1)  # [K, nS, 3]
        xlo, xhi, ylo, yhi, zlo, zhi = (v[:, None] for v in self.node_ranges(l, nodes))
        a = self._rp[nodes[:, 0]]
        return (self._key(a[:, :, 0] + xlo), self._key(a[:, :, 0] + xhi), self._key(a[:, :, 1] + ylo), self._key(a[:, :, 1] + yhi),
                self._key(a[:, :, 2] + zlo), self._key(a[:, :, 2] + zhi))

    def bounds(self, l, nodes):
        """the bound of every node [n, 3] = (k, I, J) of level l and the rule every (node, point) pair took: (counts [n], tags [n, nS])"""
        nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 3)
        cnt, tags = np.zeros(len(nodes), np.int64), np.zeros((len(nodes), self.nS), np.uint8)
        if self.nS == 0 or len(nodes) == 0:
            return cnt, tags
        cap, w, k0, d = int(self.cfg.max_kz_span), self.w[l], self.k0, self.dims
        cs = self.window(l)
        for o in range(0, len(nodes), 4096):
            kx0, kx1, ky0, ky1, kz0, kz1 = self.key_ranges(l, nodes[o:o + 4096])
            # 1. the x or y key range does not fit the window's w keys
            wide = (kx1 - kx0 >= w) | (ky1 - ky0 >= w)
            # entirely outside the box: nothing to read
            out = ~wide & ((kx1 < k0[0]) | (ky1 < k0[1]) | (kz1 < k0[2]) | (kx0 >= k0[0] + d[0]) | (ky0 >= k0[1] + d[1]) | (kz0 >= k0[2] + d[2]))
            # 2. the z range, cut to the box, spans more than max_kz_span keys
            cz0, cz1 = np.clip(kz0 - k0[2], 0, None), np.clip(kz1 - k0[2], None, d[2] - 1)
            zcap = ~wide & ~out & (cz1 - cz0 >= cap)
            # 3. the window at the start keys, the start clamped into the box, occupied at a kz of the range
            look = ~wide & ~out & ~zcap
            cx, cy = np.clip(kx0 - k0[0], 0, d[0] - 1), np.clip(ky0 - k0[1], 0, d[1] - 1)
            a0, a1 = np.where(look, cz0, 0), np.where(look, cz1, 0)
            occ = look & (cs[cx, cy, a1 + 1] - cs[cx, cy, a0] > 0)
            nw = (cz1 >> 5) - (cz0 >> 5) + 1
            t = np.where(wide, WIDE, 0) | np.where(out, OUT, 0) | np.where(zcap, ZCAP, 0)
            t |= np.where(look & (nw == 1), W1, 0) | np.where(look & (nw == 2), W2, 0) | np.where(look & (nw >= 3), W3, 0)
            t |= np.where(look & ((kx0 < k0[0]) | (ky0 < k0[1])), CLAMP, 0)
            t |= np.where(look & ((cx + w > d[0]) | (cy + w > d[1])), PAST, 0)
            tags[o:o + 4096] = t
            cnt[o:o + 4096] = np.count_nonzero(wide | zcap | occ, axis=1)
        return cnt, tags

    def bound(self, node):
        """one node (k, l, I, J) -> (count, tags [nS])"""
        k, l, I, J = node
        c, t = self.bounds(l, [[k, I, J]])
        return int(c[0]), t[0]

    def all_nodes(self, l):
        """every level-l node with a valid leaf, in the driver's order (k, I, J)"""
        if l == 0:
            raise ValueError("level 0 holds leaves")
        ok = self.zmin[l] <= self.zmax[l]
        I, J = np.nonzero(ok)
        n = len(I)
        return np.column_stack([np.repeat(np.arange(self.K), n), np.tile(I, self.K), np.tile(J, self.K)]).astype(np.int64)

    # ------------------------------------------------------------------ driver
    def _children(self, l, nodes):
        """the valid children at level l - 1 of the level-l nodes: (children, owner index); leaves come as hypothesis indices"""
        ch, owner = [], []
        for p, (k, I, J) in enumerate(np.asarray(nodes, dtype=np.int64).reshape(-1, 3).tolist()):
            for a in (0, 1):
                for c in (0, 1):
                    ci, cj = 2 * I + a, 2 * J + c
                    if ci >= self.nI(l - 1) or cj >= self.nJ(l - 1):
                        continue
                    if l == 1:
                        if self.valid[ci, cj]:
                            ch.append((k * self.NX + ci) * self.NY + cj)
                            owner.append(p)
                    elif self.zmin[l - 1][ci, cj] <= self.zmax[l - 1][ci, cj]:
                        ch.append((k, ci, cj))
                        owner.append(p)
        return np.array(ch, dtype=np.int64).reshape((-1,) if l == 1 else (-1, 3)), np.array(owner, dtype=np.int64)

    def search(self):
        """DESIGN.md section 12 "Driver" -> a namespace of tau, passes, levels, nodes_bounded[l], nodes_kept[l], leaves_scored, point_evals,
        leaves (the (hyp, score) with score >= tau in (score desc, hyp asc) order) and kept (after the greedy NMS, at most top_k)."""
        cfg, top, nS = self.cfg, self.top, self.nS
        st = SimpleNamespace(levels=top, passes=0, tau=0, nodes_bounded=[0] * (top + 1), nodes_kept=[0] * (top + 1), leaves_scored=0,
                             point_evals=0, n_counted=nS, valid_leaves=int(self.valid_flat.sum()), tau_bound_leaf=False)
        leaf = self.leaf_scores()

        def bound(l, nodes):
            st.nodes_bounded[l] += len(nodes)
            st.point_evals += len(nodes) * nS
            return self.bounds(l, nodes)[0]

        def score(hyps):
            st.leaves_scored += len(hyps)
            st.point_evals += len(hyps) * nS
            return leaf[hyps]

        if top == 0:
            front0 = np.flatnonzero(self.valid_flat)
        else:
            front0 = self.all_nodes(top)
        # the first threshold
        tau = 0
        if top >= 1 and len(front0):
            b = bound(top, front0)
            D = min(int(cfg.pool_min), len(front0))
            idx = np.lexsort((np.arange(len(b)), -b))[:D]
            path = front0[idx]
            for l in range(top, 0, -1):
                ch, owner = self._children(l, path)
                if l == 1:
                    path = ch
                    break
                nb = bound(l - 1, ch)
                nxt = []
                for p in range(len(path)):
                    q = np.flatnonzero(owner == p)
                    nxt.append(ch[q[int(np.argmax(nb[q]))]])  # the first greatest
                path = np.array(nxt, dtype=np.int64).reshape(-1, 3)
            s = np.sort(score(path))[::-1]
            if len(s):
                tau = int(s[min(int(cfg.pool_min), len(s)) - 1])
        while True:
            st.passes += 1
            st.tau = tau
            front = front0
            for l in range(top, 0, -1):
                b = bound(l, front)
                keep = b >= tau
                st.nodes_kept[l] += int(keep.sum())
                kept_nodes = front[keep]
                front = self._children(l, kept_nodes)[0]
                # a node whose bound equals tau exactly with a leaf that reaches tau under it: the `>=` of the pruning test decides it
                if not st.tau_bound_leaf and tau > 0 and np.any(b == tau):
                    lm = self.leaf_max(l)
                    eq = kept_nodes[b[keep] == tau]
                    st.tau_bound_leaf = bool(np.any(lm[eq[:, 0], eq[:, 1], eq[:, 2]] >= tau))
            s = score(front)
            ok = s >= tau
            hyps, sc = front[ok], s[ok]
            order = np.lexsort((hyps, -sc))
            st.leaves = [(int(hyps[q]), int(sc[q])) for q in order]
            kept = greedy_nms([h for h, _ in st.leaves], self.pos, int(cfg.top_k), cfg.nms_xy_m, cfg.nms_yaw_deg)
            if len(kept) >= cfg.top_k or tau == 0:
                break
            tau = tau * 3 // 4
        by = dict(st.leaves)
        st.kept = [(h, by[h]) for h in kept]
        return st

    def exhaustive(self):
        """every valid lattice pose scored, (score desc, hyp asc), greedy NMS -> the kept (hyp, score) list"""
        hyp = np.flatnonzero(self.valid_flat)
        s = self.leaf_scores()[hyp]
        order = hyp[np.lexsort((hyp, -s))]
        kept = greedy_nms(order, self.pos, int(self.cfg.top_k), self.cfg.nms_xy_m, self.cfg.nms_yaw_deg)
        return [(h, int(self.leaf_scores()[h])) for h in kept]


def score_box(S, poses, vs):
    """the key box elm_map_score_poses builds its bitmap over: per pose and row the keys of the two corners of S's bounding box that
    minimise / maximise every product (the contract's association), their union over the poses, one key of margin per side
    -> (k0 [3], dims [3])"""
    p = np.asarray(S).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    kmin, kmax = np.full(3, np.inf), np.full(3, -np.inf)
    for T in np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4):
        for r in range(3):
            a = T[r, :3]
            qlo = ((a[0] * (lo[0] if a[0] >= 0 else hi[0]) + a[1] * (lo[1] if a[1] >= 0 else hi[1])) + a[2] * (lo[2] if a[2] >= 0 else hi[2])) + T[r, 3]
            qhi = ((a[0] * (hi[0] if a[0] >= 0 else lo[0]) + a[1] * (hi[1] if a[1] >= 0 else lo[1])) + a[2] * (hi[2] if a[2] >= 0 else lo[2])) + T[r, 3]
            kmin[r], kmax[r] = min(kmin[r], np.trunc(qlo / vs)), max(kmax[r], np.trunc(qhi / vs))
    return (kmin - 1).astype(np.int64), (kmax - kmin + 3).astype(np.int64)
