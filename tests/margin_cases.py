"""Constructed inputs for the neighbour search's decision margins (tests/test_search_margins.py).  Plain numpy, no GPU.

Two things live here:

* `NpMap`: the reference's map and its three correspondence walks written once more from the rule (truncation-keyed buckets with the
  spacing rule and the cap; 27 floor-keyed neighbours x-major, insertion order inside a bucket, strict `<`; float64
  `(ex^2 + ey^2) + ez^2`; the origin as the default target), vectorised -- the independent brute force the oracle is checked against,
  and the bookkeeper that says how far from a decision boundary a query REALLY lies.
* `generate(case)`: float64 map-frame queries placed at prescribed distances from each boundary the search decides on -- winner vs
  runner-up (stored points and voxel means), the search radius, the faces of the 2 x 2 x 2 half-voxel cell block, voxel / half-voxel key
  faces -- on worlds translated up to 1e6 m from the origin.  Every query carries its family, the gap it REALISES in float64 (the bins
  are assigned from that, never from the target) and whether it survived (a third candidate did not intervene).

Placement is a two-step affair.  The coarse step solves the (exactly linear) difference of two squared distances for a shift of the
query; it reaches whatever the float64 grid of `g` permits (one ulp of a coordinate at 1e6 m is 1.2e-10 m).  The fine step -- the ulp
bins -- walks the lattice of ulp steps of the three coordinates: two axes are stepped over a square of +-ULP_R steps and the axis with the
SMALLEST slope (ulps of d^2 per ulp of the coordinate) is solved for, so the residual is below that slope and every small integer
number of ulps is met by some combination when the slopes are incommensurate.  Where a pair leaves no such axis (an axis-parallel
lattice pair at 1e6 m: the difference moves in steps of 2^-37 m^2 or not at all) only the exact tie is representable; the generator
reports what it realised and the test asserts coverage on that.
"""
import math

import numpy as np

from elimaloc_amd import synth

OFFSETS = ((0.0, 0.0, 0.0), (1234.5, -777.0, -3.0), (-50000.0, 30000.0, 100.0), (131071.5, -131072.25, 250.0), (1.0e6, -1.0e6, 0.0))
VOXEL_SIZES = (0.4, 0.5, 1.0, 1.3)
CAPS = (6, 30)
N27 = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.int64)  # vhm.cpp:208-243, x slowest
N7 = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.int64)
ULP_BINS = (0, 1, -1, 2, -2, 8, -8)
ULP_R = 60
PAIR_FAMILIES = ("runner", "runner_far", "keyface", "blockface", "vrunner")
RADIUS_FAMILIES = ("radius", "vradius", "aradius")
FAMILIES = PAIR_FAMILIES + ("blockrho",) + RADIUS_FAMILIES


def sq(e):
    """|e|^2 in the reference's association (Eigen's redux order for size 3)."""
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def cases():
    """(world, offset index, voxel size, bucket cap): the planar world at every offset x voxel size, the dense blob (bucket cap hit) and the
    dyadic lattice (exact ties by construction) at every offset with the voxel sizes and caps rotating."""
    out = []
    for o in range(len(OFFSETS)):
        for k, vs in enumerate(VOXEL_SIZES):
            out.append(("planar", o, vs, CAPS[(k + o) % 2]))
        out.append(("blob", o, VOXEL_SIZES[(o + 2) % 4], 30))
        if VOXEL_SIZES[(o + 2) % 4] != 0.4:  # the block-face family lives on oblique pairs and small cells: a fine-voxel blob at every offset
            out.append(("blob", o, 0.4, 30))
        out.append(("lattice", o, 1.0, CAPS[(o + 1) % 2]))
        out.append(("lattice", o, 0.5, CAPS[o % 2]))
    return out


def case_id(case):
    return f"{case[0]}-o{case[1]}-vs{case[2]}-cap{case[3]}"


_WORLDS = {}


def base_world(kind):
    """float32 points around the origin, before the translation."""
    if kind not in _WORLDS:
        if kind == "planar":
            w = synth.make_world(24000, seed=4101)
        elif kind == "blob":
            w = np.random.default_rng(4102).uniform(-2.5, 2.5, size=(40000, 3)).astype(np.float32)
        else:  # dyadic lattice, pitch 0.5, offset 0.125, symmetric about the origin, insertion order != spatial order
            ax = np.arange(-8, 8) * 0.5 + 0.125
            gx, gy, gz = np.meshgrid(ax, ax, ax[4:12], indexing="ij")
            w = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1)
            w = w[np.random.default_rng(4103).permutation(len(w))].astype(np.float32)
        _WORLDS[kind] = w
    return _WORLDS[kind]


def world_of(case):
    """The world translated in float64, then rounded to float32 like a PCD stores it."""
    return (base_world(case[0]).astype(np.float64) + np.array(OFFSETS[case[1]])).astype(np.float32)


class NpMap:
    """VoxelHashMap::AddPoints + the three correspondence walks, from the rule."""

    def __init__(self, points, voxel_size, max_points):
        p = np.asarray(points, dtype=np.float32).astype(np.float64)
        self.vs, self.cap = float(voxel_size), int(max_points)
        res = math.sqrt(self.vs * self.vs / self.cap)
        keys = np.trunc(p / self.vs).astype(np.int64)  # vhm.cpp:275: (int)(x / voxel_size)
        buckets = {}
        for i, k in enumerate(map(tuple, keys.tolist())):
            b = buckets.get(k)
            if b is None:
                buckets[k] = [i]
            elif len(b) < self.cap:
                if not (np.sqrt(sq(p[b] - p[i])) < res).any():
                    b.append(i)
        self.vkeys = np.array(list(buckets.keys()), dtype=np.int64).reshape(-1, 3)
        self.vcnt = np.array([len(b) for b in buckets.values()], dtype=np.int64)
        self.vstart = np.concatenate([[0], np.cumsum(self.vcnt)[:-1]]).astype(np.int64)
        self.pts = p[np.concatenate(list(buckets.values()))] if buckets else np.zeros((0, 3))
        self.pvox = np.repeat(np.arange(len(self.vcnt)), self.vcnt)
        # rowwise().mean(): the sum in insertion order, divided by n; a single point is its own mean
        s = np.zeros((len(self.vcnt), 3))
        for j in range(int(self.vcnt.max()) if len(self.vcnt) else 0):
            has = self.vcnt > j
            s[has] = s[has] + self.pts[self.vstart[has] + j]
        self.vmean = np.where((self.vcnt == 1)[:, None], s, s / self.vcnt[:, None].astype(np.float64))
        self.k0 = self.vkeys.min(axis=0) - 2
        self.dims = self.vkeys.max(axis=0) - self.k0 + 3
        code = self._code(self.vkeys)
        self._order = np.argsort(code)
        self._codes = code[self._order]

    def _code(self, k):
        r = k - self.k0
        return (r[..., 0] * self.dims[1] + r[..., 1]) * self.dims[2] + r[..., 2]

    def lookup(self, k):
        """voxel index of the STORED key k, -1 where there is none"""
        r = k - self.k0
        inside = ((r >= 0) & (r < self.dims)).all(axis=-1)
        c = np.where(inside, self._code(k), -1)
        pos = np.clip(np.searchsorted(self._codes, c), 0, len(self._codes) - 1)
        return np.where(inside & (self._codes[pos] == c), self._order[pos], -1)

    def floor_key(self, g):
        return np.floor(g / self.vs).astype(np.int64)  # vhm.hpp:176-180

    def point_candidates(self, g):
        """[n, 27 * cap] indices into pts in the reference's visiting order, -1 = no candidate"""
        v = self.lookup(self.floor_key(g)[:, None, :] + N27[None])           # [n, 27]
        j = np.arange(self.cap)
        idx = np.where(v[:, :, None] >= 0, self.vstart[np.maximum(v, 0)][:, :, None] + j, -1)
        idx = np.where(j[None, None, :] < np.where(v >= 0, self.vcnt[np.maximum(v, 0)], 0)[:, :, None], idx, -1)
        return idx.reshape(len(g), 27 * self.cap)

    def _dists(self, cand, table, g):
        d = sq(table[np.maximum(cand, 0)] - g[:, None, :])
        return np.where(cand >= 0, d, np.inf)

    def _walk(self, cand, table, g, th, best3):
        d = self._dists(cand, table, g)
        if best3:
            o = np.argsort(d, axis=1, kind="stable")[:, :3]
            return np.take_along_axis(cand, o, 1), np.take_along_axis(d, o, 1)
        w = np.argmin(d, axis=1)  # the first strict minimum of the walk
        r = np.arange(len(g))
        win = cand[r, w]
        tgt = np.where((win >= 0)[:, None], table[np.maximum(win, 0)], 0.0)  # nothing found: the default target, the origin
        dfin = sq(tgt - g)
        return dfin < th * th, tgt, win, dfin

    def _chunked(self, f, g, chunk=512):
        parts = [f(g[i:i + chunk]) for i in range(0, len(g), chunk)] or [f(g[:0])]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))

    def nearest_points(self, g, th):
        """GetCorrespondencePoints (vhm.cpp:31-88) -> accepted, target, index into pts (-1: the origin), d^2"""
        return self._chunked(lambda q: self._walk(self.point_candidates(q), self.pts, q, th, False), np.asarray(g, dtype=np.float64))

    def best3_points(self, g):
        return self._chunked(lambda q: self._walk(self.point_candidates(q), self.pts, q, 0.0, True), np.asarray(g, dtype=np.float64))

    def voxel_candidates(self, g, nb=N27):
        return self.lookup(self.floor_key(g)[:, None, :] + nb[None])

    def nearest_voxel(self, g, th):
        """GetCorrespondencesCov (vhm.cpp:90-151) -> accepted, mean, voxel index, d^2"""
        g = np.asarray(g, dtype=np.float64)
        return self._walk(self.voxel_candidates(g), self.vmean, g, th, False)

    def best3_voxels(self, g):
        g = np.asarray(g, dtype=np.float64)
        return self._walk(self.voxel_candidates(g), self.vmean, g, 0.0, True)

    def all_cov_pairs(self, g, th):
        """GetCorrespondencesAllCov (vhm.cpp:153-206) -> source index, mean, voxel index of every pair, input order"""
        g = np.asarray(g, dtype=np.float64)
        v = self.voxel_candidates(g, N7)
        ok = self._dists(v, self.vmean, g) < th * th
        src, pos = np.nonzero(ok)
        return src, self.vmean[v[src, pos]], v[src, pos]


# ---- the public cell definition: half-voxel cells that follow the STORED keys --------------------------------------
def stored_cell(q, vs):
    """half-voxel cell of a stored coordinate: truncation folds towards zero, a coordinate on a face counts to the cell further from zero"""
    t = np.floor(2.0 * (np.abs(q) / vs)).astype(np.int64)
    return np.where(q >= 0, t, -t - 1)


def block_of(g, vs):
    """per axis the (clipped) two-cell span a query leans into, and rho: the distance (m) to the block's open faces"""
    q = g / vs
    t = q + q
    cg = np.floor(t)
    fr = t - cg
    cg = cg.astype(np.int64)
    f = cg >> 1
    kl, kh = f - 1, f + 1
    alo = 2 * kl - np.where(kl <= 0, 2, 0)
    ahi = 2 * kh + np.where(kh < 0, -1, 1)
    c0 = np.where(fr >= 0.5, cg, cg - 1)
    blo, bhi = np.maximum(c0, alo), np.minimum(c0 + 1, ahi)
    dlo = np.where(blo == alo, np.inf, (cg - blo) + fr)
    dhi = np.where(bhi == ahi, np.inf, (bhi + 1 - cg) - fr)
    rho = np.minimum(dlo, dhi).min(axis=-1) * (0.5 * vs)
    return blo, bhi, rho


def in_block(q, g, vs):
    blo, bhi, _ = block_of(g, vs)
    c = stored_cell(q, vs)
    return ((c >= blo) & (c <= bhi)).all(axis=-1)


# ---- placement ---------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rng, u):
    w = rng.normal(size=u.shape)
    w -= (w * u).sum(-1, keepdims=True) * u
    return _unit(w)


def _log_gaps(rng, n, lo, hi):
    """log-uniform magnitudes, both signs"""
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n)) * rng.choice([-1.0, 1.0], n)


def _shift_pair(a, b, g, want, axis=None):
    """move g so that d_b - d_a (linear in g) becomes `want`: along a - b, or along one coordinate axis"""
    delta = sq(b - g) - sq(a - g)
    ab = a - b
    if axis is None:
        n = np.linalg.norm(ab, axis=-1)
        return g + ((want - delta) / (2.0 * n))[:, None] * (ab / n[:, None])
    out = g.copy()
    r = np.arange(len(g))
    out[r, axis] += (want - delta) / (2.0 * ab[r, axis])
    return out


def ulp_search(a, g0, b=None, th2=None, targets=ULP_BINS, R=ULP_R):
    """Queries on the ulp lattice around g0 (where d_a ~ X) at which (X - d_a) / ulp is exactly one of `targets`, X = d_b or th^2 and ulp
    = spacing(min(d_a, X)).  -> (row of g0, target, g)."""
    n = len(g0)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
    sp = np.maximum(np.spacing(np.abs(g0)), 2.0 ** -70)
    grad = 2.0 * (b - a) if b is not None else 2.0 * (g0 - a)      # d(d_a - X) / dg
    X0 = sq(b - g0) if b is not None else np.full(n, th2)
    ulp = np.spacing(np.minimum(sq(a - g0), X0))
    slope = np.abs(grad * sp) / ulp[:, None]
    cost = np.where(slope >= 0.25, slope, np.inf)
    cs = np.where(np.isfinite(cost).any(axis=1), np.argmin(cost, axis=1), np.argmax(slope, axis=1))
    o1, o2 = (cs + 1) % 3, (cs + 2) % 3
    k = np.arange(-R, R + 1, dtype=np.float64)
    k1, k2 = (x.ravel() for x in np.meshgrid(k, k, indexing="ij"))
    r = np.arange(n)
    g = np.repeat(g0[:, None, :], len(k1), axis=1)
    g[r, :, o1] += k1[None, :] * sp[r, o1][:, None]
    g[r, :, o2] += k2[None, :] * sp[r, o2][:, None]
    X = (lambda q: sq(b[:, None, :] - q)) if b is not None else (lambda q: np.full(q.shape[:2], th2))
    F = sq(a[:, None, :] - g) - X(g)
    step = (grad[r, cs] * sp[r, cs])[:, None]
    step = np.where(step == 0.0, np.inf, step)
    rows, tg, out = [], [], []
    for t in targets:  # aim the solved axis at every target in turn: d_a - X = -t ulp
        q = g.copy()
        q[r, :, cs] += np.round((-t * ulp[:, None] - F) / step) * sp[r, cs][:, None]
        da, Xg = sq(a[:, None, :] - q), X(q)
        hit = (Xg - da) / np.spacing(np.minimum(da, Xg)) == t
        has = hit.any(axis=1)
        first = np.argmax(hit, axis=1)
        rows.append(r[has]); tg.append(np.full(int(has.sum()), t)); out.append(q[r[has], first[has]])
    return np.concatenate(rows), np.concatenate(tg), np.concatenate(out)


class Queries:
    """One generated set: g [n, 3] float64 and, per query, family, kind ('log' / 'ulp'), the REALISED gap (relative: (d2 - d1) / d1 for the
    pair families, (d1 - th^2) / th^2 for the radius families, metres for the block families; signed), the realised gap in ulps, the
    intended candidates (indices into NpMap.pts or NpMap.vmean) and `ok`: the query survived.  `th` is the search radius of the family."""

    def __init__(self):
        self.g, self.family, self.kind, self.gap, self.ulps, self.ia, self.ib, self.ok, self.th, self.pos = ([] for _ in range(10))

    def add(self, family, kind, g, gap, ulps, ia, ib, ok, th, pos=None):
        n = len(g)
        self.g.append(g); self.family += [family] * n; self.kind += [kind] * n
        self.gap.append(gap); self.ulps.append(ulps); self.ia.append(ia); self.ib.append(ib); self.ok.append(ok)
        self.th.append(np.full(n, th)); self.pos.append(np.full(n, -1) if pos is None else pos)

    def close(self):
        for k in ("g", "gap", "ulps", "ia", "ib", "ok", "th", "pos"):
            setattr(self, k, np.concatenate(getattr(self, k)))
        self.family, self.kind = np.array(self.family), np.array(self.kind)
        return self

    def select(self, family):
        return np.flatnonzero(self.family == family)


def _realise_pair(best3, a_idx, b_idx, g, table):
    """the two best candidates of the walk are the intended pair and the third lies strictly behind -> realised gap, ulps, ok"""
    i3, d3 = best3(g)
    ok = (((i3[:, 0] == a_idx) & (i3[:, 1] == b_idx)) | ((i3[:, 0] == b_idx) & (i3[:, 1] == a_idx))) & (d3[:, 2] > d3[:, 1])
    da, db = sq(table[a_idx] - g), sq(table[b_idx] - g)
    d1 = np.minimum(da, db)
    ok &= (d3[:, 0] == d1) & (d3[:, 1] == np.maximum(da, db))
    return (db - da) / d1, (db - da) / np.spacing(d1), ok


def _across_a_face(rng, a, b, vs):
    """A point on the bisector of a and b from which exactly one of them lies outside the block: on some axis c a cell face F lies
    between a_c and b_c (their stored cells differ); the query slides inside the bisector plane, along the direction with the largest
    c-component, until its c-coordinate is 0.5 .. 0.95 cells beyond F -- then F is the open face of its block on that axis.  Pairs
    without such an axis get NaN (not usable)."""
    hc = 0.5 * vs
    u = _unit(a - b)
    ca, cb = stored_cell(a, vs), stored_cell(b, vs)
    w = np.eye(3)[None] - u[:, :, None] * u[:, None, :]            # row c: e_c projected into the bisector plane
    score = np.where(np.abs(ca - cb) == 1, np.abs(w[:, [0, 1, 2], [0, 1, 2]]), -1.0)
    c = np.argmax(score, axis=1)
    r = np.arange(len(a))
    good = score[r, c] > 0.2
    wc = w[r, c]                                                      # [n, 3]; its c-component is score
    F = np.maximum(ca[r, c], cb[r, c]) * hc
    side = rng.choice([-1.0, 1.0], len(a))
    gc = F + side * rng.uniform(0.5, 0.95, len(a)) * hc
    mid = 0.5 * (a + b)
    t = (gc - mid[r, c]) / np.where(good, wc[r, c], 1.0)
    return np.where(good[:, None], mid + t[:, None] * wc, np.nan)


def _pair_draws(rng, m, best3, table, ia, ib, h, th, across=False):
    """usable draws: at the point g0 = midpoint + h w on the bisector the two best candidates are a and b, within reach of the radius"""
    a, b = table[ia], table[ib]
    u = _unit(a - b)
    if across:
        g0 = _across_a_face(rng, a, b, m.vs)
        keep = np.isfinite(g0).all(axis=1)
        g0, ok = _pair_draws_at(best3, table, ia[keep], ib[keep], g0[keep], th)
        full, okf = np.zeros((len(ia), 3)), np.zeros(len(ia), bool)
        full[keep], okf[keep] = g0, ok
        return full, okf
    return _pair_draws_at(best3, table, ia, ib, 0.5 * (a + b) + h[:, None] * _perp(rng, u), th)


def _pair_draws_at(best3, table, ia, ib, g0, th):
    a, b = table[ia], table[ib]
    g0 = _shift_pair(a, b, g0, 0.0)
    _, _, ok = _realise_pair(best3, ia, ib, g0, table)
    ok &= sq(a - g0) < 0.9 * th * th
    return g0, ok


def _neighbour_pairs(rng, m, n, spot):
    """(a, b): b is the stored point nearest to a spot `spot` metres from a -- a true neighbour"""
    ia = rng.integers(0, len(m.pts), n)
    s = m.pts[ia] + spot * _unit(rng.normal(size=(n, 3)))
    ib = m.nearest_points(s, 1e9)[2]
    keep = (ib >= 0) & (ib != ia)
    return ia[keep], ib[keep]


def generate(case, m=None, n_draw=700, seed=0):
    """All families for one (world, offset, voxel size, cap).  -> (NpMap, Queries, stats) with stats[family] = (constructed, discarded)."""
    kind, o, vs, cap = case
    if m is None:
        m = NpMap(world_of(case), vs, cap)
    rng = np.random.default_rng(77000 + 131 * o + int(vs * 10) + cap + seed + {"planar": 0, "blob": 5000, "lattice": 9000}[kind])
    Q = Queries()
    spot = 0.6 * 0.5 if kind == "lattice" else 0.12
    TH = 5.0

    def pair_family(name, best3, table, ia, ib, h, th, axis_face=False, metres=False, need_xor=False):
        g0, ok = _pair_draws(rng, m, best3, table, ia, ib, h, th, across=need_xor)
        a_i, b_i, g0 = ia[ok], ib[ok], g0[ok]
        a, b = table[a_i], table[b_i]
        n = len(g0)
        ax = None
        if axis_face:
            # one coordinate sits within +-4 ulps of a voxel / half-voxel face (the axis the pair is least separated along); the gap is
            # then set along the axis the pair is most separated along, so the face coordinate stays where it was put
            ab = np.abs(a - b)
            c = np.argmin(ab, axis=1)
            ax = np.argmax(ab, axis=1)
            r = np.arange(n)
            face = np.round(g0[r, c] / (0.5 * vs)) * (0.5 * vs)
            j = rng.integers(-4, 5, n)
            g0 = g0.copy()
            g0[r, c] = face + j * np.spacing(np.abs(face) + 1e-300)
            g0 = _shift_pair(a, b, g0, 0.0, axis=ax)
            _, _, ok2 = _realise_pair(best3, a_i, b_i, g0, table)
            a_i, b_i, g0, ax = a_i[ok2], b_i[ok2], g0[ok2], ax[ok2]
            a, b = table[a_i], table[b_i]
            n = len(g0)
        if need_xor:  # exactly one of the pair lies outside the block the query leans into
            x = in_block(a, g0, vs) ^ in_block(b, g0, vs)
            a_i, b_i, g0, a, b = a_i[x], b_i[x], g0[x], a[x], b[x]
            n = len(g0)
        if need_xor:  # such draws are rare: every one carries six gaps of the sweep (tiled, so the ulp search below still sees distinct draws)
            a_i, b_i, g0, a, b = (np.tile(x, (6,) + (1,) * (x.ndim - 1)) for x in (a_i, b_i, g0, a, b))
            n = len(g0)
        d1 = sq(a - g0)
        gaps = _log_gaps(rng, n, 1e-15, 1e-3)
        if metres:  # d_b - d_a = (sqrt d_b - sqrt d_a)(sqrt d_b + sqrt d_a): a sweep of +-1e-9 .. 1e-3 m in the ROOT
            gaps = _log_gaps(rng, n, 1e-9, 1e-3) * 2.0 / np.sqrt(d1)
        gaps[rng.random(n) < 0.04] = 0.0
        g = _shift_pair(a, b, g0, gaps * d1, axis=ax)
        gap, ulps, okq = _realise_pair(best3, a_i, b_i, g, table)
        if need_xor:
            okq &= in_block(a, g, vs) ^ in_block(b, g, vs)
        if metres:
            gap = np.sqrt(sq(b - g)) - np.sqrt(sq(a - g))
        Q.add(name, "log", g, gap, ulps, a_i, b_i, okq, th)
        ns = min(n // 6, 160) if need_xor else min(n, 64)
        rows, tg, gu = ulp_search(a[:ns], g0[:ns], b=b[:ns])
        gap, ulps, okq = _realise_pair(best3, a_i[rows], b_i[rows], gu, table)
        if need_xor:
            okq &= in_block(a[rows], gu, vs) ^ in_block(b[rows], gu, vs)
        if metres:
            gap = np.sqrt(sq(b[rows] - gu)) - np.sqrt(sq(a[rows] - gu))
        Q.add(name, "ulp", gu, gap, ulps, a_i[rows], b_i[rows], okq & (ulps == tg), th)

    ia, ib = _neighbour_pairs(rng, m, 3 * n_draw, spot)
    n = len(ia)
    pair_family("runner", m.best3_points, m.pts, ia, ib, rng.uniform(0.0, 0.03, n), TH)
    # far candidates: the pair seen from up to the search radius (as far as both stay within the 27 buckets the walk visits)
    th_far = 1.5 * vs
    pair_family("runner_far", m.best3_points, m.pts, ia, ib, np.exp(rng.uniform(math.log(0.03), math.log(th_far), n)), th_far)
    pair_family("keyface", m.best3_points, m.pts, ia, ib, rng.uniform(0.0, 0.03, n), TH, axis_face=True)
    ia2, ib2 = _neighbour_pairs(rng, m, 12 * n_draw, spot)
    pair_family("blockface", m.best3_points, m.pts, ia2, ib2, rng.uniform(0.0, 0.45 * vs, len(ia2)), TH, metres=True, need_xor=True)
    # voxel means of face-adjacent voxels
    va = rng.integers(0, len(m.vmean), 3 * n_draw)
    vb = m.lookup(m.vkeys[va] + N7[rng.integers(1, 7, len(va))])
    keep = vb >= 0
    pair_family("vrunner", m.best3_voxels, m.vmean, va[keep], vb[keep], rng.uniform(0.0, 0.03, int(keep.sum())), TH)

    # ---- the nearest candidate against rho, the distance to the open faces of the block: sqrt(d1) - rho = delta ----------------------------
    # g0 somewhere within reach of the map, a = ITS nearest stored point; the query then slides along the ray from a through g0: a point's
    # Voronoi cell is star-shaped about it, so a stays the nearest candidate for every r <= |g0 - a|
    n = 3 * n_draw
    h = 0.5 * vs
    g0 = m.pts[rng.integers(0, len(m.pts), n)] + rng.uniform(0.5 * h, 1.4 * h, n)[:, None] * _unit(rng.normal(size=(n, 3)))
    _, _, ia, d0 = m.nearest_points(g0, 1e9)
    keep = ia >= 0
    g0, ia, r0 = g0[keep], ia[keep], np.sqrt(d0[keep])
    n = len(ia)
    a = m.pts[ia]
    dirn = (g0 - a) / np.maximum(r0, 1e-300)[:, None]
    delta = _log_gaps(rng, n, 1e-9, 1e-3)
    delta[rng.random(n) < 0.04] = 0.0
    f = lambda r: r - block_of(a + r[:, None] * dirn, vs)[2] - delta
    lo, hi = np.full(n, 0.02 * h), r0.copy()
    usable = (f(lo) < 0) & (f(hi) > 0)
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        neg = f(mid) < 0
        lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
    g = a + hi[:, None] * dirn
    i3, d3 = m.best3_points(g)
    real = np.sqrt(sq(a - g)) - block_of(g, vs)[2]
    usable &= np.abs(real - delta) < 0.01 * np.abs(delta) + 1e-12 * (np.abs(g).max(axis=1) + 1.0)  # the bisection ended on a root, not on a jump of rho
    okq = (i3[:, 0] == ia) & (d3[:, 1] > d3[:, 0])
    Q.add("blockrho", "log", g[usable], real[usable], np.zeros(int(usable.sum())), ia[usable], np.full(int(usable.sum()), -1), okq[usable], TH)

    # ---- the search radius: d1 = th^2 (1 + e), the strict < of the acceptance test ---------------------------------------------------------
    def radius_family(name, table, nearest, th, idx, usable_at, along_axes=False):
        a = table[idx]
        w = rng.normal(size=a.shape)
        if along_axes:  # towards one of the six face neighbours, loosely
            w = 0.3 * w + np.eye(3)[rng.integers(0, 3, len(a))] * rng.choice([-1.0, 1.0], (len(a), 1))
        w = _unit(w)
        g0 = a + th * w
        g0 = g0 + ((th * th - sq(a - g0)) / (2.0 * th))[:, None] * w
        ok, pos = usable_at(g0, idx)
        idx, a, w, g0, pos = idx[ok], a[ok], w[ok], g0[ok], pos[ok]
        n = len(idx)
        e = _log_gaps(rng, n, 1e-12, 1e-3)
        g = g0 + (0.5 * th * e)[:, None] * w
        g = g + ((th * th * (1.0 + e) - sq(a - g)) / (2.0 * th))[:, None] * w
        rows, tg, gu = ulp_search(a[:64], g0[:64], th2=th * th, targets=(0, 1, -1))
        for kind_, gg, ii, pp, want in (("log", g, idx, pos, None), ("ulp", gu, idx[rows], pos[rows], tg)):
            d = sq(table[ii] - gg)
            okq, pos2 = usable_at(gg, ii)
            ulps = (d - th * th) / np.spacing(th * th)
            if want is not None:
                okq &= ulps == -want  # (ulp_search counts th^2 - d)
            Q.add(name, kind_, gg, (d - th * th) / (th * th), ulps, ii, np.full(len(ii), -1), okq, th, pos2)

    def nearest_is(best3):
        def f(g, idx):
            i3, d3 = best3(g)
            return (i3[:, 0] == idx) & (d3[:, 1] > d3[:, 0]), np.zeros(len(g), np.int64)
        return f

    def among_seven(g, idx):
        v = m.voxel_candidates(g, N7)
        hit = v == idx[:, None]
        return hit.any(axis=1), np.argmax(hit, axis=1)

    th_p = {"planar": 0.12, "blob": 0.06, "lattice": 0.2}[kind]
    radius_family("radius", m.pts, m.nearest_points, th_p, rng.integers(0, len(m.pts), 4 * n_draw), nearest_is(m.best3_points))
    radius_family("vradius", m.vmean, m.nearest_voxel, 0.3 * vs, rng.integers(0, len(m.vmean), 2 * n_draw), nearest_is(m.best3_voxels))
    radius_family("aradius", m.vmean, None, 0.7 * vs, rng.integers(0, len(m.vmean), 2 * n_draw), among_seven)
    # a stored key f - 1 on a negative axis holds points at least one voxel from the query: that pair needs a radius beyond one voxel
    radius_family("aradius", m.vmean, None, 1.2 * vs, rng.integers(0, len(m.vmean), 2 * n_draw), among_seven, along_axes=True)
    Q.close()
    stats = {fam: (int((Q.family == fam).sum()), int(((Q.family == fam) & ~Q.ok).sum())) for fam in FAMILIES}
    return m, Q, stats


def decade(x):
    """floor(log10 |x|) of the realised gaps; 0 -> -999"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x > 0, np.floor(np.log10(np.where(x > 0, x, 1.0))), -999).astype(np.int64)


def easy_queries(m, n, seed):
    """noise-free copies of stored map points: decided by stage 1 at once"""
    return m.pts[np.random.default_rng(seed).integers(0, len(m.pts), n)].copy()
