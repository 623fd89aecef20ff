"""The rotation family of the graph back end's tests (tests/test_rotation_edges_abi.py, tests/test_rotation_edges.py):
residual rotations beyond 120 degrees, where Log (pg_log of elm_dev_pgraph.hpp; posegraph_ref.quat) leaves its first quaternion branch, with
their truth at 50 digits from mpmath.  An edge's or a loop pair's kind is the branch Log takes on R_E together with the sign of the raw
quaternion w before the flip to w >= 0: KINDS.  Here are the ladder of angles up to pi - 1e-12 about one axis per leading entry and its
negative, the exact set (ties of the diagonal, tr == 0, w == 0, built bit-exact), graphs and loop sets that carry them planted (R_E is
the family's matrix bit for bit) and embedded (the same rotations between random poses), each in an order that mixes the kinds in every
wavefront and in one that gives every kind wavefronts of its own, the truth of every output as a float64 pair (value, remainder), and
the census.  Plain numpy and mpmath; no GPU, no oracle.  `python tests/rotation_cases.py` prints the census."""
import functools
import math

import numpy as np
from mpmath import mp, mpf

import loopcov_cases as ccases
import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref

DPS = 50
KINDS = ("tr>0", "x w>=0", "x w<0", "y w>=0", "y w<0", "z w>=0", "z w<0")
NK = len(KINDS)

# Host errors against the 50-digit truth on the planted sets, measured on the development host (the figures are in the header of
# tests/test_rotation_edges_abi.py and in DESIGN.md section 22); each bound is 10 x the host library's, the margin of
# tests/test_posegraph_abi.py for libm differences between hosts.  The GPU tests hold the device to the same numbers.
BOUNDS = dict(r=4.8e-15, A=4.5e-15, B=3.5e-15, s=6.5e-15, w=2.5e-15, rho=6.6e-15, jinv=3.5e-15, pair_e=1.1e-14, pair_s=1.2e-14,
              pair_s_cov=2.1e-14)


# ---------------------------------------------------------------- kinds, by the contract's exact comparisons on float64
def kind_of(R):
    """the kind of R [..., 3, 3] -> int array: 0 for tr > 0, else 1 + 2 * (leading entry) + (raw w < 0)"""
    R = np.asarray(R, dtype=np.float64)
    m = lambda a, b: R[..., a, b]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    lead0 = (m(0, 0) >= m(1, 1)) & (m(0, 0) >= m(2, 2))
    lead1 = ~lead0 & (m(1, 1) >= m(2, 2))
    lead = np.where(lead0, 0, np.where(lead1, 1, 2))
    raw_w = np.where(lead0, m(2, 1) - m(1, 2), np.where(lead1, m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)))
    return np.where(tr > 0.0, 0, 1 + 2 * lead + (raw_w < 0.0)).astype(np.int64)


def census(kinds):
    return np.bincount(np.asarray(kinds).reshape(-1), minlength=NK)[:NK]


# ---------------------------------------------------------------- 50 digits
def _mpv(v):
    return [mpf(float(x)) if not isinstance(x, mpf) else x for x in v]


def _mpm(M):
    return [[mpf(float(M[i][j])) for j in range(3)] for i in range(3)]


def _hat(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def _mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def mp_exp(phi):
    """Rodrigues at the working precision: phi [3] of mpf -> 3 x 3 of mpf"""
    th = mp.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    I = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    if th == 0:
        return I
    K = _hat([x / th for x in phi])
    K2 = _mul(K, K)
    s, c = mp.sin(th), mp.cos(th)
    return [[I[i][j] + s * K[i][j] + (1 - c) * K2[i][j] for j in range(3)] for i in range(3)]


def to_f64(M):
    """every entry rounded once to float64"""
    return np.array([[float(x) for x in row] for row in M], dtype=np.float64)


def mp_log(R):
    """Log by the contract's branches with exact comparisons, at the working precision: R 3 x 3 of mpf -> (phi, theta, w, n).  On an
    exactly orthogonal R it is the exact Log with the contract's sign; on a float64 R_E it is the closed form on those inputs."""
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        t = mp.sqrt(tr + 1)
        q = [t / 2, (R[2][1] - R[1][2]) / (2 * t), (R[0][2] - R[2][0]) / (2 * t), (R[1][0] - R[0][1]) / (2 * t)]
    elif R[0][0] >= R[1][1] and R[0][0] >= R[2][2]:
        t = mp.sqrt(R[0][0] - R[1][1] - R[2][2] + 1)
        q = [(R[2][1] - R[1][2]) / (2 * t), t / 2, (R[1][0] + R[0][1]) / (2 * t), (R[2][0] + R[0][2]) / (2 * t)]
    elif R[1][1] >= R[2][2]:
        t = mp.sqrt(R[1][1] - R[2][2] - R[0][0] + 1)
        q = [(R[0][2] - R[2][0]) / (2 * t), (R[0][1] + R[1][0]) / (2 * t), t / 2, (R[2][1] + R[1][2]) / (2 * t)]
    else:
        t = mp.sqrt(R[2][2] - R[0][0] - R[1][1] + 1)
        q = [(R[1][0] - R[0][1]) / (2 * t), (R[0][2] + R[2][0]) / (2 * t), (R[1][2] + R[2][1]) / (2 * t), t / 2]
    if q[0] < 0:
        q = [-x for x in q]
    w, v = q[0], q[1:]
    n = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if n == 0:
        return [mpf(0)] * 3, mpf(0), w, n
    theta = 2 * mp.atan2(n, w)
    return [x * theta / n for x in v], theta, w, n


def mp_jinv(phi):
    """J^-1 = I + [phi]x / 2 + c [phi]x^2, c = 1 / theta^2 - cot(theta / 2) / (2 theta): the closed form at the working precision"""
    t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = mp.sqrt(t2)
    c = mpf(1) / 12 if th == 0 else 1 / t2 - mp.cot(th / 2) / (2 * th)
    K = _hat(phi)
    K2 = _mul(K, K)
    return [[mpf(int(i == j)) + K[i][j] / 2 + c * K2[i][j] for j in range(3)] for i in range(3)]


def _quat_of(phi):
    th = mp.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    if th == 0:
        return [mpf(1), mpf(0), mpf(0), mpf(0)]
    s = mp.sin(th / 2) / th
    return [mp.cos(th / 2), phi[0] * s, phi[1] * s, phi[2] * s]


def _quat_mul(p, q):
    return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
            p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]


def _quat_log(q):
    """2 atan2(|v|, w) v / |v| without the flip to w >= 0: the smooth continuation of Log through pi, which a derivative at pi needs"""
    n = mp.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    th = 2 * mp.atan2(n, q[0])
    return [x * th / n for x in q[1:]]


def mp_jinv_numeric(phi, h="1e-30"):
    """d Log(Exp(phi) Exp(delta)) / d delta at 0 by central differences on unit quaternions at 100 digits: the residual's derivative under
    the retraction, independent of the closed form and valid at and beyond pi (the truncation error is h^2)"""
    with mp.workdps(100):
        h = mpf(h)
        q0 = _quat_of([+x for x in phi])
        cols = []
        for k in range(3):
            d = [mpf(0)] * 3
            d[k] = h
            up = _quat_log(_quat_mul(q0, _quat_of(d)))
            d[k] = -h
            dn = _quat_log(_quat_mul(q0, _quat_of(d)))
            cols.append([(a - b) / (2 * h) for a, b in zip(up, dn)])
        return [[cols[j][i] for j in range(3)] for i in range(3)]


class DD:
    """a 50-digit array as float64 (hi, lo) with hi + lo the truth to 1e-32: err(got) = |(got - hi) - lo| is exact to that"""

    def __init__(self, nested):
        flat = np.array(nested, dtype=object)
        with mp.workdps(DPS):
            self.hi = np.vectorize(float, otypes=[np.float64])(flat)
            self.lo = np.vectorize(lambda x, h: float(x - mpf(float(h))), otypes=[np.float64])(flat, self.hi)

    def err(self, got):
        return np.abs((np.asarray(got, dtype=np.float64) - self.hi) - self.lo)

    def __getitem__(self, idx):
        out = DD.__new__(DD)
        out.hi, out.lo = self.hi[idx], self.lo[idx]
        return out


# ---------------------------------------------------------------- the family
AXES = ((0.9, 0.3, -0.3), (0.2, 0.9, -0.3), (-0.4, 0.1, 0.9))  # x, y and z lead; each with its negative
LADDER = (2.1, 2.5, 3.0, math.pi - 1e-3, math.pi - 1e-6, math.pi - 1e-9, math.pi - 1e-12)
INNER = (0.6, 0.9, 1.2, 1.5, 1.7, 1.9, 1.99)  # tr > 0: below 2 pi / 3
PER_KIND = len(LADDER)
EITHER_SIGN_WITHIN = 1.5e-9  # a ladder angle this close to pi may come back as phi or as -phi


class Member:
    """one rotation: R float64 [3, 3], phi (mpf) the truth of Log R, kind, either_sign (a ladder angle within 1e-9 of pi), exact (of the
    exact set), name"""

    def __init__(self, name, R, phi, either_sign=False, exact=False):
        self.name, self.R, self.phi, self.either_sign, self.exact = name, R, phi, either_sign, exact
        self.kind = int(kind_of(R))
        self.angle = float(mp.sqrt(sum(x * x for x in phi)))


def _ladder_member(axis, sign, angle):
    a = [mpf(float(x)) * sign for x in axis]
    n = mp.sqrt(sum(x * x for x in a))
    phi = [mpf(float(angle)) * x / n for x in a]
    return Member(f"{angle!r} about {tuple(sign * x for x in axis)}", to_f64(mp_exp(phi)), phi, either_sign=math.pi - angle <= EITHER_SIGN_WITHIN)


@functools.lru_cache(maxsize=None)
def family():
    """-> (by_kind: NK lists of PER_KIND ladder members, exact: the exact set, all rotations of angle >= 2 pi / 3 - 1e-9)"""
    with mp.workdps(DPS):
        by_kind = [[] for _ in range(NK)]
        signed = [(ax, sg) for ax in AXES for sg in (1, -1)]
        for m, ang in enumerate(INNER):
            by_kind[0].append(_ladder_member(*signed[m % len(signed)], ang))
        for lead, ax in enumerate(AXES):
            for neg, sg in enumerate((1, -1)):  # below pi the raw w has the sign of the axis's leading component
                for ang in LADDER:
                    by_kind[1 + 2 * lead + neg].append(_ladder_member(ax, sg, ang))
        for k in range(NK):
            assert [m.kind for m in by_kind[k]] == [k] * PER_KIND, (k, [m.kind for m in by_kind[k]])
        exact = []

        def add_exact(name, rows):
            R = np.array(rows, dtype=np.float64)
            phi, _, _, _ = mp_log(_mpm(R))
            exact.append(Member(name, R, phi, exact=True))

        P = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
        add_exact("cyclic permutation", P)
        add_exact("cyclic permutation transposed", _tr(P))
        add_exact("diag(1,-1,-1)", [[1, 0, 0], [0, -1, 0], [0, 0, -1]])
        add_exact("diag(-1,1,-1)", [[-1, 0, 0], [0, 1, 0], [0, 0, -1]])
        add_exact("diag(-1,-1,1)", [[-1, 0, 0], [0, -1, 0], [0, 0, 1]])
        add_exact("pi about (1,1,0)", [[0, 1, 0], [1, 0, 0], [0, 0, -1]])
        add_exact("pi about (1,0,1)", [[0, 0, 1], [0, -1, 0], [1, 0, 0]])
        add_exact("pi about (0,1,1)", [[-1, 0, 0], [0, 0, 1], [0, 1, 0]])
        for sg in (1, -1):  # tr just either side of 0; rounded like the ladder, so the leading entry is what the rounding leaves
            ang = 2 * mp.pi / 3 + sg * mpf("1e-9")
            phi = [ang / mp.sqrt(3)] * 3
            exact.append(Member(f"2 pi / 3 {'+' if sg > 0 else '-'} 1e-9 about (1,1,1)", to_f64(mp_exp(phi)), phi))
        assert [float(m.R.trace()) for m in exact[:2]] == [0.0, 0.0] and exact[-2].R.trace() < 0.0 < exact[-1].R.trace()
        return by_kind, exact


def _dyadic(rng, n, span=16, step=8):
    """translations on a grid of 1 / step: sums and differences of a few are exact"""
    return rng.integers(-span * step, span * step + 1, (n, 3)).astype(np.float64) / step


# ---------------------------------------------------------------- graphs
RUN = 64  # edges per kind in the main part: one wavefront of k_pg_cost, eight of k_pg_linearize
ORDERS = ("round_robin", "runs")
LAYOUTS = ("planted", "embedded")


def order_permutation(E, order):
    """position in the upload -> canonical edge.  Canonically kind k holds edges 64 k .. 64 k + 63 and the tail follows ("runs"); in
    "round_robin" position p of the main part has kind p % NK."""
    idx = np.arange(E)
    if order == "runs":
        return idx
    main = NK * RUN
    p = idx[:main]
    return np.concatenate([RUN * (p % NK) + p // NK, idx[main:]])


@functools.lru_cache(maxsize=None)
def canonical(layout):
    """-> dict(g: the graph in the "runs" order, members [E], kind [E]: read off the float64 R_E the mirror forms, either_sign [E],
    in_exact_set [E]).  Edge e joins node e (fixed) to node E + e."""
    by_kind, exact = family()
    rng = np.random.default_rng(2200 + LAYOUTS.index(layout))
    members = [by_kind[k][m % PER_KIND] for k in range(NK) for m in range(RUN)]
    # The embedded tail leaves out the half turns of the exact set: between random poses their raw w is a rounding residue of either
    # sign, so Log is +pi or -pi about the axis by the last bit of a product, and no two float64 evaluations need agree.
    members += exact if layout == "planted" else [m for m in exact if abs(m.angle - math.pi) > 1e-3]
    E = len(members)
    assert E >= 320 and E % 256 != 0
    Ti, Tj, Z = (np.tile(np.eye(4), (E, 1, 1)) for _ in range(3))
    for e, m in enumerate(members):
        if layout == "planted":  # products with the identity are exact: R_E is m.R bit for bit
            Ti[e, :3, 3] = _dyadic(rng, 1)[0]
            Z[e, :3, 3] = _dyadic(rng, 1, span=4)[0]
            Tj[e, :3, :3] = m.R
            Tj[e, :3, 3] = Ti[e, :3, 3] + Z[e, :3, 3] + rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-2.0, 0.5)
        else:
            Ti[e], Tj[e] = cases.rand_pose(rng, 3.0, 10.0), cases.rand_pose(rng, 3.0, 10.0)
            back = np.eye(4)
            with mp.workdps(DPS):
                back[:3, :3] = to_f64(mp_exp([-x for x in m.phi]))  # Z = T_i^-1 T_j Exp(-phi): R_E = Exp(phi)
            back[:3, 3] = rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-2.0, 0.5)
            Z[e] = cases.inv_pose(Ti[e]) @ Tj[e] @ back
    info = cases.rand_info(rng, E) * (10.0 ** rng.uniform(-1.0, 1.0, E))[:, None, None]
    fixed = np.arange(2 * E) < E
    g = ref.Graph(np.concatenate([Ti, Tj]), fixed, np.arange(E), E + np.arange(E), Z, info)
    RE = np.swapaxes(Z[:, :3, :3], 1, 2) @ (np.swapaxes(Ti[:, :3, :3], 1, 2) @ Tj[:, :3, :3])  # as posegraph_ref.edge_terms forms it
    if layout == "planted":
        assert all(np.array_equal(RE[e], m.R) for e, m in enumerate(members))
    kind = kind_of(RE)
    assert layout == "planted" or np.abs(raw_w(RE)).min() >= SIGN_CLEAR
    assert kind[:NK * RUN].tolist() == [k for k in range(NK) for _ in range(RUN)]  # the ladder's kinds survive the embedding
    return dict(g=g, members=members, kind=kind, either_sign=np.array([m.either_sign for m in members]),
                in_exact_set=np.array([m.exact for m in members]))


def graph(layout, order):
    """-> (Graph in the given order, perm: position -> canonical edge, kind [E] per position)"""
    c = canonical(layout)
    g = c["g"]
    perm = order_permutation(g.E, order)
    return ref.Graph(g.poses, g.fixed, g.i[perm], g.j[perm], g.Z[perm], g.info[perm]), perm, c["kind"][perm]


def wavefront_kinds(kind, lanes_per_edge):
    """the number of distinct kinds in each full wavefront of a kernel that gives every edge lanes_per_edge lanes, edges in upload order"""
    per = 64 // lanes_per_edge
    return [len(set(kind[w * per:(w + 1) * per].tolist())) for w in range(len(kind) // per)]


def own_wavefronts(kind, lanes_per_edge):
    """the kinds that fill at least one wavefront alone"""
    per = 64 // lanes_per_edge
    return {int(kind[w * per]) for w in range(len(kind) // per) if len(set(kind[w * per:(w + 1) * per].tolist())) == 1}


@functools.lru_cache(maxsize=None)
def planted_truth():
    """The planted graph's outputs at 50 digits, canonical order -> dict of DD: r [E, 6], A, B [E, 6, 6], s [E]; the same at -phi for the
    either_sign edges (r_neg, A_neg, B_neg; elsewhere equal to the first); jinv, jinv_numeric [E, 3, 3]: the closed form and the
    derivative of the exact residual under the retraction, at phi; and huber_k1 with w1, rho1 [E] (w and rho at huber 0 are 1 and s)."""
    c = canonical("planted")
    g, members = c["g"], c["members"]
    E = g.E
    out = {k: [] for k in ("r", "A", "B", "r_neg", "A_neg", "B_neg", "s", "jinv", "jinv_numeric")}
    cache = {}
    with mp.workdps(DPS):
        zero3 = [[mpf(0)] * 3 for _ in range(3)]

        def blocks(m, sign, d, rt):
            phi = [sign * x for x in m.phi]
            key = (id(m), sign)
            if key not in cache:
                cache[key] = (mp_jinv(phi), mp_jinv_numeric(phi))
            J, Jn = cache[key]
            R = _mpm(m.R)
            JRt = _mul(J, _tr(R))
            dx = _hat(d)
            A = [[mpf(-int(i == j)) for j in range(3)] + dx[i] for i in range(3)] + [zero3[i] + [-x for x in JRt[i]] for i in range(3)]
            B = [R[i] + zero3[i] for i in range(3)] + [zero3[i] + J[i] for i in range(3)]
            return rt + phi, A, B, J, Jn

        for e in range(E):
            m = members[e]
            ti, tj, tz = _mpv(g.poses[g.i[e], :3, 3]), _mpv(g.poses[g.j[e], :3, 3]), _mpv(g.Z[e, :3, 3])
            d = [b - a for a, b in zip(ti, tj)]  # R_i = R_Z = I
            rt = [a - b for a, b in zip(d, tz)]
            r, A, B, J, Jn = blocks(m, 1, d, rt)
            rn, An, Bn, _, _ = blocks(m, -1, d, rt) if m.either_sign else (r, A, B, None, None)
            Om = [[mpf(float(x)) for x in row] for row in g.info[e]]
            s = sum(r[a] * Om[a][b] * r[b] for a in range(6) for b in range(6))
            for key, val in (("r", r), ("A", A), ("B", B), ("r_neg", rn), ("A_neg", An), ("B_neg", Bn), ("s", s), ("jinv", J), ("jinv_numeric", Jn)):
                out[key].append(val)
        k1 = huber_k1(np.array([float(x) for x in out["s"]]), c["kind"])
        kk = mpf(k1)
        w1 = [kk / mp.sqrt(s) if s > kk * kk else mpf(1) for s in out["s"]]
        rho1 = [2 * kk * mp.sqrt(s) - kk * kk if s > kk * kk else s for s in out["s"]]
        res = {k: DD(v) for k, v in out.items()}
        res.update(huber_k1=k1, w1=DD(w1), rho1=DD(rho1))
    return res


HUBER_MARGIN = 1e-6  # no s within this of k1^2, relatively: no weight hangs on a last digit
HUBER_MIN_SIDE = 8   # inliers and outliers of every kind


def huber_k1(s, kind):
    """a Huber threshold with at least HUBER_MIN_SIDE inliers and outliers of every kind: the square root of the midpoint of two
    neighbouring sorted s nearest the median that has them"""
    v = np.sort(s)
    mid = len(v) // 2
    for off in sorted(range(1, len(v)), key=lambda q: abs(q - mid)):
        k2 = 0.5 * (v[off - 1] + v[off])
        if (v[off] - v[off - 1]) < 2.0 * HUBER_MARGIN * k2:
            continue
        inl, outl = census(kind[s <= k2]), census(kind[s > k2])
        if inl.min() >= HUBER_MIN_SIDE and outl.min() >= HUBER_MIN_SIDE:
            return float(math.sqrt(k2))
    raise AssertionError("no Huber threshold with inliers and outliers of every kind")


def edge_errors(got, truth, idx, either_sign):
    """per edge, the worst |got - truth| of r, A and B (got in any order, idx the canonical edge of each position); for the either_sign
    edges the smaller of the errors against phi and against -phi, r, A and B taken together -> (err_r, err_A, err_B) [E] each and
    negated [E] bool: the edges that came back as -phi"""
    def worst(sfx):
        return [truth[q + sfx][idx].err(got[q]).reshape(len(idx), -1).max(1) for q in ("r", "A", "B")]
    pos, neg = worst(""), worst("_neg")
    negated = either_sign[idx] & (np.maximum.reduce(neg) < np.maximum.reduce(pos))
    return tuple(np.where(negated, n, p) for p, n in zip(pos, neg)) + (negated,)


def graph_errors(got, truth, idx, either_sign, k1=True):
    """Worst error per quantity of one evaluation of the planted graph (got in any order, idx the canonical edge of each position) ->
    (dict, negated).  s and rho are relative to max(1, truth); w and rho against huber_k1's truth if k1, else against 1 and s; rho only
    if got has it."""
    er, eA, eB, negated = edge_errors(got, truth, idx, either_sign)
    s_hi = truth["s"].hi[idx]
    out = dict(r=er.max(), A=eA.max(), B=eB.max(), s=(truth["s"][idx].err(got["s"]) / np.maximum(1.0, s_hi)).max())
    out["w"] = truth["w1"][idx].err(got["w"]).max() if k1 else np.abs(got["w"] - 1.0).max()
    if "rho" in got:
        rho = truth["rho1"] if k1 else truth["s"]
        out["rho"] = (rho[idx].err(got["rho"]) / np.maximum(1.0, rho.hi[idx])).max()
    return {k: float(v) for k, v in out.items()}, negated


def truth_sums(truth):
    """chi2 and the Huber cost at huber_k1 of the planted graph: the 50-digit sums (any edge order: they are exact to 1e-30)"""
    return {k: math.fsum(truth[k].hi) + math.fsum(truth[k].lo) for k in ("s", "rho1")}


@functools.lru_cache(maxsize=None)
def huber_of(layout):
    """the Huber threshold of a graph: inliers and outliers of every kind (planted: on the truth's s; embedded: on the mirror's)"""
    if layout == "planted":
        return planted_truth()["huber_k1"]
    c = canonical(layout)
    return huber_k1(ref.edge_s(c["g"], c["g"].poses), c["kind"])


# ---------------------------------------------------------------- the optimizer: a false loop that claims a half turn
HALF_TURNS = {"x": np.diag([1.0, -1.0, -1.0]), "y": np.diag([-1.0, 1.0, -1.0])}
HALF_TURN_NODES = {"x": (1, 15), "y": (1, 15)}  # the widest margins of half_turn_search(): see __main__
HALF_TURN_CLEAR = 1e-6  # no F_new / F of the mirror's five solves is closer to 1 (today's false loop: 1.6e-6; the device agrees to 1e-9)


def half_turn_ring(axis, nodes=None):
    """posegraph_cases.ring(false_loop=True) with the false edge between `nodes` claiming a half turn about the axis (and no
    translation): between nodes whose yaw differs by less than 90 degrees R_E is the half turn times a small rotation, so the
    axis's own diagonal entry leads and w is a small number of either sign"""
    g, truth = cases.ring(false_loop=True)
    a, b = HALF_TURN_NODES[axis] if nodes is None else nodes
    g.i[-1], g.j[-1] = a, b
    g.Z[-1] = np.eye(4)
    g.Z[-1, :3, :3] = HALF_TURNS[axis]
    return g, truth


def half_turn_conditions(axis, nodes=None):
    """the mirror's run under posegraph_cases.FALSE_CFG -> dict(g, the false edge's kind at the start and at the end, accepted, ratio,
    clear: no F_new / F within HALF_TURN_CLEAR of 1, n_outliers and the false edge's weight at the end, poses, res)"""
    g, _ = half_turn_ring(axis, nodes)

    def false_kind(poses):
        RE = g.Z[-1, :3, :3].T @ (poses[g.i[-1], :3, :3].T @ poses[g.j[-1], :3, :3])
        return int(kind_of(RE))

    start_kind = false_kind(g.poses)
    poses, res = ref.optimize(g, **cases.FALSE_CFG)
    ratio = np.array([t["ratio"] for t in res["trace"]])
    lin = ref.linearize(g, poses, cases.FALSE_CFG["huber_k"])
    return dict(g=g, start_kind=start_kind, end_kind=false_kind(poses), accepted=[t["accepted"] for t in res["trace"]], ratio=ratio,
                clear=bool((np.abs(ratio - 1.0) > HALF_TURN_CLEAR).all()), n_outliers=lin["n_outliers"], w_false=float(lin["w"][-1]), poses=poses,
                res=res)


def half_turn_search(axis):
    """every third node with a partner up to 14 steps (79 degrees of heading) on"""
    for a in range(1, cases.RING_N - 2, 3):
        for gap in (2, 3, 5, 8, 11, 14):
            b = a + gap
            if b >= cases.RING_N:
                continue
            c = half_turn_conditions(axis, (a, b))
            yield (a, b), c


# ---------------------------------------------------------------- loop sets
LOOP_SIZES = (65, 130)  # more than one 64-bit word per row
LOOP_NODES = 8
LOOP_ENDS = (2, 6)


def _loop_sequence(count, half_turns=True):
    """the family round-robin over the kinds, then the exact set (without its half turns if not half_turns), repeated"""
    by_kind, exact = family()
    seq = [by_kind[k][m] for m in range(PER_KIND) for k in range(NK)] + [m for m in exact if half_turns or abs(m.angle - math.pi) > 1e-3]
    return [seq[q % len(seq)] for q in range(count)]


SIGN_CLEAR = 1e-13  # an embedded R_E whose raw quaternion w is smaller hangs its sign, and so Log's, on the rounding of a product


def raw_w(R):
    """the quaternion's w of R [..., 3, 3] before the flip to w >= 0"""
    R = np.asarray(R, dtype=np.float64)
    q = ref.quat(R)
    flipped = kind_of(R) % 2 == 0
    return np.where(flipped & (kind_of(R) > 0), -q[..., 0], q[..., 0])


def pose_of(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _pair_RE(c):
    """R_E [P, 3, 3] of the pairs k < l as the mirror forms it (loops_ref.pair_e), in np.triu_indices order"""
    L = len(c["a"])
    k, l = np.triu_indices(L, 1)
    P, a, b, Z = c["poses"], c["a"], c["b"], c["Z"]
    Zh = lref.predicted(P[a[k]], P[b[k]], P[a[l]], P[b[l]], Z[l])
    return np.swapaxes(Z[k][:, :3, :3], 1, 2) @ Zh[:, :3, :3]


def _finish_loops(c, cov):
    """the mirror's s, a gamma that halves the pairs with none of them in the band, the adjacency and the pair kinds; None if a pair is
    in the band"""
    if cov:
        s, bound, delta = ccases._mirror(c["poses"], c["a"], c["b"], c["Z"], c["Sigma"], c["Q"])
        if not np.isfinite(s).all() or bound != ccases.S_FLOOR:  # (the two float64 mirrors agree to 1e-10: the contract's 1e-9 holds)
            return None
    else:
        s = lref.pair_s(c["poses"], c["a"], c["b"], c["Z"], c["var_t"], c["var_r"], c["q_t"], c["q_r"])
    gamma = lcases.median_gamma(s)
    if lcases.in_band(s, gamma) != 0:
        return None
    L = len(c["a"])
    kinds = np.full((L, L), -1, np.int64)
    k, l = np.triu_indices(L, 1)
    kinds[k, l] = kinds[l, k] = kind_of(_pair_RE(c))
    c.update(s=s, gamma=gamma, adj=lref.adjacency(s, gamma), pair_kind=kinds)
    return c


def _loop_noise(rng, L, cov):
    if cov:
        return dict(Sigma=ccases.SIGMA_SCALE * 100.0 * cases.rand_info(rng, L), q_t=0.0, q_r=0.0)
    return dict(var_t=10.0 ** rng.uniform(-1.0, 1.0, L), var_r=10.0 ** rng.uniform(-1.0, 1.0, L), q_t=0.01, q_r=0.005)


@functools.lru_cache(maxsize=None)
def planted_loops(L, order="round_robin", cov=False):
    """Poses that are pure dyadic translations and loops that all join LOOP_ENDS: Zhat_kl is Z_l bit for bit and m = 0, so the pair
    (k, l) has R_E = R_k^T R_l.  "round_robin": loop 0 has the identity rotation and loops 1 .. the family's, kinds in turn, so row 0
    meets every kind exactly and the other rows mix them.  "runs" (L = 130): loops 0 .. NK - 1 carry the transposes of one member per
    kind and loops 64 .. 127 the identity, so the wavefront (row k, word 1) holds 64 pairs of kind k, each R_E that member bit for bit.
    cov=True adds Sigma [L, 6, 6] and Q for the covariance model (Q is never used: no odometry lies between the loops' ends).
    -> dict(poses, a, b, Z, rot: the Member of each loop, None for the identity, ("transpose", Member) for the "runs" rows, var_t,
    var_r | Sigma, Q, q_t, q_r, gamma, s, adj, pair_kind, seed)"""
    assert order in ORDERS and (order == "round_robin" or L == 130)
    by_kind, _ = family()
    for seed in range(3300 + L, 3300 + L + 50):
        rng = np.random.default_rng(seed)
        poses = np.stack([pose_of(np.eye(3), np.array([0.5 * v, 0.25 * v, -0.125 * v])) for v in range(LOOP_NODES)])
        a, b = np.full(L, LOOP_ENDS[0], np.int32), np.full(L, LOOP_ENDS[1], np.int32)
        if order == "round_robin":
            rot = [None] + _loop_sequence(L - 1)
            R = [np.eye(3)] + [m.R for m in rot[1:]]
        else:
            heads = [by_kind[k][3 + k % 4] for k in range(NK)]  # one member per kind; loop k carries its transpose
            seq = _loop_sequence(L)
            rot = [seq[q] if not (64 <= q < 128) else None for q in range(L)]
            R = [np.eye(3) if m is None else m.R for m in rot]
            for k in range(NK):
                rot[k], R[k] = ("transpose", heads[k]), np.ascontiguousarray(heads[k].R.T)
        base = poses[LOOP_ENDS[1], :3, 3] - poses[LOOP_ENDS[0], :3, 3]
        Z = np.stack([pose_of(R[q], base + rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-1.5, 0.5)) for q in range(L)])
        c = dict(poses=poses, a=a, b=b, Z=Z, rot=rot, Q=ccases.HONEST_Q, seed=seed, order=order, **_loop_noise(rng, L, cov))
        if _finish_loops(c, cov) is not None:
            RE = _pair_RE(c)
            k, l = np.triu_indices(L, 1)
            first = k == 0
            if order == "round_robin":  # row 0: R_E is the column's own matrix
                assert all(np.array_equal(RE[first][q], Z[q + 1, :3, :3]) for q in range(L - 1))
            else:
                for kk in range(NK):
                    sel = (k == kk) & (l >= 64) & (l < 128)
                    assert sel.sum() == 64 and all(np.array_equal(M, heads[kk].R) for M in RE[sel])
                    assert (c["pair_kind"][kk, 64:128] == kk).all()
            return c
    raise AssertionError("no draw without a pair in the band")


@functools.lru_cache(maxsize=None)
def embedded_loops(L, cov=False):
    """The family's rotations as measurement noise on the random chain of loops_cases with distinct end nodes:
    Z_l = T_a^-1 T_b [Exp(phi_l) | small t], loop 0 without noise.  The half turns of the exact set are left out: against loop 0 such a
    loop's R_E is a half turn conjugated by the odometry, whose raw w is a rounding residue of either sign (as in the embedded graph);
    every pair that is left has |w| >= SIGN_CLEAR."""
    for seed in range(4400 + L, 4400 + L + 50):
        rng = np.random.default_rng(seed)
        poses, a, b, _ = lcases._random_loops(L, seed)
        rot = [None] + _loop_sequence(L - 1, half_turns=False)
        Z = []
        for q in range(L):
            noise = pose_of(np.eye(3) if rot[q] is None else rot[q].R, rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(-1.5, 0.5))
            Z.append(cases.inv_pose(poses[a[q]]) @ poses[b[q]] @ noise)
        c = dict(poses=poses, a=a, b=b, Z=np.stack(Z), rot=rot, Q=ccases.Q_SCALE * cases.rand_info(np.random.default_rng(seed + 7000), lcases.CHAIN_N - 1),
                 seed=seed, order="round_robin", **_loop_noise(rng, L, cov))
        if _finish_loops(c, cov) is not None and np.abs(raw_w(_pair_RE(c))).min() >= SIGN_CLEAR:
            return c
    raise AssertionError("no draw without a pair in the band")


def loop_wavefront_kinds(c):
    """the distinct kinds among the valid lanes of every wavefront (row, word) of the adjacency kernels -> list of (row, word, valid
    lanes, distinct kinds)"""
    L = len(c["a"])
    out = []
    for row in range(L):
        for w in range((L + 63) // 64):
            cols = [q for q in range(64 * w, min(64 * w + 64, L)) if q != row]
            out.append((row, w, len(cols), len({int(c["pair_kind"][row, q]) for q in cols})))
    return out


@functools.lru_cache(maxsize=None)
def _planted_pair_e(L, order, cov):
    """e of the planted pairs at 50 digits as mpf rows, and either_sign per pair"""
    c = planted_loops(L, order, cov)
    k, l = np.triu_indices(L, 1)
    E, either = [], []
    with mp.workdps(DPS):
        Rm = [_mpm(Z[:3, :3]) for Z in c["Z"]]
        tm = [_mpv(Z[:3, 3]) for Z in c["Z"]]
        for kk, ll in zip(k.tolist(), l.tolist()):
            et = _mv(_tr(Rm[kk]), [y - x for x, y in zip(tm[kk], tm[ll])])
            exact_member = None
            if order == "round_robin" and kk == 0:
                exact_member = c["rot"][ll]
            elif order == "runs" and kk < NK and 64 <= ll < 128:
                exact_member = c["rot"][kk][1]
            if exact_member is not None and not exact_member.exact:
                phi, either_sign = exact_member.phi, exact_member.either_sign
            else:
                phi, either_sign = mp_log(_mul(_tr(Rm[kk]), Rm[ll]))[0], False
            E.append(et + list(phi))
            either.append(either_sign)
    return E, np.array(either)


def _mp_ldl_form(M, e):
    """e^T M^-1 e for a symmetric positive definite M (6 x 6 of mpf) by L D L^T at the working precision"""
    Lm = [[None] * 6 for _ in range(6)]
    d, y, s = [None] * 6, [None] * 6, mpf(0)
    for j in range(6):
        dj = M[j][j] - sum((Lm[j][p] * Lm[j][p] * d[p] for p in range(j)), mpf(0))
        d[j] = dj
        for i in range(j + 1, 6):
            Lm[i][j] = (M[j][i] - sum((Lm[i][p] * Lm[j][p] * d[p] for p in range(j)), mpf(0))) / dj
        y[j] = e[j] - sum((Lm[j][p] * y[p] for p in range(j)), mpf(0))
        s += y[j] * y[j] / dj
    return s


@functools.lru_cache(maxsize=None)
def planted_loops_truth(L, order="round_robin", cov=False):
    """e [P, 6] and s [P] of the planted pairs k < l (np.triu_indices order) at 50 digits -> dict of DD.  e = [R_k^T (t_l - t_k);
    Log(R_k^T R_l)] by the closed form on the float64 inputs (mp_log: exact comparisons, so at a half turn the sign is the contract's),
    except that for a bit-exact R_E (row 0, and the "runs" rows' word 1) the rotation part is the member's phi itself;
    s = |e_t|^2 / (var_t,k + var_t,l) + |e_r|^2 / (var_r,k + var_r,l), or e^T (Sigma_k + Sigma_l)^-1 e under the covariance model."""
    c = planted_loops(L, order, cov)
    # (Z is drawn before the noise model: with the same seed the scalar set and the one with covariances share their loops and so e)
    E, either = _planted_pair_e(L, order, cov and planted_loops(L, order)["seed"] != c["seed"])
    k, l = np.triu_indices(L, 1)
    S = []
    with mp.workdps(DPS):
        if cov:
            Sg = [[[mpf(float(x)) for x in row] for row in M] for M in c["Sigma"]]
        else:
            vt, vr = _mpv(c["var_t"]), _mpv(c["var_r"])
        for p, (kk, ll) in enumerate(zip(k.tolist(), l.tolist())):
            e = E[p]
            if cov:
                S.append(_mp_ldl_form([[Sg[kk][i][j] + Sg[ll][i][j] for j in range(6)] for i in range(6)], e))
            else:
                S.append((e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) / (vt[kk] + vt[ll]) + (e[3] * e[3] + e[4] * e[4] + e[5] * e[5]) / (vr[kk] + vr[ll]))
    return dict(e=DD(E), s=DD(S), either_sign=either, k=k, l=l)


def pair_e_error(got_e, truth):
    """per pair the worst |e - truth|, the rotation part against phi or -phi (whichever is nearer) where either_sign"""
    t = truth["e"].err(got_e)
    flipped = got_e.copy()
    flipped[:, 3:] = -flipped[:, 3:]
    tn = truth["e"].err(flipped)
    return np.where(truth["either_sign"], np.minimum(t.max(1), tn.max(1)), t.max(1))


GRAPH_SETS = [(layout, order) for layout in LAYOUTS for order in ORDERS]
LOOP_SETS = [("planted", 65, "round_robin"), ("planted", 130, "round_robin"), ("planted", 130, "runs"), ("embedded", 65, "round_robin"),
             ("embedded", 130, "round_robin")]


def loop_set(layout, L, order, cov=False):
    return planted_loops(L, order, cov) if layout == "planted" else embedded_loops(L, cov)


def loop_census(c):
    k, l = np.triu_indices(len(c["a"]), 1)
    return census(c["pair_kind"][k, l])


def census_report():
    """one line per consumer set: how many edges or pairs take each kind"""
    lines = ["kinds: " + ", ".join(KINDS)]
    for layout in LAYOUTS:
        c = canonical(layout)
        lines.append(f"graph {layout} (E = {c['g'].E}, both orders): {census(c['kind']).tolist()}")
    for cov in (False, True):
        for layout, L, order in LOOP_SETS:
            c = loop_set(layout, L, order, cov)
            lines.append(f"loops {layout} L = {L} {order}{' with covariances' if cov else ''} (seed {c['seed']}, gamma {c['gamma']:.4g}): "
                         f"{loop_census(c).tolist()}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(census_report())
    t = planted_truth()
    print("huber k1", t["huber_k1"])
    for axis in HALF_TURNS:
        for nodes, c in half_turn_search(axis):
            print(f"half turn about {axis} between {nodes}: start {KINDS[c['start_kind']]}, end {KINDS[c['end_kind']]}, accepted {c['accepted']}, "
                  f"|ratio - 1| >= {float(np.abs(c['ratio'] - 1.0).min()):.2e}, outliers {c['n_outliers']}, w_false {c['w_false']:.3f}")
