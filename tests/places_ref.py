"""The numpy mirror of the place-recognition contract (include/elimaloc_hip.h, "place recognition"): the descriptor
of a scan from the three float64 tables (the directions are the library's own bytes, the ring and layer edges are re-derived here), the
integer match of two descriptors at all 64 shifts, and the selection.  The sector rule is evaluated for all 64 sectors, as the contract
words it."""
import numpy as np

SECTORS = 64
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
MATCH_DTYPE = np.dtype([("dice_q16", np.uint32), ("inter", np.uint16), ("shift", np.uint16)])


class Cfg:
    def __init__(self, n_rings=16, n_layers=8, r_min_m=2.0, r_max_m=42.0, z_min_m=-3.0, z_max_m=9.0):
        self.n_rings, self.n_layers = int(n_rings), int(n_layers)
        self.r_min_m, self.r_max_m, self.z_min_m, self.z_max_m = float(r_min_m), float(r_max_m), float(z_min_m), float(z_max_m)

    @property
    def n_words(self):
        return self.n_rings * self.n_layers


def edges(lo, hi, n):
    """e_i = lo + ((hi - lo) * i) / n for i = 0 .. n, e_n = hi exactly (float64)"""
    e = np.array([np.float64(lo) + ((np.float64(hi) - np.float64(lo)) * np.float64(i)) / np.float64(n) for i in range(n + 1)])
    e[n] = hi
    return e


def edge_tables(cfg):
    e = edges(cfg.r_min_m, cfg.r_max_m, cfg.n_rings)
    return e * e, edges(cfg.z_min_m, cfg.z_max_m, cfg.n_layers)


def level(points, T_level=None):
    """the float32 points widened and levelled: q_r = ((R_r0 x + R_r1 y) + R_r2 z) + t_r"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    T = np.eye(4) if T_level is None else np.asarray(T_level, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):  # (0 * inf of a scan's own non-finite points)
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def bins(points, cfg, dirs, T_level=None):
    """(ring, layer, sector) per point, -1 where the point has none"""
    re, ze = edge_tables(cfg)
    q = level(points, T_level)
    with np.errstate(invalid="ignore"):
        r2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
        ring = np.full(len(q), -1)
        for i in range(cfg.n_rings):
            ring[(re[i] <= r2) & (r2 < re[i + 1])] = i
        layer = np.full(len(q), -1)
        for j in range(cfg.n_layers):
            layer[(ze[j] <= q[:, 2]) & (q[:, 2] < ze[j + 1])] = j
        cr = dirs[None, :, 0] * q[:, 1:2] - dirs[None, :, 1] * q[:, 0:1]  # [n, 64]
        ok = (cr >= 0.0) & (np.roll(cr, -1, axis=1) < 0.0)
    sector = np.where(ok.any(axis=1), ok.argmax(axis=1), -1)  # the smallest k
    return ring, layer, sector, ok.sum(axis=1)


def describe(points, cfg, dirs, T_level=None):
    """-> (words uint64 [W], dict(n_points, n_used, n_bits))"""
    ring, layer, sector, _ = bins(points, cfg, dirs, T_level)
    used = (ring >= 0) & (layer >= 0) & (sector >= 0)
    words = np.zeros(cfg.n_words, np.uint64)
    np.bitwise_or.at(words, ring[used] * cfg.n_layers + layer[used], np.uint64(1) << sector[used].astype(np.uint64))
    return words, dict(n_points=int(len(ring)), n_used=int(used.sum()), n_bits=popcount(words))


def to_bits(words):
    """uint64 [..., W] -> uint8 [..., W, 64], bit s of a word at [..., s]"""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1, bitorder="little").reshape(w.shape + (64,))


def popcount(words):
    return int(to_bits(words).sum())


def rotl(words, k):
    w = np.asarray(words, dtype=np.uint64)
    k = int(k) & 63
    return w.copy() if k == 0 else ((w << np.uint64(k)) & M64) | (w >> np.uint64(64 - k))


def inter_table(a, b):
    """inter(k) for k = 0 .. 63 of two descriptors, straight from the definition"""
    return np.array([popcount(np.asarray(a, np.uint64) & rotl(b, k)) for k in range(SECTORS)], dtype=np.int64)


def dice_q16(inter, na, nb):
    den = int(na) + int(nb)
    return (int(inter) << 17) // den if den else 0


def yaw_of_shift(k):
    k = int(k)
    return -(2.0 * np.pi * float(k)) / 64.0 if k < 32 else (2.0 * np.pi * float(64 - k)) / 64.0


def match_all(qwords, dwords):
    """every (query, entry) pair -> MATCH_DTYPE [Q, N].  rotl by k moves bit s - k to bit s, so inter(k) = sum_w sum_s a[w, s] b[w, s - k]:
    one exact float32 product of the bit matrices per shift (the counts stay below 2^24)."""
    qwords = np.asarray(qwords, np.uint64).reshape(len(qwords), -1)
    dwords = np.asarray(dwords, np.uint64).reshape(len(dwords), -1)
    Q, N = len(qwords), len(dwords)
    out = np.zeros((Q, N), MATCH_DTYPE)
    if not Q or not N:
        return out
    A = to_bits(qwords).astype(np.float32).reshape(Q, -1)
    B = to_bits(dwords)
    inter = np.zeros((SECTORS, Q, N), np.int64)
    for k in range(SECTORS):
        inter[k] = np.rint(A @ np.roll(B, k, axis=-1).astype(np.float32).reshape(N, -1).T).astype(np.int64)
    best = inter.max(axis=0)
    shift = inter.argmax(axis=0)  # the smallest k of the largest
    na, nb = A.sum(axis=1).astype(np.int64), B.reshape(N, -1).sum(axis=1).astype(np.int64)
    den = na[:, None] + nb[None, :]
    out["dice_q16"] = np.where(den > 0, (best << 17) // np.maximum(den, 1), 0)
    out["inter"] = best
    out["shift"] = shift
    return out


def select(row, ids, top_k, min_dice_q16=0, exclude=None):
    """the selection of one query from its row of matches -> candidate dicts in rank order (a stable argsort by dice descending)"""
    ids = np.asarray(ids, np.int64)
    keep = row["dice_q16"] >= min_dice_q16
    if exclude is not None and exclude[0] <= exclude[1]:
        keep &= ~((ids >= exclude[0]) & (ids <= exclude[1]))
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(-row["dice_q16"][idx].astype(np.int64), kind="stable")][:top_k]
    return [dict(entry=int(e), dice_q16=int(row["dice_q16"][e]), id=int(ids[e]), inter=int(row["inter"][e]), shift=int(row["shift"][e]),
                 yaw_rad=yaw_of_shift(row["shift"][e])) for e in idx]
