"""Loop closing: the largest set of mutually consistent loop measurements (include/elimaloc_hip_loops.h).  Every
pair of loops and the odometry between their ends form a cycle that must compose to the identity; the pairs are tested on the GPU, the
consistent ones form a graph, and a deterministic greedy clique over it is kept.  It runs before the solver and touches none of it."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ElmError, LoopsConfigC, LoopsResultC, check
from ._marshal import _config, _dp, _pose_block, _ptr
from .context import default_context


def LoopConsistencyConfig(**kw):
    """elm_loops_config with its defaults (q_t = q_r = 0, gamma = 16.81: the 99 % point of chi^2 with 6 degrees of freedom,
    steps_per_batch = 32)."""
    return _config("LoopConsistencyConfig", LoopsConfigC, "elm_loops_config_default", kw)


def PairTerms(Ta, Tb, Zk, Tc, Td, Zl):
    """e [6] of one pair: loop k = (Ta, Tb, Zk) predicted from loop l = (Tc, Td, Zl) through the odometry, the pose graph's residual of
    that prediction against Zk (host only, the code the kernel runs)."""
    e = np.zeros(6)
    check(_lib.lib().elm_loops_pair_terms(*[_dp(_pose_block(T)) for T in (Ta, Tb, Zk, Tc, Td, Zl)], _dp(e)), None, "elm_loops_pair_terms")
    return e


def LoopConsistency(poses, a, b, Z, var_t, var_r, cfg=None, ctx=None, adjacency=False, s=False):
    """poses [n, 4, 4] (a chain in index order), loops (a[k], b[k], Z[k] ~ T_a^-1 T_b) with the variances var_t[k] (m^2) and var_r[k]
    (rad^2), each one number for all or one per loop -> dict(members: the clique's loop indices ascending, mask [L] bool, size,
    adjacent_pairs, steps, degree [L]: every loop's consistent partners, adjacency_ms, greedy_ms: the device time of the two parts);
    adjacency=True adds adjacency [L, ceil(L / 64)] uint64 (bit l & 63 of word l >> 6), s=True adds s [L, L] (L <= 2 048)."""
    ctx = ctx if ctx is not None else default_context()
    cfg = cfg if cfg is not None else LoopConsistencyConfig()
    P = _pose_block(poses)
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.int32).reshape(-1))
    L = a.size
    Zb = _pose_block(Z) if L else np.zeros(0)
    vt = np.ascontiguousarray(np.broadcast_to(np.asarray(var_t, dtype=np.float64), (L,)))
    vr = np.ascontiguousarray(np.broadcast_to(np.asarray(var_r, dtype=np.float64), (L,)))
    if b.size != L or Zb.size != 16 * L:
        raise ElmError("LoopConsistency: one b and Z per loop")
    W = (L + 63) // 64
    res = LoopsResultC()
    mask, degree = np.zeros(max(L, 1), np.uint8), np.zeros(max(L, 1), np.int32)
    adj = np.zeros((max(L, 1), max(W, 1)), np.uint64) if adjacency else None
    sm = np.zeros((max(L, 1), max(L, 1))) if s else None
    some = lambda x: _ptr(x) if L else None
    check(_lib.lib().elm_loops_consistency(ctx._h, _dp(P) if P.size else None, P.size // 16, some(a), some(b), _dp(Zb) if L else None, some(vt),
                                           some(vr), L, C.byref(cfg), C.byref(res), _ptr(mask), _ptr(degree), _ptr(adj), _ptr(sm)),
          ctx._h, "elm_loops_consistency")
    mask = mask[:L] != 0
    out = dict(members=np.flatnonzero(mask), mask=mask, size=int(res.size), adjacent_pairs=int(res.adjacent_pairs), steps=int(res.steps),
               degree=degree[:L].copy(), adjacency_ms=float(res.adjacency_ms), greedy_ms=float(res.greedy_ms))
    if adjacency:
        out["adjacency"] = adj[:L, :W]
    if s:
        out["s"] = sm[:L, :L]
    return out
