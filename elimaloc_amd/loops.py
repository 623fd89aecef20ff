"""Loop closing: the largest set of mutually consistent loop measurements (include/elimaloc_hip_loops.h).  Every
pair of loops and the odometry between their ends form a cycle that must compose to the identity; the pairs are tested on the GPU, the
consistent ones form a graph, and a deterministic greedy clique over it is kept.  It runs before the solver and touches none of it.
The calls ending in Cov (include/elimaloc_hip_loopcov.h) test the pairs by a Mahalanobis distance under the 6 x 6
covariance of the odometry propagated along the chain, in place of the scalar random walk."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ElmError, LoopCovResultC, LoopsConfigC, LoopsResultC, check
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


def _cov_block(M, count, what):
    """one 6 x 6 for all or one per item -> a contiguous [count, 6, 6] float64 block"""
    M = np.asarray(M, dtype=np.float64)
    if M.shape == (6, 6):
        M = np.broadcast_to(M, (count, 6, 6))
    if M.shape != (count, 6, 6):
        raise ElmError(f"{what}: a 6 x 6 or [{count}, 6, 6]")
    return np.ascontiguousarray(M)


def _odom_block(Q, n, what):
    """Q as the C calls take it: one 6 x 6, or one per step [n - 1, 6, 6] -> (block, q_count)"""
    Q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64))
    if Q.shape == (6, 6):
        return Q.reshape(1, 6, 6), 1
    if Q.ndim != 3 or Q.shape[1:] != (6, 6):
        raise ElmError(f"{what}: Q is a 6 x 6 or [n - 1, 6, 6]")
    return Q, Q.shape[0]


def ChainCovariance(poses, Q, ctx=None, local=False):
    """W [n, 6, 6]: the covariance of the odometry from pose 0 to every pose of the chain, in the frame of pose 0, from the covariance Q of
    one step (6 x 6, or [n - 1, 6, 6]); the odometry between u and v has W[max(u, v)] - W[min(u, v)].  local=True -> (W, S) with S[v] the
    covariance of T_v relative to T_0 in v's own tangent, which is what sizes a loop search."""
    ctx = ctx if ctx is not None else default_context()
    P = _pose_block(poses)
    n = P.size // 16
    Qb, q_count = _odom_block(Q, n, "ChainCovariance")
    W = np.zeros((max(n, 1), 6, 6))
    S = np.zeros((max(n, 1), 6, 6)) if local else None
    check(_lib.lib().elm_loopcov_chain(ctx._h, _dp(P) if P.size else None, n, _dp(Qb) if Qb.size else None, q_count, _dp(W), _ptr(S)), ctx._h,
          "elm_loopcov_chain")
    return (W[:n], S[:n]) if local else W[:n]


def PairTermsCov(T0, Ta, Tb, Zk, cov_k, Tc, Td, Zl, cov_l, Ca, Cb):
    """(e [6], cov [6, 6], s) of one pair under the covariance model: loop k = (Ta, Tb, Zk, cov_k) predicted from loop l = (Tc, Td, Zl,
    cov_l) through the odometry of a chain whose pose 0 is T0, Ca and Cb being the odometry's covariance between the loops' first and
    second ends (differences of ChainCovariance's W).  Host only, the code the kernel runs; s is NaN when a pivot fails."""
    e, cov, s = np.zeros(6), np.zeros((6, 6)), np.zeros(1)
    mat = lambda M: _dp(np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(6, 6)))
    pose = lambda T: _dp(_pose_block(T))
    check(_lib.lib().elm_loopcov_pair_terms(pose(T0), pose(Ta), pose(Tb), pose(Zk), mat(cov_k), pose(Tc), pose(Td), pose(Zl), mat(cov_l), mat(Ca),
                                            mat(Cb), _dp(e), _dp(cov), _dp(s)), None, "elm_loopcov_pair_terms")
    return e, cov, float(s[0])


def LoopConsistencyCov(poses, a, b, Z, cov, Q, cfg=None, ctx=None, adjacency=False, s=False):
    """LoopConsistency under the covariance model: cov [L, 6, 6] (or one 6 x 6 for all) is each loop's covariance in the order
    [translation; rotation], Q the covariance of one odometry step (6 x 6, or [n - 1, 6, 6]); cfg gives gamma and steps_per_batch and
    leaves q_t = q_r = 0.  -> LoopConsistency's dict plus non_finite_pairs (the pairs whose s is NaN) and chain_ms."""
    ctx = ctx if ctx is not None else default_context()
    cfg = cfg if cfg is not None else LoopConsistencyConfig()
    P = _pose_block(poses)
    n = P.size // 16
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.int32).reshape(-1))
    L = a.size
    Zb = _pose_block(Z) if L else np.zeros(0)
    if b.size != L or Zb.size != 16 * L:
        raise ElmError("LoopConsistencyCov: one b and Z per loop")
    Sb = _cov_block(cov, L, "LoopConsistencyCov: cov") if L else np.zeros(0)
    Qb, q_count = _odom_block(Q, n, "LoopConsistencyCov")
    W = (L + 63) // 64
    res = LoopCovResultC()
    mask, degree = np.zeros(max(L, 1), np.uint8), np.zeros(max(L, 1), np.int32)
    adj = np.zeros((max(L, 1), max(W, 1)), np.uint64) if adjacency else None
    sm = np.zeros((max(L, 1), max(L, 1))) if s else None
    some = lambda x: _ptr(x) if L else None
    check(_lib.lib().elm_loopcov_consistency(ctx._h, _dp(P) if P.size else None, n, some(a), some(b), _dp(Zb) if L else None, _dp(Sb) if L else None,
                                             L, _dp(Qb) if Qb.size else None, q_count, C.byref(cfg), C.byref(res), _ptr(mask), _ptr(degree),
                                             _ptr(adj), _ptr(sm)),
          ctx._h, "elm_loopcov_consistency")
    mask = mask[:L] != 0
    out = dict(members=np.flatnonzero(mask), mask=mask, size=int(res.size), adjacent_pairs=int(res.adjacent_pairs), steps=int(res.steps),
               degree=degree[:L].copy(), adjacency_ms=float(res.adjacency_ms), greedy_ms=float(res.greedy_ms),
               non_finite_pairs=int(res.non_finite_pairs), chain_ms=float(res.chain_ms))
    if adjacency:
        out["adjacency"] = adj[:L, :W]
    if s:
        out["s"] = sm[:L, :L]
    return out
