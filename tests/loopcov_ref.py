"""Numpy mirror of the loop consistency check with a propagated covariance (include/elimaloc_hip_loopcov.h), written
from the header on loops_ref / posegraph_ref: the chain covariance W by a sequential cumsum, by a pairwise tree and in np.longdouble, the
plain-form pair term with its L D L^T in index order, the one-sandwich form, the direct propagation W is held against, and refusal()."""
import numpy as np

import loops_ref as lref

ORDERS = ("sequential", "pairwise", "longdouble")


def _T(a):
    return np.swapaxes(a, -1, -2)


def hat(v, dtype=np.float64):
    v = np.asarray(v, dtype=dtype)
    out = np.zeros(v.shape[:-1] + (3, 3), dtype=dtype)
    out[..., 0, 1], out[..., 0, 2] = -v[..., 2], v[..., 1]
    out[..., 1, 0], out[..., 1, 2] = v[..., 2], -v[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -v[..., 1], v[..., 0]
    return out


def adjoint(X, dtype=np.float64):
    """Ad(X) = [[R, [t]x R], [0, R]] for X [..., 4, 4]"""
    X = np.asarray(X, dtype=dtype)
    R = X[..., :3, :3]
    out = np.zeros(X.shape[:-2] + (6, 6), dtype=dtype)
    out[..., :3, :3] = R
    out[..., :3, 3:] = hat(X[..., :3, 3], dtype) @ R
    out[..., 3:, 3:] = R
    return out


def inverse(X, dtype=np.float64):
    X = np.asarray(X, dtype=dtype)
    out = np.zeros(X.shape, dtype=dtype)
    Rt = _T(X[..., :3, :3])
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ X[..., :3, 3][..., None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def sandwich(G, S):
    return G @ S @ _T(G)


def mirrored(M):
    """the upper triangle standing for both: exactly symmetric"""
    up = np.triu(M)
    return up + _T(np.triu(M, 1))


def rebased(poses, dtype=np.float64):
    """Y_v = T_0^-1 T_v"""
    poses = np.asarray(poses, dtype=dtype).reshape(-1, 4, 4)
    return lref.between(poses[:1], poses, dtype)


def step_terms(poses, Q, dtype=np.float64):
    """P [n - 1, 6, 6]: P_v = Ad(Y_{v+1}) Q_v Ad(Y_{v+1})^T, exactly symmetric"""
    Y = rebased(poses, dtype)
    n = Y.shape[0]
    Q = np.asarray(Q, dtype=dtype)
    Q = np.broadcast_to(Q.reshape(-1, 6, 6), (max(n - 1, 0), 6, 6)) if Q.size == 36 else Q.reshape(n - 1, 6, 6)
    return mirrored(sandwich(adjoint(Y[1:], dtype), Q))


def _pairwise_prefix(x):
    """inclusive prefix sums along axis 0 by a pairwise tree"""
    n = x.shape[0]
    if n == 1:
        return x.copy()
    m = n // 2
    p = _pairwise_prefix(x[0:2 * m:2] + x[1:2 * m:2])
    out = np.empty_like(x)
    out[0] = x[0]
    out[1:2 * m:2] = p
    out[2:n:2] = p[:(n - 1) // 2] + x[2:n:2]
    return out


def chain_W(poses, Q, order="sequential"):
    """W [n, 6, 6]: W_0 = 0, W_v = sum_{u < v} P_u.  order: "sequential" (np.cumsum), "pairwise" (a tree), "longdouble" (everything,
    the terms included, in np.longdouble)"""
    dtype = np.longdouble if order == "longdouble" else np.float64
    P = step_terms(poses, Q, dtype)
    n = P.shape[0] + 1
    W = np.zeros((n, 6, 6), dtype=dtype)
    if n > 1:
        W[1:] = _pairwise_prefix(P) if order == "pairwise" else np.cumsum(P, axis=0)
    return W


def chain_S(poses, W):
    """S_v = Ad(Y_v^-1) W_v Ad(Y_v^-1)^T"""
    dtype = W.dtype
    return mirrored(sandwich(adjoint(inverse(rebased(poses, dtype), dtype), dtype), W))


def direct_range(poses, Q, u, v):
    """The covariance of the odometry from u to v > u by propagating pose by pose in np.longdouble, S <- Ad(X^-1) S Ad(X^-1)^T + Q with
    X the step, then moved into the frame of pose 0: what W_v - W_u is held against."""
    ld = np.longdouble
    poses = np.asarray(poses, dtype=ld).reshape(-1, 4, 4)
    Q = np.asarray(Q, dtype=ld)
    Q = np.broadcast_to(Q.reshape(-1, 6, 6), (poses.shape[0] - 1, 6, 6)) if Q.size == 36 else Q.reshape(-1, 6, 6)
    S = np.zeros((6, 6), dtype=ld)
    for w in range(u, v):
        G = adjoint(inverse(lref.between(poses[w], poses[w + 1], ld), ld), ld)
        S = sandwich(G, S) + Q[w]
    return sandwich(adjoint(rebased(poses, ld)[v], ld), S)


def ldl_form(A, e):
    """e^T A^-1 e by an L D L^T of A [..., 6, 6] without pivoting in index order (the upper triangle is read); NaN where a pivot is not
    finite or not > 0"""
    A, e = np.asarray(A, dtype=np.float64), np.asarray(e, dtype=np.float64)
    shape = np.broadcast(A[..., 0, 0], e[..., 0]).shape
    Lm = [[None] * 6 for _ in range(6)]
    d, y = [None] * 6, [None] * 6
    ok = np.ones(shape, bool)
    s = np.zeros(shape)
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[..., j, j] + np.zeros(shape)
            for p in range(j):
                dj = dj - (Lm[j][p] * Lm[j][p]) * d[p]
            ok &= (dj > 0.0) & np.isfinite(dj)
            d[j] = dj
            for i in range(j + 1, 6):
                v = A[..., j, i] + np.zeros(shape)
                for p in range(j):
                    v = v - (Lm[i][p] * Lm[j][p]) * d[p]
                Lm[i][j] = v / dj
            yj = e[..., j] + np.zeros(shape)
            for p in range(j):
                yj = yj - Lm[j][p] * y[p]
            y[j] = yj
            s = s + (yj * yj) / dj
    return np.where(ok, s, np.nan)


def range_cov(W, u, v):
    """C(u, v) = W_max(u,v) - W_min(u,v)"""
    u, v = np.asarray(u), np.asarray(v)
    return W[np.maximum(u, v)] - W[np.minimum(u, v)]


def pair_cov(poses, ak, bk, Zk, Sk, al, bl, Zl, Sl, W):
    """Sigma_e [..., 6, 6] of the pairs (k, l) in the plain form of the header"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    Y = rebased(poses)
    B = lref.between(poses[bl], poses[bk])
    GB = adjoint(inverse(Y[bk]))
    Gl = adjoint(inverse(B))
    GA = adjoint(inverse((Y[al] @ np.asarray(Zl, dtype=np.float64)) @ B))
    Ca, Cb = range_cov(W, ak, al), range_cov(W, bk, bl)
    return np.asarray(Sk, dtype=np.float64) + ((sandwich(GA, Ca) + sandwich(Gl, np.asarray(Sl, dtype=np.float64))) + sandwich(GB, Cb))


def pair_s_one_sandwich(poses, ak, bk, Zk, Sk, al, bl, Zl, Sl, W):
    """s by the algebraically identical form in the frame of pose 0: with D_l = Y_{b_l} Z_l^-1 Y_{a_l}^-1,
    Lambda = Ad(Y_b) Sigma Ad(Y_b)^T and etilde = Ad(Y_{b_k}) e, s = etilde^T (Lambda_k + Lambda_l + C_b + Ad(D_l) C_a Ad(D_l)^T)^-1 etilde"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    Y = rebased(poses)
    e = lref.pair_e(poses[ak], poses[bk], Zk, poses[al], poses[bl], Zl)
    D = Y[bl] @ inverse(Zl) @ inverse(Y[al])
    M = sandwich(adjoint(Y[bk]), Sk) + sandwich(adjoint(Y[bl]), Sl) + range_cov(W, bk, bl) + sandwich(adjoint(D), range_cov(W, ak, al))
    et = (adjoint(Y[bk]) @ e[..., None])[..., 0]
    return (et[..., None, :] @ np.linalg.solve(M, et[..., None]))[..., 0, 0]


def pair_s(poses, a, b, Z, Sigma, W, with_e=False):
    """s [L, L]: symmetric, zero diagonal, every pair evaluated with the lower index as k; NaN where a pivot fails"""
    poses, Z = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4), np.asarray(Z, dtype=np.float64).reshape(-1, 4, 4)
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    L = a.size
    Sigma = np.broadcast_to(np.asarray(Sigma, dtype=np.float64), (L, 6, 6))
    W = np.asarray(W, dtype=np.float64)
    s = np.zeros((L, L))
    k, l = np.triu_indices(L, 1)
    e = np.zeros((0, 6))
    if k.size:
        e = lref.pair_e(poses[a[k]], poses[b[k]], Z[k], poses[a[l]], poses[b[l]], Z[l])
        cov = pair_cov(poses, a[k], b[k], Z[k], Sigma[k], a[l], b[l], Z[l], Sigma[l], W)
        s[k, l] = ldl_form(cov, e)
        s[l, k] = s[k, l]
    return (s, e) if with_e else s


def adjacency(s, gamma):
    return lref.adjacency(s, gamma)


def non_finite_pairs(s):
    k, l = np.triu_indices(s.shape[0], 1)
    return int(np.isnan(s[k, l]).sum())


def _bad_matrix(M):
    M = np.asarray(M, dtype=np.float64)
    if not np.isfinite(M).all():
        return "non-finite"
    if not np.array_equal(M, _T(M)):
        return "not symmetric"
    return None


def refusal(n, a, b, Z, Sigma, Q, q_t=0.0, q_r=0.0, gamma=lref.GAMMA_DEFAULT, steps_per_batch=32, want_s=False):
    """the precondition the header refuses first, or None.  Q: [q_count, 6, 6] (or one 6 x 6: q_count = 1)"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    L = a.size
    Q = np.asarray(Q, dtype=np.float64)
    Q = Q.reshape(1, 6, 6) if Q.shape == (6, 6) else Q
    if n < 1 or n > 1 << 20:
        return "n"
    if L > lref.MAX_L:
        return "ELM_LOOPS_MAX"
    if want_s and L > lref.MAX_L_S:
        return "ELM_LOOPS_MAX_S"
    if q_t != 0 or q_r != 0:
        return "q"
    if not (np.isfinite(gamma) and gamma > 0):
        return "gamma"
    if steps_per_batch < 1:
        return "steps_per_batch"
    if Q.shape[0] not in (1, n - 1):
        return "q_count"
    if n > 1 and _bad_matrix(Q):
        return "Q " + _bad_matrix(Q)
    if ((a < 0) | (a >= n) | (b < 0) | (b >= n)).any():
        return "index"
    if (a == b).any():
        return "a == b"
    if not np.isfinite(np.asarray(Z, dtype=np.float64)).all():
        return "non-finite Z"
    if L:
        Sigma = np.broadcast_to(np.asarray(Sigma, dtype=np.float64), (L, 6, 6))
        if _bad_matrix(Sigma):
            return "Sigma " + _bad_matrix(Sigma)
        if np.isnan(ldl_form(Sigma, np.zeros(6))).any():
            return "Sigma not positive definite"
    return None
