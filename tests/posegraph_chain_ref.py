"""Float64 mirror of the pose graph's chain preconditioner (include/elimaloc_hip_posegraph_precond.h), on top of
tests/posegraph_ref.py: the chain edges, the block-tridiagonal M (dense, scipy-sparse for large graphs), the contract's conjugate
gradients with z = M^-1 r by a direct solve, and Levenberg-Marquardt around them.  Written from the definition of M, not from the
library's elimination order."""
import numpy as np
import scipy.linalg
import scipy.sparse
import scipy.sparse.linalg

import posegraph_ref as ref

SPARSE_FROM = 400  # nodes from which chain_matrix is sparse by default


def chain_edges(g, lin):
    """-> (edge [N - 1], reversed [N - 1]): the chain edge of v, the lowest-index edge between v and v + 1 in either direction whose two
    nodes are active, or -1; reversed: stored v + 1 -> v"""
    n = max(g.N - 1, 0)
    edge, rev = np.full(n, -1, np.int64), np.zeros(n, bool)
    a = lin["active"]
    for e in range(g.E - 1, -1, -1):  # descending: the lowest index is written last
        i, j = int(g.i[e]), int(g.j[e])
        if abs(i - j) == 1 and a[i] and a[j]:
            edge[min(i, j)], rev[min(i, j)] = e, i > j
    return edge, rev


def chain_matrix(g, lin, lam, sparse=None):
    """M [6N, 6N]: the damped diagonal blocks of the active nodes, the chain edges' H_ij and its transpose; the rows and columns of
    inactive nodes are those of the identity (as ref.dense_system has them)"""
    N = g.N
    sparse = N >= SPARSE_FROM if sparse is None else sparse
    a = lin["active"]
    D = ref.damped(lin["diag"], lam)
    edge, rev = chain_edges(g, lin)
    diag = np.where(a[:, None, None], D, np.eye(6))
    at = np.flatnonzero(edge >= 0)
    up = lin["Hij"][edge[at]] if at.size else np.zeros((0, 6, 6))  # M[v][v + 1]
    up = np.where(rev[at][:, None, None], np.swapaxes(up, 1, 2), up)
    if not sparse:
        M = np.zeros((6 * N, 6 * N))
        for v in range(N):
            M[6 * v:6 * v + 6, 6 * v:6 * v + 6] = diag[v]
        for k, v in enumerate(at):
            M[6 * v:6 * v + 6, 6 * v + 6:6 * v + 12] = up[k]
            M[6 * v + 6:6 * v + 12, 6 * v:6 * v + 6] = up[k].T
        return M
    six = np.arange(6)
    rows = lambda v: np.broadcast_to((6 * v[:, None] + six)[:, :, None], (v.size, 6, 6))
    cols = lambda v: np.broadcast_to((6 * v[:, None] + six)[:, None, :], (v.size, 6, 6))
    every = np.arange(N)
    r = np.concatenate([rows(every).ravel(), rows(at).ravel(), rows(at + 1).ravel()])
    c = np.concatenate([cols(every).ravel(), cols(at + 1).ravel(), cols(at).ravel()])
    val = np.concatenate([diag.ravel(), up.ravel(), np.swapaxes(up, 1, 2).ravel()])
    return scipy.sparse.coo_matrix((val, (r, c)), shape=(6 * N, 6 * N)).tocsc()


def chain_solver(g, lin, lam, sparse=None, M=None):
    """-> solve(r [N, 6]) = M^-1 r [N, 6] by a direct factorization (of the given chain_matrix, when there is one)"""
    M = chain_matrix(g, lin, lam, sparse) if M is None else M
    if scipy.sparse.issparse(M):
        lu = scipy.sparse.linalg.splu(M)
        return lambda r: lu.solve(r.reshape(-1)).reshape(-1, 6)
    lu = scipy.linalg.lu_factor(M) if g.N else None
    return lambda r: scipy.linalg.lu_solve(lu, r.reshape(-1)).reshape(-1, 6) if g.N else r.copy()


def chain_solver_cholesky(g, lin, lam, M=None):
    """the same M^-1 by a banded Cholesky factorization of the symmetrized M: a second, equally valid direct solve, whose difference
    from chain_solver's says how many digits of M^-1 r a direct solve in float64 has at all (M's condition number times 1e-16)"""
    M = chain_matrix(g, lin, lam) if M is None else M
    n = M.shape[0]
    if not n:
        return lambda r: r.copy()
    S = (M + M.T) * 0.5
    ab = np.zeros((12, n))  # lower form: ab[k, j] = S[j + k, j]
    for k in range(min(12, n)):
        ab[k, :n - k] = S.diagonal(-k)
    cb = scipy.linalg.cholesky_banded(ab, lower=True)
    return lambda r: scipy.linalg.cho_solve_banded((cb, True), r.reshape(-1)).reshape(-1, 6)


def pcg_chain(g, lin, lam, rel_tol, max_it, sparse=None, solve=None):
    """-> (delta [N, 6], iterations, rel_residual, converged): ref.pcg with z = M^-1 r (solve: chain_solver's, or the given one)"""
    return ref.pcg(g, lin, lam, rel_tol, max_it, precond=chain_solver(g, lin, lam, sparse) if solve is None else solve)


def true_rel_residual(g, lin, lam, delta):
    """|b - H delta| / |b| in the chain M^-1 norm of the stop test, from the dense system"""
    H, b = ref.dense_system(g, lin, lam)
    if not lin["active"].any():
        return 0.0
    solve = chain_solver(g, lin, lam, sparse=False)
    res = b - H @ delta.reshape(-1)
    den = float(b @ solve(b).reshape(-1))
    return float(np.sqrt(res @ solve(res).reshape(-1)) / np.sqrt(den)) if den > 0.0 else 0.0


def backward_error(g, lin, lam, z, r, M=None):
    """max over the rows of |M z - r| / (|M| |z| + |r|), rows where the denominator is 0 left out"""
    M = chain_matrix(g, lin, lam) if M is None else M
    zf, rf = z.reshape(-1), r.reshape(-1)
    num = np.abs(M @ zf - rf)
    den = abs(M) @ np.abs(zf) + np.abs(rf)
    ok = den > 0.0
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def optimize(g, **kw):
    """ref.optimize with pcg_chain in the place of ref.pcg"""
    return ref.optimize(g, pcg=pcg_chain, **kw)
