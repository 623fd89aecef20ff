"""Float64 mirror of the pose graph's linear initialization (include/elimaloc_hip_posegraph_init.h), on top of
tests/posegraph_ref.py: the weights, the edge terms of the rotation problem and of the translation problem with their Jacobians written
out as the contract states them (R_Z and all: the library's reduced forms are checked against these), the per-node assembly in
ascending edge order, a direct solve (dense, scipy-sparse for large graphs), the closed-form projection, the preconditions, and the
whole call with a direct solve or with either conjugate-gradient mirror (posegraph_ref.pcg, posegraph_chain_ref.pcg_chain) on the same
systems.  Written from the contract, not from the library's code."""
import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import posegraph_ref as ref

ROT, TRANS = 1, 2
DEGENERATE = 1e-6
SPARSE_FROM = 400  # nodes from which the direct solve is sparse
DEFAULTS = dict(pcg_rel_tol=1e-8, pcg_max_iterations=50000, pcg_check_every=32, stages=ROT | TRANS)

_T = lambda a: np.swapaxes(a, -1, -2)


def weights(g):
    """(w_r [E], w_t [E]): trace(Omega_ww) / 3 and trace(Omega_vv) / 3"""
    tr = lambda M: (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    return tr(g.info[:, 3:, 3:]) / 3.0, tr(g.info[:, :3, :3]) / 3.0


def rows_of(poses):
    """y [N, 6]: the first two rows of every rotation"""
    return np.concatenate([poses[:, 0, :3], poses[:, 1, :3]], axis=1)


def _assemble(g, Hii, Hij, Hjj, gi, gj):
    grad, diag = np.zeros((g.N, 6)), np.zeros((g.N, 6, 6))
    for e in range(g.E):  # ascending edge index: the order of every node's sums
        grad[g.i[e]] += gi[e]
        diag[g.i[e]] += Hii[e]
        grad[g.j[e]] += gj[e]
        diag[g.j[e]] += Hjj[e]
    active = ~g.fixed & (np.abs(diag).reshape(g.N, -1).max(axis=1) > 0.0 if g.N else np.zeros(0, bool))
    return dict(Hii=Hii, Hij=Hij, Hjj=Hjj, gi=gi, gj=gj, grad=grad, diag=diag, active=active)


def _terms(g, w, A, B, e, pad=None):
    W = w[:, None, None]
    Hii, Hij, Hjj = W * (_T(A) @ A), W * (_T(A) @ B), W * (_T(B) @ B)
    if pad is not None:
        Hii, Hjj = Hii + W * pad, Hjj + W * pad
    gi, gj = w[:, None] * (_T(A) @ e[..., None])[..., 0], w[:, None] * (_T(B) @ e[..., None])[..., 0]
    return _assemble(g, Hii, Hij, Hjj, gi, gj)


def rot_system(g, poses=None):
    """the rotation problem at the rows of `poses`: a dict like ref.linearize's (Hii, Hij, Hjj, gi, gj, grad, diag, active)"""
    poses = g.poses if poses is None else poses
    y = rows_of(poses)
    RZt = _T(g.Z[:, :3, :3])
    A = np.zeros((g.E, 6, 6))
    A[:, :3, :3], A[:, 3:, 3:] = RZt, RZt
    B = np.tile(-np.eye(6), (g.E, 1, 1))
    e = (A @ y[g.i][..., None])[..., 0] - y[g.j] if g.E else np.zeros((0, 6))
    return _terms(g, weights(g)[0], A, B, e)


def trans_system(g, poses=None):
    """the translation problem at the rotations of `poses`: the unknown [v; 0], the lower three padded with the diagonal w_t"""
    poses = g.poses if poses is None else poses
    Ri, Rj, ti, tj = poses[g.i, :3, :3], poses[g.j, :3, :3], poses[g.i, :3, 3], poses[g.j, :3, 3]
    RZt, tZ = _T(g.Z[:, :3, :3]), g.Z[:, :3, 3]
    A, B, e = np.zeros((g.E, 6, 6)), np.zeros((g.E, 6, 6)), np.zeros((g.E, 6))
    if g.E:
        A[:, :3, :3] = -RZt
        B[:, :3, :3] = RZt @ (_T(Ri) @ Rj)
        e[:, :3] = (RZt @ ((_T(Ri) @ (tj - ti)[..., None])[..., 0] - tZ)[..., None])[..., 0]
    return _terms(g, weights(g)[1], A, B, e, pad=np.diag([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]))


def system(g, lin, sparse=None):
    """(H [6N, 6N], -g [6N]) at lambda = 0, the rows and columns of inactive nodes those of the identity and 0 (ref.dense_system's form;
    a scipy CSC matrix from SPARSE_FROM nodes)"""
    sparse = g.N >= SPARSE_FROM if sparse is None else sparse
    if not sparse:
        return ref.dense_system(g, lin, 0.0)
    a = lin["active"]
    six = np.arange(6)
    rows = lambda v: np.broadcast_to((6 * v[:, None] + six)[:, :, None], (v.size, 6, 6)).ravel()
    cols = lambda v: np.broadcast_to((6 * v[:, None] + six)[:, None, :], (v.size, 6, 6)).ravel()
    every = np.arange(g.N)
    diag = np.where(a[:, None, None], lin["diag"], np.eye(6))
    both = a[g.i] & a[g.j]
    i, j, Hij = g.i[both], g.j[both], lin["Hij"][both]
    r = np.concatenate([rows(every), rows(i), rows(j)])
    c = np.concatenate([cols(every), cols(j), cols(i)])
    val = np.concatenate([diag.ravel(), Hij.ravel(), _T(Hij).ravel()])
    H = scipy.sparse.coo_matrix((val, (r, c)), shape=(6 * g.N, 6 * g.N)).tocsc()
    return H, np.where(a[:, None], -lin["grad"], 0.0).reshape(-1)


def direct(g, lin, sparse=None):
    """-> (delta [N, 6], 0, 0.0, True): the solution of H delta = -g by a direct factorization, in the shape of ref.pcg's return"""
    H, b = system(g, lin, sparse)
    if not g.N:
        return np.zeros((0, 6)), 0, 0.0, True
    x = scipy.sparse.linalg.splu(H).solve(b) if scipy.sparse.issparse(H) else np.linalg.solve(H, b)
    return x.reshape(g.N, 6), 0, 0.0, True


def project(y):
    """rows y [..., 6] -> (R [..., 3, 3], degenerate [...]): the contract's closed form; a degenerate entry's R is the identity"""
    y = np.asarray(y, dtype=np.float64)
    norm = lambda a: np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    safe = lambda n: np.where(n < DEGENERATE, 1.0, n)[..., None]
    n1, n2 = norm(y[..., :3]), norm(y[..., 3:])
    u, v = y[..., :3] / safe(n1), y[..., 3:] / safe(n2)
    s, d = u + v, u - v
    ns, nd = norm(s), norm(d)
    deg = (n1 < DEGENERATE) | (n2 < DEGENERATE) | (ns < DEGENERATE) | (nd < DEGENERATE)
    s, d = s / safe(ns), d / safe(nd)
    r1, r2 = (s + d) / np.sqrt(2.0), (s - d) / np.sqrt(2.0)
    R = np.stack([r1, r2, np.cross(r1, r2)], axis=-2)
    return np.where(deg[..., None, None], np.eye(3), R), deg


def refusal(g, stages=ROT | TRANS):
    """None when the preconditions that need the graph hold, else which one does not"""
    if not g.N:
        return "no node"
    wr, wt = weights(g)
    if stages & ROT and not (wr > 0.0).all():
        return "rotation weight"
    if stages & TRANS and not (wt > 0.0).all():
        return "translation weight"
    root = list(range(g.N))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    for a, b in zip(g.i, g.j):
        a, b = find(int(a)), find(int(b))
        if a != b:
            root[max(a, b)] = min(a, b)
    anchored = {find(v) for v in range(g.N) if g.fixed[v]}
    with_edges = {find(int(v)) for v in g.i}
    return "component without a fixed node" if with_edges - anchored else None


def config_ok(pcg_rel_tol=1e-8, pcg_max_iterations=50000, pcg_check_every=32, stages=ROT | TRANS):
    return bool(np.isfinite(pcg_rel_tol) and pcg_rel_tol > 0.0 and pcg_max_iterations >= 1 and pcg_check_every >= 1 and 1 <= stages <= 3)


def initialize(g, stages=ROT | TRANS, solver=direct):
    """The whole call.  solver(g, lin) -> (delta, iterations, rel_residual, converged): `direct`, or a conjugate-gradient mirror such as
    lambda g, lin: ref.pcg(g, lin, 0.0, tol, max_it).  -> dict(poses: the trial poses, applied, rows, v, degenerate [N] bool,
    degenerate_nodes, rot / trans: (iterations, rel_residual, converged), cost_before, cost_after, rot_lin, trans_lin)"""
    assert refusal(g, stages) is None
    trial = g.poses.copy()
    out = dict(rows=rows_of(g.poses), v=np.zeros((g.N, 3)), degenerate=np.zeros(g.N, bool), rot=(0, 0.0, False), trans=(0, 0.0, False),
               rot_lin=None, trans_lin=None, cost_before=ref.cost(g, g.poses))
    if stages & ROT:
        lin = rot_system(g)
        delta, its, rel, conv = solver(g, lin)
        a = lin["active"]
        y = rows_of(g.poses)
        y[a] = y[a] + delta[a]
        R, deg = project(y)
        move = a & ~deg
        trial[move, :3, :3] = R[move]
        out.update(rows=y, degenerate=a & deg, rot=(its, rel, conv), rot_lin=lin)
    if stages & TRANS:
        lin = trans_system(g, trial)
        delta, its, rel, conv = solver(g, lin)
        a = lin["active"]
        v = np.where(a[:, None], delta[:, :3], 0.0)
        trial[:, :3, 3] = trial[:, :3, 3] + (trial[:, :3, :3] @ v[..., None])[..., 0]
        out.update(v=v, trans=(its, rel, conv), trans_lin=lin, padding=np.abs(delta[:, 3:]).max() if g.N else 0.0)
    out["applied"] = all(out[k][2] for k, bit in (("rot", ROT), ("trans", TRANS)) if stages & bit)
    out.update(poses=trial, degenerate_nodes=int(out["degenerate"].sum()), cost_after=ref.cost(g, trial))
    return out
