"""Float64 numpy mirror of the pose-graph contract (include/elimaloc_hip.h, "pose graph"): residual, Jacobians, Huber,
the block-sparse assembly with the per-node ascending-edge order, the same preconditioned conjugate gradients and the same
Levenberg-Marquardt rules; for small graphs also the dense H.  Written from the contract, not from the library's code."""
import numpy as np

LOG_SMALL_N = 1e-8
SERIES_THETA = 1e-2
STOP = {1: "max_iterations", 2: "cost_tol", 3: "step_tol", 4: "lambda_max", 5: "cost_zero"}


def hat(v):
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape[:-1] + (3, 3))
    out[..., 0, 1], out[..., 0, 2] = -v[..., 2], v[..., 1]
    out[..., 1, 0], out[..., 1, 2] = v[..., 2], -v[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -v[..., 1], v[..., 0]
    return out


def exp_so3(w):
    """Rodrigues, batched: w [..., 3] -> R [..., 3, 3]; zero -> identity"""
    w = np.asarray(w, dtype=np.float64)
    ang = np.linalg.norm(w, axis=-1)
    ax = np.where(ang[..., None] > 0.0, w / np.where(ang > 0.0, ang, 1.0)[..., None], w)
    K = hat(ax)
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


def quat(R):
    """the unit quaternion (w, x, y, z) of R [..., 3, 3], w >= 0, by the branches of the contract"""
    R = np.asarray(R, dtype=np.float64)
    m = lambda a, b: R[..., a, b]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + 1.0)
        q0 = np.stack([0.5 * t, (m(2, 1) - m(1, 2)) * (0.5 / t), (m(0, 2) - m(2, 0)) * (0.5 / t), (m(1, 0) - m(0, 1)) * (0.5 / t)], -1)
        t = np.sqrt(m(0, 0) - m(1, 1) - m(2, 2) + 1.0)
        q1 = np.stack([(m(2, 1) - m(1, 2)) * (0.5 / t), 0.5 * t, (m(1, 0) + m(0, 1)) * (0.5 / t), (m(2, 0) + m(0, 2)) * (0.5 / t)], -1)
        t = np.sqrt(m(1, 1) - m(2, 2) - m(0, 0) + 1.0)
        q2 = np.stack([(m(0, 2) - m(2, 0)) * (0.5 / t), (m(0, 1) + m(1, 0)) * (0.5 / t), 0.5 * t, (m(2, 1) + m(1, 2)) * (0.5 / t)], -1)
        t = np.sqrt(m(2, 2) - m(0, 0) - m(1, 1) + 1.0)
        q3 = np.stack([(m(1, 0) - m(0, 1)) * (0.5 / t), (m(0, 2) + m(2, 0)) * (0.5 / t), (m(1, 2) + m(2, 1)) * (0.5 / t), 0.5 * t], -1)
    lead0 = (m(0, 0) >= m(1, 1)) & (m(0, 0) >= m(2, 2))
    lead1 = ~lead0 & (m(1, 1) >= m(2, 2))
    q = np.where((tr > 0.0)[..., None], q0, np.where(lead0[..., None], q1, np.where(lead1[..., None], q2, q3)))
    return np.where((q[..., :1] < 0.0), -q, q)


def log_so3(R, full=False):
    """phi [..., 3] (and theta, w, n with full=True)"""
    q = quat(R)
    w, vec = q[..., 0], q[..., 1:]
    n = np.sqrt((vec[..., 0] * vec[..., 0] + vec[..., 1] * vec[..., 1]) + vec[..., 2] * vec[..., 2])
    small = n < LOG_SMALL_N
    theta = np.where(small, 2.0 * n, 2.0 * np.arctan2(n, w))
    k = np.where(small, 2.0, theta / np.where(small, 1.0, n))
    phi = vec * k[..., None]
    return (phi, theta, w, n) if full else phi


def jinv_c(theta, w, n):
    theta, w, n = (np.asarray(a, dtype=np.float64) for a in (theta, w, n))
    t2 = theta * theta
    series = (1.0 / 12.0 + t2 / 720.0) + (t2 * t2) / 30240.0
    big = theta >= SERIES_THETA
    ts, ns = np.where(big, theta, 1.0), np.where(big, n, 1.0)
    return np.where(big, 1.0 / (ts * ts) - w / ((2.0 * ts) * ns), series)


def jinv(phi, c):
    K = hat(phi)
    return np.eye(3) + 0.5 * K + np.asarray(c)[..., None, None] * (K @ K)


def _T(a):
    return np.swapaxes(a, -1, -2)


def residual(Ti, Tj, Z):
    """r [..., 6] of edges (batched over the leading axes)"""
    Ti, Tj, Z = (np.asarray(a, dtype=np.float64) for a in (Ti, Tj, Z))
    Ri, Rj, RZ = Ti[..., :3, :3], Tj[..., :3, :3], Z[..., :3, :3]
    d = (_T(Ri) @ (Tj[..., :3, 3] - Ti[..., :3, 3])[..., None])[..., 0]
    RE = _T(RZ) @ (_T(Ri) @ Rj)
    rt = (_T(RZ) @ (d - Z[..., :3, 3])[..., None])[..., 0]
    return np.concatenate([rt, log_so3(RE)], -1)


def edge_terms(Ti, Tj, Z):
    """(r [..., 6], A [..., 6, 6], B [..., 6, 6])"""
    Ti, Tj, Z = (np.asarray(a, dtype=np.float64) for a in (Ti, Tj, Z))
    Ri, Rj, RZ = Ti[..., :3, :3], Tj[..., :3, :3], Z[..., :3, :3]
    d = (_T(Ri) @ (Tj[..., :3, 3] - Ti[..., :3, 3])[..., None])[..., 0]
    Rij = _T(Ri) @ Rj
    RE = _T(RZ) @ Rij
    rt = (_T(RZ) @ (d - Z[..., :3, 3])[..., None])[..., 0]
    phi, theta, w, n = log_so3(RE, full=True)
    J = jinv(phi, jinv_c(theta, w, n))
    A = np.zeros(Ti.shape[:-2] + (6, 6))
    B = np.zeros_like(A)
    A[..., :3, :3] = -_T(RZ)
    A[..., :3, 3:] = _T(RZ) @ hat(d)
    A[..., 3:, 3:] = -(J @ _T(Rij))
    B[..., :3, :3] = RE
    B[..., 3:, 3:] = J
    return np.concatenate([rt, phi], -1), A, B


def huber_weight(s, k):
    s = np.asarray(s, dtype=np.float64)
    if not k > 0.0:
        return np.ones_like(s)
    out = s > k * k
    return np.where(out, k / np.sqrt(np.where(out, s, 1.0)), 1.0)


def huber_cost(s, k):
    s = np.asarray(s, dtype=np.float64)
    if not k > 0.0:
        return s.copy()
    out = s > k * k
    return np.where(out, (2.0 * k) * np.sqrt(np.where(out, s, 1.0)) - k * k, s)


class Graph:
    """poses [N, 4, 4], fixed [N] bool, edges i, j [E], Z [E, 4, 4], info [E, 6, 6]"""

    def __init__(self, poses, fixed, i, j, Z, info=None):
        self.poses = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
        self.N = self.poses.shape[0]
        self.fixed = np.zeros(self.N, bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(-1)
        self.i, self.j = np.asarray(i, dtype=np.int64).reshape(-1), np.asarray(j, dtype=np.int64).reshape(-1)
        self.E = self.i.size
        self.Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4, 4)
        self.info = np.tile(np.eye(6), (self.E, 1, 1)) if info is None else np.asarray(info, dtype=np.float64).reshape(-1, 6, 6)


def edge_s(g, poses):
    r = residual(poses[g.i], poses[g.j], g.Z) if g.E else np.zeros((0, 6))
    return np.einsum("ea,eab,eb->e", r, g.info, r)


def cost(g, poses, huber_k=0.0):
    return float(np.sum(huber_cost(edge_s(g, poses), huber_k)))


def linearize(g, poses=None, huber_k=0.0):
    """dict: r, A, B, s, w per edge; Hii, Hij, Hjj, gi, gj per edge; grad [N, 6] and diag [N, 6, 6] summed per node over its incident
    edges in ascending edge index; active [N]"""
    poses = g.poses if poses is None else poses
    if g.E:
        r, A, B = edge_terms(poses[g.i], poses[g.j], g.Z)
    else:
        r, A, B = np.zeros((0, 6)), np.zeros((0, 6, 6)), np.zeros((0, 6, 6))
    s = np.einsum("ea,eab,eb->e", r, g.info, r)
    w = huber_weight(s, huber_k)
    OA, OB, Or = g.info @ A, g.info @ B, (g.info @ r[..., None])[..., 0]
    W = w[:, None, None]
    Hii, Hij, Hjj = W * (_T(A) @ OA), W * (_T(A) @ OB), W * (_T(B) @ OB)
    gi, gj = w[:, None] * (_T(A) @ Or[..., None])[..., 0], w[:, None] * (_T(B) @ Or[..., None])[..., 0]
    grad, diag = np.zeros((g.N, 6)), np.zeros((g.N, 6, 6))
    for e in range(g.E):  # ascending edge index: the order of every node's sums
        grad[g.i[e]] += gi[e]
        diag[g.i[e]] += Hii[e]
        grad[g.j[e]] += gj[e]
        diag[g.j[e]] += Hjj[e]
    active = ~g.fixed & (np.abs(diag).reshape(g.N, -1).max(axis=1) > 0.0 if g.N else np.zeros(0, bool))
    return dict(r=r, A=A, B=B, s=s, w=w, Hii=Hii, Hij=Hij, Hjj=Hjj, gi=gi, gj=gj, grad=grad, diag=diag, active=active,
                chi2=float(s.sum()), cost=float(huber_cost(s, huber_k).sum()), n_outliers=int((w < 1.0).sum()),
                grad_inf_norm=float(np.abs(grad[active]).max()) if active.any() else 0.0)


def damped(diag, lam):
    D = diag.copy()
    idx = np.arange(6)
    D[:, idx, idx] = D[:, idx, idx] + lam * D[:, idx, idx]
    return D


def dense_system(g, lin, lam):
    """(H + lam diag H) [6N, 6N] and -g [6N], the rows and columns of inactive nodes replaced by the identity and 0"""
    N = g.N
    H = np.zeros((N, 6, N, 6))
    for e in range(g.E):
        H[g.i[e], :, g.i[e], :] += lin["Hii"][e]
        H[g.j[e], :, g.j[e], :] += lin["Hjj"][e]
        H[g.i[e], :, g.j[e], :] += lin["Hij"][e]
        H[g.j[e], :, g.i[e], :] += lin["Hij"][e].T
    H = H.reshape(6 * N, 6 * N)
    H[np.diag_indices(6 * N)] *= 1.0 + lam
    b = -lin["grad"].reshape(-1).copy()
    off = np.repeat(~lin["active"], 6)
    H[off, :] = 0.0
    H[:, off] = 0.0
    H[off, off] = 1.0
    b[off] = 0.0
    return H, b


def spmv(g, lin, lam, p):
    a = lin["active"]
    q = np.einsum("nab,nb->na", damped(lin["diag"], lam), p)
    if g.E:
        np.add.at(q, g.i, np.einsum("eab,eb->ea", lin["Hij"], p[g.j]))
        np.add.at(q, g.j, np.einsum("eba,eb->ea", lin["Hij"], p[g.i]))
    q[~a] = 0.0
    return q


def block_jacobi(g, lin, lam):
    """-> precond(r [N, 6]) = M^-1 r for the contract's default M: the damped diagonal blocks of the active nodes"""
    a = lin["active"]
    Minv = np.zeros((g.N, 6, 6))
    if a.any():
        Minv[a] = np.linalg.inv(damped(lin["diag"], lam)[a])
    return lambda r: np.einsum("nab,nb->na", Minv, r)


def pcg(g, lin, lam, rel_tol, max_it, precond=None):
    """-> (delta [N, 6], iterations, rel_residual, converged): the contract's preconditioned conjugate gradients.  precond: r -> z = M^-1 r
    (block_jacobi's by default)"""
    a = lin["active"]
    precond = block_jacobi(g, lin, lam) if precond is None else precond
    x = np.zeros((g.N, 6))
    r = np.where(a[:, None], -lin["grad"], 0.0)
    z = precond(r)
    p = z.copy()
    rz = rz0 = float(np.sum(r * z))
    if rel_tol > 0.0 and not rz0 > 0.0:
        return x, 0, 0.0, True
    it, conv = 0, False
    while it < max_it:
        q = spmv(g, lin, lam, p)
        pq = float(np.sum(p * q))
        alpha = rz / pq if pq != 0.0 else 0.0
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rz_new = float(np.sum(r * z))
        beta = rz_new / rz if rz != 0.0 else 0.0
        p = z + beta * p
        rz = rz_new
        it += 1
        if rel_tol > 0.0 and np.sqrt(rz) <= rel_tol * np.sqrt(rz0):
            conv = True
            break
    return x, it, (np.sqrt(rz) / np.sqrt(rz0) if rz0 > 0.0 else 0.0), conv


def true_rel_residual(g, lin, lam, delta):
    """|b - H delta| / |b| in the M^-1 norm of the contract's stop test, from the dense system"""
    H, b = dense_system(g, lin, lam)
    a = np.repeat(lin["active"], 6)
    if not a.any():
        return 0.0
    res = (b - H @ delta.reshape(-1))[a]
    N = g.N
    Minv = np.zeros((6 * N, 6 * N))
    D = damped(lin["diag"], lam)
    for v in np.flatnonzero(lin["active"]):
        Minv[6 * v:6 * v + 6, 6 * v:6 * v + 6] = np.linalg.inv(D[v])
    Minv = Minv[np.ix_(a, a)]
    b = b[a]
    den = float(b @ Minv @ b)
    return float(np.sqrt(res @ Minv @ res) / np.sqrt(den)) if den > 0.0 else 0.0


def retract(poses, delta, active):
    out = poses.copy()
    R = poses[:, :3, :3]
    out[:, :3, :3] = R @ exp_so3(delta[:, 3:])
    out[:, :3, 3] = poses[:, :3, 3] + (R @ delta[:, :3, None])[..., 0]
    out[~active] = poses[~active]
    return out


DEFAULTS = dict(max_iterations=20, lambda_init=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-12, lambda_max=1e8, cost_rel_tol=1e-12,
                step_tol=1e-10, pcg_max_iterations=2000, pcg_rel_tol=1e-8, pcg_check_every=32, huber_k=0.0)


def optimize(g, pcg=pcg, **kw):
    """The contract's Levenberg-Marquardt -> (poses, result dict with trace).  pcg: the conjugate gradients of its solves"""
    c = dict(DEFAULTS)
    c.update(kw)
    poses = g.poses.copy()
    k = c["huber_k"]
    F = cost(g, poses, k)
    lam = c["lambda_init"]
    res = dict(solves=0, accepted=0, rejected=0, cost_initial=F, pcg_iterations_total=0, stop_reason=None, trace=[])
    if F == 0.0:
        res["stop_reason"] = "cost_zero"
    lin = linearize(g, poses, k)
    while res["stop_reason"] is None and res["solves"] < c["max_iterations"]:
        delta, its, _, _ = pcg(g, lin, lam, c["pcg_rel_tol"], c["pcg_max_iterations"])
        trial = retract(poses, delta, lin["active"])
        F_new = cost(g, trial, k)
        dmax = float(np.abs(delta).max()) if delta.size else 0.0
        accept = F_new < F
        res["solves"] += 1
        res["pcg_iterations_total"] += its
        res["trace"].append(dict(cost=F_new, lambda_=lam, accepted=accept, pcg_iterations=its, ratio=F_new / F))
        if accept:
            res["accepted"] += 1
            poses, dec, F_old, F = trial, F - F_new, F, F_new
            lam = max(lam * c["lambda_down"], c["lambda_min"])
            if F == 0.0:
                res["stop_reason"] = "cost_zero"
            elif dec <= c["cost_rel_tol"] * F_old:
                res["stop_reason"] = "cost_tol"
            elif dmax <= c["step_tol"]:
                res["stop_reason"] = "step_tol"
            elif res["solves"] < c["max_iterations"]:
                lin = linearize(g, poses, k)
        else:
            res["rejected"] += 1
            if dmax <= c["step_tol"]:
                res["stop_reason"] = "step_tol"
            elif lam >= c["lambda_max"]:
                res["stop_reason"] = "lambda_max"
            else:
                lam = min(lam * c["lambda_up"], c["lambda_max"])
    if res["stop_reason"] is None:
        res["stop_reason"] = "max_iterations"
    res["cost_final"], res["lambda_final"] = F, lam
    return poses, res


def pose_error(Ta, Tb):
    """(largest translation difference, largest rotation angle) between two pose arrays"""
    dt = float(np.linalg.norm(Ta[:, :3, 3] - Tb[:, :3, 3], axis=1).max())
    dR = _T(Ta[:, :3, :3]) @ Tb[:, :3, :3]
    ang = np.linalg.norm(log_so3(dR), axis=-1)
    return dt, float(ang.max())
