"""Float64 numpy mirror of the pose graph's priors (include/elimaloc_hip_posegraph_prior.h), on top of
tests/posegraph_ref.py, which it leaves alone: the residual and Jacobian of an absolute pose / position factor with a lever arm, the
linearization completed in the contract's order (a node's edges first, then its priors in ascending prior index), the cost, and
posegraph_ref's Levenberg-Marquardt loop with posegraph_ref.pcg on the completed linearization.  Written from the contract, not from the
library's code."""
import numpy as np

import posegraph_ref as ref

_T = ref._T


class Priors:
    """node [P], Z [P, 4, 4], lever [P, 3], info [P, 6, 6]"""

    def __init__(self, node=(), Z=None, lever=None, info=None):
        self.node = np.asarray(node, dtype=np.int64).reshape(-1)
        self.P = self.node.size
        self.Z = np.tile(np.eye(4), (self.P, 1, 1)) if Z is None else np.array(Z, dtype=np.float64).reshape(-1, 4, 4)
        self.lever = np.zeros((self.P, 3)) if lever is None else np.array(np.broadcast_to(np.asarray(lever, dtype=np.float64), (self.P, 3)))
        self.info = np.tile(np.eye(6), (self.P, 1, 1)) if info is None else np.array(
            np.broadcast_to(np.asarray(info, dtype=np.float64), (self.P, 6, 6)))

    @classmethod
    def positions(cls, node, positions, info3=None, lever=None):
        """position measurements: Z = [I | p], the 3 x 3 information in the translation block, the rotation rows and columns zero"""
        node = np.asarray(node, dtype=np.int64).reshape(-1)
        Z = np.tile(np.eye(4), (node.size, 1, 1))
        Z[:, :3, 3] = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
        info = np.zeros((node.size, 6, 6))
        info[:, :3, :3] = np.eye(3) if info3 is None else np.asarray(info3, dtype=np.float64)
        return cls(node, Z, lever, info)

    def take(self, idx):
        idx = np.asarray(idx)
        return Priors(self.node[idx], self.Z[idx], self.lever[idx], self.info[idx])


def prior_residual(T, Z, lever):
    """r [..., 6] (batched over the leading axes)"""
    T, Z, lever = (np.asarray(a, dtype=np.float64) for a in (T, Z, lever))
    R, RZ = T[..., :3, :3], Z[..., :3, :3]
    p = T[..., :3, 3] + (R @ lever[..., None])[..., 0]
    rt = (_T(RZ) @ (p - Z[..., :3, 3])[..., None])[..., 0]
    return np.concatenate([rt, ref.log_so3(_T(RZ) @ R)], -1)


def prior_terms(T, Z, lever=None):
    """(r [..., 6], J [..., 6, 6])"""
    T, Z = np.asarray(T, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    lever = np.zeros(T.shape[:-2] + (3,)) if lever is None else np.asarray(lever, dtype=np.float64)
    R, RZ = T[..., :3, :3], Z[..., :3, :3]
    E = _T(RZ) @ R
    p = T[..., :3, 3] + (R @ lever[..., None])[..., 0]
    rt = (_T(RZ) @ (p - Z[..., :3, 3])[..., None])[..., 0]
    phi, theta, w, n = ref.log_so3(E, full=True)
    J = np.zeros(T.shape[:-2] + (6, 6))
    J[..., :3, :3] = E
    J[..., :3, 3:] = -(E @ ref.hat(lever))
    J[..., 3:, 3:] = ref.jinv(phi, ref.jinv_c(theta, w, n))
    return np.concatenate([rt, phi], -1), J


def prior_s(P, poses):
    r = prior_residual(poses[P.node], P.Z, P.lever) if P.P else np.zeros((0, 6))
    return np.einsum("qa,qab,qb->q", r, P.info, r)


def cost(g, P, poses, huber_k=0.0, prior_huber_k=0.0):
    """F = (sum rho_e) + (sum rho_q): the two totals apart, then one addition"""
    return ref.cost(g, poses, huber_k) + float(np.sum(ref.huber_cost(prior_s(P, poses), prior_huber_k)))


def linearize(g, P, poses=None, huber_k=0.0, prior_huber_k=0.0):
    """ref.linearize's dict with grad / diag / active and the stats completed by the priors in the contract's order, plus the per-prior
    arrays pr, pJ, ps, pw, pg (w J^T Omega r) and pH (w J^T Omega J)"""
    poses = g.poses if poses is None else poses
    lin = ref.linearize(g, poses, huber_k)
    if P.P:
        r, J = prior_terms(poses[P.node], P.Z, P.lever)
    else:
        r, J = np.zeros((0, 6)), np.zeros((0, 6, 6))
    s = np.einsum("qa,qab,qb->q", r, P.info, r)
    w = ref.huber_weight(s, prior_huber_k)
    OJ, Or = P.info @ J, (P.info @ r[..., None])[..., 0]
    pH = w[:, None, None] * (_T(J) @ OJ)
    pg = w[:, None] * (_T(J) @ Or[..., None])[..., 0]
    grad, diag = lin["grad"].copy(), lin["diag"].copy()
    for q in range(P.P):  # after every edge, in ascending prior index: the order of every node's sums
        grad[P.node[q]] += pg[q]
        diag[P.node[q]] += pH[q]
    active = ~g.fixed & (np.abs(diag).reshape(g.N, -1).max(axis=1) > 0.0 if g.N else np.zeros(0, bool))
    lin.update(grad=grad, diag=diag, active=active, pr=r, pJ=J, ps=s, pw=w, pg=pg, pH=pH,
               chi2=lin["chi2"] + float(s.sum()), cost=lin["cost"] + float(ref.huber_cost(s, prior_huber_k).sum()),
               n_outliers=lin["n_outliers"] + int((w < 1.0).sum()),
               grad_inf_norm=float(np.abs(grad[active]).max()) if active.any() else 0.0)
    return lin


def dense_system(g, lin, lam):
    """ref.dense_system of the completed linearization: the priors' blocks onto the diagonal blocks, before the damping and the masking"""
    N = g.N
    H = np.zeros((N, 6, N, 6))
    for e in range(g.E):
        H[g.i[e], :, g.j[e], :] += lin["Hij"][e]
        H[g.j[e], :, g.i[e], :] += lin["Hij"][e].T
    for v in range(N):
        H[v, :, v, :] = lin["diag"][v]
    H = H.reshape(6 * N, 6 * N)
    H[np.diag_indices(6 * N)] *= 1.0 + lam
    b = -lin["grad"].reshape(-1).copy()
    off = np.repeat(~lin["active"], 6)
    H[off, :] = 0.0
    H[:, off] = 0.0
    H[off, off] = 1.0
    b[off] = 0.0
    return H, b


def true_rel_residual(g, lin, lam, delta, solve=None):
    """ref.true_rel_residual on the completed dense system; solve: r [N, 6] -> M^-1 r of another preconditioner (the chain mirror's
    chain_solver on the completed linearization), as posegraph_chain_ref.true_rel_residual has it"""
    H, b = dense_system(g, lin, lam)
    a = np.repeat(lin["active"], 6)
    if not a.any():
        return 0.0
    if solve is not None:
        res = b - H @ delta.reshape(-1)
        den = float(b @ solve(b).reshape(-1))
        return float(np.sqrt(res @ solve(res).reshape(-1)) / np.sqrt(den)) if den > 0.0 else 0.0
    res = (b - H @ delta.reshape(-1))[a]
    Minv = np.zeros((6 * g.N, 6 * g.N))
    D = ref.damped(lin["diag"], lam)
    for v in np.flatnonzero(lin["active"]):
        Minv[6 * v:6 * v + 6, 6 * v:6 * v + 6] = np.linalg.inv(D[v])
    Minv = Minv[np.ix_(a, a)]
    b = b[a]
    den = float(b @ Minv @ b)
    return float(np.sqrt(res @ Minv @ res) / np.sqrt(den)) if den > 0.0 else 0.0


def cov_dense(g, lin, lam):
    """posegraph_cov_ref.dense for block Jacobi on the completed dense system: the dict posegraph_cov_ref.bound reads (Sigma, hinv_norm,
    m_lmax, minv_diag, sigma_max)"""
    H, _ = dense_system(g, lin, lam)
    act = np.repeat(lin["active"], 6)
    Ha = H[np.ix_(act, act)]
    Ha = (Ha + Ha.T) / 2.0
    Sigma = np.zeros_like(H)
    Sigma[np.ix_(act, act)] = np.linalg.inv(Ha)
    D = ref.damped(lin["diag"], lam)[lin["active"]]
    D = (D + np.swapaxes(D, 1, 2)) / 2.0
    minv = np.zeros((g.N, 6))
    minv[lin["active"]] = np.diagonal(np.linalg.inv(D), axis1=1, axis2=2)
    return dict(Sigma=Sigma, hinv_norm=1.0 / float(np.linalg.eigvalsh(Ha)[0]), m_lmax=float(np.linalg.eigvalsh(D).max()),
                minv_diag=minv.reshape(-1), sigma_max=float(np.abs(Sigma).max()))


def optimize(g, P, pcg=ref.pcg, prior_huber_k=0.0, **kw):
    """ref.optimize's loop, its cost and linearization completed by the priors -> (poses, result dict with trace)"""
    c = dict(ref.DEFAULTS)
    c.update(kw)
    poses = g.poses.copy()
    k = c["huber_k"]
    F = cost(g, P, poses, k, prior_huber_k)
    lam = c["lambda_init"]
    res = dict(solves=0, accepted=0, rejected=0, cost_initial=F, pcg_iterations_total=0, stop_reason=None, trace=[])
    if F == 0.0:
        res["stop_reason"] = "cost_zero"
    lin = linearize(g, P, poses, k, prior_huber_k)
    while res["stop_reason"] is None and res["solves"] < c["max_iterations"]:
        delta, its, _, _ = pcg(g, lin, lam, c["pcg_rel_tol"], c["pcg_max_iterations"])
        trial = ref.retract(poses, delta, lin["active"])
        F_new = cost(g, P, trial, k, prior_huber_k)
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
                lin = linearize(g, P, poses, k, prior_huber_k)
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
