"""Float64 numpy mirror of the pose graph's linear initialization with the priors in it (include/elimaloc_hip_posegraph_init_prior.h;
DESIGN.md section 28), on top of tests/posegraph_ref.py, tests/posegraph_init_ref.py and tests/posegraph_prior_ref.py, which it leaves
alone: the weights per prior, the classes of the components, the refusals, the gauge nodes, the priors' terms of both problems added in
the contract's order (a node's edges first, then its priors in ascending prior index), the weighted Kabsch alignment, and the whole
sequence S1, S2, alignment, S3 with a direct solve or either conjugate-gradient mirror.  Written from the contract, not from the
library's code."""
import numpy as np
import scipy.sparse.linalg

import posegraph_init_ref as iref
import posegraph_prior_ref as pref
import posegraph_ref as ref

ROT, TRANS = iref.ROT, iref.TRANS
ALIGN_MIN_RATIO = 1e-4
ALIGN_ROW = 28
_T = ref._T


def prior_weights(P):
    """(w_r [P], w_t [P]): trace(Omega_ww) / 3 and trace(Omega_vv) / 3"""
    tr = lambda M: (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    return tr(P.info[:, 3:, 3:]) / 3.0, tr(P.info[:, :3, :3]) / 3.0


def components(g):
    """root [N]: the smallest node of every node's connected component (union-find over the edges)"""
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
    return np.array([find(v) for v in range(g.N)], dtype=np.int64)


def classes(g, P, stages=ROT | TRANS):
    """The host's plan -> dict(refusal: None or which, cls: {root: "fixed" | "prior-anchored" | "aligned" | "free"} of the components
    with edges, gauge [A]: the smallest node of every component on the aligned path, node_comp [N]: its index there or -1, lists: per
    aligned component its priors with w_t > 0 ascending, w_rot / w_pre / w_last [P]: the priors' weights in S1, S2 and S3)"""
    out = dict(refusal=iref.refusal(ref.Graph(g.poses, np.ones(g.N, bool), g.i, g.j, g.Z, g.info), stages), cls={}, gauge=[], lists=[],
               node_comp=np.full(g.N, -1, np.int64), w_rot=np.zeros(P.P), w_pre=np.zeros(P.P), w_last=np.zeros(P.P))
    if out["refusal"] is not None:  # no node, or an edge weight (with every node fixed nothing else is refused there)
        return out
    wr, wt = prior_weights(P)
    root = components(g)
    with_edges = set(int(r) for r in root[g.i])
    for r in sorted(with_edges):
        mine = root[P.node] == r if P.P else np.zeros(0, bool)
        has_wr, has_wt = bool((wr[mine] > 0.0).any()), bool((wt[mine] > 0.0).any())
        c = "fixed" if g.fixed[root == r].any() else "prior-anchored" if has_wr else "aligned" if has_wt else "free"
        out["cls"][r] = c
        if out["refusal"] is not None:
            continue
        if c == "free":
            out["refusal"] = "component without a fixed node or a prior"
        elif c == "prior-anchored" and stages & TRANS and not has_wt:
            out["refusal"] = "prior-anchored component without a translation weight"
        elif c == "aligned" and not stages & TRANS:
            out["refusal"] = "position priors alone cannot give rotations"
        elif c == "aligned" and stages & ROT:
            out["gauge"].append(r)
    if out["refusal"] is not None:
        out["gauge"] = []
        return out
    for k, r in enumerate(out["gauge"]):
        out["node_comp"][root == r] = k
    out["w_rot"], out["w_last"] = np.where(wr > 0.0, wr, 0.0), np.where(wt > 0.0, wt, 0.0)
    in_aligned = out["node_comp"][P.node] >= 0 if P.P else np.zeros(0, bool)
    out["w_pre"] = np.where(in_aligned, 0.0, out["w_last"])
    out["lists"] = [np.flatnonzero((out["node_comp"][P.node] == k) & (out["w_last"] > 0.0)) for k in range(len(out["gauge"]))]
    return out


def _held(g, hold):
    fixed = g.fixed.copy()
    fixed[list(hold)] = True
    return ref.Graph(g.poses, fixed, g.i, g.j, g.Z, g.info)


def _complete(g, lin, P, w, pg, pH):
    """the edges' system completed by the priors' terms, after every edge in ascending prior index; a weight of 0 is not in the stage"""
    grad, diag = lin["grad"].copy(), lin["diag"].copy()
    for q in range(P.P):
        if w[q] > 0.0:
            grad[P.node[q]] += pg[q]
            diag[P.node[q]] += pH[q]
    active = ~g.fixed & (np.abs(diag).reshape(g.N, -1).max(axis=1) > 0.0 if g.N else np.zeros(0, bool))
    lin = dict(lin)
    lin.update(grad=grad, diag=diag, active=active, pg=pg, pH=pH)
    return lin


def rot_terms(P, w, poses):
    """(g_q [P, 6], H_q [P, 6, 6]) of the rotation problem: e_q = y_v - [rho1_Z; rho2_Z], H_q = w I_6, g_q = w e_q"""
    e = iref.rows_of(poses[P.node]) - iref.rows_of(P.Z) if P.P else np.zeros((0, 6))
    return w[:, None] * e, w[:, None, None] * np.eye(6)


def trans_terms(P, w, poses):
    """(g_q, H_q) of the translation problem: u_q = (t_v - t_Z) + R_v l, H_q = w I_6, g_q = [w R_v^T u_q; 0]"""
    g_q = np.zeros((P.P, 6))
    if P.P:
        R, t = poses[P.node, :3, :3], poses[P.node, :3, 3]
        u = (t - P.Z[:, :3, 3]) + (R @ P.lever[..., None])[..., 0]
        g_q[:, :3] = w[:, None] * (_T(R) @ u[..., None])[..., 0]
    return g_q, w[:, None, None] * np.eye(6)


def rot_system(g, P, w, poses=None, hold=()):
    poses = g.poses if poses is None else poses
    gh = _held(g, hold)
    return _complete(gh, iref.rot_system(gh, poses), P, w, *rot_terms(P, w, poses))


def trans_system(g, P, w, poses=None, hold=()):
    poses = g.poses if poses is None else poses
    gh = _held(g, hold)
    return _complete(gh, iref.trans_system(gh, poses), P, w, *trans_terms(P, w, poses))


def direct(g, lin):
    """-> (delta [N, 6], 0, 0.0, True): H delta = -g of the completed system by a direct factorization"""
    if g.N >= iref.SPARSE_FROM:
        H, b = iref.system(g, lin, True)
        return scipy.sparse.linalg.splu(H).solve(b).reshape(g.N, 6), 0, 0.0, True
    H, b = pref.dense_system(g, lin, 0.0)
    return np.linalg.solve(H, b).reshape(g.N, 6), 0, 0.0, True


def kabsch(a, b, w, min_ratio=ALIGN_MIN_RATIO):
    """The weighted rigid alignment of the points a [n, 3] onto b [n, 3] -> dict(ca, cb, S, W, G, sigma, det_uvt, deficient, ratio, row
    [28]): centroids, S = sum w (b - cb)(a - ca)^T in a second pass, S = U Sigma V^T, G = U diag(1, 1, det(U V^T)) V^T"""
    a, b, w = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3), np.asarray(w, dtype=np.float64)
    W = float(w.sum())
    ca, cb = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
    S = np.einsum("q,qr,qc->rc", w, b - cb, a - ca)
    U, sigma, Vt = np.linalg.svd(S)
    d = float(np.linalg.det(U @ Vt))
    G = U @ np.diag([1.0, 1.0, -1.0 if d < 0.0 else 1.0]) @ Vt
    ratio = float(sigma[1] / sigma[0]) if sigma[0] > 0.0 else 0.0
    return dict(ca=ca, cb=cb, S=S, W=W, G=G, sigma=sigma, det_uvt=d, deficient=not sigma[1] > min_ratio * sigma[0], ratio=ratio,
                row=np.concatenate([ca, cb, S.ravel(), [W], G.ravel(), sigma]))


def cost(g, P, poses):
    """edges + priors, both Huber thresholds off"""
    return pref.cost(g, P, poses, 0.0, 0.0)


def _apply_trans(trial, lin, delta):
    a = lin["active"]
    v = np.where(a[:, None], delta[:, :3], 0.0)
    trial[:, :3, 3] = trial[:, :3, 3] + (trial[:, :3, :3] @ v[..., None])[..., 0]
    return v


def initialize(g, P, stages=ROT | TRANS, solver=direct, align_min_ratio=ALIGN_MIN_RATIO):
    """The whole call.  solver(g, lin) -> (delta, iterations, rel_residual, converged) on the completed system of a stage (g carries
    the stage's fixed flags): `direct`, or a conjugate-gradient mirror such as lambda g, lin: ref.pcg(g, lin, 0.0, tol, max_it).
    -> dict(poses: the trial poses, applied, rows, v_pre, v, align [A, 28], degenerate_nodes, rot / pre / trans: (iterations,
    rel_residual, converged), aligned_components, rank_deficient_components, min_align_ratio, cost_before, cost_after, padding: the
    largest |padding solution| of the translation solves, rot_lin / pre_lin / trans_lin, kabsch: the alignments)"""
    plan = classes(g, P, stages)
    assert plan["refusal"] is None, plan["refusal"]
    gauge, A = plan["gauge"], len(plan["gauge"])
    trial = g.poses.copy()
    never = (0, 0.0, False)
    out = dict(rows=iref.rows_of(g.poses), v_pre=np.zeros((g.N, 3)), v=np.zeros((g.N, 3)), align=np.zeros((A, ALIGN_ROW)), degenerate_nodes=0,
               rot=never, pre=never, trans=never, rot_lin=None, pre_lin=None, trans_lin=None, kabsch=[], padding=0.0,
               cost_before=cost(g, P, g.poses), aligned_components=A, rank_deficient_components=0, min_align_ratio=0.0)
    ran = []
    if stages & ROT:
        lin = rot_system(g, P, plan["w_rot"], hold=gauge)
        delta, its, rel, conv = solver(_held(g, gauge), lin)
        a = lin["active"]
        y = iref.rows_of(g.poses)
        y[a] = y[a] + delta[a]
        R, deg = iref.project(y)
        move = a & ~deg
        trial[move, :3, :3] = R[move]
        out.update(rows=y, degenerate_nodes=int((a & deg).sum()), rot=(its, rel, conv), rot_lin=lin)
        ran.append(conv)
    if stages & TRANS:
        lin = trans_system(g, P, plan["w_pre"] if A else plan["w_last"], trial, hold=gauge)
        delta, its, rel, conv = solver(_held(g, gauge), lin)
        v = _apply_trans(trial, lin, delta)
        out["padding"] = max(out["padding"], float(np.abs(delta[:, 3:]).max()) if g.N else 0.0)
        out.update(**({"v_pre": v, "pre": (its, rel, conv), "pre_lin": lin} if A else {"v": v, "trans": (its, rel, conv), "trans_lin": lin}))
        ran.append(conv)
    if A:
        for k, qs in enumerate(plan["lists"]):
            pts = trial[P.node[qs], :3, 3] + (trial[P.node[qs], :3, :3] @ P.lever[qs][..., None])[..., 0]
            K = kabsch(pts, P.Z[qs, :3, 3], plan["w_last"][qs], align_min_ratio)
            out["kabsch"].append(K)
            out["align"][k] = K["row"]
            mine = plan["node_comp"] == k
            trial[mine, :3, :3] = K["G"] @ trial[mine, :3, :3]
            trial[mine, :3, 3] = K["cb"] + (K["G"] @ (trial[mine, :3, 3] - K["ca"])[..., None])[..., 0]
        out["rank_deficient_components"] = sum(K["deficient"] for K in out["kabsch"])
        out["min_align_ratio"] = min(K["ratio"] for K in out["kabsch"])
        lin = trans_system(g, P, plan["w_last"], trial)
        delta, its, rel, conv = solver(g, lin)
        out["v"] = _apply_trans(trial, lin, delta)
        out["padding"] = max(out["padding"], float(np.abs(delta[:, 3:]).max()))
        out.update(trans=(its, rel, conv), trans_lin=lin)
        ran.append(conv)
    out["applied"] = all(ran) and out["rank_deficient_components"] == 0
    out.update(poses=trial, cost_after=cost(g, P, trial))
    return out
