"""Pose graph (include/elimaloc_hip.h "pose graph"): nodes and relative-pose edges resident on the GPU, their SE(3)
linearization, the damped normal equations solved by preconditioned conjugate gradients (block Jacobi, or per object the chain
preconditioner of PoseGraph.SetPreconditioner), and Levenberg-Marquardt around that -- from odometry constraints and loop constraints
to corrected poses; with priors (include/elimaloc_hip_posegraph_prior.h, DESIGN.md section 27: absolute pose and position factors, GNSS
and map matches) to poses in the world frame."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ElmError, PG_PRECOND, PG_STOP, PoseGraphConfigC, PoseGraphLinearizeStatsC, PoseGraphResultC, PoseGraphSolveStatsC,
                   PoseGraphTraceC, PoseGraphInitConfigC, PoseGraphInitResultC, PoseGraphCovConfigC, PoseGraphCovStatsC,
                   PoseGraphInitPriorConfigC, PoseGraphInitPriorResultC, PG_INIT_ALIGN_ROW, check)
from ._marshal import _Owned, _apply, _config, _dp, _pose_block, _ptr
from .context import default_context


def PoseGraphConfig(**kw):
    """elm_posegraph_config with its defaults (20 solves, lambda 1e-4 x10 up / x0.1 down in [1e-12, 1e8], cost_rel_tol 1e-12, step_tol
    1e-10, PCG to 1e-8 in at most 2000 iterations checked every 32, Huber off)."""
    return _config("PoseGraphConfig", PoseGraphConfigC, "elm_posegraph_config_default", kw)


def PoseGraphInitConfig(**kw):
    """elm_posegraph_init_config with its defaults (both solves to 1e-8 in at most 50 000 iterations checked every 32;
    stages = PG_INIT_ROT | PG_INIT_TRANS, or one of them)."""
    return _config("PoseGraphInitConfig", PoseGraphInitConfigC, "elm_posegraph_init_config_default", kw)


def PoseGraphInitPriorConfig(**kw):
    """elm_posegraph_init_prior_config with its defaults: `base` as PoseGraphInitConfig (its fields are keywords here too, e.g.
    pcg_rel_tol=1e-10 or stages=PG_INIT_ROT) and align_min_ratio 1e-4, the smallest sigma_2 / sigma_1 of an alignment that is applied."""
    own = {k: kw.pop(k) for k in ("align_min_ratio", "base") if k in kw}
    cfg = _config("PoseGraphInitPriorConfig", PoseGraphInitPriorConfigC, "elm_posegraph_init_prior_config_default", own)
    _apply(cfg.base, kw, "PoseGraphInitPriorConfig has no field {k}")
    return cfg


def PoseGraphCovConfig(**kw):
    """elm_posegraph_cov_config with its defaults (lambda_ 0, every column to 1e-10 in at most 20 000 iterations checked every 32,
    scratch_bytes 0 = the default cap of 2 GiB)."""
    return _config("PoseGraphCovConfig", PoseGraphCovConfigC, "elm_posegraph_cov_config_default", kw)


def _cov_stats(st):
    return dict(n_columns=int(st.n_columns), n_converged=int(st.n_converged), passes=int(st.passes), iterations_max=int(st.iterations_max),
                rel_residual_max=float(st.rel_residual_max), ms_device=float(st.ms_device), scratch_bytes=int(st.scratch_bytes))


def _nodes(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int32).reshape(-1))


def EdgeTerms(Ti, Tj, Z):
    """(r [6], A [6, 6], B [6, 6]) of one edge: the library's own residual and Jacobians (host only, the code the kernel runs)."""
    r, A, B = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    check(_lib.lib().elm_posegraph_edge_terms(_dp(_pose_block(Ti)), _dp(_pose_block(Tj)), _dp(_pose_block(Z)), _dp(r), _dp(A), _dp(B)), None,
          "elm_posegraph_edge_terms")
    return r, A, B


def PriorTerms(T, Z, lever=None):
    """(r [6], J [6, 6]) of one prior (include/elimaloc_hip_posegraph_prior.h): the library's own residual and Jacobian (host only, the
    code the kernel runs).  lever: the measured point in the node's frame, default zero."""
    r, J = np.zeros(6), np.zeros((6, 6))
    lv = None if lever is None else np.ascontiguousarray(np.asarray(lever, dtype=np.float64).reshape(3))
    check(_lib.lib().elm_posegraph_prior_terms(_dp(_pose_block(T)), _dp(_pose_block(Z)), None if lv is None else _dp(lv), _dp(r), _dp(J)), None,
          "elm_posegraph_prior_terms")
    return r, J


def _per_item(a, n, shape, what):
    """one `shape` block for all n items, or one per item -> contiguous [n, *shape]"""
    a = np.asarray(a, dtype=np.float64)
    a = np.broadcast_to(a, (n,) + shape) if a.ndim == len(shape) else a.reshape((-1,) + shape)
    if a.shape[0] != n:
        raise ElmError(what)
    return np.ascontiguousarray(a)


def _result(res, trace, n):
    out = dict(solves=int(res.solves), accepted=int(res.accepted), rejected=int(res.rejected), cost_initial=float(res.cost_initial),
               cost_final=float(res.cost_final), lambda_final=float(res.lambda_final), pcg_iterations_total=int(res.pcg_iterations_total),
               stop_reason=PG_STOP.get(int(res.stop_reason), int(res.stop_reason)))
    out["trace"] = [dict(cost=float(t.cost), lambda_=float(t.lambda_), accepted=bool(t.accepted), pcg_iterations=int(t.pcg_iterations))
                    for t in trace[:min(n, out["solves"])]]
    return out


def _init_result(res):
    return dict(cost_before=float(res.cost_before), cost_after=float(res.cost_after), rot_iterations=int(res.rot_iterations),
                trans_iterations=int(res.trans_iterations), rot_rel_residual=float(res.rot_rel_residual),
                trans_rel_residual=float(res.trans_rel_residual), rot_converged=bool(res.rot_converged),
                trans_converged=bool(res.trans_converged), degenerate_nodes=int(res.degenerate_nodes), applied=bool(res.applied))


class PoseGraph(_Owned):
    """A pose graph resident on the device (elm_posegraph), of capacities fixed at creation (nodes 1 .. 2^20, edges 1 .. 2^22)."""

    def __init__(self, node_capacity=1024, edge_capacity=4096, ctx=None, prior_capacity=0):
        self.ctx = ctx if ctx is not None else default_context()
        self.node_capacity, self.edge_capacity = int(node_capacity), int(edge_capacity)
        self._h = C.c_void_p()
        check(_lib.lib().elm_posegraph_create(self.ctx._h, self.node_capacity, self.edge_capacity, C.byref(self._h)), self.ctx._h,
              "elm_posegraph_create")
        self.prior_capacity = 0
        if int(prior_capacity) > 0:
            self.ReservePriors(prior_capacity)

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ElmError("PoseGraph: closed")
        return self._h

    def _call(self, name, *args):
        check(getattr(_lib.lib(), name)(self.ctx._h, self._handle(), *args), self.ctx._h, name)

    def Size(self):
        """-> (n_nodes, n_edges)"""
        n, e = C.c_size_t(0), C.c_size_t(0)
        self._call("elm_posegraph_size", C.byref(n), C.byref(e))
        return int(n.value), int(e.value)

    def Reset(self):
        """No nodes, no edges, no priors; the preconditioner kind, the priors' capacity and their Huber threshold stay."""
        self._call("elm_posegraph_reset")

    # ---- priors: absolute pose and position factors (include/elimaloc_hip_posegraph_prior.h)
    def ReservePriors(self, capacity):
        """Room for `capacity` priors (1 .. 2^22), a second device allocation; once per object."""
        self._call("elm_posegraph_reserve_priors", int(capacity))
        self.prior_capacity = int(capacity)

    def PriorCount(self):
        n = C.c_size_t(0)
        self._call("elm_posegraph_prior_count", C.byref(n))
        return int(n.value)

    def AddPriors(self, nodes, Z, information=None, lever=None):
        """Priors (nodes[k], Z[k] ~ T_node with the measured point at lever[k] in the node's frame, information[k] 6 x 6 symmetric in the
        order [v; w], possibly singular; default identity) appended.  information and lever: one for all, or one per prior."""
        v = _nodes(nodes)
        n = v.size
        Zb = _pose_block(Z)
        what = "PoseGraph.AddPriors: one Z, information and lever per prior"
        info = _per_item(np.eye(6) if information is None else information, n, (6, 6), what)
        lv = None if lever is None else _per_item(lever, n, (3,), what)
        if Zb.size != 16 * n:
            raise ElmError(what)
        self._call("elm_posegraph_add_priors", _ptr(v) if n else None, _dp(Zb) if n else None, _dp(lv) if n and lv is not None else None,
                   _dp(info) if n else None, n)

    def AddPositionPriors(self, nodes, positions, information=None, lever=None):
        """Position measurements (GNSS at the antenna `lever`): positions [n, 3] in the world, information 3 x 3 (one for all or one per
        prior, default identity).  Z = [I | p] and a 6 x 6 information whose rotation rows and columns are zero."""
        v = _nodes(nodes)
        n = v.size
        what = "PoseGraph.AddPositionPriors: one position, information and lever per prior"
        p = _per_item(positions, n, (3,), what) if n else np.zeros((0, 3))
        Z = np.tile(np.eye(4), (n, 1, 1))
        Z[:, :3, 3] = p
        info = np.zeros((n, 6, 6))
        info[:, :3, :3] = _per_item(np.eye(3) if information is None else information, n, (3, 3), what)
        self.AddPriors(v, Z, info, lever)

    def Priors(self):
        """The priors as they were added -> dict(node [P], Z [P, 4, 4], lever [P, 3], information [P, 6, 6])."""
        P = self.PriorCount()
        n = max(P, 1)
        node, Z, lever, info = np.zeros(n, np.int32), np.zeros((n, 16)), np.zeros((n, 3)), np.zeros((n, 6, 6))
        self._call("elm_posegraph_get_priors", 0, P, _ptr(node), _dp(Z), _dp(lever), _dp(info))
        return dict(node=node[:P], Z=np.ascontiguousarray(Z[:P].reshape(-1, 4, 4).transpose(0, 2, 1)), lever=lever[:P], information=info[:P])

    def ClearPriors(self):
        """No priors; their capacity and Huber threshold stay."""
        self._call("elm_posegraph_clear_priors")

    def SetPriorHuber(self, k):
        """The priors' own Huber threshold on s_q = r^T Omega r (0, the default: off); kept across Reset."""
        self._call("elm_posegraph_set_prior_huber", float(k))

    def PriorHuber(self):
        k = C.c_double(-1.0)
        self._call("elm_posegraph_get_prior_huber", C.byref(k))
        return float(k.value)

    def PriorLinearization(self):
        """The priors' part of the current linearization -> dict(r [P, 6], J [P, 6, 6], s [P], w [P])."""
        P = self.PriorCount()
        n = max(P, 1)
        r, J, s, w = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros(n), np.zeros(n)
        self._call("elm_posegraph_download_prior_linearization", _dp(r), _dp(J), _dp(s), _dp(w))
        return dict(r=r[:P], J=J[:P], s=s[:P], w=w[:P])

    def SetPreconditioner(self, kind):
        """"block_jacobi" (the default) or "chain": the block-tridiagonal M over the index chain v, v + 1, applied by block cyclic
        reduction on the GPU (include/elimaloc_hip_posegraph_precond.h).  For Solve and Optimize alike; the linearization stays."""
        codes = {v: k for k, v in PG_PRECOND.items()}
        if kind not in codes:
            raise ElmError(f"PoseGraph.SetPreconditioner: {kind!r} is none of {sorted(codes)}")
        self._call("elm_posegraph_set_preconditioner", codes[kind])

    def Preconditioner(self):
        kind = C.c_int(-1)
        self._call("elm_posegraph_get_preconditioner", C.byref(kind))
        return PG_PRECOND[int(kind.value)]

    def AddNodes(self, poses, fixed=None):
        """poses [n, 4, 4] appended; fixed: bool per node (default: all free)."""
        P = _pose_block(poses)
        n = P.size // 16
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
        if fx is not None and fx.size != n:
            raise ElmError("PoseGraph.AddNodes: one fixed flag per node")
        self._call("elm_posegraph_add_nodes", _dp(P) if n else None, _ptr(fx) if n else None, n)

    def SetPoses(self, poses, first=0):
        P = _pose_block(poses)
        self._call("elm_posegraph_set_poses", int(first), P.size // 16, _dp(P) if P.size else None)

    def Poses(self, first=0, count=None):
        """-> poses [count, 4, 4] (default: to the end)"""
        count = self.Size()[0] - int(first) if count is None else int(count)
        if first < 0 or count < 0:
            raise ElmError("PoseGraph.Poses: beyond the graph's nodes")
        out = np.zeros((max(count, 1), 16))
        self._call("elm_posegraph_get_poses", int(first), count, _dp(out))
        return np.ascontiguousarray(out[:count].reshape(-1, 4, 4).transpose(0, 2, 1))

    def SetFixed(self, fixed, first=0):
        fx = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.uint8)
        self._call("elm_posegraph_set_fixed", int(first), fx.size, _ptr(fx) if fx.size else None)

    def AddEdges(self, i, j, Z, information=None):
        """Edges (i[k], j[k], Z[k] ~ T_i^-1 T_j, information[k] 6 x 6 symmetric in the order [v; w], default identity) appended."""
        i = np.ascontiguousarray(np.asarray(i, dtype=np.int32).reshape(-1))
        j = np.ascontiguousarray(np.asarray(j, dtype=np.int32).reshape(-1))
        Zb = _pose_block(Z)
        n = i.size
        info = np.tile(np.eye(6), (n, 1, 1)) if information is None else np.asarray(information, dtype=np.float64)
        info = np.ascontiguousarray(np.broadcast_to(info, (n, 6, 6)) if info.ndim == 2 else info.reshape(-1, 6, 6))
        if j.size != n or Zb.size != 16 * n or info.shape[0] != n:
            raise ElmError("PoseGraph.AddEdges: one j, Z and information per edge")
        self._call("elm_posegraph_add_edges", _ptr(i) if n else None, _ptr(j) if n else None, _dp(Zb) if n else None, _dp(info) if n else None, n)

    def Linearize(self, huber_k=0.0):
        """Residuals, Jacobians, weights and the normal equations' blocks at the current poses -> dict(chi2, cost, grad_inf_norm, n_outliers)."""
        st = PoseGraphLinearizeStatsC()
        self._call("elm_posegraph_linearize", float(huber_k), C.byref(st))
        return dict(chi2=float(st.chi2), cost=float(st.cost), grad_inf_norm=float(st.grad_inf_norm), n_outliers=int(st.n_outliers))

    def Linearization(self):
        """The current linearization -> dict(r [E, 6], A [E, 6, 6], B [E, 6, 6], s [E], w [E], grad [N, 6], diag [N, 6, 6])."""
        N, E = self.Size()
        n, e = max(N, 1), max(E, 1)
        r, A, B, s, w = np.zeros((e, 6)), np.zeros((e, 6, 6)), np.zeros((e, 6, 6)), np.zeros(e), np.zeros(e)
        grad, diag = np.zeros((n, 6)), np.zeros((n, 6, 6))
        self._call("elm_posegraph_download_linearization", _dp(r), _dp(A), _dp(B), _dp(s), _dp(w), _dp(grad), _dp(diag))
        return dict(r=r[:E], A=A[:E], B=B[:E], s=s[:E], w=w[:E], grad=grad[:N], diag=diag[:N])

    def Solve(self, lambda_=0.0, pcg_rel_tol=1e-8, pcg_max_iterations=2000):
        """The step of the current linearization -> (delta [N, 6], dict(iterations, rel_residual, converged))."""
        N = self.Size()[0]
        delta = np.zeros((max(N, 1), 6))
        st = PoseGraphSolveStatsC()
        self._call("elm_posegraph_solve", float(lambda_), float(pcg_rel_tol), int(pcg_max_iterations), _dp(delta), C.byref(st))
        return delta[:N], dict(iterations=int(st.iterations), rel_residual=float(st.rel_residual), converged=bool(st.converged))

    def Optimize(self, cfg=None, trace_cap=64):
        """Levenberg-Marquardt from the current poses, which it replaces -> dict(solves, accepted, rejected, cost_initial, cost_final,
        lambda_final, pcg_iterations_total, stop_reason, trace: per solve dict(cost, lambda_, accepted, pcg_iterations))."""
        cfg = cfg if cfg is not None else PoseGraphConfig()
        res = PoseGraphResultC()
        trace = (PoseGraphTraceC * max(int(trace_cap), 1))()
        self._call("elm_posegraph_optimize", C.byref(cfg), C.byref(res), trace, int(trace_cap))
        return _result(res, trace, int(trace_cap))

    def Initialize(self, cfg=None, return_stages=False):
        """The linear initialization (include/elimaloc_hip_posegraph_init.h): the rotations from one linear least-squares problem on
        their first two rows, projected back to SO(3), then the translations from an exactly linear one, both by the conjugate gradients
        and the preconditioner of this object.  Priors are ignored: the conditions, the two problems and the costs are those of the
        edges and the fixed nodes alone (InitializeWithPriors uses them).  The poses are replaced only if every requested stage converged -> dict(cost_before,
        cost_after, rot_iterations, trans_iterations, rot_rel_residual, trans_rel_residual, rot_converged, trans_converged,
        degenerate_nodes, applied); with return_stages also rows [N, 6] (the solved rows before the projection) and v [N, 3]."""
        cfg = cfg if cfg is not None else PoseGraphInitConfig()
        res = PoseGraphInitResultC()
        N = self.Size()[0] if return_stages else 0
        rows, v = np.zeros((max(N, 1), 6)), np.zeros((max(N, 1), 3))
        self._call("elm_posegraph_initialize", C.byref(cfg), C.byref(res), _dp(rows) if return_stages else None, _dp(v) if return_stages else None)
        out = _init_result(res)
        if return_stages:
            out["rows"], out["v"] = rows[:N], v[:N]
        return out

    def InitializeWithPriors(self, cfg=None, return_stages=False):
        """The linear initialization with the priors in it (include/elimaloc_hip_posegraph_init_prior.h): Initialize's two problems with
        every prior's term added, for graphs that priors hold and no fixed node does.  A component held by position priors alone is
        solved with its smallest node as gauge, moved rigidly onto its positions (weighted Kabsch) and its translations solved again with
        the priors in.  The poses are replaced only if every solve converged and no alignment is rank-deficient (fewer than three
        positions, or collinear ones) -> Initialize's dict (trans_*: the last translation solve; the costs count the priors, Huber off)
        plus pre_iterations, pre_rel_residual, pre_converged, aligned_components, rank_deficient_components, min_align_ratio; with
        return_stages also rows [N, 6], v_pre [N, 3], v [N, 3] and align [aligned_components, 28] (c_a, c_b, S, W, G, sigma)."""
        cfg = cfg if cfg is not None else PoseGraphInitPriorConfig()
        res = PoseGraphInitPriorResultC()
        N = self.Size()[0] if return_stages else 0
        n = max(N, 1)
        rows, v_pre, v = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros((n, 3))
        # an aligned component has an edge, so two nodes, and a prior of its own: no more of them than N / 2 or than the priors
        cap = min(N // 2, self.PriorCount()) if return_stages else 0
        align = np.zeros((max(cap, 1), PG_INIT_ALIGN_ROW))
        stage = lambda a: _dp(a) if return_stages else None
        self._call("elm_posegraph_initialize_priors", C.byref(cfg), C.byref(res), stage(rows), stage(v_pre), stage(v), stage(align), cap)
        out = _init_result(res.base)
        out.update(pre_iterations=int(res.pre_iterations), pre_rel_residual=float(res.pre_rel_residual), pre_converged=bool(res.pre_converged),
                   aligned_components=int(res.aligned_components), rank_deficient_components=int(res.rank_deficient_components),
                   min_align_ratio=float(res.min_align_ratio))
        if return_stages:
            out.update(rows=rows[:N], v_pre=v_pre[:N], v=v[:N], align=align[:out["aligned_components"]])
        return out

    def Covariance(self, cols, rows=None, cfg=None):
        """Blocks of the inverse of the current linearization's normal equations (include/elimaloc_hip_posegraph_cov.h), in the tangent
        [v; w] -> (diag [m, 6, 6]: Sigma(col, col) symmetrised, cross [m, n_rows, 6, 6]: Sigma(row, col) as solved, info: the call's
        stats plus iterations [m, 6] and converged [m, 6] per column).  An inactive node has zero blocks.  The object's preconditioner is
        honoured."""
        cfg = cfg if cfg is not None else PoseGraphCovConfig()
        cols, rows = _nodes(cols), _nodes([] if rows is None else rows)
        m, n = cols.size, rows.size
        diag, cross = np.zeros((max(m, 1), 6, 6)), np.zeros((max(m, 1), max(n, 1), 6, 6))
        its, conv = np.zeros((max(m, 1), 6), np.int32), np.zeros((max(m, 1), 6), np.uint8)
        st = PoseGraphCovStatsC()
        self._call("elm_posegraph_covariance", _ptr(cols) if m else None, m, _ptr(rows) if n else None, n, C.byref(cfg), _dp(diag),
                   _dp(cross) if n else None, _ptr(its), _ptr(conv), C.byref(st))
        info = _cov_stats(st)
        info["iterations"], info["converged"] = its[:m], conv[:m].astype(bool)
        return diag[:m], cross[:m, :n], info

    def Marginals(self, nodes, cfg=None, return_stats=False):
        """The marginal covariances [m, 6, 6] of the given nodes under the current linearization (with return_stats also Covariance's
        info)."""
        diag, _, info = self.Covariance(nodes, None, cfg)
        return (diag, info) if return_stats else diag

    def RelativeCovariance(self, a, b, cfg=None, return_stats=False):
        """The covariance [L, 6, 6] of the residual coordinates of T_a^-1 T_b at the current poses, from the joint covariance of the
        two nodes and the edge Jacobians."""
        cfg = cfg if cfg is not None else PoseGraphCovConfig()
        a, b = _nodes(a), _nodes(b)
        if a.size != b.size:
            raise ElmError("PoseGraph.RelativeCovariance: one b per a")
        out = np.zeros((max(a.size, 1), 6, 6))
        st = PoseGraphCovStatsC()
        self._call("elm_posegraph_relative_covariance", _ptr(a) if a.size else None, _ptr(b) if a.size else None, a.size, C.byref(cfg), _dp(out),
                   C.byref(st))
        return (out[:a.size], _cov_stats(st)) if return_stats else out[:a.size]

    def _destroy(self, h):
        _lib.lib().elm_posegraph_destroy(h)


def LoopGate(pg, a, b, Z, information, cfg=None):
    """The Mahalanobis distance of candidate loops (a[k], b[k], Z[k], information[k]) to the current estimate of pg -> d2 [L]:
    d2 = r^T (Sigma_rel + information^-1)^-1 r with r the residual of EdgeTerms(T_a, T_b, Z) and Sigma_rel PoseGraph.RelativeCovariance.
    Under the model d2 of a true loop is chi^2 with 6 degrees of freedom (16.81 is its 99 % point).  numpy on top of RelativeCovariance;
    pg needs a valid linearization at the poses it holds."""
    a, b = _nodes(a), _nodes(b)
    L = a.size
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4, 4)
    info = np.asarray(information, dtype=np.float64)
    info = np.broadcast_to(info, (L, 6, 6)) if info.ndim == 2 else info.reshape(-1, 6, 6)
    if b.size != L or Z.shape[0] != L or info.shape[0] != L:
        raise ElmError("LoopGate: one b, Z and information per a")
    if not L:
        return np.zeros(0)
    S = pg.RelativeCovariance(a, b, cfg)
    nodes = np.unique(np.concatenate([a, b]))
    T = {int(v): pg.Poses(int(v), 1)[0] for v in nodes}
    d2 = np.zeros(L)
    for k in range(L):
        r, _, _ = EdgeTerms(T[int(a[k])], T[int(b[k])], Z[k])
        d2[k] = float(r @ np.linalg.solve(S[k] + np.linalg.inv(info[k]), r))
    return d2
