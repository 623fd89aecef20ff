"""The numpy mirror of the registration information (include/elimaloc_hip_reginfo.h): one pair's terms, the 6 x 6
cyclic Jacobi, a job's sums from the pairs it is fed, and the finish.  The pair terms and the finish are written in the operation order of
elimaloc_amd/csrc/elm_dev_reginfo.hpp on Python floats (IEEE float64, no contraction), so that the host's call of that code can be held
to the last bits; what they compute is checked here against plain matrix algebra, finite differences and numpy.linalg.eigh."""
import math

import numpy as np

P2P, GICP, VGICP, AVGICP = 0, 1, 2, 3
METRIC_METHOD, METRIC_PLANE = 0, 1
NO_PAIRS, NO_DOF, DEGENERATE, NON_FINITE = 1, 2, 4, 8


def skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def exp_so3(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    K = skew(np.asarray(w) / th)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def residual(T, p, mu, x=None):
    """e = R^T (mu - t) - p' with p' = Exp(w) p + v the point moved by the right perturbation T <- T [Exp(w) | v], x = [v; w]: the target
    stays in the frame of T, which is the reference's own linearization (registration.cpp:36-41); de/dx = -J."""
    T = np.asarray(T, dtype=np.float64)
    q = T[:3, :3].T @ (np.asarray(mu, dtype=np.float64) - T[:3, 3])
    pp = np.asarray(p, dtype=np.float64)
    if x is not None:
        pp = exp_so3(x[3:]) @ pp + np.asarray(x[:3])
    return q - pp


def jacobian(p):
    """J = [I, -[p]x]"""
    return np.hstack([np.eye(3), -skew(np.asarray(p, dtype=np.float64))])


def metric_plain(T, S, normal, method, metric):
    """M of the contract by plain matrix algebra"""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    if metric == METRIC_PLANE:
        n = R.T @ np.asarray(normal, dtype=np.float64)
        return np.outer(n, n)
    if method == P2P or S is None:
        return np.eye(3)
    S = np.asarray(S, dtype=np.float64).reshape(3, 3)
    return R.T @ (0.5 * (S + S.T)) @ R


def weight_plain(T, p, mu, th, method):
    e = residual(T, p, mu)
    w0 = th * th / (th + float(e @ e)) ** 2
    if method in (VGICP, AVGICP) and w0 < 0.01:
        return 0.0
    return 0.8 * w0 + 0.2 if method == GICP else w0


def tri(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def pair_terms(T, p, mu, S, normal, th, method, metric):
    """(w, J^T M J [6, 6], J^T M e [6], e^T M e) of one pair, unweighted, or None for a pair that contributes nothing: the operations of
    reginfo_pair (elm_dev_reginfo.hpp) one by one."""
    T = np.asarray(T, dtype=np.float64)
    r = [float(T[i, j]) for i in range(3) for j in (0, 1, 2, 3)]  # rows: (R_r0, R_r1, R_r2, t_r)
    px, py, pz = (float(v) for v in p)
    mx, my, mz = (float(v) for v in mu)
    th = float(th)
    d0, d1, d2 = mx - r[3], my - r[7], mz - r[11]
    e0 = ((r[0] * d0 + r[4] * d1) + r[8] * d2) - px
    e1 = ((r[1] * d0 + r[5] * d1) + r[9] * d2) - py
    e2 = ((r[2] * d0 + r[6] * d1) + r[10] * d2) - pz
    en2 = (e0 * e0 + e1 * e1) + e2 * e2
    w0 = (th * th) / ((th + en2) * (th + en2))
    if method in (VGICP, AVGICP) and w0 < 0.01:
        return None
    w = w0 * 0.8 + 0.2 if method == GICP else w0
    m00, m01, m02, m11, m12, m22 = 1.0, 0.0, 0.0, 1.0, 0.0, 1.0
    if metric == METRIC_PLANE:
        nw = [float(v) for v in normal]
        n0 = (r[0] * nw[0] + r[4] * nw[1]) + r[8] * nw[2]
        n1 = (r[1] * nw[0] + r[5] * nw[1]) + r[9] * nw[2]
        n2 = (r[2] * nw[0] + r[6] * nw[1]) + r[10] * nw[2]
        m00, m01, m02, m11, m12, m22 = n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2
    elif method != P2P and S is not None:
        s = [float(v) for v in np.asarray(S, dtype=np.float64).reshape(9)]
        s00, s11, s22 = s[0], s[4], s[8]
        s01, s02, s12 = 0.5 * (s[1] + s[3]), 0.5 * (s[2] + s[6]), 0.5 * (s[5] + s[7])
        a = [[(sr[0] * r[j] + sr[1] * r[4 + j]) + sr[2] * r[8 + j] for j in range(3)] for sr in ((s00, s01, s02), (s01, s11, s12), (s02, s12, s22))]
        mij = lambda i, j: (r[i] * a[0][j] + r[4 + i] * a[1][j]) + r[8 + i] * a[2][j]
        m00, m01, m02, m11, m12, m22 = mij(0, 0), mij(0, 1), mij(0, 2), mij(1, 1), mij(1, 2), mij(2, 2)
    v0 = (m00 * e0 + m01 * e1) + m02 * e2
    v1 = (m01 * e0 + m11 * e1) + m12 * e2
    v2 = (m02 * e0 + m12 * e1) + m22 * e2
    chi = (e0 * v0 + e1 * v1) + e2 * v2
    b00, b01, b02 = m02 * py - m01 * pz, m00 * pz - m02 * px, m01 * px - m00 * py
    b10, b11, b12 = m12 * py - m11 * pz, m01 * pz - m12 * px, m11 * px - m01 * py
    b20, b21, b22 = m22 * py - m12 * pz, m02 * pz - m22 * px, m12 * px - m02 * py
    H = np.zeros((6, 6))
    up = {(0, 0): m00, (0, 1): m01, (0, 2): m02, (1, 1): m11, (1, 2): m12, (2, 2): m22,
          (0, 3): b00, (0, 4): b01, (0, 5): b02, (1, 3): b10, (1, 4): b11, (1, 5): b12, (2, 3): b20, (2, 4): b21, (2, 5): b22,
          (3, 3): py * b20 - pz * b10, (3, 4): py * b21 - pz * b11, (3, 5): py * b22 - pz * b12,
          (4, 4): pz * b01 - px * b21, (4, 5): pz * b02 - px * b22, (5, 5): px * b12 - py * b02}
    for (i, j), v in up.items():
        H[i, j] = H[j, i] = v
    g = np.array([v0, v1, v2, py * v2 - pz * v1, pz * v0 - px * v2, px * v1 - py * v0])
    return w, H, g, chi


def eig6_sym_asc(A):
    """eig6_sym_asc of elm_dev_reginfo.hpp: cyclic Jacobi, eigenvalues ascending, eigenvector k in column k, its largest-magnitude
    component (the first of equals) positive."""
    a = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    v = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    for _ in range(48):
        off = sum(abs(a[i][j]) for i in range(6) for j in range(i + 1, 6))
        dia = sum(abs(a[i][i]) for i in range(6))
        if off <= 1e-300 or off <= 1e-22 * dia:
            break
        for p in range(5):
            for q in range(p + 1, 6):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                th = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                a[p][p] = a[p][p] - t * apq
                a[q][q] = a[q][q] + t * apq
                a[p][q] = a[q][p] = 0.0
                for k in range(6):
                    if k != p and k != q:
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = a[p][k] = c * akp - s * akq
                        a[k][q] = a[q][k] = s * akp + c * akq
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
    w = [a[i][i] for i in range(6)]
    for i in range(5):
        pos = i
        for k in range(i + 1, 6):
            if w[k] < w[pos]:
                pos = k
        if pos != i:
            w[i], w[pos] = w[pos], w[i]
            for r in range(6):
                v[r][i], v[r][pos] = v[r][pos], v[r][i]
    for k in range(6):
        big = 0
        for r in range(1, 6):
            if abs(v[r][k]) > abs(v[big][k]):
                big = r
        if v[big][k] < 0.0:
            for r in range(6):
                v[r][k] = -v[r][k]
    return np.array(w), np.array(v)


def empty_result(n_points, status=NO_PAIRS | DEGENERATE):
    return dict(information=np.zeros((6, 6)), H=np.zeros((6, 6)), g=np.zeros(6), chi2=0.0, sigma2=0.0, length_scale=0.0, eigenvalues=np.zeros(6),
                eigenvectors=np.zeros((6, 6)), n_points=int(n_points), n_pairs=0, n_default=0, dof=0, rank=0, status=status)


def finish(H, g, chi2, sw, swr2, n_pairs, n_default, n_points, metric=METRIC_METHOD, sigma2=0.0, length_scale_m=0.0, min_eigen_ratio=0.0):
    """reginfo_finish of elm_dev_reginfo.hpp"""
    if n_pairs == 0:
        return empty_result(n_points)
    m = 1 if metric == METRIC_PLANE else 3
    r = empty_result(n_points, 0)
    H = np.array(H, dtype=np.float64)
    H = np.triu(H) + np.triu(H, 1).T
    r.update(H=H, g=np.array(g, dtype=np.float64), chi2=float(chi2), n_pairs=int(n_pairs), n_default=int(n_default))
    l = float(length_scale_m) if length_scale_m > 0.0 else math.sqrt(swr2 / sw)
    if not l > 0.0:
        l = 1.0
    dinv = [1.0, 1.0, 1.0, 1.0 / l, 1.0 / l, 1.0 / l]
    S6 = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            S6[i, j] = S6[j, i] = (dinv[i] * float(H[i, j])) * dinv[j]
    lam, V = eig6_sym_asc(S6)
    cut = float(min_eigen_ratio) * float(lam[5])
    keep = [bool(lam[k] > cut and lam[k] > 0.0) for k in range(6)]
    rank = sum(keep)
    dof = m * int(n_pairs) - rank
    status = DEGENERATE if rank < 6 else 0
    s2 = 0.0
    if sigma2 > 0.0:
        s2 = float(sigma2)
    elif dof > 0:
        s2 = float(chi2) / float(dof)
    else:
        status |= NO_DOF
    info = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        if not status & NO_DOF:
            if min_eigen_ratio > 0.0 and rank < 6:
                for i in range(6):
                    for j in range(i, 6):
                        acc = 0.0
                        for k in range(6):
                            if keep[k]:
                                acc += (float(V[i, k]) * float(lam[k])) * float(V[j, k])
                        info[i, j] = info[j, i] = np.float64(np.float64(np.float64(acc) / dinv[i]) / dinv[j]) / np.float64(s2)
            else:
                info = H / np.float64(s2)
    r.update(length_scale=l, eigenvalues=lam, eigenvectors=V, rank=rank, dof=dof, sigma2=s2, information=info, S6=S6)
    fin = all(np.all(np.isfinite(np.asarray(r[k]))) for k in ("information", "H", "g", "chi2", "sigma2", "length_scale", "eigenvalues", "eigenvectors"))
    r["status"] = status | (0 if fin else NON_FINITE)
    return r


def job(T, points, pairs, th, method, metric=METRIC_METHOD, **cfg):
    """A job's result from the pairs it is fed: pairs = [(source index, mu [3], S [3, 3] or None, normal [3] or None, is_default)], the
    pairs of the public GetCorrespondence* calls at g = T p.  The sums are plain running sums in the pairs' order."""
    pts = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    H, g = np.zeros((6, 6)), np.zeros(6)
    chi2 = sw = swr2 = 0.0
    n_pairs = n_default = 0
    for (i, mu, S, normal, dflt) in pairs:
        if dflt and metric == METRIC_PLANE:
            continue
        t = pair_terms(T, pts[i], mu, None if dflt else S, normal, th, method, METRIC_METHOD if dflt else metric)
        if t is None:
            continue
        w, Hp, gp, chi = t
        H += w * Hp
        g += w * gp
        chi2 += w * chi
        sw += w
        swr2 += w * float(pts[i] @ pts[i])
        n_pairs += 1
        n_default += int(bool(dflt))
    return finish(H, g, chi2, sw, swr2, n_pairs, n_default, len(pts), metric=metric, **cfg)


def transform(T, points):
    """g = T p of float32 points, with the association of the kernels: ((T0 px + T4 py) + T8 pz) + T12"""
    T = np.asarray(T, dtype=np.float64)
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)
