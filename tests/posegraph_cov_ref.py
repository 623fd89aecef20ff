"""Float64 numpy mirror of the pose graph's covariance columns (include/elimaloc_hip_posegraph_cov.h), written from
the contract: per column the conjugate gradients of tests/posegraph_ref.py on a unit right-hand side, every column with its own alpha,
beta, stop test and iteration count and frozen once it has stopped; the dense reference (the inverse of posegraph_ref.dense_system over
the active nodes); the error bound that turns the stop test into an error; the relative covariance and the loop gate on top of them;
and the fixed cases of tests/test_posegraph_cov_abi.py and tests/test_posegraph_cov.py."""
import functools

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

import posegraph_cases as cases
import posegraph_chain_ref as cref
import posegraph_ref as ref

TOL = 1e-10          # elm_posegraph_cov_config_default's pcg_rel_tol
MAX_IT = 20000       # and its pcg_max_iterations
SUMS_FLOOR = 1e-9    # the project's floor for float64 sums in different fixed orders, times the largest |Sigma|
GATE = 16.81         # the 99 % point of chi^2 with 6 degrees of freedom


def sparse_system(g, lin, lam):
    """(H + lam diag H) over all nodes as a CSR matrix from the blocks posegraph_ref.spmv uses, the rows and columns of inactive nodes
    zero: H @ p.reshape(-1) is posegraph_ref.spmv(g, lin, lam, p) for a p that is zero on inactive nodes"""
    N, a = g.N, lin["active"]
    k = np.arange(6)
    D = ref.damped(lin["diag"], lam)
    rows, cols, vals = [], [], []

    def add(vi, vj, blocks, keep):
        r = (6 * vi[:, None, None] + k[None, :, None]) + 0 * k[None, None, :]
        c = (6 * vj[:, None, None] + k[None, None, :]) + 0 * k[None, :, None]
        rows.append(r[keep].ravel())
        cols.append(c[keep].ravel())
        vals.append(blocks[keep].ravel())

    v = np.arange(N)
    add(v, v, D, a)
    if g.E:
        both = a[g.i] & a[g.j]
        add(g.i, g.j, lin["Hij"], both)
        add(g.j, g.i, np.swapaxes(lin["Hij"], 1, 2), both)
    return scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * N, 6 * N)).tocsr()


def columns(g, lin, lam, nodes, tol=TOL, max_it=MAX_IT, precond="block_jacobi"):
    """The conjugate gradients of the contract on the columns (node, 0 .. 5) of `nodes` -> (X [6 N, 6 m], iterations [6 m],
    converged [6 m]).  precond: "block_jacobi", or "chain" (the block-tridiagonal M of tests/posegraph_chain_ref.py, solved by a sparse
    LU).  Every column runs on its own scalars and is frozen when its stop test holds."""
    N, a = g.N, lin["active"]
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    K = 6 * nodes.size
    H = sparse_system(g, lin, lam).tobsr((6, 6))
    Minv = np.zeros((N, 6, 6))
    if a.any():
        Minv[a] = np.linalg.inv(ref.damped(lin["diag"], lam)[a])
    M = scipy.sparse.bsr_matrix((Minv, np.arange(N), np.arange(N + 1)), shape=(6 * N, 6 * N))
    if precond == "chain":
        lu = scipy.sparse.linalg.splu(cref.chain_matrix(g, lin, lam, sparse=True))

        class _Solve:
            def __matmul__(self, R):
                return lu.solve(np.ascontiguousarray(R))
        M = _Solve()
    R = np.zeros((6 * N, K))
    for q, v in enumerate(nodes):
        if a[v]:
            R[6 * v + np.arange(6), 6 * q + np.arange(6)] = 1.0
    X = np.zeros_like(R)
    Z = M @ R
    rz0 = np.sum(R * Z, axis=0)
    conv = (tol > 0.0) & ~(rz0 > 0.0)
    iters = np.zeros(K, np.int64)
    # the live columns are kept side by side (c: their indices) and written back when one of them stops
    c = np.flatnonzero(~conv)
    Xc, Rc, Pc, rz, rzc0 = X[:, c], R[:, c], Z[:, c], rz0[c], rz0[c]
    for it in range(max_it):
        if not c.size:
            break
        Q = H @ Pc
        pq = np.sum(Pc * Q, axis=0)
        alpha = np.where(pq != 0.0, rz / np.where(pq != 0.0, pq, 1.0), 0.0)
        Xc += alpha * Pc
        Rc -= alpha * Q
        Zc = M @ Rc
        rz_new = np.sum(Rc * Zc, axis=0)
        beta = np.where(rz != 0.0, rz_new / np.where(rz != 0.0, rz, 1.0), 0.0)
        Pc = Zc + beta * Pc
        rz = rz_new
        iters[c] = it + 1
        over = (tol > 0.0) & (np.sqrt(rz_new) <= tol * np.sqrt(rzc0))
        if over.any():
            X[:, c] = Xc
            conv[c[over]] = True
            keep = ~over
            c, Xc, Rc, Pc, rz, rzc0 = c[keep], Xc[:, keep], Rc[:, keep], Pc[:, keep], rz[keep], rzc0[keep]
    X[:, c] = Xc
    return X, iters, conv


def blocks(X, nodes, rows):
    """Sigma(row, col) [m, n_rows, 6, 6] from the columns X of `nodes`"""
    nodes, rows = np.asarray(nodes, dtype=np.int64).reshape(-1), np.asarray(rows, dtype=np.int64).reshape(-1)
    N = X.shape[0] // 6
    return X.reshape(N, 6, nodes.size, 6)[rows].transpose(2, 0, 1, 3)


def dense(g, lin, lam, precond="block_jacobi"):
    """The dense reference of one linearization -> dict: Sigma [6 N, 6 N] (the inverse over the active nodes, zero elsewhere),
    hinv_norm = |H^-1|_2, m_lmax = lambda_max(M), minv_diag [6 N] = e^T M^-1 e per column, sigma_max = max |Sigma|; M that of precond"""
    H, _ = ref.dense_system(g, lin, lam)
    act = np.repeat(lin["active"], 6)
    Ha = H[np.ix_(act, act)]
    Ha = (Ha + Ha.T) / 2.0
    Sigma = np.zeros_like(H)
    out = dict(Sigma=Sigma, hinv_norm=0.0, m_lmax=0.0, minv_diag=np.zeros(6 * g.N), sigma_max=0.0)
    if not act.any():
        return out
    Sigma[np.ix_(act, act)] = np.linalg.inv(Ha)
    D = ref.damped(lin["diag"], lam)[lin["active"]]
    D = (D + np.swapaxes(D, 1, 2)) / 2.0
    minv = np.zeros((g.N, 6))
    minv[lin["active"]] = np.diagonal(np.linalg.inv(D), axis1=1, axis2=2)
    out.update(hinv_norm=1.0 / float(np.linalg.eigvalsh(Ha)[0]), m_lmax=float(np.linalg.eigvalsh(D).max()), minv_diag=minv.reshape(-1),
               sigma_max=float(np.abs(Sigma).max()))
    if precond == "chain":
        Ma = cref.chain_matrix(g, lin, lam, sparse=False)[np.ix_(act, act)]
        Ma = (Ma + Ma.T) / 2.0
        md = np.zeros(6 * g.N)
        md[act] = np.diagonal(np.linalg.inv(Ma))
        out.update(m_lmax=float(np.linalg.eigvalsh(Ma)[-1]), minv_diag=md)
    return out


def bound(ref_, nodes, tol=TOL):
    """[6 m]: per column |H^-1|_2 sqrt(lambda_max(M)) tol sqrt(e^T M^-1 e) -- the stop test sqrt(r^T M^-1 r) <= tol sqrt(e^T M^-1 e) gives
    |r|_2 <= sqrt(lambda_max(M)) times its left side, and the error is H^-1 r -- plus the sums floor times the largest |Sigma|"""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    idx = (6 * nodes[:, None] + np.arange(6)[None, :]).reshape(-1)
    return ref_["hinv_norm"] * np.sqrt(ref_["m_lmax"]) * tol * np.sqrt(ref_["minv_diag"][idx]) + SUMS_FLOOR * ref_["sigma_max"]


def dense_blocks(ref_, nodes, rows):
    nodes, rows = np.asarray(nodes, dtype=np.int64).reshape(-1), np.asarray(rows, dtype=np.int64).reshape(-1)
    N = ref_["Sigma"].shape[0] // 6
    return ref_["Sigma"].reshape(N, 6, N, 6)[np.ix_(rows, np.arange(6), nodes, np.arange(6))].transpose(2, 0, 1, 3)


def block_bound(b):
    """the bound [6 m] of the columns as the bound of every entry of blocks [m, ..., 6 (row), 6 (column component)]"""
    return b.reshape(-1, 6)


def relative(poses, a, b, S):
    """A Saa A^T + A Sab B^T + B Sba A^T + B Sbb B^T at Z = T_a^-1 T_b, S(row, col) -> [6, 6] the blocks of the joint covariance"""
    Z = cases.inv_pose(poses[a]) @ poses[b]
    _, A, B = ref.edge_terms(poses[a], poses[b], Z)
    C = ((A @ S(a, a) @ A.T + A @ S(a, b) @ B.T) + B @ S(b, a) @ A.T) + B @ S(b, b) @ B.T
    return 0.5 * (C + C.T)


def gate(poses, a, b, Z, info, S):
    """d2 = r^T (Sigma_rel + info^-1)^-1 r of one candidate loop"""
    r = ref.residual(poses[a], poses[b], Z)
    return float(r @ np.linalg.solve(relative(poses, a, b, S) + np.linalg.inv(info), r))


# ---------------------------------------------------------------- the fixed cases
def hand_two(seed=41):
    """N = 2, node 0 fixed, one edge with a random SPD information, Z exactly T_0^-1 T_1"""
    rng = np.random.default_rng(seed)
    poses = np.stack([cases.rand_pose(rng, 2.0, 5.0), cases.rand_pose(rng, 2.0, 5.0)])
    return ref.Graph(poses, [True, False], [0], [1], (cases.inv_pose(poses[0]) @ poses[1])[None], cases.rand_info(rng, 1))


def _chain_cols(N):
    return [v for v in (0, 31, 32, 255, 256, 257) if v < N - 1] + [N - 1]


# name -> (graph builder, huber_k, lambda, column nodes): every case of the GPU tests that is held against the dense inverse; the
# names of CHAIN_TOO run under the chain preconditioner as well, as case(name + "+chain")
CHAIN_TOO = ("random-7-12", "chain-33", "chain-257", "chain-513")
CASES = {
    "hand-2": (hand_two, 0.0, 0.0, lambda g: [0, 1]),
    "random-7-12": (lambda: cases.random_graph(7, 12, 21), 0.0, 0.0, lambda g: list(range(7))),
    "random-11-25": (lambda: cases.random_graph(11, 25, 22), 0.0, 0.0, lambda g: list(range(11))),
    "chain-33": (lambda: cases.chain(33, 23, loops=3), 0.0, 0.0, lambda g: _chain_cols(33)),
    "chain-257": (lambda: cases.chain(257, 23, loops=3), 0.0, 0.0, lambda g: _chain_cols(257)),
    "chain-513": (lambda: cases.chain(513, 23, loops=3), 0.0, 0.0, lambda g: _chain_cols(513)),
    "star-70": (lambda: cases.star(70, 24), 0.0, 0.0, lambda g: [0, 1, 2, 70]),
    "random-7-12-damped": (lambda: cases.random_graph(7, 12, 21), 0.0, 1e-3, lambda g: list(range(7))),
    "ring-false-huber": (lambda: cases.ring(false_loop=True)[0], 1.0, 0.0, lambda g: [0, 10, 45, 63]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(g, lin, lam, huber_k, nodes, ref (dense), bound [6 m]); computed once per process and shared, never written to"""
    base, _, precond = name.partition("+")
    precond = precond or "block_jacobi"
    build, huber_k, lam, cols = CASES[base]
    g = build()
    lin = ref.linearize(g, huber_k=huber_k)
    nodes = cols(g)
    d = dense(g, lin, lam, precond)
    return dict(g=g, lin=lin, lam=lam, huber_k=huber_k, nodes=nodes, ref=d, bound=bound(d, nodes), precond=precond)


ALL_CASES = list(CASES) + [n + "+chain" for n in CHAIN_TOO]


# ---------------------------------------------------------------- three chain levels: a pure chain of 65 537 nodes
PURE_N = 65537
PURE_NODES = [32768, PURE_N - 1]


@functools.lru_cache(maxsize=None)
def pure_chain(N=PURE_N, seed=25):
    """N poses round and round a circle of 30 m (500 steps of 0.06 m a turn, with a small random roll, pitch and height change per step so
    that all six degrees of freedom take part; built vectorised), the odometry edges k -> k + 1 measured from them without noise, random
    informations, every 1000th node fixed (node 0 among them): H is block tridiagonal, so the chain preconditioner's M is H itself.
    Why not node 0 alone: a chain of 65 536 free nodes has a condition number of 4e9 and more (N^2, times the lever arms), on which two
    float64 direct solves -- the sparse LU of the mirror and the block-Thomas reference -- agree to 7e-7 of the largest |Sigma| only, 50
    times the bound; a random walk of that length has covariances of 1e9 and agrees in no digit.  With a fixed node every 1000 the graph
    still spans three chain levels and every segment boundary, and float64 carries it."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.002, 0.002, (N - 1, 3))
    w[:, 2] += 2.0 * np.pi / 500.0
    step = np.tile(np.eye(4), (N - 1, 1, 1))
    step[:, :3, :3] = ref.exp_so3(w)
    step[:, 0, 3] = 0.06
    step[:, 2, 3] = rng.uniform(-0.002, 0.002, N - 1)
    poses = np.empty((N, 4, 4))
    poses[0] = np.eye(4)
    for k in range(N - 1):
        poses[k + 1] = poses[k] @ step[k]
    poses[:, 3, :] = [0.0, 0.0, 0.0, 1.0]
    Z = np.linalg.inv(poses[:-1]) @ poses[1:]
    return ref.Graph(poses, np.arange(N) % 1000 == 0, np.arange(N - 1), np.arange(1, N), Z, cases.rand_info(rng, N - 1))


def pure_chain_blocks(g, A, B, w, diag):
    """(D [N, 6, 6], U [N - 1, 6, 6]) of the block-tridiagonal H of pure_chain over all nodes, a fixed node's block the identity and its
    couplings zero, from a linearization's A, B, w per edge and diag per node (PoseGraph.Linearization()'s, or the mirror's): U[k]
    couples node k to node k + 1"""
    Hij = w[:, None, None] * (np.swapaxes(A, 1, 2) @ g.info @ B)
    Hij[g.fixed[:-1] | g.fixed[1:]] = 0.0
    return np.where(g.fixed[:, None, None], np.eye(6), diag), Hij


def thomas_columns(D, U, at):
    """Block-Thomas solve of the block-tridiagonal system (diagonal blocks D [n, 6, 6], D[k] coupled to D[k + 1] by U[k]) for the unit
    columns of the block rows `at` -> X [n, 6, 6 len(at)].  The right-hand sides are zero above their block row, so the forward sweep
    starts there; the pivots' inverses are kept for the backward sweep."""
    n, m = D.shape[0], len(at)
    Sinv = np.empty_like(D)
    Y = np.zeros((n, 6, 6 * m))
    for q, v in enumerate(at):
        Y[v, :, 6 * q:6 * q + 6] = np.eye(6)
    Sinv[0] = np.linalg.inv(D[0])
    first = min(at)
    for k in range(1, n):
        L = U[k - 1].T @ Sinv[k - 1]  # M[k][k - 1] S_{k-1}^-1
        Sinv[k] = np.linalg.inv(D[k] - L @ U[k - 1])
        if k > first:
            Y[k] -= L @ Y[k - 1]
    X = np.empty_like(Y)
    X[n - 1] = Sinv[n - 1] @ Y[n - 1]
    for k in range(n - 2, -1, -1):
        X[k] = Sinv[k] @ (Y[k] - U[k] @ X[k + 1])
    return X


def pure_chain_bound(g, lin, X, tol=TOL):
    """[12]: the bound of the columns of PURE_NODES with M = H: the stop test is sqrt(r^T H^-1 r) <= tol sqrt(e^T H^-1 e) = tol sqrt(Sigma_jj)
    and |H^-1 r|_2 <= sqrt(|H^-1|_2) sqrt(r^T H^-1 r); |H^-1|_2 from the smallest eigenvalue by shift-invert Lanczos on the sparse H.  The
    sums floor takes the largest |Sigma| of the solved columns (the variance grows along the chain: the last node's block holds it)."""
    act = np.repeat(lin["active"], 6)
    H = sparse_system(g, lin, 0.0).tocsc()[act][:, act]
    lmin = float(scipy.sparse.linalg.eigsh(H, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    sjj = np.concatenate([np.diagonal(X[v, :, 6 * q:6 * q + 6]) for q, v in enumerate(PURE_NODES)])
    return np.sqrt(1.0 / lmin) * tol * np.sqrt(sjj) + SUMS_FLOOR * float(np.abs(X).max())


GATE_TRUE = (12, 50)   # far apart on the ring, not an edge of the graph
GATE_INFO = 100.0      # the candidates' information: sigma 0.1 m / 0.1 rad, FALSE_INFO_SCALE of posegraph_cases


def gate_candidates():
    """-> (a [3], b [3], Z [3, 4, 4], info [3, 6, 6]) on posegraph_cases.ring(): the true loop GATE_TRUE measured from the truth without
    noise (its residual at the optimum is rounding noise), the same loop measured with a noise of about its sigma (a residual that can be
    compared), and the planted false loop RING_FALSE that claims two far nodes coincide"""
    _, truth = cases.ring()
    a, b = GATE_TRUE
    Zt = cases.inv_pose(truth[a]) @ truth[b]
    Zn = Zt @ cases.rand_pose(np.random.default_rng(43), 0.1, 0.1)
    return (np.array([a, a, cases.RING_FALSE[0]]), np.array([b, b, cases.RING_FALSE[1]]), np.stack([Zt, Zn, np.eye(4)]),
            np.tile(GATE_INFO * np.eye(6), (3, 1, 1)))


def gate_mirror(g, poses):
    """d2 [3] of gate_candidates() under the graph g linearized at `poses`, from the dense inverse"""
    lin = ref.linearize(g, poses)
    Sig = dense(g, lin, 0.0)["Sigma"].reshape(g.N, 6, g.N, 6)
    a, b, Z, info = gate_candidates()
    return np.array([gate(poses, a[k], b[k], Z[k], info[k], lambda r, c: Sig[r, :, c, :]) for k in range(3)])
