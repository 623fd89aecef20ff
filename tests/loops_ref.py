"""Float64 numpy mirror of the loop consistency check (include/elimaloc_hip_loops.h), written from the header: the
pair term on the pose graph's own residual (posegraph_ref.residual), the adjacency, the deterministic greedy clique, the bit packing of
adj_out, and for L <= 16 the exact maximum clique by brute force."""
import numpy as np

import posegraph_ref as ref

GAMMA_DEFAULT = 16.81
DEFAULTS = dict(q_t=0.0, q_r=0.0, gamma=GAMMA_DEFAULT, steps_per_batch=32)
MAX_L, MAX_L_S = 16384, 2048


def _T(a):
    return np.swapaxes(a, -1, -2)


def between(Tu, Tv, dtype=np.float64):
    """X_uv = T_u^-1 T_v = [R_u^T R_v | R_u^T (t_v - t_u)], batched"""
    Tu, Tv = np.asarray(Tu, dtype=dtype), np.asarray(Tv, dtype=dtype)
    out = np.zeros(np.broadcast(Tu, Tv).shape, dtype=dtype)
    Ru = Tu[..., :3, :3]
    out[..., :3, :3] = _T(Ru) @ Tv[..., :3, :3]
    out[..., :3, 3] = (_T(Ru) @ (Tv[..., :3, 3] - Tu[..., :3, 3])[..., None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def predicted(Tak, Tbk, Tal, Tbl, Zl, dtype=np.float64):
    """Zhat = (X_{a_k a_l} Z_l) X_{b_l b_k}"""
    return (between(Tak, Tal, dtype) @ np.asarray(Zl, dtype=dtype)) @ between(Tbl, Tbk, dtype)


def pair_e(Tak, Tbk, Zk, Tal, Tbl, Zl):
    """e [..., 6]: the residual of the edge (I, Zhat, Z_k)"""
    Zh = predicted(Tak, Tbk, Tal, Tbl, Zl)
    return ref.residual(np.broadcast_to(np.eye(4), Zh.shape), Zh, np.asarray(Zk, dtype=np.float64))


def s_of(e, vt_sum, vr_sum, m, q_t, q_r):
    et = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    er = (e[..., 3] * e[..., 3] + e[..., 4] * e[..., 4]) + e[..., 5] * e[..., 5]
    return et / (vt_sum + q_t * m) + er / (vr_sum + q_r * m)


def pair_s(poses, a, b, Z, var_t, var_r, q_t=0.0, q_r=0.0):
    """s [L, L]: symmetric, zero diagonal, every pair evaluated with the lower index as k"""
    poses, Z = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4), np.asarray(Z, dtype=np.float64).reshape(-1, 4, 4)
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    L = a.size
    vt, vr = np.broadcast_to(np.asarray(var_t, dtype=np.float64), (L,)), np.broadcast_to(np.asarray(var_r, dtype=np.float64), (L,))
    s = np.zeros((L, L))
    k, l = np.triu_indices(L, 1)
    if k.size:
        e = pair_e(poses[a[k]], poses[b[k]], Z[k], poses[a[l]], poses[b[l]], Z[l])
        m = (np.abs(a[k] - a[l]) + np.abs(b[k] - b[l])).astype(np.float64)
        s[k, l] = s_of(e, vt[k] + vt[l], vr[k] + vr[l], m, q_t, q_r)
        s[l, k] = s[k, l]
    return s


def adjacency(s, gamma):
    """adj [L, L] bool: s <= gamma off the diagonal, a non-finite s is not adjacent"""
    with np.errstate(invalid="ignore"):
        adj = np.isfinite(s) & (s <= gamma)
    np.fill_diagonal(adj, False)
    return adj


def greedy(adj):
    """-> (members in pick order, degree [L] of the first step)"""
    adj = np.asarray(adj, dtype=bool)
    L = adj.shape[0]
    cand = np.ones(L, bool)
    members, degree0 = [], adj.sum(1).astype(np.int32)
    while cand.any():
        deg = np.where(cand, (adj & cand[None, :]).sum(1), -1)
        v = int(np.argmax(deg))  # the first of the largest: ties go to the lowest index
        members.append(v)
        cand = cand & adj[v]
    return members, degree0


def is_clique(adj, members):
    m = list(members)
    return all(adj[u, v] for i, u in enumerate(m) for v in m[i + 1:])


def is_maximal(adj, members):
    m = list(members)
    return not any(all(adj[u, v] for v in m) for u in range(adj.shape[0]) if u not in m)


def max_clique(adj):
    """the exact maximum cliques of a graph of at most 16 nodes -> (size, every clique of that size as a sorted tuple)"""
    adj = np.asarray(adj, dtype=bool)
    L = adj.shape[0]
    assert L <= 16
    rows = [sum(1 << v for v in range(L) if adj[u, v]) for u in range(L)]
    best, found = 0, []
    for mask in range(1 << L):
        n = bin(mask).count("1")
        if n < best:
            continue
        if all((rows[u] | (1 << u)) & mask == mask for u in range(L) if mask >> u & 1):
            if n > best:
                best, found = n, []
            found.append(tuple(u for u in range(L) if mask >> u & 1))
    return best, found


def pack(adj):
    """adj [L, L] bool -> [L, ceil(L / 64)] uint64: bit l & 63 of word l >> 6"""
    adj = np.asarray(adj, dtype=bool)
    L = adj.shape[0]
    W = (L + 63) // 64
    padded = np.zeros((L, W * 64), np.uint8)
    padded[:, :L] = adj
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(L, W)


def unpack(words, L):
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(L, -1)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)


def refusal(n, a, b, Z, var_t, var_r, q_t=0.0, q_r=0.0, gamma=GAMMA_DEFAULT, steps_per_batch=32, want_s=False):
    """the precondition the header refuses first, or None"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    L = a.size
    if n < 1 or n > 1 << 20:
        return "n"
    if L > MAX_L:
        return "ELM_LOOPS_MAX"
    if want_s and L > MAX_L_S:
        return "ELM_LOOPS_MAX_S"
    if not (np.isfinite(q_t) and q_t >= 0 and np.isfinite(q_r) and q_r >= 0):
        return "q"
    if not (np.isfinite(gamma) and gamma > 0):
        return "gamma"
    if steps_per_batch < 1:
        return "steps_per_batch"
    if ((a < 0) | (a >= n) | (b < 0) | (b >= n)).any():
        return "index"
    if (a == b).any():
        return "a == b"
    if not np.isfinite(np.asarray(Z, dtype=np.float64)).all():
        return "non-finite Z"
    vt, vr = np.broadcast_to(np.asarray(var_t, dtype=np.float64), (L,)), np.broadcast_to(np.asarray(var_r, dtype=np.float64), (L,))
    if not (np.isfinite(vt).all() and np.isfinite(vr).all()):
        return "non-finite variance"
    if (vt <= 0).any() or (vr <= 0).any():
        return "variance <= 0"
    return None
