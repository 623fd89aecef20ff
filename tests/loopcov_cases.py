"""Fixed inputs of the covariance-model loop-consistency tests (tests/test_loopcov_abi.py, tests/test_loopcov.py), on the builders of
loops_cases.py and posegraph_cases.py: the planted fixture with the honest noise (the step's and the loops' own sigmas, no inflation),
random loops with random covariances over the random chain, and the chains of the prefix sum's edges.  Every generator asserts its own
conditions on the mirror (tests/loopcov_ref.py).  `python tests/loopcov_cases.py` prints the margins for the seeds that were tried."""
import functools
import math

import numpy as np

import loopcov_ref as cref
import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref

S_FLOOR = 1e-9  # the project's sums contract


def s_bound(s_seq, s_pair):
    """The relative bound on s and the band around gamma: max(1e-9, 10 delta_s), delta_s the two float64 mirrors' difference from each
    other in the normalisation of the bound (pairs that are NaN in both are equal)."""
    both = np.isfinite(s_seq) & np.isfinite(s_pair)
    assert np.array_equal(np.isfinite(s_seq), np.isfinite(s_pair))
    delta = float((np.abs(s_seq - s_pair)[both] / np.maximum(1.0, np.abs(s_seq[both]))).max()) if both.any() else 0.0
    return max(S_FLOOR, 10.0 * delta), delta


def in_band(s, gamma, band):
    k, l = np.triu_indices(s.shape[0], 1)
    with np.errstate(invalid="ignore"):
        return int((np.abs(s[k, l] - gamma) <= band * max(1.0, abs(gamma))).sum())


def _mirror(poses, a, b, Z, Sigma, Q):
    """s by the sequential mirror (the reference), the bound from the pairwise one"""
    s = cref.pair_s(poses, a, b, Z, Sigma, cref.chain_W(poses, Q, "sequential"))
    bound, delta = s_bound(s, cref.pair_s(poses, a, b, Z, Sigma, cref.chain_W(poses, Q, "pairwise")))
    return s, bound, delta


# ---------------------------------------------------------------- the planted fixture with the honest noise
HONEST_Q = np.diag([lcases.ODOM_SIGMA_T ** 2] * 3 + [lcases.ODOM_SIGMA_R ** 2] * 3)
HONEST_SIGMA = np.diag([lcases.LOOP_SIGMA_T ** 2] * 3 + [lcases.LOOP_SIGMA_R ** 2] * 3)
HONEST_SCALAR = dict(q_t=lcases.ODOM_SIGMA_T ** 2, q_r=lcases.ODOM_SIGMA_R ** 2)  # the scalar model without its inflation
GAMMA = 16.81
HONEST_SEED = 2  # of 0 .. 5, the seed with the widest margin below gamma (see __main__)
HONEST_MARGIN = 1.0


def _planted_raw(seed):
    """the chain and loops of loops_cases.planted(seed), drawn as it draws them, without its conditions (they hold for its own seed and
    its inflated q_t only)"""
    rng = np.random.default_rng(seed)
    truth = lcases.planted_truth()
    N = lcases.PLANTED_N
    poses = [truth[0]]
    for k in range(N - 1):
        poses.append(poses[-1] @ cases.inv_pose(truth[k]) @ truth[k + 1] @ lcases._noise(rng, lcases.ODOM_SIGMA_R, lcases.ODOM_SIGMA_T))
    poses = np.stack(poses)
    loops = []
    for v in np.sort(rng.choice(N - lcases.PLANTED_PERIOD, lcases.PLANTED_TRUE, replace=False)):
        loops.append((int(v), int(v) + lcases.PLANTED_PERIOD,
                      cases.inv_pose(truth[v]) @ truth[v + lcases.PLANTED_PERIOD] @ lcases._noise(rng, lcases.LOOP_SIGMA_R, lcases.LOOP_SIGMA_T), True))
    for _ in range(lcases.PLANTED_FALSE):
        i = int(rng.integers(0, N))
        j = int((i + rng.integers(1, N)) % N)
        loops.append((i, j, cases.rand_pose(rng, 0.5, 3.0), False))
    order = rng.permutation(len(loops))
    loops = [loops[k] for k in order]
    a, b = np.array([l[0] for l in loops], np.int32), np.array([l[1] for l in loops], np.int32)
    return truth, poses, a, b, np.stack([l[2] for l in loops]), np.array([l[3] for l in loops])


@functools.lru_cache(maxsize=None)
def planted_honest(seed=HONEST_SEED):
    """-> dict(truth, poses, a, b, Z, is_true, Sigma [13, 6, 6], info, Q, gamma, s, adj, bound, ...).  The five conditions the tests rest
    on are asserted here, on the mirror."""
    truth, poses, a, b, Z, is_true = _planted_raw(seed)
    L = len(a)
    Sigma = np.tile(HONEST_SIGMA, (L, 1, 1))
    s, bound, delta = _mirror(poses, a, b, Z, Sigma, HONEST_Q)
    adj = cref.adjacency(s, GAMMA)
    k, l = np.triu_indices(L, 1)
    both = is_true[k] & is_true[l]
    members, _ = lref.greedy(adj)
    size, cliques = lref.max_clique(adj)
    s_scalar = lref.pair_s(poses, a, b, Z, lcases.PLANTED_VAR_T, lcases.PLANTED_VAR_R, **HONEST_SCALAR)
    adj_scalar = lref.adjacency(s_scalar, GAMMA)
    out = dict(truth=truth, poses=poses, a=a, b=b, Z=Z, is_true=is_true, Sigma=Sigma, info=np.tile(np.linalg.inv(HONEST_SIGMA), (L, 1, 1)), Q=HONEST_Q,
               gamma=GAMMA, s=s, adj=adj, bound=bound, delta=delta, true_true_max=float(s[k, l][both].max()),
               with_false_min=float(s[k, l][~both].min()), margin=float(np.abs(s[k, l] - GAMMA).min()), s_scalar=s_scalar, adj_scalar=adj_scalar,
               scalar_true_pairs=int(adj_scalar[k, l][both].sum()), true_pairs=int(both.sum()))
    planted_set = tuple(np.flatnonzero(is_true))
    assert np.isfinite(s).all()
    assert out["true_true_max"] <= GAMMA, out["true_true_max"]                   # 1: the true loops agree with one another
    assert out["with_false_min"] > GAMMA, out["with_false_min"]                  # 2: no false loop agrees with any other loop
    assert tuple(sorted(members)) == planted_set and size == lcases.PLANTED_TRUE and cliques == [planted_set]  # 3: greedy = planted = the maximum
    assert out["margin"] >= HONEST_MARGIN, out["margin"]                         # 4: no pair near the threshold
    assert not lref.is_clique(adj_scalar, planted_set), out["scalar_true_pairs"]  # 5: the scalar model at the same noise loses true pairs
    return out


# ---------------------------------------------------------------- random loops with random covariances over the random chain
SIZES = (1, 2, 63, 64, 65, 129, 257)  # the word and wavefront edges
SIGMA_SCALE, Q_SCALE = 1e-2, 1e-4


def _random_draw(L, seed):
    poses, a, b, Z = lcases._random_loops(L, seed)
    for k in range(L):  # half the loops run backwards along the chain: odd k has a > b, even k has a < b
        if (k % 2 == 1) != (a[k] > b[k]):
            a[k], b[k] = b[k], a[k]
            Z[k] = cases.inv_pose(Z[k])
    rng = np.random.default_rng(seed + 7000)
    Sigma = SIGMA_SCALE * cases.rand_info(rng, L)
    Q = Q_SCALE * cases.rand_info(rng, lcases.CHAIN_N - 1)
    return poses, a, b, Z, Sigma, Q


@functools.lru_cache(maxsize=None)
def random_case(L):
    """-> dict(poses, a, b, Z, Sigma, Q, gamma: the mirror's median s, s, adj, bound, delta, seed).  A draw with a pair inside the band
    around gamma is drawn again with the next seed."""
    for seed in range(2000 + L, 2000 + L + 50):
        poses, a, b, Z, Sigma, Q = _random_draw(L, seed)
        s, bound, delta = _mirror(poses, a, b, Z, Sigma, Q)
        if not np.isfinite(s).all():
            continue
        gamma = lcases.median_gamma(s)
        if in_band(s, gamma, bound) == 0:
            if L >= 2:
                assert (a[1::2] > b[1::2]).all() and (a[0::2] < b[0::2]).all()
            return dict(poses=poses, a=a, b=b, Z=Z, Sigma=Sigma, Q=Q, gamma=gamma, s=s, adj=cref.adjacency(s, gamma), bound=bound, delta=delta, seed=seed)
    raise AssertionError("no draw without a pair in the band")


# ---------------------------------------------------------------- chains
SCAN_BLOCK = 1024  # kLcvScanBlock
CHAIN_SIZES = (1, 2, 3, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 3 * SCAN_BLOCK + 1, 65537)
CHAIN_SHIFT = (1e5, -2e5, 50.0)
CHAIN_NAMES = [f"{n}-{q}" for n in CHAIN_SIZES for q in ("one", "each")] + ["257-shifted"]


def laps(n, seed):
    """a noisy drive in circles: 0.3 m and 2 pi / 4096 rad of yaw per step"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 0.002, (max(n - 1, 0), 3))
    w[:, 2] += 2.0 * math.pi / 4096.0
    steps = np.tile(np.eye(4), (max(n - 1, 0), 1, 1))
    steps[:, :3, :3] = ref.exp_so3(w)
    steps[:, :3, 3] = np.array([0.3, 0.0, 0.0]) + rng.normal(0.0, 0.02, (max(n - 1, 0), 3))
    poses = [cases.rand_pose(rng, 1.0, 5.0)]
    for k in range(n - 1):
        poses.append(poses[-1] @ steps[k])
    return np.stack(poses)


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """-> dict(poses, Q, W: the np.longdouble mirror's, S: its S, delta_W, delta_S): delta the larger of the two float64 mirrors'
    differences from the longdouble one, per node over max(1, max |W_ld[v]|)"""
    size, kind = name.split("-")
    n = int(size)
    rng = np.random.default_rng(3000 + n)
    poses = laps(n, 4000 + n)
    if kind == "shifted":
        poses = poses.copy()
        poses[:, :3, 3] += np.array(CHAIN_SHIFT)
    Q = HONEST_Q.copy() if kind == "one" else Q_SCALE * cases.rand_info(rng, max(n - 1, 1))[:max(n - 1, 0)]
    if kind != "one" and n == 1:
        Q = np.zeros((0, 6, 6))
    W = cref.chain_W(poses, HONEST_Q if Q.size == 0 else Q, "longdouble") if n > 1 else np.zeros((1, 6, 6), np.longdouble)
    S = cref.chain_S(poses, W)
    out = dict(poses=poses, Q=Q, W=W, S=S, n=n)
    for key, full, local in (("delta_W", W, False), ("delta_S", S, True)):
        delta = 0.0
        for order in ("sequential", "pairwise"):
            got = cref.chain_W(poses, Q, order) if n > 1 else np.zeros((1, 6, 6))
            got = cref.chain_S(poses, got) if local else got
            delta = max(delta, float(node_error(got, full).max()))
        out[key] = delta
    return out


def node_error(got, want):
    """per node: max |got - want| / max(1, max |want|)"""
    diff = np.abs(np.asarray(got, dtype=np.longdouble) - want).reshape(want.shape[0], -1).max(1)
    return (diff / np.maximum(1.0, np.abs(want).reshape(want.shape[0], -1).max(1))).astype(np.float64)


if __name__ == "__main__":
    for seed in range(6):
        try:
            p = planted_honest(seed)
            print(f"seed {seed}: true-true s <= {p['true_true_max']:.2f}, with a false loop s >= {p['with_false_min']:.1f}, closest to gamma "
                  f"{p['margin']:.2f}; the scalar model at the honest q keeps {p['scalar_true_pairs']} of {p['true_pairs']} true pairs; "
                  f"delta_s {p['delta']:.2e}")
        except AssertionError as e:
            print(f"seed {seed}: a condition fails ({e})")
    for L in SIZES:
        c = random_case(L)
        print(f"L {L}: seed {c['seed']}, gamma {c['gamma']:.4f}, density {c['adj'].sum() / max(L * (L - 1), 1):.3f}, delta_s {c['delta']:.2e}, "
              f"bound {c['bound']:.2e}")
    for name in CHAIN_NAMES:
        c = chain_case(name)
        print(f"chain {name}: max |W| {float(np.abs(c['W']).max()):.3e}, delta_W {c['delta_W']:.2e}, delta_S {c['delta_S']:.2e}")
