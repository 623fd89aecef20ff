"""Fixed inputs of the loop-consistency tests (tests/test_loops_abi.py, tests/test_loops.py), on the builders of posegraph_cases.py: random
loops over a random chain with the threshold at the mirror's median s, and the planted fixture: a drifted odometry chain of 96 poses with
8 true and 5 false loops whose greedy clique, exact maximum clique and planted set are the same.  `python tests/loops_cases.py` prints
the planted fixture's margins for the seeds that were tried."""
import functools
import math

import numpy as np

import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref

BAND = 1e-9  # a pair with |s - gamma| <= BAND max(1, gamma) is not judged bit for bit; the fixtures have none


def in_band(s, gamma):
    k, l = np.triu_indices(s.shape[0], 1)
    return int((np.abs(s[k, l] - gamma) <= BAND * max(1.0, gamma)).sum())


# ---------------------------------------------------------------- random loops over a random chain
SIZES = (1, 2, 63, 64, 65, 128, 129, 257, 1025)  # the word and wavefront edges; more than one loop per lane of the pick tree
CHAIN_N = 64
RANDOM_VAR_T, RANDOM_VAR_R, RANDOM_Q_T, RANDOM_Q_R = 0.1 ** 2, 0.05 ** 2, 0.01 ** 2, 0.005 ** 2


def median_gamma(s):
    """a threshold that cuts the pairs in half without touching one: the midpoint of the two middle values of s (one pair: twice its s;
    none: 1)"""
    k, l = np.triu_indices(s.shape[0], 1)
    v = np.sort(s[k, l])
    if v.size == 0:
        return 1.0
    if v.size == 1:
        return 2.0 * float(v[0])
    return 0.5 * (float(v[v.size // 2 - 1]) + float(v[v.size // 2]))


def _random_loops(L, seed):
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(CHAIN_N - 1):  # the random walk of posegraph_cases.chain
        poses.append(poses[-1] @ cases.rand_pose(rng, 0.4, 2.0))
    poses = np.stack(poses)
    a = rng.integers(0, CHAIN_N, L)
    b = (a + rng.integers(1, CHAIN_N, L)) % CHAIN_N
    Z = np.stack([cases.inv_pose(poses[i]) @ poses[j] @ cases.rand_pose(rng, 0.1, 0.3) for i, j in zip(a, b)])
    return poses, a.astype(np.int32), b.astype(np.int32), Z


@functools.lru_cache(maxsize=None)
def random_case(L):
    """-> dict(poses, a, b, Z, var_t, var_r, q_t, q_r, gamma, s: the mirror's, adj: the mirror's, seed).  A draw with a pair inside the
    band around gamma is drawn again with the next seed."""
    for seed in range(1000 + L, 1000 + L + 50):
        poses, a, b, Z = _random_loops(L, seed)
        s = lref.pair_s(poses, a, b, Z, RANDOM_VAR_T, RANDOM_VAR_R, RANDOM_Q_T, RANDOM_Q_R)
        gamma = median_gamma(s)
        if in_band(s, gamma) == 0:
            return dict(poses=poses, a=a, b=b, Z=Z, var_t=RANDOM_VAR_T, var_r=RANDOM_VAR_R, q_t=RANDOM_Q_T, q_r=RANDOM_Q_R, gamma=gamma, s=s,
                        adj=lref.adjacency(s, gamma), seed=seed)
    raise AssertionError("no draw without a pair in the band")


# ---------------------------------------------------------------- the planted fixture
PLANTED_N, PLANTED_PERIOD, PLANTED_RADIUS = 96, 64, 20.0
PLANTED_TRUE, PLANTED_FALSE = 8, 5
ODOM_SIGMA_T, ODOM_SIGMA_R = 0.02, 0.002
LOOP_SIGMA_T, LOOP_SIGMA_R = 0.03, 0.003
# q_t is inflated over the 0.02 m step noise on purpose: the scalar model has no lever arm, and with q_t = 0.02^2 the true loops reach
# s = 43 among themselves
PLANTED_CFG = dict(q_t=0.05 ** 2, q_r=0.002 ** 2, gamma=16.81)
PLANTED_VAR_T, PLANTED_VAR_R = LOOP_SIGMA_T ** 2, LOOP_SIGMA_R ** 2
PLANTED_SEED = 0
PLANTED_MARGIN = 1.0  # no s closer to gamma than this


def _noise(rng, sigma_r, sigma_t):
    T = np.eye(4)
    T[:3, :3] = ref.exp_so3(rng.normal(0.0, sigma_r, 3))
    T[:3, 3] = rng.normal(0.0, sigma_t, 3)
    return T


def planted_truth():
    truth = []
    for k in range(PLANTED_N):
        ang = 2.0 * math.pi * k / PLANTED_PERIOD
        T = np.eye(4)
        T[:3, :3] = ref.exp_so3(np.array([0.0, 0.0, ang + math.pi / 2.0]))  # heading along the circle
        T[:3, 3] = [PLANTED_RADIUS * math.cos(ang), PLANTED_RADIUS * math.sin(ang), 0.0]
        truth.append(T)
    return np.stack(truth)


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED):
    """-> dict(truth, poses: the integrated noisy odometry, a, b, Z, is_true [13] bool, info [13, 6, 6], var_t, var_r, cfg, s, adj).  The
    four conditions the tests rest on are asserted here, on the mirror."""
    rng = np.random.default_rng(seed)
    truth = planted_truth()
    poses = [truth[0]]
    for k in range(PLANTED_N - 1):
        poses.append(poses[-1] @ cases.inv_pose(truth[k]) @ truth[k + 1] @ _noise(rng, ODOM_SIGMA_R, ODOM_SIGMA_T))
    poses = np.stack(poses)
    loops = []
    for v in np.sort(rng.choice(PLANTED_N - PLANTED_PERIOD, PLANTED_TRUE, replace=False)):
        loops.append((int(v), int(v) + PLANTED_PERIOD, cases.inv_pose(truth[v]) @ truth[v + PLANTED_PERIOD] @ _noise(rng, LOOP_SIGMA_R, LOOP_SIGMA_T), True))
    for _ in range(PLANTED_FALSE):
        i = int(rng.integers(0, PLANTED_N))
        j = int((i + rng.integers(1, PLANTED_N)) % PLANTED_N)
        loops.append((i, j, cases.rand_pose(rng, 0.5, 3.0), False))
    order = rng.permutation(len(loops))
    loops = [loops[k] for k in order]
    a, b = np.array([l[0] for l in loops], np.int32), np.array([l[1] for l in loops], np.int32)
    Z, is_true = np.stack([l[2] for l in loops]), np.array([l[3] for l in loops])
    info = np.tile(np.diag([1.0 / PLANTED_VAR_T] * 3 + [1.0 / PLANTED_VAR_R] * 3), (len(loops), 1, 1))
    s = lref.pair_s(poses, a, b, Z, PLANTED_VAR_T, PLANTED_VAR_R, PLANTED_CFG["q_t"], PLANTED_CFG["q_r"])
    gamma = PLANTED_CFG["gamma"]
    adj = lref.adjacency(s, gamma)
    k, l = np.triu_indices(len(loops), 1)
    both = is_true[k] & is_true[l]
    members, _ = lref.greedy(adj)
    size, cliques = lref.max_clique(adj)
    out = dict(truth=truth, poses=poses, a=a, b=b, Z=Z, is_true=is_true, info=info, var_t=PLANTED_VAR_T, var_r=PLANTED_VAR_R, cfg=dict(PLANTED_CFG),
               s=s, adj=adj, true_true_max=float(s[k, l][both].max()), with_false_min=float(s[k, l][~both].min()),
               margin=float(np.abs(s[k, l] - gamma).min()))
    planted_set = tuple(np.flatnonzero(is_true))
    assert out["true_true_max"] <= gamma, out["true_true_max"]                  # 1: the true loops agree with one another
    assert out["with_false_min"] > gamma, out["with_false_min"]                 # 2: no false loop agrees with any other loop
    assert tuple(sorted(members)) == planted_set and size == PLANTED_TRUE and cliques == [planted_set]  # 3: greedy = planted = the maximum
    assert out["margin"] >= PLANTED_MARGIN, out["margin"]                       # 4: no pair near the threshold
    return out


if __name__ == "__main__":
    for seed in range(6):
        try:
            p = planted(seed)
            print(f"seed {seed}: true-true s <= {p['true_true_max']:.2f}, with a false loop s >= {p['with_false_min']:.1f}, "
                  f"closest to gamma {p['margin']:.2f}")
        except AssertionError as e:
            print(f"seed {seed}: a condition fails ({e})")
    for L in SIZES:
        c = random_case(L)
        print(f"L {L}: seed {c['seed']}, gamma {c['gamma']:.4f}, density {c['adj'].sum() / max(L * (L - 1), 1):.3f}")
