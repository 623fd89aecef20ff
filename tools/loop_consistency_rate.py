"""Loop-consistency cost on one GPU: prints ONE JSON line and writes it to profiles/loop_consistency_rate.json.

The planted fixture of tests/loops_cases.py at scale: 4 096 poses on four laps of a circle (period 1 024, 1 m between neighbours), the
odometry integrated with N(0, 0.01 m) and N(0, 1e-4 rad) per step (at 0.002 rad the heading drift over
a lap times the lever arm, which the scalar model does not carry, leaves only a dozen true loops mutually consistent); L loops, L in 256, 2 048 and 16 384, half of them true -- (v, v +
1 024 m) from the truth with 0.03 m / 0.003 rad noise -- and half false: random pairs with a random Z of about 0.5 rad and 3 m; the
order shuffled; var_t = 0.03^2, var_r = 0.003^2, q_t = 0.05^2, q_r = 0.002^2, gamma = 16.81.  Reported per L: the call's wall clock
(median of --reps), the device time of the pair kernel and of the greedy loop separately (the stream events elm_loops_consistency
records around them), the clique's size, the greedy steps, the adjacent pairs and how many members are true loops; and beside them
a single-thread host loop over elm_loops_pair_terms: --host-pairs pairs k < l of the same loops timed one call each, less the time of
as many calls that return at their first argument check (the binding's own cost), scaled to the L (L - 1) / 2 pairs of the upper
triangle (the kernel evaluates both triangles).  Nothing here is a requirement; the figures are recorded.

    python tools/loop_consistency_rate.py [--reps 5] [--sizes 256,2048,16384] [--host-pairs 20000] [--out profiles/loop_consistency_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_POSES, PERIOD = 4096, 1024
VAR_T, VAR_R = 0.03 ** 2, 0.003 ** 2
CFG = dict(q_t=0.05 ** 2, q_r=0.002 ** 2, gamma=16.81)


def rotvec(w):
    w = np.asarray(w, dtype=np.float64)
    ang = np.linalg.norm(w, axis=-1)
    ax = w / np.where(ang > 0.0, ang, 1.0)[..., None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -ax[..., 2], ax[..., 1], ax[..., 2], -ax[..., 0], -ax[..., 1], ax[..., 0]
    return np.eye(3) + np.sin(ang)[..., None, None] * K + (1.0 - np.cos(ang))[..., None, None] * (K @ K)


def noise(rng, n, sigma_r, sigma_t):
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = rotvec(rng.normal(0.0, sigma_r, (n, 3)))
    T[:, :3, 3] = rng.normal(0.0, sigma_t, (n, 3))
    return T


def fixture(L, seed=0, sigma_r=1e-4, sigma_t=0.01):
    """sigma_r, sigma_t: the odometry's noise per step (the defaults are this tool's own fixture)"""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(N_POSES) / PERIOD
    radius = PERIOD / (2.0 * np.pi)
    truth = np.tile(np.eye(4), (N_POSES, 1, 1))
    truth[:, :3, :3] = rotvec(np.stack([0.0 * a, 0.0 * a, a + np.pi / 2.0], 1))
    truth[:, 0, 3], truth[:, 1, 3] = radius * np.cos(a), radius * np.sin(a)
    step = np.linalg.inv(truth[:-1]) @ truth[1:] @ noise(rng, N_POSES - 1, sigma_r, sigma_t)
    poses = np.empty_like(truth)
    poses[0] = truth[0]
    for k in range(N_POSES - 1):
        poses[k + 1] = poses[k] @ step[k]
    n_true = L // 2
    laps = rng.integers(1, N_POSES // PERIOD, n_true)
    ta = rng.integers(0, N_POSES - laps * PERIOD)
    tb = ta + laps * PERIOD
    tZ = np.linalg.inv(truth[ta]) @ truth[tb] @ noise(rng, n_true, 0.003, 0.03)
    fa = rng.integers(0, N_POSES, L - n_true)
    fb = (fa + rng.integers(1, N_POSES, L - n_true)) % N_POSES
    fZ = noise(rng, L - n_true, 0.5 / np.sqrt(3.0), 3.0 / np.sqrt(3.0))
    order = rng.permutation(L)
    ia, ib = np.concatenate([ta, fa])[order].astype(np.int32), np.concatenate([tb, fb])[order].astype(np.int32)
    return poses, ia, ib, np.concatenate([tZ, fZ])[order], (np.arange(L) < n_true)[order]


def host_pair_ns(poses, a, b, Z, n_pairs, seed=1):
    """ns per pair of the host-only call, the binding's own cost per call subtracted"""
    from elimaloc_amd import _lib
    from elimaloc_amd._marshal import _pose_block
    fn = _lib.lib().elm_loops_pair_terms
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(a) - 1, n_pairs)
    l = rng.integers(k + 1, len(a))
    P, Zb = _pose_block(poses).reshape(-1, 16), _pose_block(Z).reshape(-1, 16)
    dp = C.POINTER(C.c_double)
    ptr = lambda block, idx: [block[i:i + 1].ctypes.data_as(dp) for i in idx]
    args = list(zip(ptr(P, a[k]), ptr(P, b[k]), ptr(Zb, k), ptr(P, a[l]), ptr(P, b[l]), ptr(Zb, l)))
    e = np.zeros(6)
    pe = e.ctypes.data_as(dp)
    full, empty = [], []
    for _ in range(3):  # the smaller of three passes each: the difference of two loops of a few microseconds per call is noisy
        t0 = time.perf_counter()
        for q in args:
            fn(*q, pe)
        t1 = time.perf_counter()
        for q in args:
            fn(None, q[1], q[2], q[3], q[4], q[5], pe)
        t2 = time.perf_counter()
        full.append(t1 - t0)
        empty.append(t2 - t1)
    return 1e9 * (min(full) - min(empty)) / n_pairs, 1e9 * min(empty) / n_pairs


def measure(sizes, reps, host_pairs):
    from elimaloc_amd.loops import LoopConsistency, LoopConsistencyConfig
    from elimaloc_amd.registration import Context
    ctx = Context(0)
    cfg = LoopConsistencyConfig(**CFG)
    out = {}
    for L in sizes:
        poses, a, b, Z, is_true = fixture(L)
        LoopConsistency(poses, a, b, Z, VAR_T, VAR_R, cfg, ctx)  # warm-up
        wall, adj_ms, greedy_ms = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = LoopConsistency(poses, a, b, Z, VAR_T, VAR_R, cfg, ctx)
            wall.append(1e3 * (time.perf_counter() - t0))
            adj_ms.append(res["adjacency_ms"])
            greedy_ms.append(res["greedy_ms"])
        ns, call_ns = host_pair_ns(poses, a, b, Z, min(host_pairs, L * (L - 1) // 2))
        upper = L * (L - 1) // 2
        out[f"loops_{L}"] = dict(
            loops=L, poses=N_POSES, call_ms=float(np.median(wall)), adjacency_ms=float(np.median(adj_ms)), greedy_ms=float(np.median(greedy_ms)),
            pairs_evaluated=L * L, adjacency_ns_per_pair=1e6 * float(np.median(adj_ms)) / (L * L), size=res["size"], steps=res["steps"],
            adjacent_pairs=res["adjacent_pairs"], true_loops=int(is_true.sum()), members_true=int(is_true[res["members"]].sum()),
            host_ns_per_pair=ns, host_binding_ns_per_call=call_ns, host_ms_upper_triangle=1e-6 * ns * upper)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="256,2048,16384")
    ap.add_argument("--host-pairs", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_consistency_rate.json"))
    a = ap.parse_args()
    rows = measure([int(s) for s in a.sizes.split(",")], a.reps, a.host_pairs)
    line = json.dumps(dict(tool="loop_consistency_rate", reps=a.reps, **rows))
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
