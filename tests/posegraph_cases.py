"""Fixed inputs of the pose-graph tests (tests/test_posegraph_abi.py, tests/test_posegraph.py): random graphs of given sizes, stars of a
given hub degree, the rotation family across the series switch and near pi, the two hand cases, and the loop fixture: 64 poses on a
circle, noise-free odometry, three loop edges from the truth, the start drifted.  `python tests/posegraph_cases.py` runs the mirror on
the loop fixtures, prints their traces and, when the conditions the tests assert hold, writes tests/golden/posegraph_ring.npz."""
import math
import os

import numpy as np

import posegraph_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_ring.npz")


def rand_pose(rng, ang, tr):
    """a rotation by up to `ang` rad about a random axis and a translation in [-tr, tr]^3"""
    w = rng.normal(size=3)
    w *= ang * rng.uniform() / np.linalg.norm(w)
    T = np.eye(4)
    T[:3, :3] = ref.exp_so3(w)
    T[:3, 3] = rng.uniform(-tr, tr, 3)
    return T


def rand_info(rng, n):
    """n exactly symmetric positive definite 6 x 6 matrices"""
    M = rng.normal(size=(n, 6, 6))
    S = M @ np.swapaxes(M, 1, 2) + 0.5 * np.eye(6)
    return (S + np.swapaxes(S, 1, 2)) / 2.0


def inv_pose(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def _measure(poses, i, j, rng, rot_noise=0.05, tr_noise=0.1):
    return np.stack([inv_pose(poses[a]) @ poses[b] @ rand_pose(rng, rot_noise, tr_noise) for a, b in zip(i, j)]) if len(i) else np.zeros((0, 4, 4))


def random_graph(N, E, seed, offset=0.0, fixed=(0,), ang=3.0):
    """N random poses, E edges between random distinct nodes (i > j about half the time), noisy measurements, random information"""
    rng = np.random.default_rng(seed)
    poses = np.stack([rand_pose(rng, ang, 20.0) for _ in range(N)])
    poses[:, :3, 3] += offset
    i = rng.integers(0, N, E) if N > 1 else np.zeros(0, np.int64)
    j = (i + rng.integers(1, N, E)) % N if N > 1 else np.zeros(0, np.int64)
    fx = np.zeros(N, bool)
    fx[list(fixed)] = True
    return ref.Graph(poses, fx, i, j, _measure(poses, i, j, rng), rand_info(rng, len(i)))


def chain(N, seed, loops=3, info_random=True):
    """a random walk of N nodes: odometry edges k -> k + 1, `loops` random loop edges (the first written j -> i), node 0 fixed; every
    node has an edge, the start is the truth disturbed"""
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(N - 1):
        poses.append(poses[-1] @ rand_pose(rng, 0.4, 2.0))
    poses = np.stack(poses)
    i, j = list(range(N - 1)), list(range(1, N))
    for k in range(loops if N > 3 else 0):
        a = int(rng.integers(0, N - 2))
        b = int(rng.integers(a + 2, N))
        i.append(b if k == 0 else a)
        j.append(a if k == 0 else b)
    Z = _measure(poses, i, j, rng, 0.02, 0.05)
    start = np.stack([T @ rand_pose(rng, 0.05, 0.2) for T in poses])
    fx = np.zeros(N, bool)
    fx[0] = True
    return ref.Graph(start, fx, i, j, Z, rand_info(rng, len(i)) if info_random else None)


def wild_chain():
    """a chain of 12 nodes started so far off (rotations wrong by up to 2.5 rad) that the mirror rejects the plain Gauss-Newton step:
    F_new / F = 5.4 at lambda 0, 5.2 at 1e-5, then accepted steps at 0.19 and 0.52"""
    g = chain(12, 4, info_random=False)
    rng = np.random.default_rng(104)
    g.poses = np.stack([g.poses[0]] + [T @ rand_pose(rng, 2.5, 3.0) for T in g.poses[1:]])
    return g


def star(degree, seed):
    """a hub (node 0) of the given degree: edges alternately hub -> leaf and leaf -> hub; leaf 1 is fixed"""
    rng = np.random.default_rng(seed)
    N = degree + 1
    poses = np.stack([rand_pose(rng, 3.0, 10.0) for _ in range(N)])
    leaves = np.arange(1, N)
    i = np.where(leaves % 2 == 1, 0, leaves)
    j = np.where(leaves % 2 == 1, leaves, 0)
    fx = np.zeros(N, bool)
    fx[1] = True
    return ref.Graph(poses, fx, i, j, _measure(poses, i, j, rng), rand_info(rng, degree))


ROT_FAMILY = (0.0, 1e-12, 1.9e-8, 2.1e-8, 1e-5, 9.9e-3, 1e-2, 1.01e-2, 0.5, 1.0, 3.0, math.pi - 1e-3, math.pi - 1e-6)


def rotation_family(seed=5):
    """one edge per angle of ROT_FAMILY (either side of the small-n branch of Log at 2e-8, of the series switch at 1e-2, and near pi):
    the edge's rotation residual has that angle about a random axis"""
    rng = np.random.default_rng(seed)
    n = len(ROT_FAMILY)
    poses = np.stack([rand_pose(rng, 3.0, 10.0) for _ in range(2 * n)])
    i, j = np.arange(n), np.arange(n, 2 * n)
    Z = []
    for k, th in enumerate(ROT_FAMILY):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        E = np.eye(4)
        E[:3, :3] = ref.exp_so3(-th * ax)  # Z = T_i^-1 T_j Exp(-phi): R_E = R_Z^T R_i^T R_j = Exp(phi)
        E[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        Z.append(inv_pose(poses[i[k]]) @ poses[j[k]] @ E)
    fx = np.zeros(2 * n, bool)
    fx[0] = True
    return ref.Graph(poses, fx, i, j, np.stack(Z), rand_info(rng, n))


def hand_integers():
    """identity rotations, integer translations, Omega = I: r_R = 0 and r_t the integer difference, exactly.  Edge 0 has s = 4."""
    poses = np.tile(np.eye(4), (4, 1, 1))
    poses[:, :3, 3] = [[0, 0, 0], [3, -2, 5], [7, 7, -1], [-4, 0, 2]]
    i, j = np.array([0, 1, 3, 2]), np.array([1, 2, 0, 3])
    Z = np.tile(np.eye(4), (4, 1, 1))
    Z[:, :3, 3] = [[3, -2, 3], [1, 9, -6], [5, 0, -2], [-11, -4, 0]]
    want_rt = np.array([[0, 0, 2], [3, 0, 0], [-1, 0, 0], [0, -3, 3]], np.float64)
    fx = np.array([True, False, False, False])
    return ref.Graph(poses, fx, i, j, Z, None), want_rt


RING_N, RING_RADIUS = 64, 20.0
RING_LOOPS = ((0, 63), (5, 40), (20, 58))
RING_FALSE = (10, 45)
RING_CFG = dict(max_iterations=20, pcg_rel_tol=1e-10, pcg_max_iterations=1000, step_tol=1e-7)
# exactly five solves: Huber's reweighting converges linearly, so the run is cut by the solve count and not by a tolerance that a last
# digit could meet one solve earlier or later
FALSE_CFG = dict(max_iterations=5, pcg_rel_tol=1e-10, pcg_max_iterations=1000, step_tol=0.0, cost_rel_tol=0.0, huber_k=1.0)
FALSE_INFO_SCALE = 100.0  # the true edges' information there (sigma 0.1 m / 0.1 rad); the false edge keeps the identity
DRIFT_SEED = 1


def ring(drift_seed=DRIFT_SEED, false_loop=False):
    """-> (Graph at the drifted start, truth [64, 4, 4]).  The truth runs along a circle of 20 m, facing along it, with a gentle roll,
    pitch and height wave so that all six degrees of freedom take part; odometry edges Z = T_k^-1 T_k+1 and the loop edges come from
    the truth without noise; the start is the odometry integrated with one fixed drift per step (a fraction of a degree and a few
    millimetres, drawn from drift_seed); node 0 is fixed.  false_loop adds one loop edge that claims two far nodes coincide, with the
    identity as its information against FALSE_INFO_SCALE times the identity on the true edges."""
    truth = []
    for k in range(RING_N):
        a = 2.0 * math.pi * k / RING_N
        T = np.eye(4)
        yaw = ref.exp_so3(np.array([0.0, 0.0, a + math.pi / 2.0]))
        tilt = ref.exp_so3(np.array([0.03 * math.sin(2 * a), 0.02 * math.cos(3 * a), 0.0]))
        T[:3, :3] = yaw @ tilt
        T[:3, 3] = [RING_RADIUS * math.cos(a), RING_RADIUS * math.sin(a), 0.5 * math.sin(a)]
        truth.append(T)
    truth = np.stack(truth)
    i = list(range(RING_N - 1)) + [a for a, _ in RING_LOOPS]
    j = list(range(1, RING_N)) + [b for _, b in RING_LOOPS]
    Z = [inv_pose(truth[a]) @ truth[b] for a, b in zip(i, j)]
    if false_loop:
        i.append(RING_FALSE[0])
        j.append(RING_FALSE[1])
        Z.append(np.eye(4))
    rng = np.random.default_rng(drift_seed)
    D = np.eye(4)
    D[:3, :3] = ref.exp_so3(rng.uniform(-1.0, 1.0, 3) * math.radians(0.15))
    D[:3, 3] = rng.uniform(-1.0, 1.0, 3) * 0.004
    start = [truth[0]]
    for k in range(RING_N - 1):
        start.append(start[-1] @ Z[k] @ D)
    fx = np.zeros(RING_N, bool)
    fx[0] = True
    info = None
    if false_loop:
        info = np.tile(FALSE_INFO_SCALE * np.eye(6), (len(i), 1, 1))
        info[-1] = np.eye(6)
    return ref.Graph(np.stack(start), fx, i, j, np.stack(Z), info), truth


def mirror_ring():
    """the mirror's Levenberg-Marquardt on both loop fixtures -> dict of arrays (the content of the golden file)"""
    out = {}
    for name, false_loop, cfg in (("ring", False, RING_CFG), ("false", True, FALSE_CFG)):
        g, truth = ring(false_loop=false_loop)
        poses, res = ref.optimize(g, **cfg)
        out[name + "_start"], out[name + "_poses"] = g.poses, poses
        out[name + "_cost"] = np.array([t["cost"] for t in res["trace"]])
        out[name + "_lambda"] = np.array([t["lambda_"] for t in res["trace"]])
        out[name + "_accepted"] = np.array([t["accepted"] for t in res["trace"]], np.uint8)
        out[name + "_ratio"] = np.array([t["ratio"] for t in res["trace"]])
        out[name + "_pcg"] = np.array([t["pcg_iterations"] for t in res["trace"]], np.int32)
        out[name + "_cost_initial"], out[name + "_cost_final"] = np.array(res["cost_initial"]), np.array(res["cost_final"])
        out[name + "_stop"] = np.array(res["stop_reason"])
    out["truth"] = truth
    return out


def ring_conditions(g):
    """the conditions the loop test rests on, for the mirror's run g (mirror_ring())"""
    every_step_accepted = bool(g["ring_accepted"].all())
    clear = bool((np.abs(g["ring_ratio"] - 1.0) > 1e-3).all())
    dt, dr = ref.pose_error(g["ring_poses"], g["truth"])
    return every_step_accepted, clear, dt, dr


if __name__ == "__main__":
    g = mirror_ring()
    for name in ("ring", "false"):
        print(name, "start error", ref.pose_error(g[name + "_start"], g["truth"]), "end error", ref.pose_error(g[name + "_poses"], g["truth"]),
              "stop", g[name + "_stop"], "cost", float(g[name + "_cost_initial"]), "->", float(g[name + "_cost_final"]))
        for k in range(len(g[name + "_cost"])):
            print("  solve", k, "cost", g[name + "_cost"][k], "ratio", g[name + "_ratio"][k], "lambda", g[name + "_lambda"][k], "accepted",
                  int(g[name + "_accepted"][k]), "pcg", int(g[name + "_pcg"][k]))
    acc, clear, dt, dr = ring_conditions(g)
    ok = acc and clear and dt <= 1e-4 and dr <= 1e-5
    print("conditions met:", ok, (acc, clear, dt, dr))
    if ok:
        np.savez_compressed(GOLDEN, **g)
