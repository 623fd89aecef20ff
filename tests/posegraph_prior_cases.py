"""Fixed inputs of the pose-graph prior tests (tests/test_posegraph_prior_abi.py, tests/test_posegraph_prior.py): random priors on the
graphs of tests/posegraph_cases.py, the hand case, and the two anchored-ring fixtures -- the 64-node ring of posegraph_cases.ring() with
its odometry edges only and NO fixed node, the start moved rigidly away on top of its drift, position priors at an antenna on every 8th
node; and the same ring with one position 30 m off under the priors' Huber threshold.  `python tests/posegraph_prior_cases.py` runs the
mirror on both, prints their traces and, when the conditions the tests assert hold, writes tests/golden/posegraph_prior_ring.npz."""
import os

import numpy as np

import posegraph_cases as cases
import posegraph_prior_ref as pref
import posegraph_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_prior_ring.npz")


def rand_priors(g, n, seed, kind="mixed", nodes=None, lever_max=2.0, rot_noise=0.05, tr_noise=0.1):
    """n priors on random nodes of g (or on `nodes`): Z the node's pose at the lever point, disturbed; kind "pose" (full random
    information), "position" (R_Z = I, the rotation rows and columns of the information zero) or "mixed" (alternately)"""
    rng = np.random.default_rng(seed)
    node = rng.integers(0, g.N, n) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
    lever = rng.uniform(-lever_max, lever_max, (n, 3))
    info = cases.rand_info(rng, n)
    Z = np.zeros((n, 4, 4))
    for q in range(n):
        T = g.poses[node[q]]
        noise = cases.rand_pose(rng, rot_noise, tr_noise)
        Z[q] = np.eye(4)
        Z[q, :3, 3] = T[:3, 3] + T[:3, :3] @ lever[q] + noise[:3, 3]
        position = kind == "position" or (kind == "mixed" and q % 2 == 1)
        if position:
            info[q, 3:, :] = 0.0
            info[q, :, 3:] = 0.0
        else:
            Z[q, :3, :3] = T[:3, :3] @ noise[:3, :3]
    return pref.Priors(node, Z, lever, info)


def one_node():
    """one free node, no edge, one full-rank pose prior with a lever arm"""
    g = ref.Graph(cases.rand_pose(np.random.default_rng(60), 2.0, 5.0)[None], [False], [], [], np.zeros((0, 4, 4)))
    return g, rand_priors(g, 1, 61, kind="pose", nodes=[0])


def counted(P_count, seed):
    g = cases.random_graph(40, 65, seed)
    return g, rand_priors(g, P_count, seed + 1000)


def node_counts():
    """nodes with 1, 2, 64, 65 and 70 priors among nodes with none, the priors of the five nodes interleaved"""
    g = cases.random_graph(12, 20, 70)
    nodes = np.repeat([3, 5, 7, 8, 9], [1, 2, 64, 65, 70])
    np.random.default_rng(71).shuffle(nodes)
    return g, rand_priors(g, nodes.size, 72, nodes=nodes)


def node_without_edges():
    """node 9 is free and has no edge: its three priors make it active"""
    g = cases.random_graph(9, 12, 32)
    poses = np.concatenate([g.poses, g.poses[:1] @ cases.rand_pose(np.random.default_rng(1), 1.0, 5.0)[None]])
    g = ref.Graph(poses, np.append(g.fixed, False), g.i, g.j, g.Z, g.info)
    return g, rand_priors(g, 5, 73, nodes=[9, 2, 9, 4, 9])


def fixed_node():
    g = cases.random_graph(6, 10, 74)  # node 0 is fixed
    return g, rand_priors(g, 4, 75, nodes=[0, 3, 0, 5])


def duplicates():
    g = cases.random_graph(6, 10, 76)
    P = rand_priors(g, 3, 77)
    return g, P.take([0, 1, 0, 2, 1, 0])


def star_hub():
    g = cases.star(65, 24)
    return g, rand_priors(g, 9, 78, nodes=[0, 0, 5, 0, 0, 17, 0, 0, 0])


def far_away():
    g = cases.random_graph(30, 60, 34, offset=1e5)
    return g, rand_priors(g, 20, 79)


def rotation_family(seed=80):
    """one pose prior per angle of posegraph_cases.ROT_FAMILY: its rotation residual has that angle about a random axis"""
    rng = np.random.default_rng(seed)
    n = len(cases.ROT_FAMILY)
    g = cases.random_graph(n, 2 * n, 81)
    Z = np.zeros((n, 4, 4))
    lever = rng.uniform(-2.0, 2.0, (n, 3))
    for k, th in enumerate(cases.ROT_FAMILY):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        T = g.poses[k]
        Z[k] = np.eye(4)
        Z[k, :3, :3] = T[:3, :3] @ ref.exp_so3(-th * ax)  # R_E = R_Z^T R_v = Exp(phi)
        Z[k, :3, 3] = T[:3, 3] + T[:3, :3] @ lever[k] + rng.uniform(-0.1, 0.1, 3)
    return g, pref.Priors(np.arange(n), Z, lever, cases.rand_info(rng, n))


def hand_integers():
    """identity rotations, integer translations and lever arms, diagonal informations of small integers: r, J = [I, -[l]x; 0, I] and s
    are exact.  -> (Graph of three free nodes without edges, Priors, r [3, 6], s [3])"""
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, :3, 3] = [[1, 2, 3], [-4, 0, 5], [7, -7, 0]]
    g = ref.Graph(poses, [False] * 3, [], [], np.zeros((0, 4, 4)))
    lever = np.array([[1.0, -2.0, 3.0], [0.0, 0.0, 0.0], [2.0, 1.0, -1.0]])
    Z = np.tile(np.eye(4), (3, 1, 1))
    Z[:, :3, 3] = [[1, 0, 4], [-4, 0, 5], [10, -8, 1]]
    info = np.stack([np.diag([1.0, 2.0, 3.0, 1.0, 1.0, 1.0]), np.diag([4.0, 4.0, 1.0, 0.0, 0.0, 0.0]), np.diag([2.0, 1.0, 1.0, 3.0, 2.0, 1.0])])
    want_r = np.zeros((3, 6))
    want_r[:, :3] = [[1, 0, 2], [0, 0, 0], [-1, 2, -2]]  # t + l - t_Z
    want_s = np.array([13.0, 0.0, 10.0])                 # 1 + 3 * 4;  0;  2 + 4 + 4
    return g, pref.Priors([0, 1, 2], Z, lever, info), want_r, want_s


# ---------------------------------------------------------------- the anchored ring
ANCHOR_EVERY = 8
ANCHOR_LEVER = (0.5, -0.2, 1.2)
ANCHOR_INFO = np.diag([4.0, 4.0, 1.0])
ANCHOR_SHIFT_M, ANCHOR_TURN_RAD = 3.7, 0.2
ANCHOR_CFG = dict(cases.RING_CFG)
# the outlier: informations 100 I on edges and positions, one position 30 m off, the priors' threshold 1; the solve count fixed as
# posegraph_cases.FALSE_CFG fixes it (no tolerance that a last digit could meet one solve earlier or later), the edges' Huber off
OUTLIER_SOLVES = 6  # the fewest after which every other prior is an inlier again (5 leave prior 4 at s = 1.7; at 6 it has s = 0.72)
OUTLIER_CFG = dict(cases.FALSE_CFG, huber_k=0.0, max_iterations=OUTLIER_SOLVES)
OUTLIER_PRIOR_HUBER = 1.0
OUTLIER_AT, OUTLIER_SHIFT_M = 3, 30.0  # the prior (of node 24) whose position is moved
OUTLIER_DIRECTION = (0.6, 0.8, 0.0)   # ... along this unit vector: at the end every other prior is an inlier again (weight 1)


def anchored_ring(drift_seed=cases.DRIFT_SEED, every=ANCHOR_EVERY, outlier=False):
    """-> (Graph, Priors, truth): the odometry edges of posegraph_cases.ring() alone, no fixed node; the drifted start moved rigidly by
    ANCHOR_SHIFT_M and ANCHOR_TURN_RAD; position priors from the truth, without noise, at the antenna ANCHOR_LEVER on every `every`-th
    node.  outlier: the informations of edges and positions are FALSE_INFO_SCALE times the identity and prior OUTLIER_AT lies
    OUTLIER_SHIFT_M off."""
    g, truth = cases.ring(drift_seed)
    n = cases.RING_N - 1
    move = np.eye(4)
    move[:3, :3] = ref.exp_so3(np.array([0.0, 0.0, ANCHOR_TURN_RAD]))
    d = np.array([3.0, -2.0, 0.8])
    move[:3, 3] = d * (ANCHOR_SHIFT_M / np.linalg.norm(d))
    info = np.tile(cases.FALSE_INFO_SCALE * np.eye(6), (n, 1, 1)) if outlier else None
    g = ref.Graph(move @ g.poses, np.zeros(cases.RING_N, bool), g.i[:n], g.j[:n], g.Z[:n], info)
    node = np.arange(0, cases.RING_N, every)
    lever = np.array(ANCHOR_LEVER)
    pos = truth[node, :3, 3] + truth[node, :3, :3] @ lever
    if outlier:
        pos[OUTLIER_AT] += OUTLIER_SHIFT_M * np.array(OUTLIER_DIRECTION)
    P = pref.Priors.positions(node, pos, cases.FALSE_INFO_SCALE * np.eye(3) if outlier else ANCHOR_INFO, lever)
    return g, P, truth


def fixed_and_priors():
    """posegraph_cases.chain(12, 2), node 0 fixed, with seven mixed priors"""
    g = cases.chain(12, 2)
    return g, rand_priors(g, 7, 90)


def priors_only():
    """the same chain without a fixed node, tied to the world by nine pose priors"""
    g = cases.chain(12, 2)
    g.fixed[:] = False
    return g, rand_priors(g, 9, 91, kind="pose")


def _record(out, name, g, poses, res):
    out[name + "_start"], out[name + "_poses"] = g.poses, poses
    out[name + "_cost"] = np.array([t["cost"] for t in res["trace"]])
    out[name + "_lambda"] = np.array([t["lambda_"] for t in res["trace"]])
    out[name + "_accepted"] = np.array([t["accepted"] for t in res["trace"]], np.uint8)
    out[name + "_ratio"] = np.array([t["ratio"] for t in res["trace"]])
    out[name + "_pcg"] = np.array([t["pcg_iterations"] for t in res["trace"]], np.int32)
    out[name + "_cost_initial"], out[name + "_cost_final"] = np.array(res["cost_initial"]), np.array(res["cost_final"])
    out[name + "_stop"] = np.array(res["stop_reason"])


def mirror_rings():
    """the mirror's Levenberg-Marquardt on both fixtures, and on the outlier with the threshold off -> dict of arrays (the content of
    the golden file)"""
    out = {}
    g, P, truth = anchored_ring()
    poses, res = pref.optimize(g, P, **ANCHOR_CFG)
    _record(out, "anchor", g, poses, res)
    g, P, _ = anchored_ring(outlier=True)
    poses, res = pref.optimize(g, P, prior_huber_k=OUTLIER_PRIOR_HUBER, **OUTLIER_CFG)
    _record(out, "outlier", g, poses, res)
    poses, res = pref.optimize(g, P, prior_huber_k=0.0, **OUTLIER_CFG)
    _record(out, "plain", g, poses, res)
    out["truth"] = truth
    return out


def anchor_conditions(run):
    every_step_accepted = bool(run["anchor_accepted"].all())
    clear = bool((np.abs(run["anchor_ratio"] - 1.0) > 1e-3).all())
    dt, dr = ref.pose_error(run["anchor_poses"], run["truth"])
    dt0, _ = ref.pose_error(run["anchor_start"], run["truth"])
    return every_step_accepted, clear, dt, dr, dt0


def outlier_conditions(run):
    """(every step accepted, the planted prior the only one with a weight below 0.1 at the end, error with the threshold, error without)"""
    g, P, truth = anchored_ring(outlier=True)
    w = pref.linearize(g, P, run["outlier_poses"], 0.0, OUTLIER_PRIOR_HUBER)["pw"]
    only = bool(w[OUTLIER_AT] < 0.1 and (np.delete(w, OUTLIER_AT) >= 0.1).all())
    return bool(run["outlier_accepted"].all()), only, ref.pose_error(run["outlier_poses"], truth)[0], ref.pose_error(run["plain_poses"], truth)[0]


if __name__ == "__main__":
    run = mirror_rings()
    for name in ("anchor", "outlier", "plain"):
        print(name, "start error", ref.pose_error(run[name + "_start"], run["truth"]), "end error", ref.pose_error(run[name + "_poses"], run["truth"]),
              "stop", run[name + "_stop"], "cost", float(run[name + "_cost_initial"]), "->", float(run[name + "_cost_final"]))
        for k in range(len(run[name + "_cost"])):
            print("  solve", k, "cost", run[name + "_cost"][k], "ratio", run[name + "_ratio"][k], "lambda", run[name + "_lambda"][k], "accepted",
                  int(run[name + "_accepted"][k]), "pcg", int(run[name + "_pcg"][k]))
    acc, clear, dt, dr, dt0 = anchor_conditions(run)
    oacc, only, d_on, d_off = outlier_conditions(run)
    ok = acc and clear and dt <= 1e-4 and dr <= 1e-5 and dt0 > 1.0 and oacc and only and d_on < d_off
    print("conditions met:", ok, (acc, clear, dt, dr, dt0), (oacc, only, d_on, d_off))
    if ok:
        np.savez_compressed(GOLDEN, **run)
