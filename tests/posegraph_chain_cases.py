"""Fixed inputs of the chain-preconditioner tests (tests/test_posegraph_chain_abi.py, tests/test_posegraph_chain.py), on the builders of
tests/posegraph_cases.py: chains of the sizes at which the block cyclic reduction changes path (its segment is 256 nodes; one, two and
three levels), chains broken by a fixed interior node and by a missing odometry edge, a chain edge stored reversed, a duplicate chain
edge, and the graphs without any chain."""
import numpy as np

import posegraph_cases as cases
import posegraph_ref as ref

SEGMENT = 256                      # elm_internal.hpp: kPgcSeg
THREE_LEVELS = SEGMENT * SEGMENT + 1  # the first size whose second level has two segments


def _with(g, poses=None, fixed=None, i=None, j=None, Z=None, info=None):
    return ref.Graph(g.poses if poses is None else poses, g.fixed if fixed is None else fixed, g.i if i is None else i, g.j if j is None else j,
                     g.Z if Z is None else Z, g.info if info is None else info)


def fixed_interior(N=12, seed=2, at=5):
    """chain(N) with the interior node `at` fixed as well: the chain breaks on both of its sides"""
    g = cases.chain(N, seed)
    fx = g.fixed.copy()
    fx[at] = True
    return _with(g, fixed=fx)


def missing_edge(N=12, seed=2, at=6):
    """chain(N) without the odometry edge at -> at + 1; an edge at - 1 -> at + 1 keeps the far part tied to the fixed node"""
    g = cases.chain(N, seed)
    keep = np.arange(g.E) != at
    rng = np.random.default_rng(seed + 100)
    extra = cases.inv_pose(g.poses[at - 1]) @ g.poses[at + 1] @ cases.rand_pose(rng, 0.02, 0.05)
    return _with(g, i=np.append(g.i[keep], at - 1), j=np.append(g.j[keep], at + 1), Z=np.concatenate([g.Z[keep], extra[None]]),
                 info=np.concatenate([g.info[keep], cases.rand_info(rng, 1)]))


def reversed_edge(N=12, seed=2, at=4):
    """chain(N) with the odometry edge at -> at + 1 stored as at + 1 -> at (the inverse measurement)"""
    g = cases.chain(N, seed)
    i, j, Z = g.i.copy(), g.j.copy(), g.Z.copy()
    i[at], j[at], Z[at] = g.j[at], g.i[at], cases.inv_pose(g.Z[at])
    return _with(g, i=i, j=j, Z=Z)


def duplicate_edge(N=12, seed=2, at=3):
    """chain(N) and, appended, a second edge between at and at + 1, stored reversed with its own measurement and information: the chain
    edge is the first, the second counts in the diagonal blocks alone"""
    g = cases.chain(N, seed)
    rng = np.random.default_rng(seed + 200)
    Z2 = cases.inv_pose(g.poses[at + 1]) @ g.poses[at] @ cases.rand_pose(rng, 0.02, 0.05)
    return _with(g, i=np.append(g.i, at + 1), j=np.append(g.j, at), Z=np.concatenate([g.Z, Z2[None]]), info=np.concatenate([g.info, cases.rand_info(rng, 1)]))


def isolated_free_node():
    g = cases.random_graph(9, 12, 32)
    poses = np.concatenate([g.poses, g.poses[:1] @ cases.rand_pose(np.random.default_rng(1), 1.0, 5.0)[None]])
    return ref.Graph(poses, np.append(g.fixed, False), g.i, g.j, g.Z, g.info)  # node 9: free, no edge


def long_chain(N, seed, loops):
    """cases.chain's kind of graph for large N, drawn in batches: a random walk, odometry edges, `loops` loop edges, node 0 fixed"""
    rng = np.random.default_rng(seed)

    def noise(n, ang, tr):
        w = rng.normal(size=(n, 3))
        w *= (ang * rng.uniform(size=n) / np.linalg.norm(w, axis=1))[:, None]
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, :3, :3] = ref.exp_so3(w)
        T[:, :3, 3] = rng.uniform(-tr, tr, (n, 3))
        return T

    steps = noise(N - 1, 0.4, 2.0)
    poses = np.empty((N, 4, 4))
    poses[0] = np.eye(4)
    for k in range(N - 1):
        poses[k + 1] = poses[k] @ steps[k]
    a = rng.integers(0, N - 2, loops)
    b = a + 2 + (rng.integers(0, N, loops) % (N - a - 2))
    i, j = np.concatenate([np.arange(N - 1), a]), np.concatenate([np.arange(1, N), b])
    Z = np.linalg.inv(poses[i]) @ poses[j] @ noise(i.size, 0.02, 0.05)
    fx = np.zeros(N, bool)
    fx[0] = True
    return ref.Graph(poses @ noise(N, 0.05, 0.2), fx, i, j, Z, cases.rand_info(rng, i.size))


SIZES = {
    "N1_fixed": lambda: ref.Graph(np.eye(4)[None], [True], [], [], np.zeros((0, 4, 4))),
    "N2": lambda: cases.chain(2, 1, loops=0),
    "N3": lambda: cases.chain(3, 5, loops=0),
    "N255": lambda: cases.chain(SEGMENT - 1, 41, loops=4),
    "N256": lambda: cases.chain(SEGMENT, 42, loops=4),
    "N257": lambda: cases.chain(SEGMENT + 1, 43, loops=4),
    "N512": lambda: cases.chain(2 * SEGMENT, 44, loops=4),
    "N513": lambda: cases.chain(2 * SEGMENT + 1, 45, loops=4),
    "N8193": lambda: cases.chain(8193, 40, loops=20),  # the 8 193-node chain of tests/test_posegraph.py
}
SPECIAL = {
    "fixed_interior": fixed_interior,
    "missing_edge": missing_edge,
    "reversed_edge": reversed_edge,
    "duplicate_edge": duplicate_edge,
    "star5": lambda: cases.star(5, 3),
    "isolated_free_node": isolated_free_node,
    "all_fixed": lambda: cases.random_graph(6, 8, 33, fixed=range(6)),
}
SMALL = {"two": lambda: cases.chain(2, 1, loops=0), "chain12": lambda: cases.chain(12, 2), "star5": lambda: cases.star(5, 3),
         "random9": lambda: cases.random_graph(9, 20, 4, fixed=(0, 4), ang=0.3), "fixed_interior": fixed_interior, "missing_edge": missing_edge,
         "reversed_edge": reversed_edge, "duplicate_edge": duplicate_edge}
# (N, seed, loops) of cases.chain for which the mirror's PCG at lambda = 0 reaches 1e-10 within 12 loops + 1 iterations in float64.  The
# bound is one of exact arithmetic; in float64 the finite termination is delayed by rounding on most graphs: of the seeds 1 .. 60 it
# holds for 9 at (24, 1 loop), 7 at (40, 2), 4 at (64, 3) and none at (128, 4), the others needing up to twice the bound.  These seeds
# take 13, 16 and 35 iterations.
RANK_BOUND = ((24, 14, 1), (40, 8, 2), (64, 36, 3))
