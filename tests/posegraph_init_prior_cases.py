"""Fixed inputs of the tests of the pose graph's initialization with priors (tests/test_posegraph_init_prior_abi.py,
tests/test_posegraph_init_prior.py): the noisy open chain that position priors alone correct, the graph with one component of every
class, chains and rings with a given number of priors, and the recording.  `python tests/posegraph_init_prior_cases.py` runs the mirror
(tests/posegraph_init_prior_ref.py) on the recorded fixtures, prints their figures and writes tests/golden/posegraph_init_prior.npz."""
import os

import numpy as np

import posegraph_cases as cases
import posegraph_init_prior_ref as ipref
import posegraph_prior_cases as pcases
import posegraph_prior_ref as pref
import posegraph_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_init_prior.npz")

GNSS_N, GNSS_EVERY = 200, 10
GNSS_LEVER = (0.5, -0.2, 1.2)
GNSS_INFO = 400.0


def _pose(w, t):
    T = np.eye(4)
    T[:3, :3] = ref.exp_so3(np.asarray(w, dtype=np.float64))
    T[:3, 3] = t
    return T


def gnss_chain():
    """-> (Graph, Priors, truth): 200 nodes on a gentle helix, odometry with noise as the only edges, no fixed node, the start turned by
    1 rad and moved by (50, -20, 3), noisy position priors at an antenna on every 10th node: the priors are the only correction"""
    step = _pose((0.002, 0.001, 0.03), (1.0, 0.0, 0.01))
    rng = np.random.default_rng(5)
    truth, Z = [np.eye(4)], []
    for _ in range(GNSS_N - 1):
        truth.append(truth[-1] @ step)
        nr = rng.normal(0.0, 0.004, 3)
        nt = rng.normal(0.0, 0.02, 3)
        Z.append(step @ _pose(nr, nt))
    truth, Z = np.stack(truth), np.stack(Z)
    start = [_pose((0.0, 0.0, 1.0), (50.0, -20.0, 3.0))]
    for k in range(GNSS_N - 1):
        start.append(start[-1] @ Z[k])
    g = ref.Graph(np.stack(start), np.zeros(GNSS_N, bool), np.arange(GNSS_N - 1), np.arange(1, GNSS_N), Z)
    node = np.arange(0, GNSS_N, GNSS_EVERY)
    lever = np.array(GNSS_LEVER)
    pos = truth[node, :3, 3] + truth[node, :3, :3] @ lever + rng.normal(0.0, 0.05, (node.size, 3))
    return g, pref.Priors.positions(node, pos, GNSS_INFO * np.eye(3), lever), truth


def chain_priors(N, n_priors, seed, kind="position", fixed=False, lever_max=2.0, offset=0.0, nodes=None):
    """posegraph_cases.chain(N, seed) with n_priors priors on evenly spread nodes (or `nodes`); without a fixed node unless asked"""
    g = cases.chain(N, seed)
    if offset:
        g.poses[:, :3, 3] += offset
    g.fixed[:] = False
    g.fixed[0] = fixed
    nodes = np.linspace(0, N - 1, n_priors).astype(np.int64) if nodes is None else np.asarray(nodes)
    return g, pcases.rand_priors(g, nodes.size, seed + 500, kind=kind, nodes=nodes, lever_max=lever_max)


def _shift(g, first):
    return g.i + first, g.j + first


def every_class():
    """One graph: a fixed component (nodes 0 .. 11, node 0 fixed, mixed priors, one of them on the fixed node), a prior-anchored one
    (12 .. 23, pose priors), two aligned ones (24 .. 35 with four position priors, one on its gauge node 24; 36 .. 49 with five), and
    node 50 without edges, free, with two position priors"""
    parts = [cases.chain(12, 2), cases.chain(12, 3), cases.chain(12, 4), cases.chain(14, 5)]
    lone = cases.rand_pose(np.random.default_rng(6), 1.0, 5.0)[None]
    first = np.cumsum([0] + [p.N for p in parts])
    poses = np.concatenate([p.poses for p in parts] + [lone])
    i = np.concatenate([p.i + f for p, f in zip(parts, first)])
    j = np.concatenate([p.j + f for p, f in zip(parts, first)])
    fixed = np.zeros(poses.shape[0], bool)
    fixed[0] = True
    g = ref.Graph(poses, fixed, i, j, np.concatenate([p.Z for p in parts]), np.concatenate([p.info for p in parts]))
    sets = [pcases.rand_priors(g, 5, 100, kind="mixed", nodes=[0, 3, 7, 7, 11]),
            pcases.rand_priors(g, 4, 101, kind="pose", nodes=[13, 17, 22, 17]),
            pcases.rand_priors(g, 4, 102, kind="position", nodes=[24, 28, 31, 35]),
            pcases.rand_priors(g, 5, 103, kind="position", nodes=[37, 40, 44, 48, 49]),
            pcases.rand_priors(g, 2, 104, kind="position", nodes=[50, 50])]
    order = np.random.default_rng(105).permutation(sum(s.P for s in sets))  # the priors of the components interleaved
    P = pref.Priors(np.concatenate([s.node for s in sets])[order], np.concatenate([s.Z for s in sets])[order],
                    np.concatenate([s.lever for s in sets])[order], np.concatenate([s.info for s in sets])[order])
    return g, P


def scramble(g, seed, hold=()):
    """another start of the free nodes: every pose but those of `hold` replaced by a random one"""
    rng = np.random.default_rng(seed)
    poses = np.stack([cases.rand_pose(rng, 3.0, 50.0) for _ in range(g.N)])
    keep = g.fixed.copy()
    keep[list(hold)] = True
    poses[keep] = g.poses[keep]
    return ref.Graph(poses, g.fixed, g.i, g.j, g.Z, g.info)


def node_counts():
    """chain(12, 2) with node 0 fixed: nodes with 1, 2 and 70 mixed priors among nodes with none, the priors interleaved"""
    nodes = np.repeat([3, 5, 7], [1, 2, 70])
    np.random.default_rng(71).shuffle(nodes)
    return chain_priors(12, 0, 2, kind="mixed", fixed=True, nodes=nodes)


# Every shape of the GPU test, the smallest at which each path can go wrong: the prior kernels' workgroup is 256 priors, the alignment's
# lanes take 256 entries at a time, the chain factor's segment is 256 nodes.  The chains and their seeds are those of
# posegraph_init_cases.SHAPES; tests/test_posegraph_init_prior_abi.py checks every shape here for fitness to judge five iterations, as
# tests/test_posegraph_init_abi.py does for those.
SHAPES = {
    "N255_P1_fixed": lambda: chain_priors(255, 1, 41, kind="pose", fixed=True, nodes=[200]),
    "N255_P255_anchored": lambda: chain_priors(255, 255, 41, kind="mixed"),
    "N256_P256_aligned": lambda: chain_priors(256, 256, 42),
    "N257_P257_aligned": lambda: chain_priors(257, 257, 44),
    "N513_P513_aligned": lambda: chain_priors(513, 513, 45),
    "N513_P513_anchored": lambda: chain_priors(513, 513, 45, kind="mixed"),
    "aligned3": lambda: chain_priors(12, 3, 2),
    "aligned4_lever0": lambda: chain_priors(12, 4, 3, lever_max=0.0),
    "node_counts": node_counts,
    "far_1e5": lambda: chain_priors(30, 6, 7, offset=1e5),
    "every_class": every_class,
    "anchored_ring": lambda: pcases.anchored_ring()[:2],
    "gnss_chain": lambda: gnss_chain()[:2],
}

RECORDED = {"anchored_ring": lambda: pcases.anchored_ring()[:2], "gnss_chain": lambda: gnss_chain()[:2]}


def mirror_recording():
    """the mirror's direct-solve results on the recorded fixtures -> dict of arrays (the content of the golden file)"""
    out = {}
    for name, make in RECORDED.items():
        g, P = make()
        res = ipref.initialize(g, P)
        out[name + "_poses"], out[name + "_rows"], out[name + "_v_pre"], out[name + "_v"] = res["poses"], res["rows"], res["v_pre"], res["v"]
        out[name + "_align"] = res["align"]
        out[name + "_cost"] = np.array([res["cost_before"], res["cost_after"]])
    return out


if __name__ == "__main__":
    for every in (8, 16, 32):
        g, P, truth = pcases.anchored_ring(every=every)
        res = ipref.initialize(g, P)
        print("anchored_ring every", every, "start", ref.pose_error(g.poses, truth), "after", ref.pose_error(res["poses"], truth), "cost",
              res["cost_before"], "->", res["cost_after"], "sigma", res["align"][0, 25:], "applied", res["applied"])
    g, P, truth = gnss_chain()
    res = ipref.initialize(g, P)
    print("gnss_chain start", ref.pose_error(g.poses, truth), "after", ref.pose_error(res["poses"], truth), "cost", res["cost_before"], "->",
          res["cost_after"], "last solve moves by", np.abs(res["v"]).max())
    _, alone = pref.optimize(g, P, **cases.RING_CFG)
    poses, then = pref.optimize(ref.Graph(res["poses"], g.fixed, g.i, g.j, g.Z, g.info), P, **cases.RING_CFG)
    print("  Optimize alone:", alone["solves"], alone["accepted"], alone["stop_reason"], "; after the initialization:", then["solves"],
          then["accepted"], then["stop_reason"], ref.pose_error(poses, truth), then["cost_final"])
    g, P = pcases.priors_only()
    res = ipref.initialize(g, P)
    print("priors_only cost", res["cost_before"], "->", res["cost_after"])
    np.savez_compressed(GOLDEN, **mirror_recording())
