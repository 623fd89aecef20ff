"""Writes tests/golden/local_map_loop.npz: the odometry loop of tests/local_map_cases.py run with the oracle's registration on mirror-built
maps (tests/local_map_ref.py: oracle_loop), per method the poses [steps, 4, 4], is_success, inserted and iterations of every step.  CPU
only.  Run from the repository root: python tests/golden/make_local_map_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import local_map_cases as cases  # noqa: E402
import local_map_ref as ref  # noqa: E402
from oracle import oracle as O  # noqa: E402


def run(method, n_steps):
    poses, scans = cases.loop_inputs()
    steps, stored = ref.oracle_loop(O, method, poses[:n_steps], scans[:n_steps], cases.loop_guesses(poses)[:n_steps], cases.VOXEL, cases.CAP,
                                    cases.LOOP_MAX_RANGE, **cases.LOOP_REG)
    return dict(T=np.stack([s["T"] for s in steps]), is_success=np.array([s["is_success"] for s in steps]),
                inserted=np.array([s["inserted"] for s in steps]), iterations=np.array([s["iterations"] for s in steps], np.int32),
                n_stored=np.int64(len(stored)))


if __name__ == "__main__":
    O.build()
    out = {}
    for name, method, n in (("p2p", O.P2P, cases.LOOP_STEPS), ("gicp", O.GICP, cases.LOOP_STEPS), ("vgicp", O.VGICP, 3)):
        for k, v in run(method, n).items():
            out[name + "_" + k] = v
        print(name, out[name + "_is_success"].tolist(), out[name + "_iterations"].tolist())
    np.savez(os.path.join(HERE, cases.LOOP_GOLDEN), **out)
