#!/usr/bin/env python3
"""Record tests/golden/stage2_parent.npz: the registrations of tests/stage2_cases.py run on the library that ELM_LIB points at -- one
built from the PARENT of a change of stage 2 of k_accumulate_grid that must not move a bit of its results.

    ELM_LIB=/path/to/parent/libelimaloc_hip.so python tools/record_stage2_golden.py <parent commit hash> [output.npz]

The fixture holds, per case, every iteration's packed sums (JTJ, JTr, residual, count), the final pose, the iteration count, the fitness
score and the covariance, of the production and of the instrumented kernels, the two work counters of the first iteration (points served
by stage 2, candidates tested), and the commit hash.  tests/test_stage2_groups.py compares them as bit patterns."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    commit = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "stage2_parent.npz")
    import stage2_cases as sc
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import Context
    ctx, cctx = Context(0), Context(0)
    cctx.set_work_counters(True)
    try:
        out, counters = sc.run_all(ctx, cctx)
    finally:
        cctx.close()
        ctx.close()
    flat = {f"{case}/{field}": arr for case, rec in out.items() for field, arr in rec.items()}
    flat["parent_commit"] = np.array(commit)
    for k, (served, tested) in counters.items():
        flat[f"stage2_points/{k}"] = np.array([served], np.float64)
        flat[f"tested/{k}"] = np.array([tested], np.float64)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    np.savez_compressed(dst, **flat)
    print(f"{dst}: {len(out)} records from {_lib.LIB_PATH} (parent {commit}), {os.path.getsize(dst)} bytes")
    for k, v in counters.items():
        print(f"  {k}: stage-2 points {v[0]:.0f}, candidates tested {v[1]:.0f}")


if __name__ == "__main__":
    main()
