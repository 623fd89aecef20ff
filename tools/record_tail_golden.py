#!/usr/bin/env python3
"""Record tests/golden/accumulate_tail_parent.npz: the registrations of tests/accumulate_tail_cases.py run on the library that
ELM_LIB points at -- one built from the PARENT of a change that must not move a bit of the accumulate kernels' results.

    ELM_LIB=/path/to/parent/libelimaloc_hip.so python tools/record_tail_golden.py <parent commit hash> [output.npz]

The fixture holds, per case, every iteration's packed sums (JTJ, JTr, residual, count), the final pose, the iteration count, the
fitness score and the covariance, plus the commit hash.  tests/test_accumulate_tail.py compares them as bit patterns."""
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
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "accumulate_tail_parent.npz")
    import accumulate_tail_cases as tc
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import Context
    ctx, cctx = Context(0), Context(0)
    cctx.set_work_counters(True)
    try:
        out, counters = tc.run_all(ctx, cctx)
    finally:
        cctx.close()
        ctx.close()
    flat = {f"{case}/{field}": arr for case, rec in out.items() for field, arr in rec.items()}
    flat["parent_commit"] = np.array(commit)
    for k, v in counters.items():
        flat[f"stage2_points/{k}"] = np.array([v], np.float64)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    np.savez_compressed(dst, **flat)
    print(f"{dst}: {len(out)} cases from {_lib.LIB_PATH} (parent {commit}), {os.path.getsize(dst)} bytes; stage-2 points {counters}")


if __name__ == "__main__":
    main()
