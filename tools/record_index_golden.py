#!/usr/bin/env python3
"""Record tests/golden/index_forms_parent.npz: the cases of tests/index_form_cases.py run on the library that ELM_LIB points at -- one
built from the PARENT of a change that must not move the search indices: which index a map gets, its byte accounting, a pair or a bit of
a registration.

    ELM_LIB=/path/to/parent/libelimaloc_hip.so python tools/record_index_golden.py <parent commit hash> [output.npz]

The fixture holds, per (map, index form), the map's info, the (source, target) indices of the three correspondence calls and one traced
registration per method, plus the commit hash.  Arrays that several cases share (most forms find the same pairs) are stored once, under
their digest.  tests/test_index_forms.py compares everything exactly.  Writes that one file and nothing else."""
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
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "index_forms_parent.npz")
    import index_form_cases as ic
    from elimaloc_amd import _lib
    flat = {"parent_commit": np.array(commit)}
    n_fields = 0
    for name in ic.MAPS:
        for form in ic.FORMS:
            rec = ic.run_case(name, form)
            for field, arr in rec.items():
                d = ic.digest(arr)
                flat[f"case/{name}/{form}/{field}"] = np.array(d)
                flat[f"blob/{d}"] = arr
                n_fields += 1
            print(f"{name:9s} {form:19s} info {rec['info_end'].tolist()} pairs "
                  f"{[len(rec[c + '/src']) for c in ('GetCorrespondencePoints', 'GetCorrespondencesCov', 'GetCorrespondencesAllCov')]}", flush=True)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    np.savez_compressed(dst, **flat)
    n_blobs = sum(k.startswith("blob/") for k in flat)
    print(f"{dst}: {n_fields} fields in {n_blobs} arrays from {_lib.LIB_PATH} (parent {commit}), {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
