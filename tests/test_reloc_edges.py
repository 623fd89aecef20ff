"""The relocalization kernels at their edges (k_reloc_bitmap, k_reloc_window_or, k_reloc_bound, k_reloc_score, the driver of
elm_relocalize_global) against the numpy mirror of tests/reloc_ref.py on the hand-built cases of tests/reloc_cases.py, whose bite
tests/test_reloc_cases.py checks on the CPU.  Integers and bit patterns only: no tolerance anywhere.

The exhaustive reference of these cases is numpy, not ScorePoses.  The candidates pin the leaf scores and the driver; the search counters
(tau, passes, nodes bounded and kept per level, leaves scored) pin every bound: one that is too loose keeps a node the mirror prunes, one
that is too tight prunes a node the mirror keeps."""
import numpy as np
import pytest

import reloc_cases as rc
import reloc_ref as rr
from elimaloc_amd.registration import (Context, GlobalRelocConfig, IcpMethod, Registration, RegistrationConfig, RelocConfig, Scan,
                                       VoxelHashMap)

pytestmark = pytest.mark.gpu

FORMS = [dict(), dict(lds_budget_bytes=0), dict(lds_budget_bytes=0, bitmap_max_bytes=0)]  # LDS bitmap (when it fits), global bitmap, probes


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", rc.GLOBAL_NAMES)
def test_global_case(ctx, name):
    c = rc.global_case(name)
    vm = VoxelHashMap(c.vs, c.cap, ctx)
    vm.AddPoints(c.map)
    cfg = GlobalRelocConfig(**vars(c.cfg))
    # the lattice: the library's poses are the numpy ones (translations, ground heights and validity bit for bit; the rotations to the
    # rounding of cos / sin), and the map keeps the points the numpy rule keeps
    H, valid = vm.GlobalHypotheses(c.T_tilt, cfg)
    m = rc.mirror(name)
    assert vm.Pointcloud().shape[0] == rr.stored_points(c.map, c.vs, c.cap).shape[0]
    assert H.shape == m.H.shape and np.array_equal(valid, m.valid_flat) and np.array_equal(H[:, :, 3], m.H[:, :, 3])
    np.testing.assert_allclose(H[:, :3, :3], m.H[:, :3, :3], rtol=0, atol=1e-12)
    if not np.array_equal(H, m.H):  # the mirror runs on the library's own poses
        m = rr.Mirror(m.vox, m.vs, m.S, H, valid, c.cfg)
        ref = m.search()
    else:
        ref = rc.searched(name)
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P, max_iteration=2), ctx)
    _, _, _, _, cands, st = reg.RelocalizeGlobal(c.scan, vm, c.T_tilt, cfg)
    print(name, {k: st[k] for k in ("tau", "passes", "levels", "nodes_bounded", "nodes_kept", "leaves_scored", "point_evals")}, vars(ref) | {"leaves": None})
    assert [(q["hyp_index"], q["score"]) for q in cands] == ref.kept, (st, ref.kept[:6])
    for q in cands:
        assert np.array_equal(q["T0"], H[q["hyp_index"]])
    for k in ("tau", "passes", "levels", "nodes_bounded", "nodes_kept", "leaves_scored", "point_evals", "n_counted", "valid_leaves"):
        assert st[k] == getattr(ref, k), (k, st[k], getattr(ref, k))


@pytest.mark.parametrize("name", rc.SCORE_NAMES)
def test_score_case(ctx, name):
    c, ref = rc.score_case(name), rc.score_ref(name)
    vm = VoxelHashMap(c.vs, 30, ctx)
    vm.AddPoints(c.map)
    sc = Scan(ctx, c.scan)
    for f in FORMS:
        got = vm.ScorePoses(sc, c.poses, RelocConfig(score_max_range_m=c.r_max, **f))
        assert np.array_equal(got, ref), (f, got[:8], ref[:8], np.flatnonzero(got != ref)[:10])
