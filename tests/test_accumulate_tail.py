"""The skeleton of an accumulate workgroup -- its head (block -> scan, the early exits), the queue of undecided points and where stage 2
leaves its results, the DPP steps of the block reduction, the expansion of the reduced P2P values into the packed record -- carries no
arithmetic of its own, so a change to it must not move one bit of any result.  Every registration of tests/accumulate_tail_cases.py is
compared, as bit patterns, with tests/golden/accumulate_tail_parent.npz: the same registrations recorded on the library of the parent
commit (tools/record_tail_golden.py; the hash is in the fixture)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import accumulate_tail_cases as tc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accumulate_tail_parent.npz")
CASES = tuple(f"p2p_n{n}" for n in tc.P2P_SIZES) + ("p2p_far", "p2p_beyond_radius", "p2p_queue", "p2p_queue_counters", "gicp_queue",
                                                    "gicp_queue_counters", "vgicp_n257")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ctxs():
    from elimaloc_amd.registration import Context
    ctx, cctx = Context(0), Context(0)
    cctx.set_work_counters(True)
    yield ctx, cctx
    cctx.close()
    ctx.close()


@pytest.fixture(scope="module")
def runs(ctxs):
    """Every registration once; the tests below only read."""
    return tc.run_all(*ctxs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("case", CASES)
def test_bits_match_parent(runs, golden, case):
    """Packed sums of every iteration, final pose, iteration count, fitness score, covariance: bit for bit the parent's."""
    rec = runs[0][case]
    for field in tc.FIELDS:
        want, got = golden[f"{case}/{field}"], rec[field]
        assert got.shape == want.shape and got.dtype == want.dtype, (case, field, got.shape, want.shape)
        assert np.array_equal(_bits(got), _bits(want)), (case, field, got, want)


def test_all_zero_sums_keep_their_signed_zeros(runs, golden):
    """No pair at all: every sum of the record is a zero, and each is the parent's zero -- the negated slots of the P2P expansion
    included, the six structural slots +0.0 (compared as bit patterns, so -0.0 != +0.0 here).  What the trace holds is the record after
    k_solve has added up the scan's workgroups from +0.0, so a -0.0 of a negated slot reads +0.0 here on both sides; a NaN or a
    non-zero from a mis-expanded slot would not."""
    for case in ("p2p_far", "p2p_beyond_radius"):
        rec = runs[0][case]
        assert rec["n_corr"][0] == 0.0 and not rec["JTJ"][0].any() and not rec["JTr"][0].any()
        for field in ("JTJ", "JTr", "residual_sum"):
            assert np.array_equal(_bits(rec[field]), _bits(golden[f"{case}/{field}"])), (case, field)


@pytest.mark.parametrize("name,method", [("p2p", tc.P2P), ("gicp", tc.GICP)])
def test_queue_takes_a_second_pass(ctxs, runs, golden, oracle, name, method):
    """The lifted scan's workgroup queues at least 65 points, so stage 2 makes a second pass over the queue and reads later records after
    earlier ones were written into.  First on the CPU oracle (nearest neighbour beyond the block's open faces), then on the GPU's own
    count of points served by stage 2."""
    _, om = tc._maps(ctxs[0], oracle, tc.sparse_patch(), tc.P2P)
    n_sure = int(tc.surely_undecided(om, tc.lifted_scan().astype(np.float64)).sum())
    assert n_sure >= tc.QUEUE_MIN, n_sure
    served = runs[1][name]
    print(f"{name}: {n_sure} points surely undecided (oracle), {served:.0f} served by stage 2 in the first iteration")
    assert served >= n_sure and served <= 256
    assert served == float(golden[f"stage2_points/{name}"][0])


def test_query_build_pairs_equal_the_oracle(ctxs, oracle):
    """elm_map_get_correspondences (the search alone, STATS = 2) on the lifted scan: every pair the oracle's, none left out."""
    vm, om = tc._maps(ctxs[0], oracle, tc.sparse_patch(), tc.P2P)
    g = tc.lifted_scan().astype(np.float64)
    acc, tgt, _ = om.nearest_points(g, 5.0)
    _, tp, si, ti = vm.GetCorrespondencePoints(g, 5.0, indices=True)
    assert np.asarray(acc, bool).all() and len(si) == len(g)
    assert np.array_equal(si, np.arange(len(g))) and np.array_equal(tp, tgt)
    # and with a radius that rejects part of them
    acc, tgt, _ = om.nearest_points(g, 0.42)
    _, tp, si, ti = vm.GetCorrespondencePoints(g, 0.42, indices=True)
    acc = np.asarray(acc, bool)
    assert 0 < acc.sum() < len(g)
    assert np.array_equal(si, np.flatnonzero(acc)) and np.array_equal(tp, tgt[acc])
