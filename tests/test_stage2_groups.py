"""Stage 2 of k_accumulate_grid serves the undecided points of a workgroup by groups of lanes, every search in it exact: which lane walks
which column of a point's ball, how wide a group is and where a point's record lies in the queue must not move one bit of any result.
Every registration of tests/stage2_cases.py -- one workgroup with 0 .. 256 undecided points at every queue length where a group width or
the number of passes would change, workgroups of different queue lengths in one launch, the seeded walk of points whose block came back
empty, both grid forms, GICP -- is compared, as bit patterns, with tests/golden/stage2_parent.npz: the same registrations recorded on
the library of the parent commit (tools/record_stage2_golden.py; the hash is in the fixture).  The pairs of exact float64 ties and of the
search-only build are compared with the CPU oracle's."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import accumulate_tail_cases as tc  # noqa: E402
import stage2_cases as sc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage2_parent.npz")
QUEUE_CASES = tuple((f"p2p_k{k}", k) for k in sc.QUEUE_K) + (("p2p_mixed", sum(sc.MIXED_K)),) + tuple((f"p2p_seed_k{k}", k) for k in sc.SEED_K) \
    + tuple((f"gicp_k{k}", k) for k in sc.FORM_K) + tuple((f"tiled_p2p_k{k}", k) for k in sc.FORM_K)


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
    return sc.run_all(*ctxs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _scan_of(case):
    if case == "p2p_mixed":
        return sc.mixed_scan(), 5.0
    k = int(case.rsplit("_k", 1)[1])
    if "_seed_" in case:
        return sc.seed_scan(k), sc.SEED_RADIUS
    return sc.workgroup_scan(k), 5.0


@pytest.mark.parametrize("tag", ["", "_counters"])
@pytest.mark.parametrize("case", sc.CASES)
def test_bits_match_parent(runs, golden, case, tag):
    """Packed sums of every iteration, final pose, iteration count, fitness score, covariance: bit for bit the parent's, on the
    production and on the instrumented kernels."""
    rec = runs[0][case + tag]
    for field in sc.FIELDS:
        want, got = golden[f"{case}{tag}/{field}"], rec[field]
        assert got.shape == want.shape and got.dtype == want.dtype, (case, field, got.shape, want.shape)
        assert np.array_equal(_bits(got), _bits(want)), (case, field, got, want)


@pytest.mark.parametrize("case,k", QUEUE_CASES)
def test_queue_length_and_work_counters(runs, golden, oracle, case, k):
    """The workgroup queues the k points the case lifted: at least k - 2 of them are undecided by the CPU oracle's own distances (nearest
    neighbour beyond the open faces of the point's block), the GPU's count of points served by stage 2 in the first iteration is at least
    that, is k itself (the other points sit within 0.04 m of a map point with no second one within a quarter metre: decided), and equals
    the parent's; so does the number of candidates tested -- the walked slots do not depend on which lane walks which column."""
    scan, th = _scan_of(case)
    om = oracle.Map(1.0, 30)
    om.add_points(tc.sparse_patch())
    n_sure = int(tc.surely_undecided(om, scan.astype(np.float64), th).sum())
    served, tested = runs[1][case]
    print(f"{case}: k = {k}, {n_sure} surely undecided (oracle), {served:.0f} served by stage 2, {tested:.0f} candidates tested")
    assert k - 2 <= n_sure <= k
    assert served >= n_sure
    assert served == k
    assert served == float(golden[f"stage2_points/{case}"][0])
    assert tested == float(golden[f"tested/{case}"][0])


@pytest.mark.parametrize("k,calls", sc.TIE_RUNS)
def test_exact_ties_pair_like_the_oracle(ctxs, oracle, k, calls):
    """Queries exactly midway between two and between four lattice points (float32-exact coordinates, so the float64 distances tie
    exactly): the float32 pass cannot certify them, the float64 walk decides by bucket rank, then insertion order -- whichever lanes
    hold the tied candidates.  k ties per workgroup: the queue lengths at which groups sized to the queue would be 16 (k <= 4), 8 (k <= 8)
    and 4 lanes wide."""
    from elimaloc_amd.registration import VoxelHashMap
    pts = sc.lattice_map()
    vm = VoxelHashMap(1.0, 30, ctxs[0])
    vm.AddPoints(pts)
    om = oracle.Map(1.0, 30)
    om.add_points(pts)
    n_ties = 0
    for call in range(calls):
        q, where = sc.tie_queries(k, call)
        acc, tgt, d2 = om.nearest_points(q, 5.0)
        assert np.asarray(acc, bool).all()
        # ties in the oracle's own float64 distances: its winner's distance is met by two or more map points
        e = q[:, None, :] - pts[None, :, :].astype(np.float64)
        dd = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
        tied = (dd == d2[:, None]).sum(axis=1) >= 2
        assert tied[where].all() and int(tied.sum()) == k, (k, call, int(tied.sum()))
        n_ties += int(tied.sum())
        _, tp, si, _ = vm.GetCorrespondencePoints(q, 5.0, indices=True)
        assert np.array_equal(si, np.arange(len(q))), (k, call)
        assert np.array_equal(tp, tgt), (k, call, np.flatnonzero((tp != tgt).any(axis=1)))
    assert n_ties >= 32, n_ties
    vm.Clear()


def test_query_build_pairs_equal_the_oracle(ctxs, oracle):
    """elm_map_get_correspondences (the search alone) on the k = 5 workgroup: every pair the oracle's, none left out."""
    vm, om = tc._maps(ctxs[0], oracle, tc.sparse_patch(), tc.P2P)
    g = sc.workgroup_scan(sc.QUERY_K).astype(np.float64)
    acc, tgt, _ = om.nearest_points(g, 5.0)
    _, tp, si, _ = vm.GetCorrespondencePoints(g, 5.0, indices=True)
    assert np.asarray(acc, bool).all()
    assert np.array_equal(si, np.arange(len(g))) and np.array_equal(tp, tgt)
