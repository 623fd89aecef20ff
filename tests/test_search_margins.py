"""The float32-certified neighbour search at its decision margins: queries CONSTRUCTED (tests/margin_cases.py) to lie a prescribed
distance -- from exact ties and single float64 ulps up to 1e-3 relative -- from every boundary the search decides on (winner vs runner-up
for stored points and voxel means, the search radius, the faces of the 2 x 2 x 2 cell block, voxel / half-voxel key faces), on worlds
translated up to 1e6 m from the origin where the magnitude terms of the margins reach millimetres.

CPU part: the inputs are what they claim (coverage per bin from the REALISED gaps, the discard cap) and the oracle agrees with an
independent numpy brute force on every one of them.  GPU part: the product's pairs against the oracle's, index for index and bit for
bit, on every search form, at lengths that split waves and stage-2 groups unevenly, and through the registration kernels proper."""
import collections

import numpy as np
import pytest

import margin_cases as mc

CASES = mc.cases()
MAX_DISCARD = 0.25
_GEN = {}


def _gen(case):
    if case not in _GEN:
        _GEN[case] = mc.generate(case)
    return _GEN[case]


def _oracle_map(oracle, case):
    om = oracle.Map(case[2], case[3])
    om.add_points(mc.world_of(case))
    om.cal_voxel_cov_all()
    return om


def _th_groups(Q):
    return [(float(th), np.flatnonzero(Q.th == th)) for th in np.unique(Q.th)]


# ---- CPU: the inputs are what they claim -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", range(len(mc.OFFSETS)))
def test_generated_queries_sit_where_they_claim(oracle, o, capsys):
    """Per (family, offset), pooled over the worlds and voxel sizes of that offset: >= 200 surviving queries, >= 32 in every decade of
    realised gap from 1e-9 to 1e-4 (from 1e-14 at offset 0), >= 16 in every ulp bin, at most 25 % of the constructed queries discarded;
    and the oracle's winner of every surviving pair query is one of the intended pair, at the smaller of the two float64 distances."""
    n_con, n_dis = collections.Counter(), collections.Counter()
    dec, ulp, surv, pos7 = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter), collections.Counter(), collections.Counter()
    for case in [c for c in CASES if c[1] == o]:
        m, Q, stats = _gen(case)
        om = _oracle_map(oracle, case)
        for fam in mc.FAMILIES:
            n_con[fam] += stats[fam][0]; n_dis[fam] += stats[fam][1]
            s = Q.select(fam)
            s = s[Q.ok[s]]
            surv[fam] += len(s)
            for d, k in zip(*np.unique(mc.decade(Q.gap[s]), return_counts=True)):
                dec[fam][int(d)] += int(k)
            u = s[Q.kind[s] == "ulp"]
            for t, k in zip(*np.unique(Q.ulps[u], return_counts=True)):
                ulp[fam][int(t)] += int(k)
            table = m.vmean if fam in ("vrunner", "vradius", "aradius") else m.pts
            if fam in mc.PAIR_FAMILIES:
                th = float(Q.th[s[0]]) if len(s) else 5.0
                acc, tgt, d2 = (om.nearest_points(Q.g[s], th) if fam != "vrunner" else om.nearest_voxel(Q.g[s], th)[:2] + (None,))
                a, b = table[Q.ia[s]], table[Q.ib[s]]
                da, db = mc.sq(a - Q.g[s]), mc.sq(b - Q.g[s])
                is_a, is_b = (tgt == a).all(axis=1), (tgt == b).all(axis=1)
                assert (is_a | is_b).all() and acc.all(), (fam, case)
                assert (np.where(is_a, da, db) == np.minimum(da, db)).all(), (fam, case)
                assert (is_a[da < db]).all() and (is_b[db < da]).all(), (fam, case)
            if fam == "aradius":
                for p, k in zip(*np.unique(Q.pos[s], return_counts=True)):
                    pos7[int(p)] += int(k)
    with capsys.disabled():
        print(f"\noffset {mc.OFFSETS[o]}:")
        for fam in mc.FAMILIES:
            print(f"  {fam:10s} constructed {n_con[fam]:6d} discarded {n_dis[fam]:5d} ({100.0 * n_dis[fam] / max(n_con[fam], 1):4.1f} %) "
                  f"decades {dict(sorted((d, k) for d, k in dec[fam].items() if d > -900))} exact {dec[fam].get(-999, 0)} ulp bins {dict(sorted(ulp[fam].items()))}")
    for fam in mc.FAMILIES:
        assert n_dis[fam] <= MAX_DISCARD * n_con[fam], (fam, n_dis[fam], n_con[fam])
        assert surv[fam] >= 200, (fam, surv[fam])
        # at offset 0 also 1e-14 .. 1e-10 -- for the relative gaps.  The two block sweeps are in METRES (the issue gives them +-1e-3 m and 0,
        # no lower end; theirs is 1e-9 m) and the radius sweep starts at 1e-12 (below): those decades do not exist for them
        for d in range(-14 if o == 0 and fam not in ("blockrho", "blockface") + mc.RADIUS_FAMILIES else -9, -3):
            assert dec[fam][d] >= 32, (fam, d, dec[fam][d])
        if fam in mc.RADIUS_FAMILIES:
            if o == 0:
                for d in range(-12, -9):  # the radius sweep starts at 1e-12
                    assert dec[fam][d] >= 32, (fam, d, dec[fam][d])
            for t in (0, 1, -1):
                assert ulp[fam][t] >= 16, (fam, t, ulp[fam][t])
        elif fam != "blockrho":  # (rho is a face distance, not a candidate: nothing to tie with, its sweep is in metres)
            for t in mc.ULP_BINS:
                assert ulp[fam][t] >= 16, (fam, t, ulp[fam][t])
    assert all(pos7[p] >= 16 for p in range(7)), pos7  # each of AVGICP's seven pairs sits on the radius for some query


# ---- CPU: the oracle is right on these inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=mc.case_id)
def test_oracle_equals_the_numpy_brute_force(oracle, case):
    m, Q, _ = _gen(case)
    om = _oracle_map(oracle, case)
    # the same map: buckets, insertion order, means
    keys, npts, _, means = om.voxels()
    op = om.pointcloud()[0]
    starts = np.concatenate([[0], np.cumsum(npts)])
    v = m.lookup(keys.astype(np.int64))
    assert len(keys) == len(m.vkeys) and (v >= 0).all() and np.array_equal(m.vcnt[v], npts)
    assert np.array_equal(m.vmean[v], means)
    for i in range(len(keys)):
        assert np.array_equal(m.pts[m.vstart[v[i]]:m.vstart[v[i]] + npts[i]], op[starts[i]:starts[i + 1]])
    for th, s in _th_groups(Q):
        g = Q.g[s]
        acc, tgt, d2 = om.nearest_points(g, th)
        nacc, ntgt, _, nd2 = m.nearest_points(g, th)
        assert np.array_equal(acc, nacc) and np.array_equal(tgt, ntgt) and np.array_equal(d2, nd2)
        acc, mean, _ = om.nearest_voxel(g, th)
        nacc, nmean, _, _ = m.nearest_voxel(g, th)
        assert np.array_equal(acc, nacc) and np.array_equal(mean, nmean)
        src, mean, _ = om.all_cov_pairs(g, th)
        nsrc, nmean, _ = m.all_cov_pairs(g, th)
        assert np.array_equal(src, nsrc) and np.array_equal(mean, nmean)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
FORMS = {
    "grid": {},
    "tiled": {"ELM_GRID": "tiled"},
    "wide": {"ELM_GRID": "max_block_bytes=48"},
    "wide_tiled": {"ELM_GRID": "max_block_bytes=48,tiled"},
    "lists": {"ELM_KERNEL": "lists"},
    "direct": {"ELM_KERNEL": "direct"},
    "hash": {"ELM_GRID": "max_cells=1000"},
}
_REF = {}


def _reference(oracle, case):
    """the oracle's pairs of every radius group of a case (computed once, shared by the search forms)"""
    if case not in _REF:
        _, Q, _ = _gen(case)
        om = _oracle_map(oracle, case)
        _REF[case] = [(th, s, om.nearest_points(Q.g[s], th), om.nearest_voxel(Q.g[s], th), om.all_cov_pairs(Q.g[s], th)) for th, s in _th_groups(Q)]
    return _REF[case]


def _device_map(ctx, case):
    from elimaloc_amd.registration import VoxelHashMap
    vm = VoxelHashMap(case[2], case[3], ctx)
    vm.AddPoints(mc.world_of(case))
    vm.CalVoxelCovAll()
    return vm


def _mismatches(vm, g, th, ref_p, ref_v, ref_a):
    """number of queries whose pairs differ from the oracle's, per call"""
    bad = {}
    acc, tgt, _ = ref_p
    _, tp, si, _ = vm.GetCorrespondencePoints(g, th, indices=True)
    got = np.zeros(len(g), bool); got[si] = True
    full = np.zeros((len(g), 3)); full[si] = tp
    bad["points"] = int(((got != acc) | (acc & got & (full != tgt).any(axis=1))).sum())
    acc, mean, _ = ref_v
    _, tm, _, si, _ = vm.GetCorrespondencesCov(g, th, indices=True)
    got = np.zeros(len(g), bool); got[si] = True
    full = np.zeros((len(g), 3)); full[si] = tm
    bad["voxel"] = int(((got != acc) | (acc & got & (full != mean).any(axis=1))).sum())
    src, mean, _ = ref_a
    _, tm, _, si, _ = vm.GetCorrespondencesAllCov(g, th, indices=True)
    bad["all"] = 0 if (np.array_equal(si, src) and np.array_equal(tm, mean)) else max(1, abs(len(si) - len(src)), int((si[:min(len(si), len(src))] != src[:min(len(si), len(src))]).sum()))
    return bad


def _report(Q, s, wrong):
    """family / kind / realised gap of the first few queries that came out wrong"""
    return [(Q.family[i], Q.kind[i], float(Q.gap[i]), float(Q.ulps[i]), bool(Q.ok[i])) for i in s[wrong][:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=mc.case_id)
def test_pairs_at_the_margins_equal_the_oracle_s(oracle, case, form, monkeypatch, capsys):
    """Every generated query of the case, on one search form: GetCorrespondencePoints / GetCorrespondencesCov / GetCorrespondencesAllCov
    against the oracle -- same accepted set, same source indices, same targets bit for bit.  Nothing is forgiven."""
    from elimaloc_amd.registration import Context
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    _, Q, _ = _gen(case)
    c = Context(0)
    try:
        vm = _device_map(c, case)
        for th, s, ref_p, ref_v, ref_a in _reference(oracle, case):
            g = Q.g[s]
            acc, tgt, _ = ref_p
            _, tp, si, _ = vm.GetCorrespondencePoints(g, th, indices=True)
            ok = np.array_equal(si, np.flatnonzero(acc)) and np.array_equal(tp, tgt[acc])
            if not ok:
                got = np.zeros(len(g), bool); got[si] = True
                full = np.zeros((len(g), 3)); full[si] = tp
                wrong = (got != acc) | (acc & got & (full != tgt).any(axis=1))
                pytest.fail(f"{int(wrong.sum())} of {len(g)} point pairs differ (th {th}): {_report(Q, s, wrong)}")
            acc, mean, _ = ref_v
            _, tm, _, si, _ = vm.GetCorrespondencesCov(g, th, indices=True)
            if not (np.array_equal(si, np.flatnonzero(acc)) and np.array_equal(tm, mean[acc])):
                got = np.zeros(len(g), bool); got[si] = True
                full = np.zeros((len(g), 3)); full[si] = tm
                wrong = (got != acc) | (acc & got & (full != mean).any(axis=1))
                pytest.fail(f"{int(wrong.sum())} of {len(g)} voxel pairs differ (th {th}): {_report(Q, s, wrong)}")
            src, mean, _ = ref_a
            _, tm, _, si, _ = vm.GetCorrespondencesAllCov(g, th, indices=True)
            if not (np.array_equal(si, src) and np.array_equal(tm, mean)):
                cnt_o, cnt_g = np.bincount(src, minlength=len(g)), np.bincount(si, minlength=len(g))
                pytest.fail(f"all-cov pairs differ (th {th}): {_report(Q, s, cnt_o != cnt_g)}")
        if form == "grid":
            with capsys.disabled():
                bins = {fam: dict(sorted(collections.Counter(mc.decade(Q.gap[Q.select(fam)][Q.ok[Q.select(fam)]]).tolist()).items())) for fam in mc.FAMILIES}
                print(f"\n{mc.case_id(case)}: {len(Q.g)} queries, 0 mismatching pairs; surviving queries per decade of realised gap (-999: exact): {bins}")
    finally:
        c.close()


LENGTH_CASES = [("planar", 0, 1.0, 30), ("planar", 4, 0.5, 6), ("lattice", 3, 1.0, 6), ("blob", 2, 0.4, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["grid", "lists", "tiled"])
@pytest.mark.parametrize("case", LENGTH_CASES, ids=mc.case_id)
def test_margin_queries_at_uneven_group_sizes(oracle, case, form, monkeypatch):
    """Lengths 1, 63, 64, 65, 255, 257 (waves and stage-2 groups split unevenly), the hard queries interleaved 1 : 15 with noise-free
    copies of map points (stage 2's queue holds a few points per workgroup) and all hard (it overflows one pass).  To bound the GPU time
    only the dense grid, its tiled form and the lists run these sets (the wide, direct and hash forms see the full sets above), on four
    cases and on the queries of the 5 m radius group (the pair and block families)."""
    from elimaloc_amd.registration import Context
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    m, Q, _ = _gen(case)
    om = _oracle_map(oracle, case)
    hard = Q.g[np.flatnonzero((Q.th == 5.0) & Q.ok)]
    hard = hard[np.random.default_rng(5).permutation(len(hard))]
    assert len(hard) >= 705, f"{mc.case_id(case)}: only {len(hard)} surviving hard queries for the length sets"
    mixed = mc.easy_queries(m, 16 * 512, seed=6)
    mixed[::16] = hard[:512]
    c = Context(0)
    try:
        vm = _device_map(c, case)
        sets = [hard[k:k + n] for k, n in ((0, 1), (1, 63), (64, 64), (128, 65), (193, 255), (448, 257))] + [mixed, hard]
        for g in sets:
            bad = _mismatches(vm, g, 5.0, om.nearest_points(g, 5.0), om.nearest_voxel(g, 5.0), om.all_cov_pairs(g, 5.0))
            assert bad == {"points": 0, "voxel": 0, "all": 0}, (len(g), bad)
    finally:
        c.close()


SUM_RTOL = 1e-9  # tests/test_gpu_parity.py: the project's bar for the sums


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1, 2, 3])
@pytest.mark.parametrize("o", range(len(mc.OFFSETS)))
def test_registration_kernels_at_the_margins(oracle, o, method, capsys):
    """The non-QUERY instantiation (the kernel computes g itself): one iteration with T0 = identity + the offset's translation and the
    float32 scan p = float32(g - t), so the kernel's g' = ((1 px + 0 py) + 0 pz) + t lies within half a float32 ulp of p of the generated g.
    The gaps g' REALISES are recomputed with the generator's bookkeeping and printed per decade; the decades from 1e-7 upwards stay
    populated.  n_corr exact, JTJ / JTr / residual sum within SUM_RTOL of the oracle's.
    What this can detect: a wrong ACCEPTANCE (n_corr is exact) and wrong winners in bulk.  A single wrong winner at a relative gap of
    1e-7 among thousands of pairs moves the sums by less than SUM_RTOL, and the trace exposes no pairs -- the pair-for-pair verdict on the
    search is the QUERY instantiation's above, which runs the same search code on the same g."""
    from elimaloc_amd.registration import Context, VoxelHashMap, Registration, RegistrationConfig, IcpMethod
    t = np.array(mc.OFFSETS[o])
    T0 = np.eye(4); T0[:3, 3] = t
    c = Context(0)
    hist = collections.Counter()
    try:
        for case in [cs for cs in CASES if cs[1] == o and (cs[0] != "planar" or cs[2] in (0.4, 1.0))]:
            m, Q, _ = _gen(case)
            fams = ("vrunner",) if method >= 2 else ("runner", "runner_far", "keyface", "blockface")
            s = np.flatnonzero(np.isin(Q.family, fams) & Q.ok)
            scan = (Q.g[s] - t).astype(np.float32)
            g2 = np.stack([((1.0 * scan[:, 0].astype(np.float64) + 0.0 * scan[:, 1]) + 0.0 * scan[:, 2]) + t[0],
                           ((0.0 * scan[:, 0] + 1.0 * scan[:, 1].astype(np.float64)) + 0.0 * scan[:, 2]) + t[1],
                           ((0.0 * scan[:, 0] + 0.0 * scan[:, 1]) + 1.0 * scan[:, 2].astype(np.float64)) + t[2]], 1)
            table, best3 = (m.vmean, m.best3_voxels) if method >= 2 else (m.pts, m.best3_points)
            gap, _, ok = mc._realise_pair(best3, Q.ia[s], Q.ib[s], g2, table)
            hist.update(mc.decade(gap[ok]).tolist())
            vm = VoxelHashMap(case[2], case[3], c)
            vm.AddPoints(mc.world_of(case))
            om = oracle.Map(case[2], case[3])
            om.add_points(mc.world_of(case))
            if method >= 2:
                vm.CalVoxelCovAll(); om.cal_voxel_cov_all()
            if method == 1:
                vm.CalPointCovAll(0.4); om.cal_point_cov_all(0.4)
            kw = dict(max_iteration=1, min_overlap_ratio=0.0, max_fitness_score=1e9)
            *_, det = Registration(RegistrationConfig(icp_method=IcpMethod(method), **kw), c).RunRegister(scan, vm, T0, trace=True)
            ref = oracle.register(om, scan, T0, oracle.default_config(method, **kw))
            gi, ri = det["iters"][0], ref["iters"][0]
            assert gi["n_corr"] == ri["n_corr"], mc.case_id(case)
            scale = np.abs(ri["JTJ"]).max()
            np.testing.assert_allclose(gi["JTJ"], ri["JTJ"], rtol=0, atol=SUM_RTOL * scale, err_msg=mc.case_id(case))
            np.testing.assert_allclose(gi["JTr"], ri["JTr"], rtol=0, atol=SUM_RTOL * max(np.abs(ri["JTr"]).max(), scale * 1e-3), err_msg=mc.case_id(case))
            np.testing.assert_allclose(gi["residual_sum"], ri["residual_sum"], rtol=SUM_RTOL, err_msg=mc.case_id(case))
            del vm
    finally:
        c.close()
    with capsys.disabled():
        print(f"\noffset {mc.OFFSETS[o]} method {method}: queries per decade of the gap realised after the float32 rounding of the scan: {dict(sorted(hist.items()))}")
    for d in range(-7, -3):
        assert hist[d] >= 1, (d, dict(hist))
