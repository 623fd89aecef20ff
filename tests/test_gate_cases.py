"""The constructed registrations of tests/gate_cases.py are what they claim, the CPU oracle gives the stated verdict on every one of
them, and two deliberately wrong overlap gates written in numpy contradict the stated verdicts -- so a device that formed the quotient
in double, or compared with `<=`, cannot pass tests/test_solve_gates.py, which runs the same cases on the kernels.  No GPU."""
import math

import numpy as np
import pytest

import gate_cases as G

EXACT = G.exact_cases()


def _ids(cases):
    return [c["name"] for c in cases]


# ---- the families are what they claim ----------------------------------------------------------------------------------------------
def test_map_is_a_one_point_per_voxel_lattice_far_from_the_origin():
    w = G.world().astype(np.float64)
    assert w.shape == (1024, 3) and np.sqrt((w * w).sum(1)).min() >= 30.0
    keys = np.trunc(w / G.VOXEL_SIZE).astype(np.int64)
    assert len(np.unique(keys, axis=0)) == len(w)                      # one point per voxel: every point is stored
    assert np.array_equal(keys, np.floor(w / G.VOXEL_SIZE).astype(np.int64))
    assert np.all((w * 2.0) % 1.0 == 0.0)                              # dyadic


def test_family_a_counts_and_quotients():
    below, above, differ = G.quotient_pairs()
    assert differ == 1824                                              # of the 2 016 pairs k < N <= 64
    assert len(below) >= 12 and len(above) >= 12
    assert all(G.quotient32(k, n) < G.quotient64(k, n) for k, n in below) and all(G.quotient32(k, n) > G.quotient64(k, n) for k, n in above)
    assert all(G.quotient32(k, n) == G.quotient64(k, n) for k, n in G.A_AGREE if n)
    assert {(7, 10), (5, 6)} <= set(below) and {(1, 3), (3, 10)} <= set(above)
    # the two constructions named in the issue
    assert G.overlap_fails(7, 10, 0.7) and not G.overlap_fails(7, 10, 0.7, quotient="f64")
    third = G.quotient32(1, 3)
    assert not G.overlap_fails(1, 3, third) and G.overlap_fails(1, 3, float(np.nextafter(third, np.inf)))
    f32_only, f64_only, le_only = G.a_disagreements()
    assert f32_only >= G.A_MIN_DISAGREE // 2 and f64_only >= G.A_MIN_DISAGREE // 2
    assert (f32_only, f64_only, le_only) == (36, 36, 34)
    cases = G.family_a()
    assert all(len(c["scan"]) == c["n"] <= 64 and int(c["paired"].sum()) == c["k"] for c in cases)
    assert any(c["k"] == 0 and c["thr"] == 0.0 and math.copysign(1.0, c["thr"]) < 0 for c in cases)       # k = 0 against -0.0
    assert {c["method"] for c in cases} == {G.P2P, G.GICP, G.VGICP}
    assert any("-nan-" in c["name"] for c in cases) and any("-far-" in c["name"] for c in cases)


ALL = EXACT + G.stream_cases("half") + G.stream_cases("zero")


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_paired_points_pair_and_unpaired_points_cannot(case):
    """float64: under T0 every unpaired point is NaN or beyond max_search_dist of every map point AND of the origin, every paired point
    lies within 0.25 m of exactly one map point"""
    scan, T = case["scan"].astype(np.float64), case["T0"]
    assert len(case["paired"]) == len(scan)
    g = scan @ T[:3, :3].T + T[:3, 3]
    w = G.world().astype(np.float64)
    th = case["cfg"]["max_search_dist"]
    loose = g[~case["paired"]]
    fin = loose[np.isfinite(loose).all(1)]
    if case["family"] != "D" or case["cfg"]["max_iteration"] > 0:       # (no search ever runs in the max_iteration <= 0 cases)
        assert np.isnan(loose[~np.isfinite(loose).all(1)]).any(1).all()
        if len(fin):
            d = np.sqrt(((fin[:, None, :] - w[None, :, :]) ** 2).sum(-1))
            assert d.min() > th + 1.0 and np.sqrt((fin * fin).sum(1)).min() > th + 1.0
    tied = g[case["paired"]]
    if len(tied):
        d = np.sqrt(((tied[:, None, :] - w[None, :, :]) ** 2).sum(-1))
        assert np.all(np.sort(d, axis=1)[:, 0] <= G.LIFT) and np.all(np.sort(d, axis=1)[:, 1] >= 0.75)


def test_lattice_fitness_is_exactly_a_quarter():
    for c in [c for c in G.family_c() if c["name"].startswith("C-lift")] + [c for c in G.stream_cases("half") if c["label"] == "gate3"]:
        p = c["scan"][c["paired"]].astype(np.float64)
        w = G.world().astype(np.float64)
        near = w[np.argmin(((p[:, None, :] - w[None, :, :]) ** 2).sum(-1), axis=1)]
        r = near - p
        norms = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        n = len(p)
        assert n & (n - 1) == 0 and np.all(norms == 0.25)
        assert math.fsum(norms) / n == 0.25
        fwd = 0.0
        for v in norms:
            fwd += v
        pair = norms.copy()
        while len(pair) > 1:                                            # a reduction tree
            pair = pair[0::2] + pair[1::2]
        assert fwd / n == 0.25 and pair[0] / n == 0.25 and norms[::-1].cumsum()[-1] / n == 0.25


def test_balanced_scan_balances():
    for c in [c for c in G.stream_cases("zero") if c["label"] == "gate3"]:
        p = c["scan"].astype(np.float64)
        dz = p[:, 2] - (np.floor(p[:, 2]) + 0.5)
        assert set(np.unique(dz)) == {-0.25, 0.25}
        assert dz.sum() == 0.0 and (dz * p[:, 0]).sum() == 0.0 and (dz * p[:, 1]).sum() == 0.0     # no net force, no net moment


def test_expected_iterations_rule():
    steps = [0.5, 0.2, 0.2, 0.05, 0.0]
    assert G.expected_iterations(steps, 0.0, 5) == 5 and G.expected_iterations(steps, G.TINY, 5) == 5
    assert G.expected_iterations(steps, 0.2, 5) == 4                    # equal does not stop
    assert G.expected_iterations(steps, float(np.nextafter(0.2, np.inf)), 5) == 2
    assert G.expected_iterations(steps, 1.0, 5) == 1 and G.expected_iterations(steps, 0.01, 3) == 3
    assert G.expected_iterations(steps, float("nan"), 5) == 5
    assert not G.fitness_fails(float("nan"), 1.0) and not G.fitness_fails(0.25, float("nan")) and not G.fitness_fails(0.25, 0.25)
    assert G.fitness_fails(0.25, float(np.nextafter(0.25, 0.0)))


def test_stream_cases_interleave_every_ending():
    half, zero = G.stream_cases("half"), G.stream_cases("zero")
    assert {c["label"] for c in half} == {"stop-after-1", "gate2", "gate3", "max-iteration", "gate2-nothing-pairs", "empty-scan"}
    assert {c["label"] for c in zero} == {"stop-after-1", "gate3", "max-iteration", "empty-system", "empty-scan"}
    for cs in (half, zero):
        sizes = [len(c["scan"]) for c in cs]
        assert len(cs) == 24 and min(sizes) == 0 and max(sizes) == 700 and len(set(sizes)) >= 10
    assert all(a["label"] != b["label"] for a, b in zip(half, half[1:]))                            # interleaved: no ending twice in a row


# ---- the oracle gives the stated verdict on every case -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_maps(oracle):
    maps = {}
    for m in (G.P2P, G.GICP, G.VGICP, G.AVGICP):
        om = oracle.Map(G.VOXEL_SIZE, G.VOXEL_CAP)
        om.add_points(G.world())
        if m in (G.VGICP, G.AVGICP):
            om.cal_voxel_cov_all()
        if m == G.GICP:
            om.cal_point_cov_all(G.COV_SEARCH_DIST)
        maps[m] = om
    assert maps[G.P2P].num_points == len(G.world())
    return maps


def _oracle_run(oracle, maps, case):
    ref = oracle.register(maps[case["method"]], case["scan"], case["T0"], oracle.default_config(case["method"], **case["cfg"]))
    return dict(gate=ref["gate"], is_success=ref["is_success"], iterations=ref["iterations"], T=ref["T"], iters=ref["iters"],
                fitness=ref["fitness"] if ref["is_success"] else None)   # the caller's fitness_score is written on success only (reg.cpp:415)


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_oracle_gives_the_stated_verdict(oracle, oracle_maps, case):
    assert G.mismatches(case, _oracle_run(oracle, oracle_maps, case)) == []


@pytest.mark.parametrize("which", ["half", "zero"])
def test_oracle_gives_the_stated_verdict_on_the_stream_cases(oracle, oracle_maps, which):
    for case in G.stream_cases(which):
        got = _oracle_run(oracle, oracle_maps, case)
        assert G.mismatches(case, got) == [], case["name"]
        if case["label"] == "max-iteration":    # the margins its verdict leans on
            thr = case["cfg"]["icp_termination_threshold_m"]
            assert min(i["step_norm"] for i in got["iters"]) > 2.0 * thr and got["fitness"] < 0.5 * case["cfg"]["max_fitness_score"]
        if case["label"] == "gate3":
            assert got["iters"][0]["step_norm"] < 1e-12


# ---- the suite can fail ------------------------------------------------------------------------------------------------------------
def test_wrong_comparators_contradict_the_stated_verdicts():
    cases = G.family_a()

    def contradicted(**rule):
        return sum((2 if G.overlap_fails(c["k"], c["n"], c["thr"], **rule) else 0) != c["expect"]["gate"] for c in cases)
    assert contradicted() == 0                                           # the contract itself agrees with every stated verdict
    f32_only, f64_only, le_only = G.a_disagreements()
    assert contradicted(quotient="f64") == f32_only + f64_only >= G.A_MIN_DISAGREE
    assert contradicted(strict=False) == le_only >= G.A_MIN_DISAGREE
    # termination restated with `<=`: family B's steps are all exactly 0.0, so the rule applied to them gives the stated count when strict
    # and another one for the thresholds 0.0 and -0.0 when not
    fam_b = G.family_b()

    def b_contradicted(strict):
        return sum(G.expected_iterations([0.0] * 5, c["cfg"]["icp_termination_threshold_m"], 5, strict=strict) != c["expect"]["iterations"] for c in fam_b)
    assert b_contradicted(True) == 0 and b_contradicted(False) == 12
    # the fitness gate restated with `>=`, on the cases whose fitness the construction makes exact (0.25, 0.0) or NaN
    fam_c = G.family_c()

    def c_fitness(c):
        return float("nan") if c["name"].startswith("C-nanfit") else G.LIFT if c["name"].startswith("C-lift") else 0.0

    def c_contradicted(strict):
        return sum((3 if G.fitness_fails(c_fitness(c), c["cfg"]["max_fitness_score"], strict=strict) else 0) != c["expect"]["gate"] for c in fam_c)
    assert c_contradicted(True) == 0 and c_contradicted(False) == 7
