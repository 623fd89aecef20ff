"""The solve step's three discrete decisions -- overlap gate, termination, fitness gate (k_solve; the degenerate-call branches of the
host API) -- on the device, at their thresholds.  tests/gate_cases.py builds the registrations and states each verdict from the rule;
tests/test_gate_cases.py shows on the CPU that the oracle gives those verdicts and that a float64 quotient or a `<=` would not.

Every exact case runs through every driver that can take it:
  elm_register on the caller's buffer (C ABI, with a sentinel in the fitness out-parameter), elm_register_batch on the resident scan alone
  and inside a ragged batch with the other cases of its configuration, elm_register_stream with 2 slots and more registrations than
  slots, elm_register_stream_host, and a two-rank device group on one GPU (host buffers cut unevenly, resident scans, a stream).
One call has ONE configuration, so a ragged batch holds the cases that share the case's configuration; for family A those are the other
(k, N) scans of the method under the case's threshold, each with the verdict the rule gives it there.
Not taken, and why: elm_register_stream_host on a device group (host-fed streams run on one rank: slot assignment follows scan
arrival)."""
import ctypes as C

import numpy as np
import pytest

import gate_cases as G

pytestmark = pytest.mark.gpu

GROUPS = G.call_groups()
SENTINEL = -7.5          # what the fitness out-parameter holds before elm_register: it must still hold it after gate 2 or 3


class _Rig:
    """one context with the map prepared for every method, resident scans uploaded once"""

    def __init__(self, ctx, points):
        from elimaloc_amd.registration import VoxelHashMap
        self.ctx, self.maps, self.scans = ctx, {}, {}
        for m in (G.P2P, G.GICP, G.VGICP, G.AVGICP):
            vm = VoxelHashMap(G.VOXEL_SIZE, G.VOXEL_CAP, ctx)
            vm.AddPoints(points)
            if m in (G.VGICP, G.AVGICP):
                vm.CalVoxelCovAll()
            if m == G.GICP:
                vm.CalPointCovAll(G.COV_SEARCH_DIST)
            self.maps[m] = vm

    def scan(self, xyz):
        from elimaloc_amd.registration import Scan
        key = xyz.tobytes()
        if key not in self.scans:
            self.scans[key] = Scan(self.ctx, xyz)
        return self.scans[key]

    def reg(self, case):
        from elimaloc_amd.registration import Registration, RegistrationConfig
        return Registration(RegistrationConfig(icp_method=case["method"], **case["cfg"]), self.ctx)

    def close(self):
        for s in self.scans.values():
            s.close()
        self.scans.clear()
        for vm in self.maps.values():
            vm.Clear()
        self.maps.clear()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    from elimaloc_amd.registration import Context
    r = _Rig(Context(0), G.world())
    yield r
    r.close()


@pytest.fixture(scope="module")
def group_rig():
    """the two-rank group, in a context of its own"""
    from elimaloc_amd.registration import Context
    g = Context.multi([0, 0])
    assert g.group_info() == (2, 2, [0, 0])
    r = _Rig(g, G.world())
    yield r
    r.close()


def _got(r):
    if not r["is_success"]:
        assert r["fitness_score"] == 0.0   # elm_reg_result.fitness_score is written on success only
    return dict(gate=r["gate"], is_success=r["is_success"], iterations=r["iterations"], T=r["T"], iters=r.get("iters"),
                fitness=r["fitness_score"] if r["is_success"] else None)


def _register_abi(rig, case, scan=None):
    """elm_register as a C caller sees it: the fitness out-parameter holds SENTINEL before the call"""
    from elimaloc_amd import _lib
    from elimaloc_amd.registration import RegistrationConfig, _colmajor16, _dp, _fp, _result_dict
    scan = np.ascontiguousarray(case["scan"] if scan is None else scan, dtype=np.float32).reshape(-1, 3)
    cfg = RegistrationConfig(icp_method=case["method"], **case["cfg"])
    T0 = _colmajor16(case["T0"])
    Tout = np.full(16, np.nan); ok = C.c_int(-1); fit = C.c_double(SENTINEL); cov = np.empty(36)
    res = _lib.RegResult()
    tr = (_lib.IterTrace * _lib.MAX_ITER_TRACE)()
    _lib.check(_lib.lib().elm_register(rig.ctx._h, rig.maps[case["method"]]._handle(), _fp(scan), scan.shape[0], _dp(T0), C.byref(cfg), _dp(Tout),
                                       C.byref(ok), C.byref(fit), _dp(cov), C.byref(res), tr), rig.ctx._h, "elm_register")
    d = _result_dict(res, tr)
    assert bool(ok.value) == d["is_success"] and np.array_equal(Tout.reshape(4, 4).T, d["T"])
    untouched = np.float64(fit.value).tobytes() == np.float64(SENTINEL).tobytes()
    assert untouched == (not d["is_success"]), f"fitness out-parameter {fit.value!r} with is_success {d['is_success']}"
    if d["is_success"]:
        assert np.float64(fit.value).tobytes() == np.float64(d["fitness_score"]).tobytes()
    return d


def _iter_bytes(i):
    return b"".join(np.asarray(i[k], dtype=np.float64).tobytes() for k in ("JTJ", "JTr", "residual_sum", "n_corr", "x", "step_norm", "T"))


def _sig(r):
    """every byte a registration hands back that does not depend on the driver"""
    return [r["T"].tobytes(), r["local_cov"].tobytes(), (r["iterations"], r["is_success"], r["gate"]),
            np.array([r["fitness_score"], r["d_fitness"], r["n_corr_last"], r["point_iterations"]]).tobytes()] + [_iter_bytes(i) for i in r.get("iters") or []]


def _complies(case, r, where):
    bad = G.mismatches(case, _got(r))
    assert bad == [], f"{case['name']} ({case['label']}) through {where}: {bad}"


def _paired_at_one_end(case, last):
    """the caller's buffer reordered so that a contiguous cut separates paired from unpaired points"""
    order = np.argsort(case["paired"] if last else ~case["paired"], kind="stable")
    return np.ascontiguousarray(case["scan"][order])


def _ids(groups):
    return [cs[0]["name"] + (f"+{len(cs) + len(co) - 1}" if len(cs) + len(co) > 1 else "") for cs, co in groups]


@pytest.mark.parametrize("named,companions", GROUPS, ids=_ids(GROUPS))
def test_stated_verdict_on_every_driver(rig, named, companions):
    vm, reg = rig.maps[named[0]["method"]], rig.reg(named[0])
    alone = {}
    for c in named:
        _complies(c, _register_abi(rig, c), "elm_register")
        alone[c["name"]] = reg.RunRegisterBatch([rig.scan(c["scan"])], vm, [c["T0"]], trace=True)[0]
        _complies(c, alone[c["name"]], "elm_register_batch alone")
    allc = named + companions
    while len(allc) < 3:                                       # more registrations than the stream's 2 slots
        allc = allc + named
    scans, T0s = [rig.scan(c["scan"]) for c in allc], [c["T0"] for c in allc]
    runs = {"a ragged elm_register_batch": reg.RunRegisterBatch(scans, vm, T0s, trace=True),
            "elm_register_stream, 2 slots": reg.RunRegisterStream(scans, vm, T0s, slots=2, trace=True),
            "elm_register_stream_host, 2 slots": reg.RunRegisterStreamHost(reg.pack_host_inputs([c["scan"] for c in allc], T0s), vm, slots=2, trace=True)}
    for where, out in runs.items():
        for c, r in zip(allc, out):
            _complies(c, r, where)
            if c["name"] in alone:
                assert _sig(r) == _sig(alone[c["name"]]), f"{c['name']} through {where} differs from the same registration alone"


@pytest.mark.parametrize("named,companions", GROUPS, ids=_ids(GROUPS))
def test_stated_verdict_on_a_two_rank_group(group_rig, named, companions):
    """the gate must use the whole scan's n_total and the all-reduced n_corr, whichever rank holds the paired points"""
    rig = group_rig
    vm, reg = rig.maps[named[0]["method"]], rig.reg(named[0])
    for c in named:
        _complies(c, _register_abi(rig, c), "elm_register on the group")
        # the caller's order cut in two: paired points first (rank 1 gets none of them when k <= N / 2), then last (rank 0 gets none)
        for last in (False, True):
            _complies(c, _register_abi(rig, c, _paired_at_one_end(c, last)), "elm_register on the group, paired points at one end")
    allc = named + companions
    while len(allc) < 3:
        allc = allc + named
    scans, T0s = [rig.scan(c["scan"]) for c in allc], [c["T0"] for c in allc]
    for where, out in (("elm_register_batch on the group", reg.RunRegisterBatch(scans, vm, T0s, trace=True)),
                       ("elm_register_stream on the group, 2 slots", reg.RunRegisterStream(scans, vm, T0s, slots=2, trace=True))):
        for c, r in zip(allc, out):
            _complies(c, r, where)


def test_group_shards_are_uneven_and_some_hold_no_paired_point(group_rig):
    """what the group test above leans on: odd scans (the cut is uneven), and ranks without a single paired point -- in the caller's
    order reordered by _paired_at_one_end, and in the resident scans' own spatial order"""
    odd_starved = [c for c in G.family_a() if c["n"] % 2 == 1 and 0 < c["k"] <= c["n"] // 2]
    assert len({(c["k"], c["n"]) for c in odd_starved}) >= 5
    w = G.world().astype(np.float64)
    lo, hi = w.min(0) - 0.5, w.max(0) + 0.5
    starved = 0
    for s in G.a_scans():
        if s["k"] == 0:
            continue
        pts = group_rig.scan(s["scan"]).points().astype(np.float64)   # rank 0's shard, then rank 1's
        inside = np.all((pts >= lo) & (pts <= hi), axis=1)
        assert int(inside.sum()) == s["k"]
        cut = len(pts) // 2
        starved += (not inside[:cut].any()) or (not inside[cut:].any())
    assert starved >= 3


# ---- the own-value straddles -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def straddle(rig):
    """the straddle scene on the plain context: its map prepared per method and its resident scan, released explicitly"""
    from elimaloc_amd.registration import Scan, VoxelHashMap
    world, scan, T0 = G.straddle_scene()
    maps = {}
    for m in (G.P2P, G.VGICP):
        maps[m] = VoxelHashMap(G.VOXEL_SIZE, G.VOXEL_CAP, rig.ctx)
        maps[m].AddPoints(world)
    maps[G.VGICP].CalVoxelCovAll()
    res = Scan(rig.ctx, scan)
    yield dict(maps=maps, scan=scan, resident=res, T0=T0)
    res.close()
    for vm in maps.values():
        vm.Clear()


def _straddle_run(ctx, vm, method, driver, scan_host, scan_res, T0, **cfg):
    from elimaloc_amd.registration import Registration, RegistrationConfig
    reg = Registration(RegistrationConfig(icp_method=method, **cfg), ctx)
    if driver == "host":
        return reg.RunRegister(scan_host, vm, T0, trace=True)[-1]
    if driver == "batch":
        return reg.RunRegisterBatch([scan_res], vm, [T0], trace=True)[0]
    return reg.RunRegisterStream([scan_res] * 3, vm, [T0] * 3, slots=2, trace=True)[2]


@pytest.mark.parametrize("driver", ["host", "batch", "stream"])
@pytest.mark.parametrize("method", [G.P2P, G.VGICP])
def test_own_value_straddles(rig, straddle, method, driver):
    """A run's own recorded step norms and fitness as the thresholds of its re-runs: a threshold EQUAL to the step must not stop, the next
    double above it must; max_fitness_score EQUAL to the fitness succeeds, the next double below it is gate 3.  The run is deterministic,
    so the expectation is the rule applied to the recorded values -- no tolerance.  (The oracle is not asked here: its sums differ from
    the device's at 1e-13, so at a one-ulp threshold it may rightly land on the other side.)"""
    vm, scan, res, T0 = straddle["maps"][method], straddle["scan"], straddle["resident"], straddle["T0"]
    run = lambda **cfg: _straddle_run(rig.ctx, vm, method, driver, scan, res, T0, max_iteration=8, **cfg)   # noqa: E731
    base = run(icp_termination_threshold_m=0.0)
    steps = [i["step_norm"] for i in base["iters"]]
    fit = base["fitness_score"]
    assert base["iterations"] == 8 and base["is_success"] and len(steps) == 8 and all(s > 0.0 for s in steps) and 0.0 < fit < 0.5
    assert _sig(run(icp_termination_threshold_m=0.0)) == _sig(base)                                       # deterministic
    for j in (1, 2, 3):
        for thr in (steps[j], float(np.nextafter(steps[j], np.inf))):
            want = G.expected_iterations(steps, thr, 8)
            r = run(icp_termination_threshold_m=thr)
            assert r["iterations"] == want, f"threshold {thr!r} against step {steps[j]!r}: {r['iterations']} iterations, the rule gives {want}"
            assert r["is_success"] and len(r["iters"]) == want
            assert [_iter_bytes(i) for i in r["iters"]] == [_iter_bytes(i) for i in base["iters"][:want]]
            assert np.array_equal(r["T"], base["iters"][want - 1]["T"])
            assert r["fitness_score"] == base["iters"][want - 1]["residual_sum"] / base["iters"][want - 1]["n_corr"]
    ok = run(icp_termination_threshold_m=0.0, max_fitness_score=fit)
    assert ok["is_success"] and ok["gate"] == 0 and _sig(ok) == _sig(base)
    gate3 = run(icp_termination_threshold_m=0.0, max_fitness_score=float(np.nextafter(fit, -np.inf)))
    assert not gate3["is_success"] and gate3["gate"] == 3 and gate3["iterations"] == 8 and gate3["fitness_score"] == 0.0
    assert np.array_equal(gate3["T"], base["T"]) and gate3["d_fitness"] == fit                            # the current estimate is returned


# ---- every ending in one stream ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["half", "zero"])
def test_every_ending_in_one_stream(rig, which):
    """24 registrations through 3 slots, the endings interleaved (each leaves through another branch of finish_slot and the refill), sizes
    0 .. 700: resident and host-fed, twice -- the stated verdicts, and every byte of every result and trace as from the registration alone"""
    cases = G.stream_cases(which)
    vm, reg = rig.maps[G.P2P], rig.reg(cases[0])
    scans, T0s = [rig.scan(c["scan"]) for c in cases], [c["T0"] for c in cases]
    alone = [reg.RunRegisterBatch([s], vm, [T0], trace=True)[0] for s, T0 in zip(scans, T0s)]
    packed = reg.pack_host_inputs([c["scan"] for c in cases], T0s)
    for where, call in (("elm_register_stream", lambda: reg.RunRegisterStream(scans, vm, T0s, slots=3, trace=True)),
                        ("elm_register_stream_host", lambda: reg.RunRegisterStreamHost(packed, vm, slots=3, trace=True))):
        first, second = call(), call()
        for c, a, r1, r2 in zip(cases, alone, first, second):
            _complies(c, a, "elm_register_batch alone")
            _complies(c, r1, where)
            assert _sig(r1) == _sig(a), f"{c['name']} through {where} differs from the same registration alone"
            assert _sig(r2) == _sig(r1), f"{c['name']} through {where}: two runs differ"
    assert len({(r["gate"], r["iterations"]) for r in alone}) >= 3


@pytest.mark.parametrize("which", ["half", "zero"])
def test_every_ending_in_one_stream_on_a_two_rank_group(group_rig, which):
    rig, cases = group_rig, G.stream_cases(which)
    vm, reg = rig.maps[G.P2P], rig.reg(cases[0])
    scans, T0s = [rig.scan(c["scan"]) for c in cases], [c["T0"] for c in cases]
    alone = [reg.RunRegisterBatch([s], vm, [T0], trace=True)[0] for s, T0 in zip(scans, T0s)]
    first = reg.RunRegisterStream(scans, vm, T0s, slots=3, trace=True)
    second = reg.RunRegisterStream(scans, vm, T0s, slots=3, trace=True)
    for c, a, r1, r2 in zip(cases, alone, first, second):
        _complies(c, r1, "elm_register_stream on the group")
        assert _sig(r1) == _sig(a), f"{c['name']} through the group's stream differs from the same registration alone on the group"
        assert _sig(r2) == _sig(r1), f"{c['name']}: two runs of the group's stream differ"
