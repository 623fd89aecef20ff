"""Constructed registrations that sit ON the three discrete decisions of the solve step (tests/test_gate_cases.py on the CPU oracle,
tests/test_solve_gates.py on the device).  Plain numpy, no GPU, no oracle.

The decisions, as registration.hpp / DESIGN.md section 7 word them (reg.cpp:351-356, 385-387, 405-409):

* overlap gate   `corres_ratio = (float)n_corr / n_total;  if (corres_ratio < min_overlap_ratio) fail`  -- the quotient is formed in
  float32, widened, and compared strictly with the double threshold.  Gate 2: not a success, the current pose, fitness untouched.
* termination    `if (step_norm < icp_termination_threshold_m) break` -- strict; else the loop runs to `max_iteration`.
* fitness gate   `if (fitness > max_fitness_score) fail` -- strict, and a NaN on either side compares false: it passes.  Gate 3.

Every case is a dict: the scan (float32, sensor frame), `T0`, the method, config keywords, the verdict the rule demands (`expect`) and a
label saying which decision it straddles and from which side.  The verdicts are derived here, one statement per line, from the rule and
from what the construction makes exact -- never from a run.

One map serves every case: a dyadic lattice of 1 m pitch, 16 x 16 x 4 points at (40.5 + i, 32.5 + j, 0.5 + k), 52 m or more from the
origin, one point per 1 m voxel (so every point is stored, every voxel mean is its point, every 0.4 m neighbourhood is the point alone).
A scan made of stored points, at T0 = I, has residual exactly 0 for P2P, GICP and VGICP: J^T r = 0, x = 0, step_norm = 0, T unchanged.
Unpaired scan points lie more than `max_search_dist` from every map point AND from the world origin (a point without any neighbour
bucket pairs with the origin when that is in range); in the `nan` variants they are NaN points, which count in n_total and never pair.
"""
import math

import numpy as np

P2P, GICP, VGICP, AVGICP = 0, 1, 2, 3
METHOD_NAMES = {P2P: "p2p", GICP: "gicp", VGICP: "vgicp", AVGICP: "avgicp"}
VOXEL_SIZE, VOXEL_CAP = 1.0, 30
SEARCH_DIST = 5.0          # max_search_dist of every case (the shipped default)
COV_SEARCH_DIST = 0.4      # CalPointCovAll for GICP
MAX_ITER_TRACE = 64        # ELM_MAX_ITER_TRACE
TINY = 5e-324              # the smallest positive double
NAN = float("nan")

_CACHE = {}


def world():
    """The map: float32 [1024, 3], inserted in a shuffled order."""
    if "world" not in _CACHE:
        gx, gy, gz = np.meshgrid(40.5 + np.arange(16), 32.5 + np.arange(16), 0.5 + np.arange(4), indexing="ij")
        w = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1)
        _CACHE["world"] = np.ascontiguousarray(w[np.random.default_rng(7301).permutation(len(w))].astype(np.float32))
    return _CACHE["world"]


def stored(n, seed):
    """n distinct map points, picked all over the lattice."""
    w = world()
    return w[np.random.default_rng(seed).permutation(len(w))[:n]].copy()


def far_points(n, seed):
    """n points nowhere near the map or the origin: two boxes, one with negative coordinates, one beyond the +-64 m of the scan order."""
    rng = np.random.default_rng(seed)
    a = rng.uniform([-40.0, -50.0, 10.0], [-20.0, -30.0, 20.0], size=(n, 3))
    b = rng.uniform([110.0, -95.0, 6.0], [140.0, -70.0, 9.0], size=(n, 3))
    return np.where((np.arange(n) % 2 == 0)[:, None], a, b).astype(np.float32)


def nan_points(n):
    """n points that never pair: all three coordinates NaN, or one of them only (every third point x, every third z)."""
    p = np.full((n, 3), np.nan, np.float32)
    for i in range(n):
        if i % 3 == 1:
            p[i] = (np.nan, 33.5, 1.5)   # finite y, z inside the map's box
        elif i % 3 == 2:
            p[i] = (41.5, 34.5, np.nan)
    return p


def unpaired(n, kind, seed):
    return nan_points(n) if kind == "nan" else far_points(n, seed)


def mix(paired, loose, seed):
    """paired and unpaired points interleaved by a fixed permutation -> (scan, mask of the paired points)."""
    pts = np.concatenate([paired, loose]).astype(np.float32)
    mask = np.arange(len(pts)) < len(paired)
    order = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[order]), mask[order]


def generic_pose():
    """a pose that is not the identity (E and the max_iteration <= 0 cases: nothing there needs an exact transform)"""
    c, s = math.cos(0.3), math.sin(0.3)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [1.25, -0.5, 0.125]
    return T


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def quotient32(k, n):
    """(float)k / n as the reference forms it: both operands float32, one float32 division, widened to double.  0 / 0 is NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float32(k) / np.float32(n))


def quotient64(k, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(k) / np.float64(n))


def overlap_fails(k, n, thr, quotient="f32", strict=True):
    """The overlap gate.  quotient / strict select the contract ("f32", True) or one of the two wrong comparators the suite must catch."""
    q = quotient32(k, n) if quotient == "f32" else quotient64(k, n)
    return bool(q < thr) if strict else bool(q <= thr)


def expected_iterations(steps, thr, max_iteration, strict=True):
    """Termination: the loop ends after the FIRST iteration whose step_norm is strictly below thr, else after max_iteration.
    strict=False: the wrong comparator `<=` the suite must catch."""
    for j, s in enumerate(steps[:max_iteration]):
        if (s < thr) if strict else (s <= thr):
            return j + 1
    return max_iteration


def fitness_fails(fitness, max_fitness, strict=True):
    """The fitness gate: strict, NaN on either side passes.  strict=False: the wrong comparator `>=` the suite must catch."""
    return bool(fitness > max_fitness) if strict else bool(fitness >= max_fitness)


def _expect(gate, iterations, n_corr, fitness, pose_is_T0, fixed_point=False, zero_system=False):
    return dict(gate=gate, is_success=(gate == 0), iterations=iterations,
                n_corr=None if n_corr is None else [n_corr] * min(max(iterations, 0), MAX_ITER_TRACE),
                fitness=fitness if gate == 0 else ("none",),            # gates 2 and 3 leave the out-parameter untouched
                pose_is_T0=pose_is_T0, trace_len=min(max(iterations, 0), MAX_ITER_TRACE), fixed_point=fixed_point, zero_system=zero_system)


def _case(name, family, label, method, scan, paired, T0, expect, **cfg):
    cfg.setdefault("max_search_dist", SEARCH_DIST)
    return dict(name=name, family=family, label=label, method=method, scan=np.ascontiguousarray(scan, dtype=np.float32).reshape(-1, 3),
                paired=np.asarray(paired, dtype=bool), T0=np.array(T0, dtype=np.float64), cfg=cfg, expect=expect)


# ---- family A: the overlap gate and its float32 quotient ---------------------------------------------------------------------------
A_NAMED_BELOW = [(7, 10), (5, 6)]   # float32 quotient below the float64 one
A_NAMED_ABOVE = [(1, 3), (3, 10)]   # ... above it
A_PER_DIRECTION = 12
A_AGREE = [(0, 5), (0, 64), (9, 9), (64, 64), (1, 2), (8, 16), (3, 6), (32, 64)]   # k / N of 0, 1 and 1 / 2: both quotients exact


def quotient_pairs():
    """(below, above, n_differ): (k, N) with 1 <= k < N <= 64 in lowest terms whose float32 quotient lies below / above the float64 one, the
    named ones first, the others drawn so that N spreads over 3 .. 63; and how many of ALL pairs k < N <= 64 differ at all."""
    if "pairs" not in _CACHE:
        below, above, differ = [], [], 0
        for n in range(2, 65):
            for k in range(1, n):
                q32, q64 = quotient32(k, n), quotient64(k, n)
                differ += q32 != q64
                if math.gcd(k, n) == 1 and q32 != q64:
                    (below if q32 < q64 else above).append((k, n))

        def pick(pool, named):
            rest = [p for p in pool if p not in named]
            idx = np.random.default_rng(7302).permutation(len(rest))[:A_PER_DIRECTION - len(named)]
            return named + [rest[i] for i in sorted(idx)]
        _CACHE["pairs"] = (pick(below, A_NAMED_BELOW), pick(above, A_NAMED_ABOVE), differ)
    return _CACHE["pairs"]


def thresholds_of(k, n):
    """the six thresholds of a pair: each quotient and its two double neighbours (duplicates dropped, order kept)"""
    out = []
    for name, q in (("q64", quotient64(k, n)), ("q32", quotient32(k, n))):
        for tag, v in ((name, q), (name + "+", float(np.nextafter(q, np.inf))), (name + "-", float(np.nextafter(q, -np.inf)))):
            if not any(v == o[1] and math.copysign(1.0, v) == math.copysign(1.0, o[1]) for o in out):
                out.append((tag, v))
    return out


def a_scan(k, n, index):
    """The scan of a pair: k stored points, n - k unpaired ones (NaN points for every third pair), method rotating P2P / GICP / VGICP."""
    kind = "nan" if index % 3 == 2 else "far"
    scan, mask = mix(stored(k, 7400 + index), unpaired(n - k, kind, 7500 + index), 7600 + index)
    return dict(k=k, n=n, kind=kind, method=(P2P, GICP, VGICP)[index % 3], scan=scan, paired=mask)


def a_scans():
    if "a_scans" not in _CACHE:
        below, above, _ = quotient_pairs()
        _CACHE["a_scans"] = [a_scan(k, n, i) for i, (k, n) in enumerate(below + above + A_AGREE)]
    return _CACHE["a_scans"]


def a_expect(k, n, thr):
    """The verdict of k paired points of n under min_overlap_ratio = thr, max_iteration = 1, max_fitness_score = 100 at T0 = I."""
    if overlap_fails(k, n, thr):                                      # float32 quotient strictly below the threshold
        return _expect(2, 1, k, None, pose_is_T0=True)                # gate 2 in iteration 1: the current pose is T0, no step was taken
    if k == 0:                                                        # passed with nothing paired: the empty system
        return _expect(0, 1, 0, ("nan",), pose_is_T0=True, fixed_point=True, zero_system=True)
    return _expect(0, 1, k, ("exact", 0.0), pose_is_T0=True, fixed_point=True)   # residuals exactly 0: fitness 0 / k, x = 0


def a_case(s, tag, thr):
    k, n = s["k"], s["n"]
    f32, f64 = overlap_fails(k, n, thr), overlap_fails(k, n, thr, quotient="f64")
    c = _case(f"A-{k}of{n}-{METHOD_NAMES[s['method']]}-{s['kind']}-{tag}", "A",
              f"overlap gate, {k}/{n} against {tag} = {thr!r}: float32 {'fails' if f32 else 'passes'}, float64 {'fails' if f64 else 'passes'}",
              s["method"], s["scan"], s["paired"], np.eye(4), a_expect(k, n, thr),
              min_overlap_ratio=thr, max_iteration=1, max_fitness_score=100.0)
    c.update(k=k, n=n, thr=thr, f32_fails=f32, f64_fails=f64, le_fails=overlap_fails(k, n, thr, strict=False))
    return c


def family_a():
    if "A" not in _CACHE:
        out = []
        for s in a_scans():
            ths = thresholds_of(s["k"], s["n"])
            if s["k"] == 0:
                ths = [("zero", 0.0), ("negzero", -0.0), ("tiny", TINY), ("-tiny", -TINY)]
            out += [a_case(s, tag, thr) for tag, thr in ths]
        _CACHE["A"] = out
    return _CACHE["A"]


def a_companions(named):
    """The family-A scans of the named cases' method that are not among them, under their (shared) threshold, each with the verdict the
    rule gives it there: what a ragged batch or a stream runs next to the named cases (one configuration per call)."""
    case, taken = named[0], {(c["k"], c["n"]) for c in named}
    return [a_case(s, "with-" + case["name"], case["thr"]) for s in a_scans() if s["method"] == case["method"] and (s["k"], s["n"]) not in taken]


def a_disagreements(cases=None):
    """(float32 fails where float64 passes, float32 passes where float64 fails, strict passes where <= fails)"""
    cases = family_a() if cases is None else cases
    return (sum(c["f32_fails"] and not c["f64_fails"] for c in cases), sum(c["f64_fails"] and not c["f32_fails"] for c in cases),
            sum(c["le_fails"] and not c["f32_fails"] for c in cases))


A_MIN_DISAGREE = 24       # cases that separate the float32 quotient from the float64 one, half in each direction
_b, _a, _ = quotient_pairs()
assert len(_b) >= A_PER_DIRECTION and len(_a) >= A_PER_DIRECTION and set(A_NAMED_BELOW) <= set(_b) and set(A_NAMED_ABOVE) <= set(_a)
assert all(n <= 64 for _, n in _b + _a + A_AGREE)
_d = a_disagreements()
assert _d[0] >= A_MIN_DISAGREE // 2 and _d[1] >= A_MIN_DISAGREE // 2 and _d[0] + _d[1] >= A_MIN_DISAGREE, _d
assert _d[2] >= A_MIN_DISAGREE, _d   # thresholds EQUAL to the float32 quotient: the strict gate passes them, a `<=` gate would not


# ---- the zero-step scene (families B, C, D) ----------------------------------------------------------------------------------------
def zero_step_scan(n, kind, seed):
    """n stored points (+ n / 8 unpaired ones unless kind is "none") at T0 = I: n_corr = n every iteration, residual exactly 0."""
    pts = stored(n, seed)
    if kind == "none":
        return pts, np.ones(n, bool)
    return mix(pts, unpaired(max(1, n // 8), kind, seed + 1), seed + 2)


def family_b():
    """Termination is strict.  step_norm is exactly 0.0: `0.0 < thr` holds for 5e-324 and 0.02, not for 0.0 or -0.0."""
    out = []
    for method in (P2P, GICP):
        for kind, n in (("none", 64), ("far", 48), ("nan", 40)):
            scan, mask = zero_step_scan(n, kind, 7700 + 10 * method + len(kind))
            for tag, thr, iters in (("zero", 0.0, 5), ("negzero", -0.0, 5), ("tiny", TINY, 1), ("default", 0.02, 1)):
                # 0.0 < 0.0 and 0.0 < -0.0 are false: every iteration goes on, to max_iteration = 5
                # 0.0 < 5e-324 and 0.0 < 0.02 are true: the first iteration ends the run
                # fitness 0 / n = 0.0 passes `0.0 > 0.5`; the ratio n / (n + n / 8) = 8 / 9 passes the default 0.4
                out.append(_case(f"B-{METHOD_NAMES[method]}-{kind}-{tag}", "B", f"termination, step 0.0 against {thr!r}", method, scan, mask, np.eye(4),
                                 _expect(0, iters, n, ("exact", 0.0), pose_is_T0=True, fixed_point=True),
                                 icp_termination_threshold_m=thr, max_iteration=5))
    return out


# ---- family C: the fitness gate ----------------------------------------------------------------------------------------------------
LIFT = 0.25


def lifted_scan(n, kind, seed):
    """n stored points (n a power of two) raised by 0.25 m.  P2P at T0 = I: the raised point stays in its voxel (z = k + 0.75), its own
    lattice point is the nearest (0.25 m; every other one is 0.75 m or more away), each residual norm is sqrt(0.0625) = 0.25 exactly, any
    order of adding n of them is exact (multiples of 0.25 below 2^53) and the quotient by n = 2^m is exact: fitness == 0.25."""
    assert n & (n - 1) == 0
    pts = stored(n, seed).astype(np.float64)
    pts[:, 2] += LIFT
    pts = pts.astype(np.float32)
    if kind == "none":
        return pts, np.ones(n, bool)
    return mix(pts, unpaired(n // 4, kind, seed + 1), seed + 2)


def family_c():
    out = []
    below, above = float(np.nextafter(LIFT, 0.0)), float(np.nextafter(LIFT, 1.0))
    for kind, n in (("none", 32), ("far", 16), ("nan", 64)):
        scan, mask = lifted_scan(n, kind, 7800 + len(kind))
        for tag, thr, gate in (("equal", LIFT, 0), ("below", below, 3), ("above", above, 0), ("nan", NAN, 0)):
            # max_iteration = 1: the run ends after one iteration whatever the step; the pose has moved (no fixed point)
            # 0.25 > 0.25 false: success.  0.25 > nextafter(0.25, 0) true: gate 3.  0.25 > nextafter(0.25, 1) false.  0.25 > NaN false.
            out.append(_case(f"C-lift-{kind}-{tag}", "C", f"fitness gate, fitness 0.25 against {thr!r}", P2P, scan, mask, np.eye(4),
                             _expect(gate, 1, n, ("exact", LIFT), pose_is_T0=False), max_fitness_score=thr, max_iteration=1))
    for method in (P2P, GICP):
        scan, mask = zero_step_scan(32, "far" if method == P2P else "nan", 7810 + method)
        for tag, thr, gate in (("zero", 0.0, 0), ("negzero", -0.0, 0), ("-tiny", -TINY, 3), ("nan", NAN, 0)):
            # fitness 0.0: 0.0 > 0.0 and 0.0 > -0.0 are false, 0.0 > -5e-324 is true, 0.0 > NaN is false; step 0 < 0.02: one iteration
            out.append(_case(f"C-zero-{METHOD_NAMES[method]}-{tag}", "C", f"fitness gate, fitness 0.0 against {thr!r}", method, scan, mask, np.eye(4),
                             _expect(gate, 1, 32, ("exact", 0.0), pose_is_T0=True, fixed_point=True), max_fitness_score=thr))
    for kind in ("far", "nan"):
        scan = unpaired(7, kind, 7820)
        for tag, thr in (("one", 1.0), ("minus-one", -1.0), ("nan", NAN)):
            # nothing pairs, ratio threshold 0: fitness 0 / 0 = NaN; NaN > anything is false: success
            out.append(_case(f"C-nanfit-{kind}-{tag}", "C", f"fitness gate, fitness NaN against {thr!r}", P2P, scan, np.zeros(7, bool), generic_pose(),
                             _expect(0, 1, 0, ("nan",), pose_is_T0=True, fixed_point=True, zero_system=True),
                             max_fitness_score=thr, min_overlap_ratio=0.0))
    return out


# ---- family D: iteration limits ----------------------------------------------------------------------------------------------------
def family_d():
    out = []
    for kind in ("far", "nan"):
        scan, mask = zero_step_scan(24, kind, 7900)
        for mi in (1, 63, 64, 65, 70):
            # threshold 0.0 never stops a zero step: max_iteration iterations, each a fixed point; the trace keeps the first 64
            # (24 of the 27 points pair in every one of them, the 3 far or NaN points never)
            out.append(_case(f"D-run-{kind}-{mi}", "D", f"max_iteration {mi}, never terminating", P2P, scan, mask, np.eye(4),
                             _expect(0, mi, 24, ("exact", 0.0), pose_is_T0=True, fixed_point=True),
                             icp_termination_threshold_m=0.0, max_iteration=mi))
    scan, _ = zero_step_scan(24, "far", 7900)
    far, _ = mix(stored(10, 7901), far_points(30, 7902), 7903)
    nan, _ = mix(stored(10, 7901), nan_points(30), 7903)
    for mi in (0, -3):
        for tag, pts in (("paired", scan), ("unpaired", far), ("nan", nan), ("empty", np.zeros((0, 3), np.float32))):
            # the loop body never runs: 0 iterations, the pose is the guess, d_fitness_score_ is still its initial 0.0 and `0.0 > 0.5` is
            # false: success with fitness 0.0 (no overlap gate was ever evaluated, whatever the scan)
            out.append(_case(f"D-none-{mi}-{tag}", "D", f"max_iteration {mi}: no iteration", P2P, pts, np.zeros(len(pts), bool), generic_pose(),
                             _expect(0, 0, None, ("exact", 0.0), pose_is_T0=True), max_iteration=mi))
    return out


# ---- family E: the empty system ----------------------------------------------------------------------------------------------------
def family_e():
    out = []
    for method in (P2P, GICP, VGICP, AVGICP):
        for kind, n in (("far", 9), ("nan", 5), ("empty", 0)):
            scan = unpaired(n, kind, 8000 + method) if n else np.zeros((0, 3), np.float32)
            # n_corr = 0: all 36 + 6 sums are 0.0, LDLT of the zero matrix gives x = 0, the step is the identity, step_norm 0.0 < 0.02 ends the
            # run after one iteration; ratio 0 / n = 0 is not below 0.0 (an empty scan: 0 / 0 = NaN is below nothing, even the default 0.4);
            # fitness 0 / 0 = NaN passes
            out.append(_case(f"E-{METHOD_NAMES[method]}-{kind}", "E", "empty system: nothing pairs, ratio threshold 0", method, scan, np.zeros(n, bool), generic_pose(),
                             _expect(0, 1, 0, ("nan",), pose_is_T0=True, fixed_point=True, zero_system=True),
                             **({"min_overlap_ratio": 0.0} if n else {})))
    return out


def cfg_key(case):
    """cases with equal keys can share one call (NaN and -0.0 told apart by their repr)"""
    return (case["method"],) + tuple(sorted((k, repr(v)) for k, v in case["cfg"].items()))


def call_groups():
    """The exact cases grouped into calls of one configuration: [(named cases, companions)]; family A's companions are the other scans of
    the method under the case's threshold, the other families share their configuration among their variants."""
    if "groups" not in _CACHE:
        groups = {}
        for c in exact_cases():
            groups.setdefault(cfg_key(c), []).append(c)
        _CACHE["groups"] = [(cs, a_companions(cs) if cs[0]["family"] == "A" else []) for cs in groups.values()]
    return _CACHE["groups"]


def exact_cases():
    """every case whose verdict holds for the oracle and the device alike"""
    if "exact" not in _CACHE:
        _CACHE["exact"] = family_a() + family_b() + family_c() + family_d() + family_e()
        names = [c["name"] for c in _CACHE["exact"]]
        assert len(names) == len(set(names))
    return _CACHE["exact"]


# ---- the own-value straddles (B and C on a run's own recorded values) --------------------------------------------------------------
def straddle_scene():
    """A 3 000-point planar world (ground, two walls, a few posts; 30 m or more from the origin), a 256-point scan taken from it at a known
    pose and a guess 0.2 m / 1 degree away.  Nothing here is exact: the device's own recorded steps and fitness become the thresholds."""
    if "straddle" not in _CACHE:
        rng = np.random.default_rng(8100)
        ground = np.column_stack([rng.uniform(40, 70, 1500), rng.uniform(30, 60, 1500), rng.normal(0.0, 0.01, 1500)])
        wall_a = np.column_stack([rng.uniform(40, 70, 600), np.full(600, 60.0) + rng.normal(0, 0.01, 600), rng.uniform(0, 4, 600)])
        wall_b = np.column_stack([np.full(600, 70.0) + rng.normal(0, 0.01, 600), rng.uniform(30, 60, 600), rng.uniform(0, 4, 600)])
        posts = np.column_stack([50.0 + 5.0 * rng.integers(0, 3, 300) + rng.normal(0, 0.05, 300), 40.0 + 5.0 * rng.integers(0, 3, 300) + rng.normal(0, 0.05, 300),
                                 rng.uniform(0, 3, 300)])
        w = np.concatenate([ground, wall_a, wall_b, posts]).astype(np.float32)
        w = w[rng.permutation(len(w))]
        T = np.eye(4)
        c, s = math.cos(0.4), math.sin(0.4)
        T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = [55.0, 45.0, 1.5]
        pick = w[rng.permutation(len(w))[:256]].astype(np.float64)
        scan = ((pick - T[:3, 3]) @ T[:3, :3] + rng.normal(0, 0.01, (256, 3))).astype(np.float32)   # R^T (p - t) + sensor noise
        a = math.radians(1.0)
        dT = np.eye(4)
        dT[:3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
        dT[:3, 3] = [0.15, -0.1, 0.087]   # |t| = 0.2 m
        _CACHE["straddle"] = (np.ascontiguousarray(w), np.ascontiguousarray(scan), T @ dT)
    return _CACHE["straddle"]


# ---- every ending in one stream ----------------------------------------------------------------------------------------------------
def balanced_scan(groups, seed):
    """4 * groups stored points, half raised and half lowered by 0.25 m so that no rigid motion helps: in every group of four on the corners
    of an axis-parallel rectangle (x1, y1)+ (x2, y2)+ (x1, y2)- (x2, y1)- the forces and the moments cancel.  P2P at T0 = I: every residual
    norm is exactly 0.25 (fitness 0.25 exactly), J^T r cancels up to rounding (a step of ~1e-16, far below the threshold): one iteration."""
    rng = np.random.default_rng(seed)
    pts, used = [], set()
    while len(pts) < 4 * groups:
        i1, i2 = sorted(rng.choice(16, 2, replace=False))
        j1, j2 = sorted(rng.choice(16, 2, replace=False))
        k = int(rng.integers(0, 4))
        quad = [(i1, j1, k, 1), (i2, j2, k, 1), (i1, j2, k, -1), (i2, j1, k, -1)]
        if any(q[:3] in used for q in quad):
            continue
        used.update(q[:3] for q in quad)
        pts += [(40.5 + i, 32.5 + j, 0.5 + kk + LIFT * sg) for i, j, kk, sg in quad]
    return np.array(pts, dtype=np.float32)


STREAM_CFG = {
    # gate 2 needs a positive ratio threshold; the empty SYSTEM (a scan none of whose points pair passing the gate) needs one of 0: two
    # configurations, every other ending in both
    "half": dict(min_overlap_ratio=0.5, max_fitness_score=0.15, max_iteration=2, icp_termination_threshold_m=0.005, max_search_dist=SEARCH_DIST),
    "zero": dict(min_overlap_ratio=0.0, max_fitness_score=0.15, max_iteration=2, icp_termination_threshold_m=0.005, max_search_dist=SEARCH_DIST),
}


def stream_cases(which):
    """24 P2P registrations at T0 = I under STREAM_CFG[which], the endings interleaved, sizes 0 .. 700.
    (ending, scan, verdict); verdict keys as `expect`, with iterations None where the rule leaves them to the run."""
    cfg = STREAM_CFG[which]
    thr = cfg["min_overlap_ratio"]
    out = []

    def add(ending, scan, mask, exp):
        out.append(_case(f"S-{which}-{len(out):02d}-{ending}", "S", ending, P2P, scan, mask, np.eye(4), exp, **cfg))

    for r, (n_stop, n_run, k2, n2, n_bal, n_loose) in enumerate([(700, 256, 300, 700, 64, 33), (257, 64, 1, 3, 16, 1), (1, 512, 127, 257, 128, 300), (64, 16, 31, 64, 4, 64)]):
        kind = "nan" if r % 2 else "far"
        scan, mask = (stored(n_stop, 8200 + r), np.ones(n_stop, bool)) if r % 2 == 0 else mix(stored(n_stop, 8200 + r), unpaired(max(1, n_stop // 16), kind, 8210 + r), 8220 + r)
        # stored points: step 0.0 < 0.005 ends the run after one iteration; fitness 0.0
        add("stop-after-1", scan, mask, _expect(0, 1, n_stop, ("exact", 0.0), pose_is_T0=True, fixed_point=True))
        scan, mask = mix(stored(k2, 8230 + r), unpaired(n2 - k2, kind, 8240 + r), 8250 + r)
        if overlap_fails(k2, n2, thr):     # k2 / n2 is below 0.5 in float32 and float64 alike (0.4286, 0.3333, 0.4942, 0.4844)
            add("gate2", scan, mask, _expect(2, 1, k2, None, pose_is_T0=True))
        else:                              # threshold 0: the same scan passes, and stops on its zero step
            add("stop-after-1", scan, mask, _expect(0, 1, k2, ("exact", 0.0), pose_is_T0=True, fixed_point=True))
        # balanced +-0.25 m: fitness exactly 0.25 > 0.15 after the one iteration its ~1e-16 step allows: gate 3
        bal = balanced_scan(n_bal // 4, 8260 + r)
        add("gate3", bal, np.ones(len(bal), bool), _expect(3, 1, len(bal), ("exact", LIFT), pose_is_T0=False))
        # raised by 0.25 m: two damped steps do not settle it -- both are above the 0.005 threshold, so max_iteration = 2 ends the run, and
        # what the second iteration measures is below 0.15: success.  This one verdict leans on magnitudes, not on exact values:
        # tests/test_gate_cases.py checks on the oracle's trace that both steps are more than twice the threshold (0.075 and 0.012) and the
        # fitness less than half the bound (0.037).
        scan, mask = lifted_scan(n_run, "none", 8270 + r)
        add("max-iteration", scan, mask, _expect(0, 2, n_run, ("finite",), pose_is_T0=False))
        loose = unpaired(n_loose, kind, 8280 + r)
        if overlap_fails(0, n_loose, thr):
            add("gate2-nothing-pairs", loose, np.zeros(n_loose, bool), _expect(2, 1, 0, None, pose_is_T0=True))
        else:
            add("empty-system", loose, np.zeros(n_loose, bool), _expect(0, 1, 0, ("nan",), pose_is_T0=True, fixed_point=True, zero_system=True))
        # an empty scan: 0 / 0 = NaN is not below the threshold, the zero system stops after one iteration, fitness NaN passes
        add("empty-scan", np.zeros((0, 3), np.float32), np.zeros(0, bool), _expect(0, 1, 0, ("nan",), pose_is_T0=True, fixed_point=True, zero_system=True))
    assert len(out) == 24 and max(len(c["scan"]) for c in out) == 700
    return out


# ---- comparing a run with a verdict ------------------------------------------------------------------------------------------------
def mismatches(case, got):
    """Where a run departs from the case's verdict -> list of strings (empty: it complies).
    got: gate, is_success, iterations, fitness (None when the out-parameter was left untouched), T [4, 4] and, where a trace was taken,
    iters: dicts of n_corr, x, step_norm, T, JTJ, JTr."""
    e, bad = case["expect"], []
    for key in ("gate", "is_success", "iterations"):
        if e[key] is not None and got[key] != e[key]:
            bad.append(f"{key}: {got[key]!r}, expected {e[key]!r}")
    f, kind = got["fitness"], e["fitness"][0]
    if kind == "none" and f is not None:
        bad.append(f"fitness {f!r}, expected untouched")
    if kind == "nan" and not (f is not None and math.isnan(f)):
        bad.append(f"fitness {f!r}, expected NaN")
    if kind == "exact" and not (f is not None and f == e["fitness"][1]):
        bad.append(f"fitness {f!r}, expected exactly {e['fitness'][1]!r}")
    if kind == "finite" and not (f is not None and math.isfinite(f)):
        bad.append(f"fitness {f!r}, expected a finite number")
    T0 = case["T0"]
    if e["pose_is_T0"] and not np.array_equal(np.asarray(got["T"]), T0):
        bad.append("the returned pose is not the initial guess bit for bit")
    its = got.get("iters")
    if its is None:
        return bad
    if len(its) != e["trace_len"]:
        bad.append(f"{len(its)} trace entries, expected {e['trace_len']}")
    if e["n_corr"] is not None and [int(i["n_corr"]) for i in its] != e["n_corr"]:
        bad.append(f"n_corr per iteration {[int(i['n_corr']) for i in its]}, expected {e['n_corr']}")
    if e["gate"] == 3 and its and not np.array_equal(np.asarray(got["T"]), its[-1]["T"]):
        bad.append("gate 3: the returned pose is not the current estimate (the last iteration's)")
    if e["fixed_point"] and e["gate"] == 0:
        for j, i in enumerate(its):
            if not (np.all(np.asarray(i["x"]) == 0.0) and i["step_norm"] == 0.0 and np.array_equal(np.asarray(i["T"]), T0)):
                bad.append(f"iteration {j + 1} is not a fixed point: x {np.asarray(i['x'])}, step {i['step_norm']!r}")
                break
    if e["zero_system"]:
        for j, i in enumerate(its):
            if np.any(np.asarray(i["JTJ"]) != 0.0) or np.any(np.asarray(i["JTr"]) != 0.0):
                bad.append(f"iteration {j + 1}: the sums of an empty system are not all zero")
                break
    return bad
