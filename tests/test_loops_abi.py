"""The loop consistency check (include/elimaloc_hip_loops.h) on the CPU: the three calls' symbols, signatures and
struct layouts against the fourth signature table, the argument errors that need no device, the C++ shim's call lines, the host-only
pair term against the mirror (tests/loops_ref.py), and the mirror's own properties: the greedy clique is a clique and maximal, equals
the exact maximum on the planted fixture, and breaks ties towards the lowest index."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loops_cases as lcases
import loops_ref as lref
import posegraph_cases as cases
import posegraph_ref as ref
import test_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_loops.h"
NAMES = {"elm_loops_config_default", "elm_loops_pair_terms", "elm_loops_consistency"}
OTHERS = ("elimaloc_hip.h", "elimaloc_hip_posegraph_precond.h", "elimaloc_hip_posegraph_init.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the ABI
def test_the_new_header_against_its_signature_table(L):
    from elimaloc_amd import _lib
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_LOOPS
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_LOOPS == list(table) and len(table) == 3
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params, name
        assert (restype is None) == (ret == "void") and (restype is C.c_int) == (ret == "int"), name
        fn = getattr(L, name)  # exported, and carrying what the table says
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for other in OTHERS:  # no new name in the text of the other three headers, comments aside; one include line and nothing else
        assert not re.search(r"elm_loops|ELM_LOOPS", strip(other)), other
    assert not NAMES & (set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT))
    assert open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read().count("elimaloc_hip_loops") == 1
    assert '#include "elimaloc_hip_loops.h"\n' in open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    src = strip(HEADER)
    assert re.search(r"#define ELM_LOOPS_MAX %d\b" % _lib.LOOPS_MAX, src) and re.search(r"#define ELM_LOOPS_MAX_S %d\b" % _lib.LOOPS_MAX_S, src)
    assert (_lib.LOOPS_MAX, _lib.LOOPS_MAX_S) == (lref.MAX_L, lref.MAX_L_S) == (16384, 2048)
    import __graft_entry__ as g
    assert "EXPORTS_LOOPS" in open(g.__file__).read()  # build()'s missing-symbol check reads the fourth table


def test_struct_layouts_and_defaults(L, tmp_path):
    from elimaloc_amd import _lib
    from elimaloc_amd.loops import LoopConsistencyConfig
    structs = {"elm_loops_config": _lib.LoopsConfigC, "elm_loops_result": _lib.LoopsResultC}
    lines = []
    for name, cls in structs.items():
        offs = ", ".join("offsetof(%s, %s)" % (name, f) for f, _ in cls._fields_)
        lines.append('  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs))
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for row, (name, cls) in zip(rows, structs.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], name
    assert [r[0] for r in rows] == [32, 32]
    c = LoopConsistencyConfig()
    assert {k: getattr(c, k) for k in lref.DEFAULTS} == lref.DEFAULTS and c.reserved == 0
    L.elm_loops_config_default(None)


def test_config_factory_refuses_unknown_names():
    from elimaloc_amd.loops import LoopConsistencyConfig
    c = LoopConsistencyConfig(q_t=0.25, gamma=2, steps_per_batch=np.int64(7))
    assert (c.q_t, c.q_r, c.gamma, c.steps_per_batch) == (0.25, 0.0, 2.0, 7)
    for bad in ("no_such_field", "lambda_init", "_pad"):
        with pytest.raises(AttributeError, match=re.escape("LoopConsistencyConfig has no field " + bad)):
            LoopConsistencyConfig(**{bad: 1})


def test_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.loops import LoopConsistencyConfig
    cfg, res = LoopConsistencyConfig(), _lib.LoopsResultC()
    res.size = 7
    I = np.eye(4).ravel()
    member, degree = np.full(1, 9, np.uint8), np.full(1, 9, np.int32)
    dp, ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_double)), lambda x, t: x.ctypes.data_as(C.POINTER(t))
    # a NULL context is refused before anything is read
    assert L.elm_loops_consistency(None, dp(I), 1, None, None, None, None, None, 0, C.byref(cfg), C.byref(res), ptr(member, C.c_uint8),
                                   ptr(degree, C.c_int32), None, None) == INVALID
    assert res.size == 7 and member[0] == 9 and degree[0] == 9
    e = np.full(6, 5.0)
    bad = I.copy()
    bad[13] = np.nan
    inf = I.copy()
    inf[0] = np.inf
    for args in ([None, I, I, I, I, I], [I, I, I, I, I, None], [I, bad, I, I, I, I], [I, I, I, I, I, inf]):
        assert L.elm_loops_pair_terms(*[None if x is None else dp(np.ascontiguousarray(x)) for x in args], dp(e)) == INVALID
    assert L.elm_loops_pair_terms(*[dp(I)] * 6, None) == INVALID and (e == 5.0).all()
    # the mirror names the same preconditions
    ok = dict(n=4, a=[0, 1], b=[2, 3], Z=np.tile(np.eye(4), (2, 1, 1)), var_t=1.0, var_r=1.0)
    assert lref.refusal(**ok) is None
    for change, why in ((dict(a=[0, 4]), "index"), (dict(b=[2, -1]), "index"), (dict(a=[2, 1]), "a == b"), (dict(var_t=0.0), "variance <= 0"),
                        (dict(var_r=[1.0, -2.0]), "variance <= 0"), (dict(var_t=np.nan), "non-finite variance"), (dict(q_t=-1e-9), "q"),
                        (dict(q_r=np.inf), "q"), (dict(gamma=0.0), "gamma"), (dict(gamma=np.nan), "gamma"), (dict(steps_per_batch=0), "steps_per_batch"),
                        (dict(n=0), "n"), (dict(Z=np.full((2, 4, 4), np.inf)), "non-finite Z")):
        assert lref.refusal(**{**ok, **change}) == why, change
    big = dict(n=4, a=np.zeros(2049, int), b=np.ones(2049, int), Z=np.tile(np.eye(4), (2049, 1, 1)), var_t=1.0, var_r=1.0)
    assert lref.refusal(**big) is None and lref.refusal(**big, want_s=True) == "ELM_LOOPS_MAX_S"


def test_shim_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/loop_consistency_calls.cpp, built as tests/test_posegraph_init_abi.py builds posegraph_init_calls.cpp"""
    exe = tmp_path / "loop_consistency_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "loop_consistency_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the pair term
def _close(e, want, what):
    err = float(np.abs(e - want).max())
    bound = 1e-12 * max(1.0, float(np.abs(want).max()))
    print(f"  {what}: |lib - mirror| {err:.3e} (bound {bound:.1e}), |e| {float(np.abs(want).max()):.3e}")
    assert err <= bound, what


def test_pair_terms_against_the_mirror():
    from elimaloc_amd.loops import PairTerms
    rng = np.random.default_rng(21)
    for trial in range(200):
        T = [cases.rand_pose(rng, 3.0, 10.0) for _ in range(4)]
        Zl = cases.inv_pose(T[2]) @ T[3] @ cases.rand_pose(rng, 0.3, 0.5)
        Zk = cases.inv_pose(T[0]) @ T[1] @ cases.rand_pose(rng, 0.3, 0.5)
        _close(PairTerms(T[0], T[1], Zk, T[2], T[3], Zl), lref.pair_e(T[0], T[1], Zk, T[2], T[3], Zl), f"random pair {trial}")
    # the planted fixture's pairs, each as the library orders it, and their s from the library's e
    p = lcases.planted()
    k, l = np.triu_indices(len(p["a"]), 1)
    worst = 0.0
    for u, v in zip(k, l):
        args = (p["poses"][p["a"][u]], p["poses"][p["b"][u]], p["Z"][u], p["poses"][p["a"][v]], p["poses"][p["b"][v]], p["Z"][v])
        e = PairTerms(*args)
        m = float(abs(int(p["a"][u]) - int(p["a"][v])) + abs(int(p["b"][u]) - int(p["b"][v])))
        s = lref.s_of(e, 2 * p["var_t"], 2 * p["var_r"], m, p["cfg"]["q_t"], p["cfg"]["q_r"])
        worst = max(worst, abs(s - p["s"][u, v]) / max(1.0, abs(p["s"][u, v])))
        assert np.abs(e - lref.pair_e(*args)).max() <= 1e-12 * max(1.0, np.abs(e).max())
    print(f"  planted fixture: s from the library's e against the mirror's, worst relative {worst:.3e}")
    assert worst <= 1e-9


def test_pair_terms_are_exactly_zero_on_an_exact_cycle():
    """integer translations and quarter turns: every product is exact, the cycle composes to the identity, Log(I) is exactly 0"""
    from elimaloc_amd.loops import PairTerms

    def pose(quarter_z, quarter_x, t):
        Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
        Rx = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
        T = np.eye(4)
        T[:3, :3] = np.linalg.matrix_power(Rz, quarter_z) @ np.linalg.matrix_power(Rx, quarter_x)
        T[:3, 3] = t
        return np.round(T)

    T = [pose(1, 0, [3, -2, 5]), pose(2, 1, [7, 7, -1]), pose(3, 3, [-4, 0, 2]), pose(0, 2, [10, -6, 1])]
    Zk = np.round(cases.inv_pose(T[0]) @ T[1])
    Zl = np.round(cases.inv_pose(T[2]) @ T[3])
    e = PairTerms(T[0], T[1], Zk, T[2], T[3], Zl)
    assert (e == 0.0).all() and (lref.pair_e(T[0], T[1], Zk, T[2], T[3], Zl) == 0.0).all()
    Zk[:3, 3] += [1, 0, -2]  # and an integer offset comes back as it is, turned into Z_k's frame
    e = PairTerms(T[0], T[1], Zk, T[2], T[3], Zl)
    assert np.array_equal(e[:3], -(Zk[:3, :3].T @ np.array([1.0, 0.0, -2.0]))) and (e[3:] == 0.0).all()


def test_pair_terms_over_the_rotation_family():
    """the cycle's residual rotation has each angle of posegraph_cases.ROT_FAMILY about a random axis (either side of Log's small-n
    branch, of the series switch, and near pi)"""
    from elimaloc_amd.loops import PairTerms
    rng = np.random.default_rng(22)
    for th in cases.ROT_FAMILY:
        T = [cases.rand_pose(rng, 3.0, 10.0) for _ in range(4)]
        Zl = cases.inv_pose(T[2]) @ T[3] @ cases.rand_pose(rng, 0.3, 0.5)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        E = np.eye(4)
        E[:3, :3] = ref.exp_so3(-th * ax)  # Z_k = Zhat Exp(-phi): R_Zk^T R_Zhat = Exp(phi)
        E[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        Zk = lref.predicted(T[0], T[1], T[2], T[3], Zl) @ E
        e, want = PairTerms(T[0], T[1], Zk, T[2], T[3], Zl), lref.pair_e(T[0], T[1], Zk, T[2], T[3], Zl)
        _close(e, want, f"angle {th!r}")
        assert abs(np.linalg.norm(want[3:]) - th) <= 1e-9 * max(1.0, th) + 1e-14


# ---------------------------------------------------------------- the mirror's clique
def _random_adj(rng, L, density):
    upper = np.triu(rng.uniform(size=(L, L)) < density, 1)
    return upper | upper.T


def test_greedy_clique_is_a_clique_and_maximal():
    rng = np.random.default_rng(23)
    for L, density in ((1, 0.5), (2, 1.0), (5, 0.0), (12, 0.3), (16, 0.6), (16, 0.9), (40, 0.5), (130, 0.5), (130, 0.95)):
        adj = _random_adj(rng, L, density)
        members, degree0 = lref.greedy(adj)
        assert len(set(members)) == len(members) >= 1 and lref.is_clique(adj, members) and lref.is_maximal(adj, members), (L, density)
        assert np.array_equal(degree0, adj.sum(1)) and members[0] == int(np.argmax(degree0))
        if L <= 16:  # never larger than the maximum, and the brute force agrees with itself on clique-ness
            size, cliques = lref.max_clique(adj)
            assert len(members) <= size and all(lref.is_clique(adj, c) for c in cliques)
    assert np.array_equal(lref.unpack(lref.pack(adj), 130)[:, :130], adj) and not lref.unpack(lref.pack(adj), 130)[:, 130:].any()


def test_greedy_equals_the_exact_maximum_on_the_planted_fixture():
    p = lcases.planted()
    assert len(p["a"]) == 13 and int(p["is_true"].sum()) == 8
    members, _ = lref.greedy(p["adj"])
    size, cliques = lref.max_clique(p["adj"])
    print(f"  planted: true-true s <= {p['true_true_max']:.2f}, with a false loop s >= {p['with_false_min']:.1f}, closest to gamma {p['margin']:.2f}")
    assert sorted(members) == list(np.flatnonzero(p["is_true"])) and size == 8 and cliques == [tuple(np.flatnonzero(p["is_true"]))]
    assert lcases.in_band(p["s"], p["cfg"]["gamma"]) == 0


def test_tie_rule_prefers_the_clique_holding_the_lowest_index():
    # two disjoint triangles {1, 3, 5} and {0, 2, 4}: every degree is 2, index 0 is picked first and its triangle follows
    adj = np.zeros((6, 6), bool)
    for tri in ((1, 3, 5), (0, 2, 4)):
        for u in tri:
            for v in tri:
                adj[u, v] = u != v
    members, _ = lref.greedy(adj)
    assert members == [0, 2, 4]
    assert lref.greedy(adj[::-1, ::-1])[0] == [0, 2, 4]  # the relabelled graph: again the triangle of index 0
    assert lref.max_clique(adj) == (3, [(0, 2, 4), (1, 3, 5)])
    # an empty graph keeps index 0 alone
    assert lref.greedy(np.zeros((4, 4), bool))[0] == [0]


def test_the_random_cases_have_no_pair_in_the_band():
    for L in lcases.SIZES:
        c = lcases.random_case(L)
        assert lcases.in_band(c["s"], c["gamma"]) == 0 and lref.refusal(lcases.CHAIN_N, c["a"], c["b"], c["Z"], c["var_t"], c["var_r"]) is None
        if L >= 63:
            density = c["adj"].sum() / (L * (L - 1))
            assert 0.45 <= density <= 0.55, (L, density)
