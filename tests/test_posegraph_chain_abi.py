"""The pose graph's chain preconditioner (include/elimaloc_hip_posegraph_precond.h) on the CPU: the two calls'
symbols and argument errors without a device, the C++ shim's call lines, and the algebra of the mirror (tests/posegraph_chain_ref.py):
the chain edges, M symmetric and positive definite, the conjugate gradients against the dense solve, and the 12 L + 1 bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_cases as ccases
import posegraph_chain_ref as cref
import posegraph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NAMES = {"elm_posegraph_set_preconditioner", "elm_posegraph_get_preconditioner"}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the ABI
def test_symbols_are_declared_and_exported(L):
    from elimaloc_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "elimaloc_hip_posegraph_precond.h")).read(), flags=re.S)
    assert NAMES == set(re.findall(r"\b(elm_[a-z0-9_]+)\s*\(", src)) == set(_lib.EXPORTS_PRECOND)
    for n in NAMES:
        assert hasattr(L, n)
    for k, v in _lib.PG_PRECOND.items():
        assert re.search(r"#define ELM_PG_PRECOND_%s %d\b" % (v.upper(), k), src), v
    main = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    assert '#include "elimaloc_hip_posegraph_precond.h"' in main
    probe = '#include "elimaloc_hip.h"\nint main(void) { return elm_posegraph_set_preconditioner(0, 0, ELM_PG_PRECOND_CHAIN) == ELM_ERR_INVALID ? 0 : 1; }\n'
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=probe.encode(), check=True)


def test_invalid_arguments_without_device(L):
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    kind = C.c_int(7)
    assert L.elm_posegraph_set_preconditioner(None, one, 0) == INVALID and L.elm_posegraph_set_preconditioner(one, None, 1) == INVALID
    for bad in (-1, 2, 3, 1 << 20):
        assert L.elm_posegraph_set_preconditioner(one, one, bad) == INVALID, bad
    assert L.elm_posegraph_get_preconditioner(None, one, C.byref(kind)) == INVALID
    assert L.elm_posegraph_get_preconditioner(one, None, C.byref(kind)) == INVALID
    assert L.elm_posegraph_get_preconditioner(one, one, None) == INVALID and kind.value == 7
    from elimaloc_amd._lib import ElmError
    from elimaloc_amd.posegraph import PoseGraph
    pg = PoseGraph.__new__(PoseGraph)  # no device: the name is checked before the library is asked
    with pytest.raises(ElmError, match="none of"):
        pg.SetPreconditioner("jacobi")


def test_shim_chain_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/posegraph_chain_calls.cpp, built as tests/test_posegraph_abi.py builds posegraph_calls.cpp"""
    exe = tmp_path / "posegraph_chain_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "posegraph_chain_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the chain edges
def _edges(g):
    return cref.chain_edges(g, ref.linearize(g))


def test_chain_edges_of_a_plain_chain_and_of_a_star():
    g = cases.chain(12, 2)
    edge, rev = _edges(g)
    assert edge.tolist() == [-1] + list(range(1, 11)) and not rev.any()  # node 0 is fixed: no chain edge between 0 and 1
    edge, rev = _edges(cases.star(5, 3))
    assert edge.tolist() == [-1] * 5  # leaf 1 is fixed; no other edge joins neighbours in index


def test_chain_edges_pick_the_lowest_index_of_a_duplicate():
    g = ccases.duplicate_edge(at=3)
    assert (int(g.i[-1]), int(g.j[-1])) == (4, 3) and (int(g.i[3]), int(g.j[3])) == (3, 4)
    edge, rev = _edges(g)
    assert edge[3] == 3 and not rev[3]
    # the reversed copy first, the forward one after it: still the lowest index
    order = np.concatenate([[g.E - 1], np.arange(g.E - 1)])
    g2 = ref.Graph(g.poses, g.fixed, g.i[order], g.j[order], g.Z[order], g.info[order])
    edge, rev = _edges(g2)
    assert edge[3] == 0 and rev[3] and edge[4] == 5


def test_chain_edges_accept_a_reversed_edge():
    g = ccases.reversed_edge(at=4)
    assert (int(g.i[4]), int(g.j[4])) == (5, 4)
    edge, rev = _edges(g)
    assert edge[4] == 4 and rev[4] and rev.sum() == 1
    lin = ref.linearize(g)
    M = cref.chain_matrix(g, lin, 0.0)
    assert np.array_equal(M[6 * 5:6 * 6, 6 * 4:6 * 5], lin["Hij"][4]) and np.array_equal(M[6 * 4:6 * 5, 6 * 5:6 * 6], lin["Hij"][4].T)
    assert np.array_equal(M[6 * 3:6 * 4, 6 * 4:6 * 5], lin["Hij"][3])


def test_chain_edges_break_at_a_fixed_node_and_at_a_missing_edge():
    edge, _ = _edges(ccases.fixed_interior(at=5))
    assert edge.tolist() == [-1, 1, 2, 3, -1, -1, 6, 7, 8, 9, 10]
    g = ccases.missing_edge(at=6)
    edge, _ = _edges(g)
    assert edge.tolist() == [-1, 1, 2, 3, 4, 5, -1, 6, 7, 8, 9]  # the edges after the removed one moved down by one
    edge, _ = _edges(ccases.isolated_free_node())
    assert edge[-1] == -1  # a free node without an edge is not active
    assert (_edges(cases.random_graph(6, 8, 33, fixed=range(6)))[0] == -1).all()


# ---------------------------------------------------------------- M and the conjugate gradients
@pytest.mark.parametrize("name", list(ccases.SMALL))
def test_chain_matrix_is_symmetric_positive_definite(name):
    g = ccases.SMALL[name]()
    lin = ref.linearize(g, huber_k=1.5)
    for lam in (0.0, 1.0):  # every fixture has a fixed node
        M = cref.chain_matrix(g, lin, lam, sparse=False)
        Ms = cref.chain_matrix(g, lin, lam, sparse=True).toarray()
        # (the summed diagonal blocks are symmetric to rounding, as the mirror's H is; the chain blocks are exact transposes)
        assert np.array_equal(M, Ms) and np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
        low = float(np.linalg.eigvalsh((M + M.T) / 2.0).min())
        print(f"{name} lambda {lam}: smallest eigenvalue of M {low:.3e}")
        assert low > 0.0
        # H - M: nothing on the block diagonal, nothing on a chain edge's block
        H, _ = ref.dense_system(g, lin, lam)
        R = (H - M).reshape(g.N, 6, g.N, 6)
        edge, _ = cref.chain_edges(g, lin)
        assert all(np.abs(R[v, :, v, :]).max() <= 1e-12 * np.abs(H).max() for v in range(g.N))
        if not np.array_equal(g.i, ccases.duplicate_edge().i):  # (there H carries both edges of the pair, M the first alone)
            assert all(np.abs(R[v, :, v + 1, :]).max() <= 1e-12 * np.abs(H).max() for v in np.flatnonzero(edge >= 0))


@pytest.mark.parametrize("name", list(ccases.SMALL))
def test_mirror_pcg_chain_reaches_the_dense_solution(name):
    g = ccases.SMALL[name]()
    lin = ref.linearize(g, huber_k=1.5)
    for lam in (0.0, 1.0):
        H, b = ref.dense_system(g, lin, lam)
        delta, its, rel, conv = cref.pcg_chain(g, lin, lam, 1e-10, 500)
        x = np.linalg.solve(H, b).reshape(g.N, 6)
        rho = cref.true_rel_residual(g, lin, lam, delta)
        _, its_bj, _, _ = ref.pcg(g, lin, lam, 1e-10, 500)
        print(f"{name} lambda {lam}: {its} iterations (block Jacobi {its_bj}), recurrence residual {rel:.2e}, true relative residual {rho:.2e}")
        assert conv and rho <= 1e-8 and np.abs(delta - x).max() <= 1e-7 * max(1.0, np.abs(x).max())  # the bounds of the block-Jacobi mirror test
        assert (delta[~lin["active"]] == 0.0).all() and its <= its_bj


@pytest.mark.parametrize("N,seed,loops", ccases.RANK_BOUND)
def test_mirror_converges_within_twelve_per_loop_plus_one(N, seed, loops):
    g = cases.chain(N, seed, loops=loops)
    lin = ref.linearize(g)
    edge, _ = cref.chain_edges(g, lin)
    # the non-chain edges: the loops, and the odometry edge 0 -> 1 whose block the fixed node 0 takes out of H anyway
    assert (edge >= 0).sum() == N - 2 and g.E - (N - 1) == loops
    _, its, rel, conv = cref.pcg_chain(g, lin, 0.0, 1e-10, 12 * loops + 1)
    print(f"chain({N}, {seed}, loops={loops}) lambda 0: {its} iterations of at most {12 * loops + 1}, recurrence residual {rel:.2e}")
    assert conv and its <= 12 * loops + 1


def test_sparse_and_dense_solvers_agree():
    g = cases.chain(70, 2)
    lin = ref.linearize(g)
    r = np.where(lin["active"][:, None], -lin["grad"], 0.0)
    zd, zs = cref.chain_solver(g, lin, 0.5, sparse=False)(r), cref.chain_solver(g, lin, 0.5, sparse=True)(r)
    assert np.abs(zd - zs).max() <= 1e-12 * max(1.0, np.abs(zd).max()) and cref.backward_error(g, lin, 0.5, zd, r) <= 1e-14
