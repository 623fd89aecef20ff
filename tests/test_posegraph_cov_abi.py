"""The pose graph's covariances (include/elimaloc_hip_posegraph_cov.h) on the CPU: the three calls' symbols,
signatures and struct layouts against the sixth signature table, the gcc probe of the header, the argument errors that need no device,
the C++ shim's call lines, and the mirror alone (tests/posegraph_cov_ref.py): its product against posegraph_ref.spmv, and its columns
against the dense inverse within 1 x bound on every case of the GPU test -- the condition that lets the GPU test use a margin of 2.

The mirror's largest |Sigma_mirror - Sigma_dense| / bound over the dense cases is 0.0024 (chain-257, block Jacobi); every case converges.
The chain cases under block Jacobi take 330 (33 nodes), 9 200 (257) and 15 600 (513) iterations per column, so the mirror solves all
columns of every case but chain-513 under block Jacobi, where it solves the columns of nodes 257 and 512 (12 of the 42; about 4 ms of
numpy per iteration otherwise).  The pure chain of 65 537 nodes is held against the block-Thomas solve: 0.22 of its bound, 1 or 2
iterations per column; posegraph_cov_ref.pure_chain says why it has a fixed node every 1000 and not node 0 alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_cov_ref as cov
import posegraph_ref as ref
import test_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
HEADER = "elimaloc_hip_posegraph_cov.h"
NAMES = {"elm_posegraph_cov_config_default", "elm_posegraph_covariance", "elm_posegraph_relative_covariance"}
OTHERS = ("elimaloc_hip.h", "elimaloc_hip_posegraph_precond.h", "elimaloc_hip_posegraph_init.h", "elimaloc_hip_loops.h", "elimaloc_hip_loopcov.h")
MIRROR_NODES = {"chain-513": [257, 512]}  # the docstring says why


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
    protos, table = test_binding._prototypes(HEADER), _lib.DECLS_PGCOV
    assert set(protos) == set(table) == NAMES and _lib.EXPORTS_PGCOV == list(table) and len(table) == 3
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params, name
        assert (restype is None and ret == "void") or (restype is C.c_int and ret == "int"), name
        fn = getattr(L, name)  # exported, and carrying what the table says
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert [len(table[n][1]) for n in ("elm_posegraph_cov_config_default", "elm_posegraph_covariance", "elm_posegraph_relative_covariance")] == [1, 12, 8]
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for other in OTHERS:  # no new name in the text of the other headers, comments aside; one include line and nothing else
        assert not re.search(r"elm_posegraph_cov|elm_posegraph_relative", strip(other)), other
    assert not NAMES & (set(_lib.EXPORTS) | set(_lib.EXPORTS_PRECOND) | set(_lib.EXPORTS_INIT) | set(_lib.EXPORTS_LOOPS) | set(_lib.EXPORTS_LOOPCOV))
    top = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    assert top.count("elimaloc_hip_posegraph_cov") == 1 and '#include "elimaloc_hip_loopcov.h"\n#include "elimaloc_hip_posegraph_cov.h"\n' in top
    import __graft_entry__ as g
    assert "EXPORTS_PGCOV" in open(g.__file__).read()  # build()'s missing-symbol check reads the sixth table


def test_the_header_compiles_as_c():
    probe = ('#include "elimaloc_hip.h"\nint main(void) { elm_posegraph_cov_config c; elm_posegraph_cov_stats s; elm_posegraph_cov_config_default(&c);\n'
             '  s.n_columns = 0; return elm_posegraph_covariance(0, 0, 0, 0, 0, 0, &c, 0, 0, 0, 0, &s) == ELM_ERR_INVALID && s.n_columns == 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=probe.encode(), check=True)


def test_struct_layouts(L, tmp_path):
    from elimaloc_amd import _lib
    structs = (("elm_posegraph_cov_config", _lib.PoseGraphCovConfigC, {"lambda_": "lambda"}, 32), ("elm_posegraph_cov_stats", _lib.PoseGraphCovStatsC, {}, 40))
    lines = []
    for name, cls, rename, _ in structs:
        offs = ", ".join("offsetof(%s, %s)" % (name, rename.get(f, f)) for f, _ in cls._fields_)
        lines.append('  printf("%s\\n", sizeof(%s), %s);' % (" ".join(["%zu"] * (len(cls._fields_) + 1)), name, offs))
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "elimaloc_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0; }\n"
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(probe)
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    rows = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    for (name, cls, _, size), row in zip(structs, rows):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_] and row[0] == size, name


def test_defaults_and_invalid_arguments_without_device(L):
    from elimaloc_amd import _lib
    from elimaloc_amd.posegraph import PoseGraphCovConfig
    cfg = PoseGraphCovConfig()
    assert (cfg.lambda_, cfg.pcg_rel_tol, cfg.pcg_max_iterations, cfg.pcg_check_every, cfg.scratch_bytes) == (0.0, 1e-10, 20000, 32, 0)
    assert PoseGraphCovConfig(lambda_=1e-3, scratch_bytes=1 << 20).scratch_bytes == 1 << 20
    L.elm_posegraph_cov_config_default(None)  # a NULL config is ignored
    one = C.c_void_p(1)  # never dereferenced: the argument checks come first
    node = np.zeros(1, np.int32)
    ip = node.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.full(36, 5.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    st = _lib.PoseGraphCovStatsC()
    st.n_columns = 7
    ok = C.byref(cfg)
    assert L.elm_posegraph_covariance(None, one, ip, 1, None, 0, ok, dp, None, None, None, C.byref(st)) == INVALID
    assert L.elm_posegraph_covariance(one, None, ip, 1, None, 0, ok, dp, None, None, None, C.byref(st)) == INVALID
    assert L.elm_posegraph_covariance(one, one, ip, 1, None, 0, None, dp, None, None, None, C.byref(st)) == INVALID
    assert L.elm_posegraph_covariance(one, one, None, 1, None, 0, ok, dp, None, None, None, C.byref(st)) == INVALID  # columns without a list
    assert L.elm_posegraph_covariance(one, one, ip, 1, None, 1, ok, dp, None, None, None, C.byref(st)) == INVALID  # rows without a list
    assert L.elm_posegraph_covariance(one, one, ip, 1, None, 0, ok, dp, dp, None, None, C.byref(st)) == INVALID  # cross36 without rows
    assert L.elm_posegraph_covariance(one, one, ip, (1 << 20) + 1, None, 0, ok, dp, None, None, None, C.byref(st)) == INVALID
    for bad in (dict(lambda_=-1.0), dict(lambda_=float("nan")), dict(pcg_rel_tol=-1e-3), dict(pcg_rel_tol=float("inf")), dict(pcg_max_iterations=0),
                dict(pcg_check_every=0)):
        assert L.elm_posegraph_covariance(one, one, ip, 1, None, 0, C.byref(PoseGraphCovConfig(**bad)), dp, None, None, None, C.byref(st)) == INVALID, bad
    assert L.elm_posegraph_relative_covariance(None, one, ip, ip, 1, ok, dp, C.byref(st)) == INVALID
    assert L.elm_posegraph_relative_covariance(one, None, ip, ip, 1, ok, dp, C.byref(st)) == INVALID
    assert L.elm_posegraph_relative_covariance(one, one, None, ip, 1, ok, dp, C.byref(st)) == INVALID
    assert L.elm_posegraph_relative_covariance(one, one, ip, None, 1, ok, dp, C.byref(st)) == INVALID
    assert L.elm_posegraph_relative_covariance(one, one, ip, ip, 1, ok, None, C.byref(st)) == INVALID
    assert L.elm_posegraph_relative_covariance(one, one, ip, ip, 1, None, dp, C.byref(st)) == INVALID
    assert st.n_columns == 7 and (out == 5.0).all()
    from elimaloc_amd._lib import ElmError
    from elimaloc_amd.posegraph import PoseGraph
    pg = PoseGraph.__new__(PoseGraph)  # no device: the lengths are checked before the library is asked
    with pytest.raises(ElmError, match="one b per a"):
        pg.RelativeCovariance([0, 1], [2])


def test_shim_call_lines_compile_link_and_run(L, tmp_path):
    """tests/shim_harness/posegraph_cov_calls.cpp, built as tests/test_posegraph_init_abi.py builds posegraph_init_calls.cpp"""
    exe = tmp_path / "posegraph_cov_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "posegraph_cov_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0


# ---------------------------------------------------------------- the mirror
def test_the_mirrors_product_is_posegraph_refs():
    for name in ("random-11-25", "star-70", "random-7-12-damped"):
        c = cov.case(name)
        g, lin = c["g"], c["lin"]
        p = np.random.default_rng(51).normal(size=(g.N, 6))
        p[~lin["active"]] = 0.0
        want = ref.spmv(g, lin, c["lam"], p).reshape(-1)
        got = cov.sparse_system(g, lin, c["lam"]) @ p.reshape(-1)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


@pytest.mark.parametrize("name", cov.ALL_CASES)
def test_the_mirror_is_within_one_bound_of_the_dense_inverse(name):
    c = cov.case(name)
    nodes = np.array(MIRROR_NODES.get(name, c["nodes"]))
    X, its, conv = cov.columns(c["g"], c["lin"], c["lam"], nodes, precond=c["precond"])
    idx = (6 * nodes[:, None] + np.arange(6)[None, :]).reshape(-1)
    want = c["ref"]["Sigma"][:, idx]
    b = cov.bound(c["ref"], nodes)
    ratio = float((np.abs(X - want).max(axis=0) / b).max())
    active = c["lin"]["active"][nodes]
    print(f"  {name}: {idx.size} columns, iterations {int(its.min())} .. {int(its.max())}, |mirror - dense| / bound {ratio:.2e}, bound {b.min():.2e} .. "
          f"{b.max():.2e}, max |Sigma| {c['ref']['sigma_max']:.2e}")
    assert conv.all() and ratio <= 1.0
    # an inactive node: zero column, zero iterations; a zero row in every column
    assert not X[:, np.repeat(~active, 6)].any() and not its[np.repeat(~active, 6)].any()
    assert not X[np.repeat(~c["lin"]["active"], 6)].any()
    assert np.array_equal(cov.blocks(X, nodes, nodes)[1, 0], X.reshape(-1, 6, nodes.size, 6)[nodes[0], :, 1, :])


def test_the_mirror_on_the_pure_chain_is_within_one_bound_of_block_thomas():
    g = cov.pure_chain()
    lin = ref.linearize(g)
    assert g.N == 65537 and lin["active"].sum() == g.N - 66 and lin["active"][cov.PURE_NODES].all()
    D, U = cov.pure_chain_blocks(g, lin["A"], lin["B"], lin["w"], lin["diag"])
    want = cov.thomas_columns(D, U, cov.PURE_NODES)
    b = cov.pure_chain_bound(g, lin, want)
    X, its, conv = cov.columns(g, lin, 0.0, cov.PURE_NODES, precond="chain")
    ratio = float((np.abs(X.reshape(g.N, 6, 12) - want).max(axis=(0, 1)) / b).max())
    print(f"  pure chain: iterations {its.tolist()}, |mirror - thomas| / bound {ratio:.2e}, bound {b.min():.2e} .. {b.max():.2e}, max |Sigma| {np.abs(want).max():.2e}")
    assert conv.all() and its.max() <= 3 and ratio <= 1.0  # M = H
    # the reference against the dense inverse on a short pure chain
    small = cov.pure_chain(N=40, seed=26)
    ls = ref.linearize(small)
    Ds, Us = cov.pure_chain_blocks(small, ls["A"], ls["B"], ls["w"], ls["diag"])
    Xs = cov.thomas_columns(Ds, Us, [7, 39]).reshape(240, 12)
    Sig = cov.dense(small, ls, 0.0)["Sigma"]
    idx = (6 * np.array([7, 39])[:, None] + np.arange(6)).reshape(-1)
    act = np.repeat(ls["active"], 6)
    assert np.abs(Xs[act] - Sig[np.ix_(act, idx)]).max() <= 1e-9 * np.abs(Sig).max()


def test_the_hand_case_is_the_inverse_information():
    c = cov.case("hand-2")
    g = c["g"]
    Sig = c["ref"]["Sigma"].reshape(2, 6, 2, 6)
    rel = cov.relative(g.poses, 0, 1, lambda r, k: Sig[r, :, k, :])
    want = np.linalg.inv(g.info[0])
    assert np.abs(rel - want).max() <= 1e-12 * np.abs(want).max() and not Sig[0].any()


def test_the_gate_fixture_separates_on_the_mirror():
    """posegraph_cases.ring() as it is (identity informations), at the mirror's optimum: no information scale had to be chosen"""
    g, _ = cases.ring()
    d2 = cov.gate_mirror(g, np.load(cases.GOLDEN)["ring_poses"])
    print(f"  d2: exact true loop {d2[0]:.3e}, noisy true loop {d2[1]:.3e}, false loop {d2[2]:.3e} (gate {cov.GATE})")
    assert d2[0] < 1e-20 and 1e-6 < d2[1] < cov.GATE < d2[2]
