"""The pose graph's chain preconditioner on the GPU (include/elimaloc_hip_posegraph_precond.h): M^-1 r of the block
cyclic reduction against the mirror's direct solve (tests/posegraph_chain_ref.py) by its backward error, at every size at which the
reduction changes path (its segment is 256 nodes; one, two and three levels) and on the broken, reversed, duplicate and chain-less
graphs; five iterations under the project's 1e-9 contract; convergence, Optimize and the refactor after a rejection against the
mirror; the run-to-run bytes; the default left byte for byte as it was; Reset, misuse and the device group."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import posegraph_cases as cases
import posegraph_chain_cases as ccases
import posegraph_chain_ref as cref
import posegraph_ref as ref
from elimaloc_amd import _lib
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.posegraph import PoseGraph, PoseGraphConfig
from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig, Scan, VoxelHashMap

pytestmark = pytest.mark.gpu

# The backward error max |M z - r| / (|M| |z| + |r|) of the GPU's z = M^-1 r, measured on one MI355X over every shape of SHAPES at
# lambda 0 and 1 ("Measured accuracy"): the largest value was MEASURED_BACKWARD; the bound is 10 x that.
MEASURED_BACKWARD = 3.2e-13
BACKWARD_BOUND = 10.0 * MEASURED_BACKWARD

SHAPES = dict(ccases.SIZES)
SHAPES.update(ccases.SPECIAL)
SHAPES["N65537_three_levels"] = lambda: ccases.long_chain(ccases.THREE_LEVELS, 46, loops=30)
HUBER = 1.5


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(graph, mirror linearization), built once and left unchanged"""
    g = SHAPES[name]()
    return g, ref.linearize(g, huber_k=HUBER)


def _upload(ctx, g, kind="chain"):
    pg = PoseGraph(max(g.N, 1), max(g.E, 1), ctx)
    pg.SetPreconditioner(kind)
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    return pg


def _close(got, want, what, ref_own_error=0.0):
    """The project's contract 1e-9 max(1, max |ref|).  Where the reference does not have those digits itself -- two direct solves of
    the same ill-conditioned M differ by ref_own_error -- the bound is 10 x that difference instead (DESIGN.md section 22 names the
    shape: the 8 193-node chain at lambda = 0)."""
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(np.asarray(got) - want).max()) if want.size else 0.0
    contract = 1e-9 * max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    bound = max(contract, 10.0 * ref_own_error)
    print(f"  {what}: |gpu - ref| {err:.3e} (bound {bound:.1e}: contract {contract:.1e}, the mirror against itself {ref_own_error:.1e})")
    assert np.asarray(got).shape == want.shape and err <= bound, what


def _cfg(d):
    return PoseGraphConfig(**d)


# ---------------------------------------------------------------- M^-1 r alone
@pytest.mark.parametrize("name", list(SHAPES))
def test_minv_r_backward_error(ctx, name):
    """One iteration without a stop test: delta = alpha M^-1 (-g).  alpha is taken out by the least-squares fit of M delta to r (its
    error is of second order in the residual), and z = delta / alpha is judged by its backward error against the mirror's M."""
    t0 = time.time()
    g, lin = _case(name)
    pg = _upload(ctx, g)
    try:
        assert pg.Preconditioner() == "chain"
        pg.Linearize(HUBER)
        r = np.where(lin["active"][:, None], -lin["grad"], 0.0)
        for lam in (0.0, 1.0):
            M = cref.chain_matrix(g, lin, lam)
            z_ref = cref.chain_solver(g, lin, lam, M=M)(r)
            pq = float(np.sum(z_ref * ref.spmv(g, lin, lam, z_ref)))
            want = (float(np.sum(r * z_ref)) / pq if pq != 0.0 else 0.0) * z_ref  # pcg_chain's first iterate, on one factorization
            delta, st = pg.Solve(lam, 0.0, 1)
            assert st["iterations"] == 1 and not st["converged"] and delta.shape == want.shape
            assert (delta[~lin["active"]] == 0.0).all() and np.isfinite(delta).all()
            err = float(np.abs(delta - want).max()) / max(1.0, float(np.abs(want).max())) if want.size else 0.0
            if not lin["active"].any():
                assert (delta == 0.0).all()
                print(f"  {name} lambda {lam}: no active node, delta is zero")
                continue
            Md = M @ delta.reshape(-1)
            alpha = float(Md @ r.reshape(-1)) / float(r.reshape(-1) @ r.reshape(-1))
            bwd = cref.backward_error(g, lin, lam, delta / alpha, r, M=M)
            bwd_ref = cref.backward_error(g, lin, lam, z_ref, r, M=M)
            print(f"  {name} lambda {lam}: backward error {bwd:.3e} (mirror's direct solve {bwd_ref:.3e}), |gpu - ref| / max(1, |ref|) {err:.3e}")
            assert alpha > 0.0 and bwd <= BACKWARD_BOUND
    finally:
        pg.close()
    print(f"  {name}: {time.time() - t0:.2f} s")


# ---------------------------------------------------------------- five iterations
@pytest.mark.parametrize("name", [n for n in SHAPES if n != "N65537_three_levels"])
def test_five_iterations_against_the_mirror(ctx, name):
    g, lin = _case(name)
    pg = _upload(ctx, g)
    try:
        pg.Linearize(HUBER)
        for lam in (0.0, 1.0):
            want, its, _, conv = cref.pcg_chain(g, lin, lam, 0.0, 5)
            delta, st = pg.Solve(lam, 0.0, 5)
            assert (its, conv) == (5, False) and st["iterations"] == 5 and not st["converged"]
            # what the reference itself has of these digits: the same five iterations on a second direct solve of the same M
            own = 0.0
            if lin["active"].any():
                other = cref.pcg_chain(g, lin, lam, 0.0, 5, solve=cref.chain_solver_cholesky(g, lin, lam))[0]
                own = float(np.abs(other - want).max())
            _close(delta, want, f"{name} lambda {lam} delta after 5 iterations", own)
            assert (delta[~lin["active"]] == 0.0).all() and (delta[g.fixed] == 0.0).all()
    finally:
        pg.close()


# ---------------------------------------------------------------- convergence
CONVERGE = {"chain64_loops3": lambda: cases.chain(*ccases.RANK_BOUND[2][:2], loops=ccases.RANK_BOUND[2][2]), "ring": lambda: cases.ring()[0]}


@pytest.mark.parametrize("name", list(CONVERGE))
def test_solve_to_tolerance_iterations_and_true_residual(ctx, name):
    tol = 1e-10
    g = CONVERGE[name]()
    lin = ref.linearize(g)
    pg = _upload(ctx, g)
    try:
        pg.Linearize()
        for lam in (0.0, 1.0):
            d_ref, its_ref, _, conv_ref = cref.pcg_chain(g, lin, lam, tol, 2000)
            rho_ref = cref.true_rel_residual(g, lin, lam, d_ref)
            pg.SetPreconditioner("chain")
            delta, st = pg.Solve(lam, tol, 2000)
            rho = cref.true_rel_residual(g, lin, lam, delta)
            pg.SetPreconditioner("block_jacobi")  # the linearization stays valid
            _, st_bj = pg.Solve(lam, tol, 2000)
            print(f"  {name} lambda {lam}: chain {st['iterations']} iterations (mirror {its_ref}), block Jacobi {st_bj['iterations']}; "
                  f"true relative residual {rho:.2e} (mirror {rho_ref:.2e})")
            assert conv_ref and st["converged"] and st["rel_residual"] <= tol and st_bj["converged"]
            assert rho <= 10.0 * max(tol, rho_ref)
            assert st["iterations"] <= its_ref + 2
            assert st["iterations"] < st_bj["iterations"]
            assert (delta[g.fixed] == 0.0).all()
    finally:
        pg.close()


# ---------------------------------------------------------------- optimize
def test_optimize_the_ring(ctx):
    g, truth = cases.ring()
    pg = _upload(ctx, g)
    try:
        res = pg.Optimize(_cfg(cases.RING_CFG))
        poses = pg.Poses()
        dt, dr = ref.pose_error(poses, truth)
        pg.SetPreconditioner("block_jacobi")
        pg.SetPoses(g.poses)
        res_bj = pg.Optimize(_cfg(cases.RING_CFG))
        print(f"  ring with the chain preconditioner: {dt:.3e} m, {dr:.3e} rad of the truth; {res['solves']} solves, "
              f"{res['pcg_iterations_total']} PCG iterations (block Jacobi {res_bj['solves']} solves, {res_bj['pcg_iterations_total']})")
        assert res["solves"] == res["accepted"] > 0 and res["rejected"] == 0 and all(t["accepted"] for t in res["trace"])
        assert dt <= 1e-4 and dr <= 1e-5
        assert res["pcg_iterations_total"] == sum(t["pcg_iterations"] for t in res["trace"]) < res_bj["pcg_iterations_total"]
        assert poses[0].tobytes() == g.poses[0].tobytes()  # the fixed node
    finally:
        pg.close()


def test_a_rejection_refactors(ctx):
    """cases.wild_chain() from lambda 1e-9 with lambda_up 1e4: rejections, each of which changes lambda and so the factor, followed by
    accepted steps -- the accept/reject sequence and the dampings are those of the mirror's Levenberg-Marquardt with pcg_chain."""
    g = cases.wild_chain()
    kw = dict(lambda_init=1e-9, lambda_up=1e4, max_iterations=4, pcg_rel_tol=1e-10, pcg_max_iterations=500)
    want_poses, want = cref.optimize(g, **kw)
    pg = _upload(ctx, g)
    try:
        res = pg.Optimize(_cfg(kw))
        seq = [t["accepted"] for t in want["trace"]]
        print(f"  accepted: {[t['accepted'] for t in res['trace']]} (mirror {seq}); PCG iterations {[t['pcg_iterations'] for t in res['trace']]} "
              f"(mirror {[t['pcg_iterations'] for t in want['trace']]})")
        assert seq == [t["accepted"] for t in res["trace"]] and False in seq and seq[-1] is True and seq.index(True) > seq.index(False)
        assert all(abs(t["ratio"] - 1.0) > 0.04 for t in want["trace"])  # no decision hangs on a last digit
        assert np.allclose([t["lambda_"] for t in res["trace"]], [t["lambda_"] for t in want["trace"]], rtol=1e-12)
        assert np.allclose([t["cost"] for t in res["trace"]], [t["cost"] for t in want["trace"]], rtol=1e-6)
        assert max(ref.pose_error(pg.Poses(), want_poses)) <= 1e-6 and res["cost_final"] < res["cost_initial"]
    finally:
        pg.close()


# ---------------------------------------------------------------- bytes
def test_solves_are_byte_identical_from_run_to_run(ctx):
    g, _ = _case("N513")
    pg = _upload(ctx, g)
    try:
        pg.Linearize(HUBER)
        runs = []
        for _ in range(5):
            delta, st = pg.Solve(0.5, 0.0, 7)
            runs.append((delta.tobytes(), repr(st)))
        assert all(r == runs[0] for r in runs[1:])
        g2, _ = cases.ring(false_loop=True)
        pg2 = _upload(ctx, g2)
        try:
            outs = []
            for _ in range(5):
                pg2.SetPoses(g2.poses)
                res = pg2.Optimize(_cfg(dict(cases.FALSE_CFG, max_iterations=3)))
                outs.append((pg2.Poses().tobytes(), repr(res)))
            assert all(r == outs[0] for r in outs[1:])
        finally:
            pg2.close()
    finally:
        pg.close()


def _scan_points(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32))


def test_the_default_is_untouched(ctx):
    for g, cfg in ((cases.chain(12, 2), dict(max_iterations=3)), (cases.ring(false_loop=True)[0], dict(cases.FALSE_CFG, max_iterations=3))):
        out = []
        for explicit in (False, True):
            pg = PoseGraph(g.N, g.E, ctx)
            try:
                if explicit:
                    pg.SetPreconditioner("chain")
                    pg.SetPreconditioner("block_jacobi")
                assert pg.Preconditioner() == "block_jacobi"
                pg.AddNodes(g.poses, g.fixed)
                pg.AddEdges(g.i, g.j, g.Z, g.info)
                pg.Linearize(HUBER)
                solves = [(d.tobytes(), repr(st)) for d, st in (pg.Solve(lam, 1e-8, 40) for lam in (0.0, 1e-3))]
                res = pg.Optimize(_cfg(cfg))
                out.append((solves, repr(res), pg.Poses().tobytes()))
            finally:
                pg.close()
        assert out[0] == out[1]
    # LoopCloser.Close without the argument, with the default named, and with the chain
    g, truth = cases.ring()
    n = 12
    db = PlaceDatabase(PlaceConfig(), n, ctx)
    try:
        lc = LoopCloser(db)
        for k in range(n):
            lc.Insert(_scan_points(256, 900 + k), g.poses[k])
        lc.AddLoop(0, n - 1, cases.inv_pose(truth[0]) @ truth[n - 1])
        cfg = _cfg(dict(cases.RING_CFG))
        poses, res = lc.Close(cfg)
        poses_named, res_named = lc.Close(cfg, preconditioner="block_jacobi")
        assert poses.tobytes() == poses_named.tobytes() and repr(res) == repr(res_named)
        poses_chain, res_chain = lc.Close(cfg, preconditioner="chain")
        dt, dr = ref.pose_error(poses_chain, poses)
        print(f"  Close with the chain against the default: {dt:.3e} m, {dr:.3e} rad; PCG iterations {res_chain['pcg_iterations_total']} "
              f"against {res['pcg_iterations_total']}")
        assert dt <= 1e-4 and dr <= 1e-5 and res_chain["pcg_iterations_total"] < res["pcg_iterations_total"]
        with pytest.raises(ElmError, match="none of"):
            lc.Close(cfg, preconditioner="tree")
    finally:
        db.close()


# ---------------------------------------------------------------- Reset, misuse, the device group
def _set_raw(ctx, pg, kind):
    return _lib.lib().elm_posegraph_set_preconditioner(ctx._h, pg._h, kind)


def test_reset_keeps_the_kind_and_misuse_is_followed_by_a_correct_call(ctx):
    g = cases.chain(6, 9)
    pg = _upload(ctx, g)
    first = pg.Optimize(_cfg(dict(max_iterations=2)))
    pg.Reset()
    assert pg.Size() == (0, 0) and pg.Preconditioner() == "chain"
    pg.AddNodes(g.poses, g.fixed)
    pg.AddEdges(g.i, g.j, g.Z, g.info)
    assert repr(pg.Optimize(_cfg(dict(max_iterations=2)))) == repr(first)  # the same graph after a Reset: the same run, the chain's
    for bad in (-1, 2, 77):
        assert _set_raw(ctx, pg, bad) == -1 and pg.Preconditioner() == "chain"
    with pytest.raises(ElmError, match="none of"):
        pg.SetPreconditioner("spanning_tree")
    kind = C.c_int(9)
    assert _lib.lib().elm_posegraph_get_preconditioner(ctx._h, pg._h, None) == -1
    other = Context(0)
    try:
        assert _set_raw(other, pg, 0) == -1 and _lib.lib().elm_posegraph_get_preconditioner(other._h, pg._h, C.byref(kind)) == -1  # another context's
        assert kind.value == 9 and pg.Preconditioner() == "chain"
    finally:
        other.close()
    # setting the kind leaves the linearization: a solve follows without a new Linearize
    pg.SetPoses(g.poses)
    pg.Linearize()
    pg.SetPreconditioner("block_jacobi")
    d_bj, st_bj = pg.Solve(1.0, 1e-10, 200)
    pg.SetPreconditioner("chain")
    d_ch, st_ch = pg.Solve(1.0, 1e-10, 200)
    assert st_bj["converged"] and st_ch["converged"]
    _close(d_ch, d_bj, "the converged step of either preconditioner")
    # a batch in flight: refused, and served again once the batch is finished
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(_scan_points(2000, 77))
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    sc = Scan(ctx, _scan_points(300, 78))
    reg.EnqueueBatch([sc], vm, [np.eye(4)])
    for bad in (lambda: pg.SetPreconditioner("block_jacobi"), lambda: pg.Preconditioner()):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
    reg.FinishBatch()
    assert pg.Preconditioner() == "chain"
    pg.SetPreconditioner("block_jacobi")
    assert pg.Preconditioner() == "block_jacobi"
    pg.close()
    with pytest.raises(ElmError, match="closed"):
        pg.SetPreconditioner("chain")


def test_a_device_groups_lead_is_refused(ctx):
    pg = PoseGraph(4, 4, ctx)
    grp = Context.multi([0, 0])
    try:
        kind = C.c_int(9)
        assert _set_raw(grp, pg, 1) == -5  # ELM_ERR_UNSUPPORTED: one rank only
        assert _lib.lib().elm_posegraph_get_preconditioner(grp._h, pg._h, C.byref(kind)) == -5 and kind.value == 9
    finally:
        grp.close()
    assert pg.Preconditioner() == "block_jacobi"  # the plain context next to it is served
    pg.SetPreconditioner("chain")
    assert pg.Preconditioner() == "chain"
    pg.close()
