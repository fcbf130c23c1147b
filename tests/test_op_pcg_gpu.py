"""`gsi_op_solve_pcg` on the device: the panel kernels of csrc/block_pcg.hip (path 1, "fused") under the checks of
tests/pcg_cases.py, the device randsvd as the source of the basis, the FFT operators the CPU backend does not carry, one
size beyond a sweep of the kernels' fixed grid, the A/B legs (poll interval, composed path), `condition_fields` and the
device memory account."""
import numpy as np
import pytest

import pcg_cases as pg
import solve_cases as sc

pytestmark = pytest.mark.gpu

PATH = "fused"
NS = (24, 20)


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


@pytest.fixture(scope="module")
def big(gsi, ctx):
    """The dense n = 1000 case with its rank-64 basis from the device randsvd, made once."""
    op, d, A = pg.dense_inputs(gsi, ctx, 1000, "u")
    pc = gsi.lowrank_preconditioner(op, rank=64, diag=d, seed=3)
    yield op, d, pc
    pc.close()
    op.close()


def _grid_op(gsi, ctx):
    return gsi.fft_gridcov_operator(ctx, list(NS), kind="exponential", ell=3.0)


def _scattered(m, seed=0):
    rng = np.random.default_rng(40 + seed)
    return np.asfortranarray(np.vstack([rng.random(m) * 23.0, rng.random(m) * 19.0])), [0.0, 0.0, 23.0, 19.0]


@pytest.mark.parametrize("n,b,diag,K", pg.DENSE[:-1])
def test_dense(gsi, ctx, n, b, diag, K):
    pg.dense_solve(gsi, ctx, n, b, diag, K, PATH)


def test_dense_1000_with_the_randsvd_basis(gsi, ctx, big):
    op, d, pc = big
    assert pc.rank == 64
    pg.halves_the_iterations(gsi, op, d, pc, PATH, "pcg dense n=1000, rank 64 from the device randsvd")


@pytest.mark.parametrize("which", ["pointcov2", "pointcov3", "powerlaw"])
def test_operators(gsi, ctx, which):
    pg.operator_solve(gsi, ctx, which, PATH)


@pytest.mark.parametrize("which", ["gridcov", "fft_at"])
def test_fft_operators_with_the_randsvd_basis(gsi, ctx, which):
    """rank = 32 from the device randsvd of the operator itself: both bars, and no more iterations than plain CG."""
    extra = []
    if which == "gridcov":
        op, d, b = _grid_op(gsi, ctx), sc.diag_values("vec", 480), 16
    else:
        P, box = _scattered(150)
        extra.append(_grid_op(gsi, ctx))
        op, d, b = gsi.fft_operator_at(ctx, extra[0], P, box=box), sc.diag_values(0.1, 150), 65
    pc = gsi.lowrank_preconditioner(op, rank=32, diag=d, seed=1)
    try:
        # the inputs are fair (the CPU file cannot say so of these operators): numpy's recurrences with this very P^-1
        n = op.shape[0]
        M = sc.dense_of(op, d)
        pg.fair(f"{which} rank 32", M, sc.rhs(n, 3, seed=n + b), lambda r: pc.apply(r), 10 * n)
        X, rep, B = pg.run_case(gsi, op, d, b, pc, f"pcg {which} rank 32", PATH, M=M)
        _, plain = op.solve(B, diag=d, tol=sc.TOL, return_info=True)
        print(f"{which}: iterations {rep['iters'].min()}..{rep['iters'].max()}, plain CG {plain['iters'].min()}..{plain['iters'].max()}")
        assert (rep["iters"] <= plain["iters"]).all(), (rep["iters"], plain["iters"])
    finally:
        pc.close()
        op.close()
        for h in extra:
            h.close()


def test_another_diag(gsi, ctx):
    pg.other_diag(gsi, ctx, PATH)


def test_zero_basis_is_jacobi(gsi, ctx):
    pg.zero_basis(gsi, ctx, PATH)


def test_exact_factor_converges_at_once(gsi, ctx):
    pg.does_its_work_lowrank(gsi, ctx, PATH)


def test_beyond_one_sweep_of_the_fixed_grid(gsi, ctx):
    """n = 128 * 256 + 1: a second trip of the grid-stride loops, odd so the 8-byte form runs.  A diagonal matrix, lambda_i
    = 1 + i mod 5, d_i = 0.25 (1 + i mod 2), Z with one nonzero row per column: 10 distinct values of (lambda + d) / d and 3
    touched rows, at most 13 iterations (numpy: 10).  The reference is b / (lambda + d)."""
    n = 128 * 256 + 1
    lam = 1.0 + (np.arange(n) % 5).astype(float)
    d = 0.25 * (1.0 + (np.arange(n) % 2))
    A = np.zeros((n, n), order="F")
    A[np.arange(n), np.arange(n)] = lam
    op = gsi.dense_operator(ctx, A)
    del A
    Z = np.zeros((n, 3), order="F")
    Z[0, 0], Z[n - 1, 1], Z[n // 2, 2] = 1.0, 2.0, 0.5
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d)
    try:
        B = sc.rhs(n, 2, seed=1)
        X, rep = op.solve(B, diag=d, tol=sc.TOL, return_info=True, precond=pc)
        assert rep["path"] == PATH and rep["converged"] == 2 and rep["rank"] == 3, rep
        m = (lam + d)[:, None].astype(sc.LD)
        bb = (B.astype(sc.LD) ** 2).sum(axis=0)
        rho = np.sqrt(((B.astype(sc.LD) - m * X.astype(sc.LD)) ** 2).sum(axis=0) / bb).astype(float)
        Xref = B / (lam + d)[:, None]
        rref = np.sqrt(((B.astype(sc.LD) - m * Xref.astype(sc.LD)) ** 2).sum(axis=0) / bb).astype(float)
        kappa = (lam + d).max() / (lam + d).min()
        err = np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0)
        print(f"n={n}: iters {rep['iters']}, true relres {rho.max():.3e}, error {err.max():.3e}, bound {(kappa * (rho + rref)).min():.3e}")
        assert (rho <= 2 * sc.TOL).all() and (err <= kappa * (rho + rref)).all()
        assert rep["iters"].max() <= 13, rep["iters"]
    finally:
        pc.close()
        op.close()


@pytest.mark.parametrize("n,K,b", pg.APPLY)
def test_apply(gsi, ctx, n, K, b):
    pg.apply_case(gsi, ctx, n, K, b)


def test_special_columns(gsi, ctx):
    pg.special_columns(gsi, ctx, PATH)


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_determinism(gsi, ctx, monkeypatch, path):
    if path == "composed":
        monkeypatch.setenv("GSI_CG_COMPOSED", "1")
    pg.determinism(gsi, ctx, path)


def test_poll_interval_and_composed_path(gsi, ctx, monkeypatch):
    """The in-process A/B legs: the poll interval changes no bit of what the fused path returns; the composed path reaches
    the same bars with iteration counts within 2 per column."""
    op, d, A = pg.dense_inputs(gsi, ctx, 257, 0.01)
    pc = gsi.lowrank_preconditioner(op, basis=pg.eig_basis(A, 32), diag=d)
    try:
        B = sc.rhs(257, 5, seed=2)
        Xf, rf = op.solve(B, diag=d, return_info=True, precond=pc)
        for poll in ("1", "7"):
            monkeypatch.setenv("GSI_CG_POLL", poll)
            Xp, rp = op.solve(B, diag=d, return_info=True, precond=pc)
            assert np.array_equal(Xp, Xf) and np.array_equal(rp["iters"], rf["iters"]) and np.array_equal(rp["relres"], rf["relres"])
        monkeypatch.setenv("GSI_CG_COMPOSED", "1")
        Xc, rc = op.solve(B, diag=d, return_info=True, precond=pc)
        assert rc["path"] == "composed" and rf["path"] == "fused"
        sc.check_solve("pcg composed on the device", sc.dense_of(op, d), Xc, B, rc)
        assert np.abs(rc["iters"] - rf["iters"]).max() <= 2
    finally:
        pc.close()
        op.close()


def test_budget(gsi, ctx):
    pg.budget(gsi, ctx, PATH)


def test_breakdown(gsi, ctx):
    pg.breakdown(gsi, ctx, PATH)


def test_refusals(gsi, ctx):
    other = gsi.Context(0)
    try:
        pg.refusals(gsi, ctx, other, PATH)
    finally:
        other.close()


def test_refuses_a_communicator(gsi, monkeypatch):
    monkeypatch.setenv("GSI_LOCAL_COMM", "1")
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0)
    try:
        cc.comm_init(1, 0, cc.unique_id())
        op = gsi.dense_operator(cc, np.eye(4))
        sc.refused(gsi, lambda: gsi.lowrank_preconditioner(op, basis=np.ones((4, 1)), shift=1.0), "communicator")
        op.close()
    finally:
        cc.close()


# ---------------------------------------------------------------- kriging on the FFT operator at points
@pytest.fixture(scope="module")
def at_setup(gsi, ctx):
    """The 24 x 20 exponential grid operator read at 150 points, with the dense C (n x n) and W (m x n)."""
    P, box = _scattered(150, seed=1)
    gop = _grid_op(gsi, ctx)
    at = gsi.fft_operator_at(ctx, gop, P, box=box)
    n = NS[0] * NS[1]
    Cd = gop.matmul(np.eye(n))
    Wd_dev = gsi.FFTRF.interpolate(ctx, P, np.eye(n), NS, box=box)
    Wd = Wd_dev.to_host()
    Wd_dev.close()
    yield {"P": P, "box": box, "gop": gop, "at": at, "C": Cd, "W": Wd, "n": n}
    at.close()
    gop.close()


def test_kriging_weights_with_drift(gsi, ctx, at_setup):
    s = at_setup
    pc = gsi.lowrank_preconditioner(s["at"], rank=32, diag=0.05, seed=2)
    try:
        pg.kriging_drift(gsi, ctx, s["at"], s["P"], 0.05, pc, "pcg kriging drift, fft_at m=150")
    finally:
        pc.close()


def test_condition_fields(gsi, ctx, at_setup):
    """`condition_fields(..., precond=pc)` to the entry-wise bound tests/test_op_solve_gpu.py derives for the plain solve."""
    s = at_setup
    m, b = 150, 3
    rng = np.random.default_rng(32)
    sampler = gsi.gridcov_sampler(ctx, list(NS), kind="exponential", ell=3.0)
    F = sampler.fields(b, seed=5)
    y = rng.standard_normal(m)
    d = 0.05 + 0.05 * rng.random(m)
    eps = rng.standard_normal((m, b))
    pc = gsi.lowrank_preconditioner(s["at"], rank=32, diag=d, seed=2)
    try:
        Fh = F.to_host()
        Fc = gsi.condition_fields(s["at"], F, y, d, eps=eps, tol=sc.TOL, precond=pc)
        got = Fc.to_host()
        Fc.close()
        assert np.array_equal(F.to_host(), Fh)                               # F is not modified
        C_, W = s["C"], s["W"]
        A = W @ C_ @ W.T
        M = 0.5 * (A + A.T) + np.diag(d)
        WF_dev = gsi.FFTRF.interpolate(ctx, s["P"], F, NS, box=s["box"])
        rhs = (y[:, None] + np.sqrt(d)[:, None] * eps) - WF_dev.to_host()   # the right-hand side the device formed, bit for bit
        WF_dev.close()
        xi_ref = np.linalg.solve(M, rhs)
        want = Fh + C_ @ (W.T @ xi_ref)
        # the solution bar: the device's xi for the same right-hand side (deterministic) and its true residual
        xi, rep = s["at"].solve(rhs, diag=d, tol=sc.TOL, return_info=True, precond=pc)
        assert rep["path"] == PATH and rep["rank"] == 32
        Md = sc.dense_of(s["at"], d)
        beta = np.linalg.cond(M) * (sc.true_relres(Md, xi, rhs) + sc.true_relres(Md, xi_ref, rhs))    # per column
        dxi = beta * np.linalg.norm(xi_ref, axis=0)                          # bound on |xi - xi_ref|_2 per column
        CWt = C_ @ W.T
        # |(C W' (xi - xi_ref))_i| <= |row i of C W'|_2 |xi - xi_ref|_2, plus 1e-12 of the update's size for the products
        bound = np.linalg.norm(CWt, axis=1)[:, None] * dxi[None, :] + 1e-12 * np.abs(want - Fh).max()
        print(f"condition_fields with precond: max error {np.abs(got - want).max():.3e}, smallest bound {bound.min():.3e}, "
              f"largest ratio {(np.abs(got - want) / bound).max():.3e}")
        assert (np.abs(got - want) <= bound).all()
    finally:
        pc.close()
        F.close()
        sampler.close()


def test_device_memory_returns(gsi, ctx):
    """After close() of everything the context holds what it held before.  The backend keeps released blocks and its
    workspaces for reuse and counts them in `device_bytes`, so a first cycle fills that cache and the second one is measured:
    it finds every block it needs there and must leave nothing behind."""
    def cycle():
        op, d, A = pg.dense_inputs(gsi, ctx, 257, "vec")
        pc = gsi.lowrank_preconditioner(op, rank=16, diag=d, seed=4)
        Bd = gsi.DeviceMatrix.from_host(ctx, sc.rhs(257, 4))
        Xd = op.solve(Bd, diag=d, precond=pc)
        Zd = pc.apply(Bd)
        for h in (Zd, Xd, Bd, pc, op):
            h.close()
    cycle()
    before = ctx.device_bytes()
    cycle()
    assert ctx.device_bytes() == before
