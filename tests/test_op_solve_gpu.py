"""`gsi_op_solve_cg` on the device: the fused panel kernels of csrc/block_cg.hip (path 1, "fused") under the checks of
tests/solve_cases.py, the FFT operators the CPU backend does not carry, one size beyond a sweep of the kernels' fixed grid,
`krige_to_grid` and `condition_fields`.  OP_SOLVE_ERRORS=<path>: the largest ratios seen, as profiles/op_solve_errors.json."""
import json
import os

import numpy as np
import pytest

import solve_cases as sc

pytestmark = pytest.mark.gpu

PATH = "fused"
NS = (24, 20)


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("OP_SOLVE_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"tol": sc.TOL, "bars": {"true_relres_over_tol": 2.0, "solution_error_over_bound": 1.0},
                       "largest_true_relres_over_tol": max(v.get("true_relres_over_tol", 0.0) for v in sc.RATIOS.values()),
                       "cases": sc.RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


def _grid_op(gsi, ctx):
    return gsi.fft_gridcov_operator(ctx, list(NS), kind="exponential", ell=3.0)


def _scattered(m, seed=0):
    """m points inside the 24 x 20 grid's box [0, 23] x [0, 19], none on a node line."""
    rng = np.random.default_rng(40 + seed)
    return np.asfortranarray(np.vstack([rng.random(m) * 23.0, rng.random(m) * 19.0])), [0.0, 0.0, 23.0, 19.0]


@pytest.mark.parametrize("n,b,diag", sc.DENSE)
def test_dense(gsi, ctx, n, b, diag):
    op, d = sc.dense_case(gsi, ctx, n, diag)
    try:
        sc.run_case(gsi, op, d, b, f"dense n={n} b={b} diag={diag}", PATH)
    finally:
        op.close()


@pytest.mark.parametrize("which", ["pointcov2", "pointcov3", "lowrank", "powerlaw", "gridcov", "fft_at"])
def test_operators(gsi, ctx, which):
    extra = []
    if which == "gridcov":
        op, d, b = _grid_op(gsi, ctx), sc.diag_values("vec", 480), 16
    elif which == "fft_at":
        P, box = _scattered(150)
        extra.append(_grid_op(gsi, ctx))
        op, d, b = gsi.fft_operator_at(ctx, extra[0], P, box=box), sc.diag_values(0.1, 150), 65
    else:
        make, b = {"pointcov2": (lambda: sc.pointcov_case(gsi, ctx, 2), 2), "pointcov3": (lambda: sc.pointcov_case(gsi, ctx, 3), 3),
                   "lowrank": (lambda: sc.lowrank_case(gsi, ctx), 16), "powerlaw": (lambda: sc.powerlaw_case(gsi, ctx), 17)}[which]
        op, d = make()
    try:
        sc.run_case(gsi, op, d, b, which, PATH)
    finally:
        op.close()
        for h in extra:
            h.close()


def test_beyond_one_sweep_of_the_fixed_grid(gsi, ctx):
    """n = 128 * 256 + 1: the kernels' 128 row parts of 256 lanes take a second trip of their grid-stride loops (odd n: the
    8-byte form).  A dense operator whose matrix is diagonal, so that the reference is b / lambda: 10 distinct values of
    lambda + d, at most 10 iterations."""
    n = 128 * 256 + 1
    lam = 1.0 + (np.arange(n) % 5).astype(float)
    d = 0.25 * (1.0 + (np.arange(n) % 2))
    A = np.zeros((n, n), order="F")
    A[np.arange(n), np.arange(n)] = lam
    op = gsi.dense_operator(ctx, A)
    del A
    try:
        B = sc.rhs(n, 2, seed=1)
        X, rep = op.solve(B, diag=d, tol=sc.TOL, return_info=True)
        assert rep["path"] == PATH and rep["converged"] == 2 and rep["iters"].max() <= 10, rep
        m = (lam + d)[:, None].astype(sc.LD)
        rho = np.sqrt((((B.astype(sc.LD) - m * X.astype(sc.LD)) ** 2).sum(axis=0)) / (B.astype(sc.LD) ** 2).sum(axis=0)).astype(float)
        Xref = B / (lam + d)[:, None]
        rref = np.sqrt((((B.astype(sc.LD) - m * Xref.astype(sc.LD)) ** 2).sum(axis=0)) / (B.astype(sc.LD) ** 2).sum(axis=0)).astype(float)
        kappa = (lam + d).max() / (lam + d).min()
        err = np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0)
        print(f"n={n}: iters {rep['iters']}, true relres {rho.max():.3e}, error {err.max():.3e}, bound {(kappa * (rho + rref)).min():.3e}")
        assert (rho <= 2 * sc.TOL).all() and (err <= kappa * (rho + rref)).all()
        sc.RATIOS["dense diagonal n=32769"] = {"true_relres_over_tol": float(rho.max() / sc.TOL),
                                               "solution_error_over_bound": float((err / (kappa * (rho + rref))).max())}
    finally:
        op.close()


def test_device_matrix_in_device_matrix_out(gsi, ctx):
    op, d = sc.dense_case(gsi, ctx, 65, "vec")
    B = sc.rhs(65, 3)
    Bd = gsi.DeviceMatrix.from_host(ctx, B)
    try:
        Xd, rep = op.solve(Bd, diag=d, return_info=True)
        assert isinstance(Xd, gsi.DeviceMatrix) and rep["path"] == PATH
        assert np.array_equal(Xd.to_host(), op.solve(B, diag=d))
        assert np.array_equal(Bd.to_host(), B)
        Xd.close()
    finally:
        Bd.close()
        op.close()


def test_special_columns(gsi, ctx):
    sc.special_columns(gsi, ctx, PATH)


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_determinism(gsi, ctx, monkeypatch, path):
    if path == "composed":
        monkeypatch.setenv("GSI_CG_COMPOSED", "1")
    sc.determinism(gsi, ctx, path)


def test_composed_path_agrees(gsi, ctx, monkeypatch):
    """The in-process A/B leg: the same recurrences from the BLAS-1 entry points reach the same bars, and the poll interval
    changes nothing in what the fused path returns."""
    op, d = sc.dense_case(gsi, ctx, 257, 0.01)
    try:
        B = sc.rhs(257, 5, seed=2)
        Xf, rf = op.solve(B, diag=d, return_info=True)
        for poll in ("1", "7"):
            monkeypatch.setenv("GSI_CG_POLL", poll)
            Xp, rp = op.solve(B, diag=d, return_info=True)
            assert np.array_equal(Xp, Xf) and np.array_equal(rp["iters"], rf["iters"]) and np.array_equal(rp["relres"], rf["relres"])
        monkeypatch.setenv("GSI_CG_COMPOSED", "1")
        Xc, rc = op.solve(B, diag=d, return_info=True)
        assert rc["path"] == "composed" and rf["path"] == "fused"
        sc.check_solve("composed on the device", sc.dense_of(op, d), Xc, B, rc)
        assert np.abs(rc["iters"] - rf["iters"]).max() <= 2
    finally:
        op.close()


def test_budget(gsi, ctx):
    sc.budget(gsi, ctx, PATH)


def test_breakdown(gsi, ctx):
    sc.breakdown(gsi, ctx, PATH)


def test_refusals(gsi, ctx):
    sc.refusals(gsi, ctx, PATH)


def test_refuses_a_communicator(gsi, monkeypatch):
    monkeypatch.setenv("GSI_LOCAL_COMM", "1")
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0)
    try:
        cc.comm_init(1, 0, cc.unique_id())
        op = gsi.dense_operator(cc, np.eye(4))
        sc.refused(gsi, lambda: op.solve(np.ones(4)), "communicator")
        op.close()
    finally:
        cc.close()


def test_mat_axpy(gsi, ctx):
    sc.mat_axpy_cases(gsi, ctx)


# ---------------------------------------------------------------- kriging on the FFT operator at points
@pytest.fixture(scope="module")
def at_setup(gsi, ctx):
    """The 24 x 20 exponential grid operator read at 150 points, with the dense C (n x n), W (m x n) and A = W C W'."""
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
    sc.kriging_drift(gsi, ctx, s["at"], s["P"], 0.05, "kriging drift, fft_at m=150")


def test_krige_to_grid(gsi, ctx, at_setup):
    s = at_setup
    rng = np.random.default_rng(31)
    y = rng.standard_normal(150)
    xi, beta = gsi.kriging_weights(s["at"], y, noise=0.05, tol=sc.TOL)
    want = s["C"] @ (s["W"].T @ xi)                       # the dense C, W and the device's own xi
    got = gsi.krige_to_grid(s["at"], xi)
    assert got.shape == (s["n"],)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"krige_to_grid: {err:.3e} of max |s|")
    assert err <= 1e-12
    sc.RATIOS["krige_to_grid"] = {"error_over_1e-12_of_max": float(err / 1e-12)}
    # with a drift: + drift_grid beta
    D = np.column_stack([np.ones(s["n"]), np.arange(s["n"]) % NS[0]])
    got2 = gsi.krige_to_grid(s["at"], xi, beta=np.array([0.5, -0.25]), drift_grid=D)
    assert np.abs(got2 - (got + D @ np.array([0.5, -0.25]))).max() <= 1e-14 * np.abs(got2).max()


@pytest.mark.parametrize("zero_eps", [False, True])
def test_condition_fields(gsi, ctx, at_setup, zero_eps):
    s = at_setup
    m, n, b = 150, s["n"], 3
    rng = np.random.default_rng(32)
    sampler = gsi.gridcov_sampler(ctx, list(NS), kind="exponential", ell=3.0)
    F = sampler.fields(b, seed=5)
    try:
        Fh = F.to_host()
        y = rng.standard_normal(m)
        d = 0.05 + 0.05 * rng.random(m)
        eps = np.zeros((m, b)) if zero_eps else rng.standard_normal((m, b))
        Fc = gsi.condition_fields(s["at"], F, y, d, eps=eps, tol=sc.TOL)
        got = Fc.to_host()
        assert np.array_equal(F.to_host(), Fh)                               # F is not modified
        # the dense formula
        C_, W = s["C"], s["W"]
        A = W @ C_ @ W.T
        M = 0.5 * (A + A.T) + np.diag(d)
        WF_dev = gsi.FFTRF.interpolate(ctx, s["P"], F, NS, box=s["box"])
        rhs = (y[:, None] + np.sqrt(d)[:, None] * eps) - WF_dev.to_host()   # the right-hand side the device formed, bit for bit
        WF_dev.close()
        xi_ref = np.linalg.solve(M, rhs)
        want = Fh + C_ @ (W.T @ xi_ref)
        # the solution bar: the device's xi for the same right-hand side (deterministic) and its true residual
        xi, rep = s["at"].solve(rhs, diag=d, tol=sc.TOL, return_info=True)
        Md = sc.dense_of(s["at"], d)
        beta = np.linalg.cond(M) * (sc.true_relres(Md, xi, rhs) + sc.true_relres(Md, xi_ref, rhs))    # per column
        dxi = beta * np.linalg.norm(xi_ref, axis=0)                          # bound on |xi - xi_ref|_2 per column
        CWt = C_ @ W.T
        # |(C W' (xi - xi_ref))_i| <= |row i of C W'|_2 |xi - xi_ref|_2, plus 1e-12 of the update's size for the products
        bound = np.linalg.norm(CWt, axis=1)[:, None] * dxi[None, :] + 1e-12 * np.abs(want - Fh).max()
        print(f"condition_fields eps={'0' if zero_eps else 'given'}: max error {np.abs(got - want).max():.3e}, "
              f"smallest bound {bound.min():.3e}, largest ratio {(np.abs(got - want) / bound).max():.3e}")
        assert (np.abs(got - want) <= bound).all()
        sc.RATIOS[f"condition_fields zero_eps={zero_eps}"] = {"entry_error_over_bound": float((np.abs(got - want) / bound).max())}
        if zero_eps:
            WFc_dev = gsi.FFTRF.interpolate(ctx, s["P"], Fc, NS, box=s["box"])
            WFc = WFc_dev.to_host()
            WFc_dev.close()
            want_pts = y[:, None] - d[:, None] * xi_ref                      # y - D (A + D)^-1 (y - W F)
            bound_pts = np.linalg.norm(A, axis=1)[:, None] * dxi[None, :] + 1e-12 * np.abs(want_pts).max()
            assert (np.abs(WFc - want_pts) <= bound_pts).all(), (np.abs(WFc - want_pts) / bound_pts).max()
        Fc.close()
    finally:
        F.close()
        sampler.close()


def test_condition_fields_draws_eps(gsi, ctx, at_setup):
    s = at_setup
    sampler = gsi.gridcov_sampler(ctx, list(NS), kind="exponential", ell=3.0)
    F = sampler.fields(2, seed=1)
    try:
        y = np.random.default_rng(1).standard_normal(150)
        a = gsi.condition_fields(s["at"], F, y, 0.1, seed=11)
        gsi.RandMatFact.seed(11)
        eps = gsi.RandMatFact.randn(150, 2)
        b = gsi.condition_fields(s["at"], F, y, 0.1, eps=eps)
        assert np.array_equal(a.to_host(), b.to_host())
        a.close()
        b.close()
    finally:
        F.close()
        sampler.close()
