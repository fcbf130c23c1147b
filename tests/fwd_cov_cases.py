"""Shared cases and checks of the operator H C H' of a linear forward model (`gsi_op_fwd_cov`, `linear_data_operator`) and of
what is built on it (`linear_inversion`, `estimate_field`, `condition_on_linear_data`) for
tests/test_fwd_cov_cpu.py (the CPU reference library: the host paths, C a power-law FFT operator) and
tests/test_fwd_cov_gpu.py (the kernels, C a grid covariance function).  Not a test module.

H is `fwd_adjoint_model.rays`: 40 rays of 64 samples (samples in one cell repeat its index and add), 20 point samples, a row
that repeats row 0 and an empty row.  The noise variance is 0.01 throughout: with it M = H C H' + D is well conditioned
although two rows of H are equal and one is zero (`test_inputs_are_fair` prints the condition numbers).

Bars.  Products: err < 1e-12 max|Y_ref| against the dense H C H' (test_fft_gridcov_gpu._close).  Solves: solve_cases'
(true residual <= 2 tol with tol = 1e-10; solution error <= kappa (rho + rho_ref)).  The saddle system of the inversion:
solve_cases.kriging_drift's two -- the solution bar with the saddle matrix, |G' xi| <= 10 tol |G| |xi| -- and, because the
solution bar holds for any vector, a residual bar derived from the stopping rule: xi = M^-1 y - M^-1 G beta from columns
whose true residuals are at most 2 tol |column|, so |y - M xi - G beta| <= 2 tol (|y| + sum_i |beta_i| |G_i|), plus the
products' own 1e-12 sqrt(nobs) |M| |xi| because M is numpy's here, not the operator's."""
import numpy as np

import fwd_adjoint_model as fm
import solve_cases as sc
from test_fft_gridcov_cpu import dense_matrix

LD = np.longdouble
NOISE = 1e-2
# name -> (Ns, kind name, kind code of dense_matrix, ell per axis)
GRIDCOV = {"exp-24x20": ((24, 20), "exponential", 1, (5.0, 5.0)), "gauss-24x20": ((24, 20), "gaussian", 0, (3.0, 3.0)),
           "exp-6x4x5": ((6, 4, 5), "exponential", 1, (2.0, 2.0, 2.0)), "gauss-6x4x5": ((6, 4, 5), "gaussian", 0, (1.5, 1.5, 1.5))}
POWERLAW = {"powerlaw-12x10": ((12, 10), -3.5), "powerlaw-6x4x5": ((6, 4, 5), -3.5)}     # small: the CPU backend's FFT is slow


def csr(Ns):
    return fm.rays(tuple(Ns))


def dense_H(Ns, w=None):
    indptr, indices, data = csr(Ns)
    return fm.dense(indptr, indices, data, int(np.prod(Ns)), w)


def model(gsi, ctx, Ns, w=None, link="identity"):
    indptr, indices, data = csr(Ns)
    return gsi.LinearForwardModel((indptr, indices, data, (len(indptr) - 1, int(np.prod(Ns)))), weights=w, link=link, ctx=ctx)


def gridcov_dense(name):
    Ns, _, k, ell = GRIDCOV[name]
    return dense_matrix(Ns, k, ell, 0.0, 1.0, 0.0)


def gridcov_operator(gsi, ctx, name):
    Ns, kind, _, ell = GRIDCOV[name]
    return gsi.fft_gridcov_operator(ctx, list(Ns), kind=kind, ell=list(ell))


def drift_grid(Ns):
    """[1, x, y(, z)] at the cells, coordinates scaled to [0, 1], vec() order."""
    idx = np.unravel_index(np.arange(int(np.prod(Ns))), Ns, order="F")
    return np.column_stack([np.ones(len(idx[0]))] + [ia / (N - 1.0) for ia, N in zip(idx, Ns)])


def close(Y, Yref, what, factor=1.0):
    err, scale = np.abs(Y - Yref).max(), np.abs(Yref).max()
    print(f"{what}: max|Y - Yref| / max|Yref| = {err / scale:.2e}")
    assert err < factor * 1e-12 * scale, (what, err / scale)
    return err / scale / 1e-12


def fair(name, M):
    """The condition behind the factor 2 of the residual bar: a plain numpy CG on M ends within 1 tol (true residual)."""
    n = M.shape[0]
    B = sc.rhs(n, 3, seed=n)
    X, its = sc.numpy_cg(0.5 * (M + M.T), B, sc.TOL, 10 * n)
    rho = sc.true_relres(M, X, B)
    print(f"{name}: cond {np.linalg.cond(M):.3e}, numpy CG {its.max()} iterations of at most {10 * n}, true relres {rho.max():.3e}")
    assert (rho <= sc.TOL).all(), (name, rho.max())


def products(gsi, op, A, name, monkeypatch):
    """A X and A' X against the dense matrix for X of 1, 5 and 8 columns, with and without GSI_FWD_COV_BATCH=2; A' X has the
    bits of A X.  Returns the largest error in units of the bar."""
    nobs = A.shape[0]
    assert op.shape == (nobs, nobs) and op.size(1) == nobs
    row0, mloc = gsi._lib.c_i64(), gsi._lib.c_i64()
    gsi._lib.check(op.ctx.lib.gsi_op_size(op.h, None, None, row0, mloc), op.ctx.lib)
    assert (row0.value, mloc.value) == (0, nobs)
    worst = 0.0
    for l in (1, 5, 8):
        X = np.random.default_rng([nobs, l]).standard_normal((nobs, l))
        Yref = A @ X
        for batch in (None, "2"):
            if batch is None:
                monkeypatch.delenv("GSI_FWD_COV_BATCH", raising=False)
            else:
                monkeypatch.setenv("GSI_FWD_COV_BATCH", batch)
            Y = op.matmul(X)
            worst = max(worst, close(Y, Yref, f"{name} l={l} batch={batch} A X"))
            assert np.array_equal(op.rmatmul_t(X), Y), (name, l, batch)
            assert np.array_equal(op.matmul(X), Y), (name, l, batch)
        monkeypatch.delenv("GSI_FWD_COV_BATCH", raising=False)
    return worst


def solve_case(gsi, op, A, name, path, precond=None):
    """`solve` at tol 1e-10 with the noise on the diagonal, through solve_cases.check_solve with the dense M of numpy."""
    nobs = A.shape[0]
    B = sc.rhs(nobs, 3, seed=nobs)
    X, rep = gsi.solve(op, B, diag=NOISE, tol=sc.TOL, return_info=True, precond=precond)
    assert rep["path"] == path, rep["path"]
    sc.check_solve(name, A + NOISE * np.eye(nobs), X, B, rep)
    return rep


def inversion(gsi, grid_op, mdl, H, Cm, name, precond=None):
    """`linear_inversion` with the drift [1, x, y(, z)] against the dense saddle system, and `estimate_field` against
    X beta + C H' xi formed densely from the returned xi and beta."""
    Ns = grid_op.Ns
    nobs = H.shape[0]
    Xg = drift_grid(Ns)
    p = Xg.shape[1]
    G = H @ Xg
    rng = np.random.default_rng(12)
    y = G @ np.array([2.0, -1.0, 0.5, 0.25][:p]) + rng.standard_normal(nobs)
    s_hat, xi, beta, rep = gsi.linear_inversion(grid_op, mdl, y, NOISE, drift_grid=Xg, tol=sc.TOL, precond=precond, return_info=True)
    assert rep["columns"] == 1 + p and rep["converged"] == 1 + p            # one solve of the 1 + p columns
    A = H @ Cm @ H.T
    M = A + NOISE * np.eye(nobs)
    Ms = 0.5 * (M + M.T)
    K = np.block([[Ms, G], [G.T, np.zeros((p, p))]])
    rhs_ = np.concatenate([y, np.zeros(p)])
    ref = np.linalg.solve(K, rhs_)
    z = np.concatenate([xi, beta])
    Kl = np.block([[M, G], [G.T, np.zeros((p, p))]]).astype(LD)
    rho = float(np.linalg.norm(rhs_.astype(LD) - Kl @ z.astype(LD)) / np.linalg.norm(rhs_))
    rref = float(np.linalg.norm(rhs_.astype(LD) - Kl @ ref.astype(LD)) / np.linalg.norm(rhs_))
    kappa = np.linalg.cond(K)
    err = np.linalg.norm(z - ref) / np.linalg.norm(ref)
    res1 = float(np.linalg.norm(y.astype(LD) - M.astype(LD) @ xi.astype(LD) - G.astype(LD) @ beta.astype(LD)))
    res_bar = 2 * sc.TOL * (np.linalg.norm(y) + np.abs(beta) @ np.linalg.norm(G, axis=0)) \
        + 1e-12 * np.sqrt(nobs) * np.linalg.norm(M, 2) * np.linalg.norm(xi)
    print(f"{name}: iterations {rep['iters']}, saddle kappa {kappa:.3e}, rho {rho:.3e}, rho_ref {rref:.3e}, error {err:.3e}, "
          f"bound {kappa * (rho + rref):.3e}; first-block residual {res1:.3e}, bar {res_bar:.3e}")
    assert err <= kappa * (rho + rref)
    assert res1 <= res_bar
    assert np.abs(G.T @ xi).max() <= 10 * sc.TOL * np.linalg.norm(G, 2) * np.linalg.norm(xi)
    s_ref = Xg @ beta + Cm @ (H.T @ xi)
    close(s_hat, s_ref, f"{name} s_hat", factor=2.0)                         # the drift term and C H' xi: two rounded parts
    op = gsi.linear_data_operator(grid_op, mdl)
    try:
        assert op.grid_op is grid_op and op.model is mdl
        # (the same device product; the host's X beta may round differently with the memory layout of X)
        assert (np.abs(gsi.estimate_field(op, xi, beta, Xg) - s_hat) <= 8 * fm.EPS * (np.abs(Xg) @ np.abs(beta))).all()
        E2 = gsi.estimate_field(op, np.column_stack([xi, 2.0 * xi]))
        assert E2.shape == (Cm.shape[0], 2)
        close(E2[:, 0], Cm @ (H.T @ xi), f"{name} estimate_field without a drift")
    finally:
        op.close()
    # without a drift: xi = M^-1 y, beta empty
    s0, xi0, beta0 = gsi.linear_inversion(grid_op, mdl, y, NOISE, tol=sc.TOL, precond=precond)
    assert beta0.size == 0 and (sc.true_relres(M, xi0[:, None], y[:, None]) <= 2 * sc.TOL).all()
    close(s0, Cm @ (H.T @ xi0), f"{name} s_hat without a drift")
    return rep


def conditioning(gsi, op, H, Cm, name):
    """`condition_on_linear_data` with eps = 0 and D = 0.01 on b = 3 arbitrary fields F (the identities below hold for any F):
    |H F_c - y| <= |D M^-1 (y - H F)| + 2 tol |rhs| per field, the bound from the dense matrices; and F_c against
    F + C H' M^-1 (y - H F) within |C H'| |M^-1| 2 tol |rhs| (the solve's residual through the two maps) + 4e-12 sqrt(n)
    max|F_c| (four rounded device products)."""
    nobs, n = H.shape
    rng = np.random.default_rng(5)
    Fh = np.asfortranarray(rng.standard_normal((n, 3)))
    y = rng.standard_normal(nobs)
    M = H @ Cm @ H.T + NOISE * np.eye(nobs)
    rhs_ = y[:, None] - H @ Fh
    xi_ref = np.linalg.solve(0.5 * (M + M.T), rhs_)
    Fref = Fh + Cm @ (H.T @ xi_ref)
    F = gsi.DeviceMatrix.from_host(op.ctx, Fh)
    try:
        Fc = gsi.condition_on_linear_data(op, F, y, NOISE, eps=np.zeros((nobs, 3)), tol=sc.TOL)
        assert isinstance(Fc, gsi.DeviceMatrix) and np.array_equal(F.to_host(), Fh)          # F is not modified
        Fch = Fc.to_host()
        Fc.close()
    finally:
        F.close()
    rn = np.linalg.norm(rhs_, axis=0)
    misfit = np.linalg.norm(H @ Fch - y[:, None], axis=0)
    bound = np.linalg.norm(NOISE * xi_ref, axis=0) + 2 * sc.TOL * rn
    print(f"{name}: |H F_c - y| / bound = {(misfit / bound).max():.6f}")
    assert (misfit <= bound).all(), misfit / bound
    err = np.linalg.norm(Fch - Fref, axis=0)
    ebar = np.linalg.norm(Cm @ H.T, 2) * np.linalg.norm(np.linalg.inv(M), 2) * 2 * sc.TOL * rn \
        + 4e-12 * np.sqrt(n) * np.abs(Fref).max(axis=0)
    print(f"{name}: |F_c - F_ref| / bar = {(err / ebar).max():.3e}")
    assert (err <= ebar).all(), err / ebar


def refusals(gsi, ctx, grid_op, make_ctx):
    """Every refusal of gsi_op_fwd_cov and of the adjoint, by name, with nothing allocated on the way."""
    import ctypes as C
    Ns = grid_op.Ns
    n = int(np.prod(Ns))
    mdl = model(gsi, ctx, Ns)
    dense = gsi.dense_operator(ctx, np.eye(n))
    small = gsi.LinearForwardModel((np.array([0, 1]), np.array([0]), np.array([1.0]), (1, n - 1)), ctx=ctx)
    expm = model(gsi, ctx, Ns, link="exp")
    line = gsi.fft_powerlaw_operator(ctx, [n], -3.5)
    other = make_ctx()
    try:
        ctx.release_cache()
        before = ctx.device_bytes()
        sc.refused(gsi, lambda: gsi.linear_data_operator(dense, mdl), "grid_op must be an FFT covariance operator")
        sc.refused(gsi, lambda: gsi.linear_data_operator(line, mdl), "2 or 3 axes")
        sc.refused(gsi, lambda: gsi.linear_data_operator(grid_op, small), f"fwd has n = {n - 1}")
        sc.refused(gsi, lambda: gsi.linear_data_operator(grid_op, expm), "link = 1")
        sc.refused(gsi, lambda: expm.adjoint(np.ones(expm.nobs)), "link = 1")
        h = C.c_void_p()

        def raw(cx, g, f):
            st = cx.lib.gsi_op_fwd_cov(cx.h, C.byref(h), g.h, f.h)
            if st != 0:
                raise gsi.GsiError(st, cx.lib.gsi_last_error().decode())
        sc.refused(gsi, lambda: raw(other, grid_op, mdl), "grid operator (grid_op) belongs to another context")
        og = gsi.fft_powerlaw_operator(other, list(Ns), -3.5)
        sc.refused(gsi, lambda: raw(other, og, mdl), "forward model (fwd) belongs to another context")
        og.close()
        Vbad = gsi.DeviceMatrix(ctx, mdl.nobs + 1, 2)
        sc.refused(gsi, lambda: mdl.adjoint(Vbad), "V is")
        Vbad.close()
        Pbad = gsi.DeviceMatrix(ctx, n + 1, 2)
        sc.refused(gsi, lambda: mdl.apply_dev(Pbad), "P is")
        Pbad.close()
        ctx.release_cache()
        assert ctx.device_bytes() == before and not mdl.adjoint_info()["built"]
        op = gsi.linear_data_operator(grid_op, mdl)                       # a following valid call succeeds
        assert np.isfinite(op.matmul(np.ones(mdl.nobs))).all()
        op.close()
    finally:
        other.close()
        for hnd in (mdl, dense, small, expm, line):
            hnd.close()


def lifetimes(gsi, ctx, make_grid_op, Ns):
    """The grid operator, the model and the operator destroyed in all six orders; after every destruction each survivor
    runs one more product and returns the bits it returned before."""
    import itertools
    n = int(np.prod(Ns))
    X = np.random.default_rng(1).standard_normal((len(csr(Ns)[0]) - 1, 3))
    P = np.random.default_rng(2).standard_normal((n, 2))
    want = {}
    for order in itertools.permutations(("grid", "model", "op")):
        live = {"grid": make_grid_op(), "model": model(gsi, ctx, Ns)}
        live["op"] = gsi.linear_data_operator(live["grid"], live["model"])
        run = {"grid": lambda o: o.matmul(P), "model": lambda o: o.adjoint(X), "op": lambda o: o.matmul(X)}
        for k in live:
            got = run[k](live[k])
            assert np.array_equal(got, want.setdefault(k, got)), (order, k)
        for gone in order:
            live.pop(gone).close()
            for k in live:
                assert np.array_equal(run[k](live[k]), want[k]), (order, gone, k)
