"""Shared cases and checks of the multi-column conjugate-gradient solver (`gsi_op_solve_cg`, `Operator.solve`) for
tests/test_op_solve_cpu.py (the CPU reference library, composed path) and tests/test_op_solve_gpu.py (the fused device
kernels).  Not a test module.

The bars.  True residuals are computed in np.longdouble from the operator's own dense matrix, `op.matmul(I)` (+ diag),
which is symmetrised only for the reference solve.
  residual   with tol = 1e-10 every column's TRUE relative residual is <= 2 tol: the factor 2 is the drift between the
             recurred and the true residual, and is a condition on the INPUTS -- they are chosen such that a plain numpy CG
             ends within 1 tol (`test_inputs_are_fair` in the CPU file asserts that for every case here).
  solution   |x - x_ref| / |x_ref| <= kappa_2(A + D) (rho + rho_ref) with x_ref from np.linalg.solve and rho, rho_ref the two
             true relative residuals: an inequality, no margin.
"""
import ctypes as C

import numpy as np

TOL = 1e-10
LD = np.longdouble


# ---------------------------------------------------------------- inputs
def points(n, d=2, seed=0):
    return np.asfortranarray(np.random.default_rng(1000 * d + seed).random((d, n)))


def expcov(P, ell=0.3):
    D = np.sqrt(((P[:, :, None] - P[:, None, :]) ** 2).sum(axis=0))
    return np.exp(-D / ell)


def rhs(n, b, seed=0):
    return np.asfortranarray(np.random.default_rng(77 + seed).standard_normal((n, b)))


def diag_values(kind, n):
    """None; a number; or 'vec': n values between 0.1 and 0.2."""
    if kind is None:
        return None
    if kind == "vec":
        return 0.1 + 0.1 * np.random.default_rng(5).random(n)
    return np.full(n, float(kind))


# (n, b, diag): a dense exponential covariance (ell = 0.3) of n random points in the unit square; without a diag the 0.1 is
# part of the matrix.  b covers {1, 2, 3, 16, 17, 64, 65}, n the tile edges and one size beyond a thousand rows.
DENSE = [(1, 1, None), (2, 2, 0.1), (63, 3, None), (64, 16, "vec"), (65, 17, None), (257, 64, 0.01), (257, 65, None),
         (1000, 3, 1.0)]


def dense_case(gsi, ctx, n, diag):
    A = expcov(points(n, 2, seed=n))
    if diag is None:
        A = A + 0.1 * np.eye(n)
    return gsi.dense_operator(ctx, A), diag_values(diag, n)


def pointcov_case(gsi, ctx, d):
    return gsi.pointcov_implicit_operator(ctx, points(300, d, seed=3), kind="exponential", ell=0.3), diag_values(0.1, 300)


def lowrank_case(gsi, ctx):
    S = np.random.default_rng(9).standard_normal((40, 200))
    return gsi.LowRankCovMatrix(S, ctx=ctx)._device_operator(ctx), diag_values(0.1, 200)     # singular without the diagonal


def powerlaw_case(gsi, ctx):
    return gsi.fft_powerlaw_operator(ctx, [12, 9], -3.5), diag_values("vec", 108)


def dense_of(op, d):
    n = op.shape[0]
    M = op.matmul(np.eye(n))
    return M + (np.diag(d) if d is not None else 0.0)


# ---------------------------------------------------------------- references
def numpy_cg(M, B, tol, maxiter):
    """Plain CG per column in float64, the recurrences of cg_state.hpp."""
    X = np.zeros_like(B)
    its = np.zeros(B.shape[1], dtype=np.int64)
    for j in range(B.shape[1]):
        b = B[:, j]
        x, r = np.zeros_like(b), b.copy()
        p, rho, bn = r.copy(), r @ r, np.linalg.norm(b)
        if bn == 0.0:
            continue
        for k in range(maxiter):
            q = M @ p
            a = rho / (p @ q)
            x += a * p
            r -= a * q
            rn = r @ r
            its[j] = k + 1
            if np.sqrt(rn) <= tol * bn:
                break
            p = r + (rn / rho) * p
            rho = rn
        X[:, j] = x
    return X, its


def true_relres(M, X, B):
    R = B.astype(LD) - M.astype(LD) @ X.astype(LD)
    bn = np.sqrt((B.astype(LD) ** 2).sum(axis=0))
    rn = np.sqrt((R ** 2).sum(axis=0))
    return np.array([float(rn[j] / bn[j]) if bn[j] > 0 else float(rn[j]) for j in range(B.shape[1])])


RATIOS = {}       # case name -> largest true relative residual / tol, and solution error / its bound


def check_solve(name, M, X, B, rep, tol=TOL):
    """The two bars for a converged solve; returns nothing, records the ratios."""
    b = B.shape[1]
    assert rep["converged"] == b and rep["breakdown"] == 0, (name, rep)
    assert np.isfinite(X).all()
    rho = true_relres(M, X, B)
    print(f"{name}: iters {rep['iters'].min()}..{rep['iters'].max()}, products {rep['products']}, "
          f"true relres max {rho.max():.3e}, recurred max {rep['relres'].max():.3e}")
    assert (rep["relres"] <= tol).all(), (name, rep["relres"].max())
    assert (rho <= 2.0 * tol).all(), (name, rho.max())
    Ms = 0.5 * (M + M.T)
    Xref = np.linalg.solve(Ms, B)
    rref = true_relres(M, Xref, B)
    kappa = np.linalg.cond(Ms)
    err = np.linalg.norm(X - Xref, axis=0) / np.linalg.norm(Xref, axis=0)
    bound = kappa * (rho + rref)
    print(f"{name}: kappa {kappa:.3e}, solution error max {err.max():.3e}, bound min {bound.min():.3e}")
    assert (err <= bound).all(), (name, (err / bound).max())
    RATIOS[name] = {"true_relres_over_tol": float(rho.max() / tol), "solution_error_over_bound": float((err / bound).max()),
                    "kappa": float(kappa), "iters_max": int(rep["iters"].max())}


def run_case(gsi, op, d, b, name, path):
    n = op.shape[0]
    B = rhs(n, b, seed=n + b)
    X, rep = op.solve(B, diag=d, tol=TOL, return_info=True)
    assert rep["path"] == path, rep["path"]
    check_solve(name, dense_of(op, d), X, B, rep)
    return X, rep


# ---------------------------------------------------------------- special columns, determinism, budget, breakdown
def special_columns(gsi, ctx, path):
    n, k = 64, 10
    lam = np.linspace(1.0, 50.0, n)
    op = gsi.dense_operator(ctx, np.diag(lam))
    try:
        rng = np.random.default_rng(3)
        B = np.zeros((n, 5), order="F")
        B[k, 1] = 1.0                                   # e_k: one iteration
        B[:, 2] = rng.standard_normal(n)
        B[:, 3] = rng.standard_normal(n) * lam ** 2
        B[:8, 4] = 1.0                                  # 8 eigenvectors: 8 iterations
        X, rep = op.solve(B, tol=TOL, return_info=True)
        assert rep["path"] == path
        assert np.isfinite(X).all()
        assert rep["iters"][0] == 0 and rep["relres"][0] == 0.0
        assert np.array_equal(X[:, 0], np.zeros(n)) and not np.signbit(X[:, 0]).any()
        assert rep["iters"][1] == 1, rep["iters"]
        want = np.zeros(n)
        want[k] = 1.0 / lam[k]
        assert np.all(X[np.arange(n) != k, 1] == 0.0)
        assert abs(X[k, 1] - want[k]) <= 2.0 * np.spacing(want[k])
        assert rep["iters"][4] <= 9 < rep["iters"][2], rep["iters"]
        assert len(set(rep["iters"].tolist())) >= 4, rep["iters"]
        assert rep["iters"].max() >= 30, rep["iters"]   # the frozen columns sat through the others' iterations
        # frozen: the same column solved alone stops after the same single iteration -- bit for bit the same x
        X1, rep1 = op.solve(B[:, 1], tol=TOL, return_info=True)
        assert rep1["iters"][0] == 1 and np.array_equal(X1, X[:, 1])
        X4, _ = op.solve(B[:, 4], tol=TOL, return_info=True)
        assert np.array_equal(X4, X[:, 4])
        check_solve("special columns", np.diag(lam), X[:, 1:], B[:, 1:],
                    {**rep, "converged": rep["converged"] - 1, "iters": rep["iters"][1:], "relres": rep["relres"][1:]})
    finally:
        op.close()


def determinism(gsi, ctx, path):
    op, d = dense_case(gsi, ctx, 257, "vec")
    try:
        B = rhs(257, 17, seed=4)
        B[:, 5] = 0.0
        a = op.solve(B, diag=d, tol=TOL, return_info=True)
        b = op.solve(B, diag=d, tol=TOL, return_info=True)
        assert a[1]["path"] == path
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["relres"], b[1]["relres"])
        assert np.array_equal(a[1]["iters"], b[1]["iters"]) and a[1]["products"] == b[1]["products"]
    finally:
        op.close()


def budget(gsi, ctx, path):
    op, d = pointcov_case(gsi, ctx, 2)
    try:
        B = rhs(300, 3, seed=8)
        X3, r3 = op.solve(B, diag=d, tol=TOL, maxiter=3, strict=False, return_info=True)
        assert r3["path"] == path and r3["converged"] == 0 and r3["breakdown"] == 0
        assert (r3["iters"] == 3).all() and r3["products"] == 3
        assert np.isfinite(r3["relres"]).all() and (r3["relres"] > TOL).all()
        X40, r40 = op.solve(B, diag=d, tol=TOL, maxiter=40, strict=False, return_info=True)
        assert (r40["relres"] < r3["relres"]).all()
        try:
            op.solve(B, diag=d, tol=TOL, maxiter=3)
        except RuntimeError as e:
            assert "3 of 3 columns" in str(e), str(e)
        else:
            raise AssertionError("strict=True must raise for unconverged columns")
    finally:
        op.close()


def breakdown(gsi, ctx, path):
    n = 40
    rng = np.random.default_rng(6)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.linspace(1.0, 4.0, n)
    lam[7] = -1.0
    M = (Q * lam) @ Q.T
    M = 0.5 * (M + M.T)
    op = gsi.dense_operator(ctx, M)
    try:
        B = np.asfortranarray(np.column_stack([Q[:, 3], np.zeros(n), Q[:, 7], Q[:, 11]]))
        info = (C.c_int64 * 4)()
        relres, iters = np.zeros(4), np.zeros(4, dtype=np.int64)
        X = np.zeros((n, 4), order="F")
        dp = C.POINTER(C.c_double)
        st = ctx.lib.gsi_op_solve(ctx.h, op.h, None, B.ctypes.data_as(dp), n, 4, X.ctypes.data_as(dp), n, TOL, 100, info,
                                  relres.ctypes.data_as(dp), iters.ctypes.data_as(C.POINTER(C.c_int64)))
        assert st == 7, st
        assert b"column 3" in ctx.lib.gsi_last_error()
        assert info[3] == 3 and info[2] == {"fused": 1, "composed": 3}[path]
        assert np.isfinite(X).all()
        try:
            op.solve(B)
        except gsi.GsiError as e:
            assert e.code == 7
        else:
            raise AssertionError("an indefinite operator must raise")
    finally:
        op.close()
    # the context is as good as before
    op, d = dense_case(gsi, ctx, 63, None)
    try:
        run_case(gsi, op, d, 3, "dense n=63 after a breakdown", path)
    finally:
        op.close()


# ---------------------------------------------------------------- refusals
def refused(gsi, call, word):
    try:
        call()
    except gsi.GsiError as e:
        assert e.code == 1 and word in str(e), str(e)
    else:
        raise AssertionError(f"not refused ({word})")


def refusals(gsi, ctx, path):
    n = 12
    A = expcov(points(n)) + 0.1 * np.eye(n)
    op = gsi.dense_operator(ctx, A)
    rect = gsi.dense_operator(ctx, np.ones((n, n + 1)))
    Bm = gsi.DeviceMatrix.from_host(ctx, rhs(n, 2))
    Bad = gsi.DeviceMatrix(ctx, n + 1, 2)
    Xbad = gsi.DeviceMatrix(ctx, n, 3)
    Xok = gsi.DeviceMatrix(ctx, n, 2)
    lib = ctx.lib

    def raw(o, B, X, tol=TOL, maxiter=50, diag=None):
        d = np.ascontiguousarray(diag, dtype=np.float64) if diag is not None else None
        st = lib.gsi_op_solve_cg(ctx.h, o.h, d.ctypes.data_as(C.POINTER(C.c_double)) if d is not None else None, B.h, X.h,
                                 float(tol), int(maxiter), None, None, None)
        if st != 0:
            raise gsi.GsiError(st, lib.gsi_last_error().decode())
    try:
        before = ctx.device_bytes()
        refused(gsi, lambda: raw(rect, Bm, Xok), "op")
        refused(gsi, lambda: raw(op, Bad, Xok), "B")
        refused(gsi, lambda: raw(op, Bm, Xbad), "X")
        refused(gsi, lambda: raw(op, Bm, Bm), "X must not be B")
        for t in (0.0, 1.0, -1e-3, float("nan")):
            refused(gsi, lambda: raw(op, Bm, Xok, tol=t), "tol")
        refused(gsi, lambda: raw(op, Bm, Xok, maxiter=0), "maxiter")
        for bad in (-1e-300, float("nan"), float("inf")):
            d = np.full(n, 0.1)
            d[5] = bad
            refused(gsi, lambda: raw(op, Bm, Xok, diag=d), "diag[5]")
        assert ctx.device_bytes() == before                      # nothing was allocated on the way to a refusal
        raw(op, Bm, Xok)                                         # a following valid call succeeds
        M = A
        assert (true_relres(M, Xok.to_host(), Bm.to_host()) <= 2 * TOL).all()
    finally:
        for h in (op, rect, Bm, Bad, Xbad, Xok):
            h.close()


def mat_axpy_cases(gsi, ctx):
    rng = np.random.default_rng(2)
    Xh = rng.integers(-50, 50, size=(37, 5)).astype(float)
    Yh = rng.integers(-50, 50, size=(37, 5)).astype(float)
    X, Y = gsi.DeviceMatrix.from_host(ctx, Xh), gsi.DeviceMatrix.from_host(ctx, Yh)
    Z = gsi.DeviceMatrix(ctx, 5, 37)
    try:
        assert gsi.mat_axpy(-3.0, X, Y) is Y
        assert np.array_equal(Y.to_host(), Yh - 3.0 * Xh)
        assert np.array_equal(X.to_host(), Xh)
        refused(gsi, lambda: gsi.mat_axpy(1.0, X, Z), "shape")
    finally:
        for h in (X, Y, Z):
            h.close()


# ---------------------------------------------------------------- kriging with a drift
def kriging_drift(gsi, ctx, op, P, noise, name):
    """`kriging_weights` with drift [1, x, y] against the dense saddle-point solve; op is the m x m covariance at P (2 x m)."""
    m = P.shape[1]
    rng = np.random.default_rng(12)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([2.0, -1.0, 0.5]) + rng.standard_normal(m)
    d = np.full(m, float(noise))
    xi, beta = gsi.kriging_weights(op, y, noise=noise, drift=G, tol=TOL)
    M = dense_of(op, d)
    Ms = 0.5 * (M + M.T)
    K = np.block([[Ms, G], [G.T, np.zeros((3, 3))]])
    ref = np.linalg.solve(K, np.concatenate([y, np.zeros(3)]))
    # the solution bar with the saddle matrix: residuals of both solutions in longdouble
    z = np.concatenate([xi, beta])
    rhs_ = np.concatenate([y, np.zeros(3)])
    Kl = np.block([[M, G], [G.T, np.zeros((3, 3))]]).astype(LD)
    rho = float(np.linalg.norm(rhs_.astype(LD) - Kl @ z.astype(LD)) / np.linalg.norm(rhs_))
    rref = float(np.linalg.norm(rhs_.astype(LD) - Kl @ ref.astype(LD)) / np.linalg.norm(rhs_))
    kappa = np.linalg.cond(K)
    err = np.linalg.norm(z - ref) / np.linalg.norm(ref)
    print(f"{name}: saddle kappa {kappa:.3e}, rho {rho:.3e}, rho_ref {rref:.3e}, error {err:.3e}, bound {kappa * (rho + rref):.3e}")
    assert err <= kappa * (rho + rref)
    assert np.abs(G.T @ xi).max() <= 10 * TOL * np.linalg.norm(G, 2) * np.linalg.norm(xi)
    RATIOS[name] = {"solution_error_over_bound": float(err / (kappa * (rho + rref))), "kappa": float(kappa)}
    # without a drift: xi = M^-1 y, beta empty
    xi0, beta0 = gsi.kriging_weights(op, y, noise=noise, tol=TOL)
    assert beta0.size == 0 and (true_relres(M, xi0[:, None], y[:, None]) <= 2 * TOL).all()
    return xi, beta
