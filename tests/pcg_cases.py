"""Shared cases and checks of the preconditioned multi-column conjugate-gradient solver (`gsi_op_solve_pcg`,
`lowrank_preconditioner`, `solve(..., precond=)`) for tests/test_op_pcg_cpu.py (the CPU reference library, composed path)
and tests/test_op_pcg_gpu.py (csrc/block_pcg.hip).  Not a test module.  Inputs and the two bars of a solve come from
tests/solve_cases.py; here are the numpy restatement of the preconditioned recurrences of csrc/cg_state.hpp and the dense
formulas of the preconditioner P = Z[:, :K] Z[:, :K]' + diag(d + shift).
"""
import ctypes as C

import numpy as np

import solve_cases as sc

TOL = sc.TOL
LD = sc.LD


# ---------------------------------------------------------------- the dense formulas
def eig_basis(A, K, keep=None):
    """Z = V sqrt(lambda) of the K largest eigenpairs of the symmetric part of A (keep: drop lambda <= keep * lambda_1)."""
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    lam, V = lam[::-1], V[:, ::-1]
    if keep is not None:
        K = int((lam > keep * lam[0]).sum())
    return np.asfortranarray(V[:, :K] * np.sqrt(np.maximum(lam[:K], 0.0)))


def pdiag(d, shift, n):
    return (np.zeros(n) if d is None else np.asarray(d, dtype=float)) + shift


def dense_P(Z, K, d, shift):
    """P in np.longdouble: the float64 inputs widened first, so that P is the matrix they define."""
    n = Z.shape[0]
    Zl = Z[:, :K].astype(LD)
    return Zl @ Zl.T + np.diag(pdiag(d, shift, n).astype(LD))


def pinv_ld(P, R):
    """P^-1 R by np.linalg.solve, checked and refined in np.longdouble: residuals of the longdouble P, corrections from the
    float64 solve, until a correction is below 1e-15 of the solution -- a hundredth of the floor of the bar it serves, and
    near what kappa(P) times the longdouble epsilon allows."""
    Pl, Rl = P.astype(LD), R.astype(LD)
    P64 = P.astype(float)
    X = np.linalg.solve(P64, R).astype(LD)
    for _ in range(8):
        dX = np.linalg.solve(P64, (Rl - Pl @ X).astype(float)).astype(LD)
        X = X + dX
        if float(np.abs(dX).max()) <= 1e-15 * float(np.abs(X).max()):
            break
    else:
        raise AssertionError("the longdouble reference of P^-1 R did not settle")
    return X


def woodbury_f64(Z, K, d, shift, R):
    """The float64 restatement of what the library computes: e = 1 / (d + shift), C = I + Z'EZ = U'U, W = E Z U^-1,
    P^-1 R = E R - W (W'R)."""
    n = Z.shape[0]
    e = 1.0 / pdiag(d, shift, n)
    Zk = Z[:, :K]
    Cm = np.eye(K) + Zk.T @ (e[:, None] * Zk)
    U = np.linalg.cholesky(Cm).T
    W = np.linalg.solve(U.T, (e[:, None] * Zk).T).T
    return e[:, None] * R - W @ (W.T @ R)


def numpy_pcg(M, B, pinv, tol, maxiter):
    """Preconditioned CG per column in float64: the pcg_* recurrences of cg_state.hpp.  pinv(r) = P^-1 r."""
    X = np.zeros_like(B)
    its = np.zeros(B.shape[1], dtype=np.int64)
    for j in range(B.shape[1]):
        b = B[:, j]
        bn = np.linalg.norm(b)
        if bn == 0.0:
            continue
        x, r = np.zeros_like(b), b.copy()
        z = pinv(r)
        p, rho = z.copy(), r @ z
        for k in range(maxiter):
            w = M @ p
            a = rho / (p @ w)
            x += a * p
            r -= a * w
            its[j] = k + 1
            if np.sqrt(r @ r) <= tol * bn:
                break
            z = pinv(r)
            rz = r @ z
            p = z + (rz / rho) * p
            rho = rz
        X[:, j] = x
    return X, its


def numpy_pinv(Z, K, d, shift):
    n = Z.shape[0]
    e = 1.0 / pdiag(d, shift, n)
    Zk = Z[:, :K]
    U = np.linalg.cholesky(np.eye(K) + Zk.T @ (e[:, None] * Zk)).T
    W = np.linalg.solve(U.T, (e[:, None] * Zk).T).T
    return lambda r: e * r - W @ (W.T @ r)


# ---------------------------------------------------------------- cases
# (n, b, diag, K): dense exponential covariances of sc.dense_case; the basis is the top-K eigenpairs of the dense matrix, the
# preconditioner's diag is the solve's, and where diag is None the preconditioner gets shift = 0.1.  "u": 0.01 (1 + u).
DENSE = [(1, 1, None, 1), (2, 2, 0.1, 1), (63, 3, None, 2), (64, 16, "vec", 16), (65, 17, None, 17), (257, 64, 0.01, 32),
         (257, 65, None, 64), (1000, 3, "u", 64)]
APPLY = [(1, 1, 1), (2, 1, 2), (63, 2, 3), (64, 16, 16), (65, 17, 17), (257, 64, 65)]


def dense_inputs(gsi, ctx, n, diag):
    """op, the solve's diag (n values or None), the dense A (without the diag)."""
    if diag == "u":
        op, _ = sc.dense_case(gsi, ctx, n, 0.01)
        d = 0.01 * (1.0 + np.random.default_rng(11).random(n))
    else:
        op, d = sc.dense_case(gsi, ctx, n, diag)
    A = sc.expcov(sc.points(n, 2, seed=n))
    if diag is None:
        A = A + 0.1 * np.eye(n)
    return op, d, A


def shift_for(d):
    return 0.1 if d is None else 0.0


def operator_inputs(gsi, ctx, which):
    op, d = {"pointcov2": lambda: sc.pointcov_case(gsi, ctx, 2), "pointcov3": lambda: sc.pointcov_case(gsi, ctx, 3),
             "powerlaw": lambda: sc.powerlaw_case(gsi, ctx)}[which]()
    b = {"pointcov2": 2, "pointcov3": 3, "powerlaw": 17}[which]
    return op, d, sc.dense_of(op, None), b


def run_case(gsi, op, d, b, pc, name, path, M=None):
    n = op.shape[0]
    B = sc.rhs(n, b, seed=n + b)
    X, rep = op.solve(B, diag=d, tol=TOL, return_info=True, precond=pc)
    assert rep["path"] == path, rep["path"]
    assert rep["rank"] == pc.rank and rep["breakdown_kind"] == 0, rep
    M = sc.dense_of(op, d) if M is None else M
    sc.check_solve(name, M, X, B, rep)
    return X, rep, B


def fair(name, M, B, pinv, maxiter):
    """The condition behind the factor 2 of the residual bar: the numpy restatement ends within 1 tol (true residual)."""
    X, its = numpy_pcg(0.5 * (M + M.T), B, pinv, TOL, maxiter)
    rho = sc.true_relres(M, X, B)
    print(f"{name}: numpy PCG {its.max()} iterations, true relres {rho.max():.3e}")
    assert (rho <= TOL).all(), (name, rho.max())
    return its


# ---------------------------------------------------------------- the checks both files run
def dense_solve(gsi, ctx, n, b, diag, K, path):
    op, d, A = dense_inputs(gsi, ctx, n, diag)
    Z = eig_basis(A, K)
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d, shift=shift_for(d))
    try:
        assert pc.rank == K and pc.info["n"] == n
        return run_case(gsi, op, d, b, pc, f"pcg dense n={n} b={b} diag={diag} K={K}", path)
    finally:
        pc.close()
        op.close()


def operator_solve(gsi, ctx, which, path):
    op, d, A, b = operator_inputs(gsi, ctx, which)
    pc = gsi.lowrank_preconditioner(op, basis=eig_basis(A, 8), diag=d)
    try:
        return run_case(gsi, op, d, b, pc, f"pcg {which} K=8", path)
    finally:
        pc.close()
        op.close()


def other_diag(gsi, ctx, path):
    """The preconditioner's diag differs from the solve's."""
    op, d, A = dense_inputs(gsi, ctx, 257, "vec")
    pc = gsi.lowrank_preconditioner(op, basis=eig_basis(A, 16), diag=0.05, shift=0.01)
    try:
        assert abs(pc.info["diag_min"] - 0.06) < 1e-15 and abs(pc.info["diag_max"] - 0.06) < 1e-15
        return run_case(gsi, op, d, 5, pc, "pcg dense n=257, another diag", path)
    finally:
        pc.close()
        op.close()


def zero_basis(gsi, ctx, path):
    """An all-zero basis: P = diag(d), Jacobi; the counts are the numpy restatement's within 2."""
    op, d, A = dense_inputs(gsi, ctx, 257, "vec")
    pc = gsi.lowrank_preconditioner(op, basis=np.zeros((257, 1)), diag=d)
    try:
        X, rep, B = run_case(gsi, op, d, 5, pc, "pcg dense n=257, zero basis", path)
        M = A + np.diag(d)
        _, its = numpy_pcg(M, B, lambda r: r / d, TOL, 2570)
        print(f"zero basis: iterations {rep['iters']}, numpy {its}")
        assert np.abs(rep["iters"] - its).max() <= 2, (rep["iters"], its)
    finally:
        pc.close()
        op.close()


def does_its_work_lowrank(gsi, ctx, path):
    op, d = sc.lowrank_case(gsi, ctx)
    A = sc.dense_of(op, None)
    Z = eig_basis(A, None, keep=1e-12)
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d)
    try:
        X, rep, B = run_case(gsi, op, d, 16, pc, "pcg lowrank, exact factor", path)
        _, plain = op.solve(B, diag=d, tol=TOL, return_info=True)
        print(f"lowrank exact factor: rank {pc.rank}, iterations {rep['iters']}, plain CG {plain['iters']}")
        assert (rep["iters"] <= 2).all(), rep["iters"]
    finally:
        pc.close()
        op.close()


def halves_the_iterations(gsi, op, d, pc, path, name):
    """Every column's iterations <= 0.5 x the same column's plain-CG iterations in the same process."""
    X, rep, B = run_case(gsi, op, d, 3, pc, name, path)
    _, plain = op.solve(B, diag=d, tol=TOL, return_info=True)
    print(f"{name}: iterations {rep['iters']}, plain CG {plain['iters']}")
    assert (2 * rep["iters"] <= plain["iters"]).all(), (rep["iters"], plain["iters"])
    return rep, plain


APPLY_RATIOS = {}


def apply_case(gsi, ctx, n, K, b):
    """`Preconditioner.apply` against the dense longdouble P^-1 R: per column, a relative 2-norm error of at most 4 x the
    error the float64 restatement of the same Woodbury formula makes against the same reference (floor 1e-13)."""
    rng = np.random.default_rng(100 * n + K)
    Z = np.asfortranarray(rng.standard_normal((n, K)))
    d = 0.05 + 0.1 * rng.random(n)
    shift = 0.01
    R = sc.rhs(n, b, seed=n + K)
    ref = pinv_ld(dense_P(Z, K, d, shift), R)
    refn = np.sqrt((ref ** 2).sum(axis=0)).astype(float)
    e64 = np.sqrt(((woodbury_f64(Z, K, d, shift, R).astype(LD) - ref) ** 2).sum(axis=0)).astype(float) / refn
    bar = np.maximum(4.0 * e64, 1e-13)
    Zd = gsi.DeviceMatrix.from_host(ctx, Z)
    pc = None
    try:
        op = gsi.dense_operator(ctx, np.eye(n))
        try:
            pc = gsi.lowrank_preconditioner(op, basis=Zd, diag=d, shift=shift)
        finally:
            op.close()
        got = pc.apply(R)
        err = np.sqrt(((got.astype(LD) - ref) ** 2).sum(axis=0)).astype(float) / refn
        print(f"apply n={n} K={K} b={b}: error {err.max():.3e}, float64 restatement {e64.max():.3e}, "
              f"largest ratio to the bar {(err / bar).max():.3f}")
        APPLY_RATIOS[f"n={n} K={K} b={b}"] = float((err / bar).max())
        assert (err <= bar).all(), (err / bar).max()
        # a DeviceMatrix in, a DeviceMatrix out, the same bits; a vector in, a vector out
        Rd = gsi.DeviceMatrix.from_host(ctx, R)
        Gd = pc.apply(Rd)
        assert isinstance(Gd, gsi.DeviceMatrix) and np.array_equal(Gd.to_host(), got)
        Gd.close()
        Rd.close()
        assert pc.apply(R[:, 0]).shape == (n,)
    finally:
        if pc is not None:
            pc.close()
        Zd.close()


def _diag_setup(gsi, ctx, K=4, shift=0.5):
    """The diagonal operator of sc.special_columns with the exact basis of its K largest eigenvalues."""
    n = 64
    lam = np.linspace(1.0, 50.0, n)
    op = gsi.dense_operator(ctx, np.diag(lam))
    pc = gsi.lowrank_preconditioner(op, basis=eig_basis(np.diag(lam), K), shift=shift)
    return n, lam, op, pc


def special_columns(gsi, ctx, path):
    """A zero column stops at iteration 0 with x = 0; a column that converges early is frozen while the others go on: the
    same batch stopped by maxiter at that column's count leaves the same bits in it; a column equal to another passes the
    same bars (bit equality is not asserted: the contractions do not promise one summation order for every column)."""
    n, lam, op, pc = _diag_setup(gsi, ctx)
    try:
        rng = np.random.default_rng(3)
        k = 10
        B = np.zeros((n, 5), order="F")
        B[k, 1] = 1.0                                   # an eigenvector outside the basis: P^-1 e_k = e_k / shift, one iteration
        B[:, 2] = rng.standard_normal(n)
        B[:, 3] = B[:, 2]
        B[:8, 4] = 1.0
        X, rep = op.solve(B, tol=TOL, return_info=True, precond=pc)
        assert rep["path"] == path and np.isfinite(X).all()
        assert rep["iters"][0] == 0 and rep["relres"][0] == 0.0
        assert np.array_equal(X[:, 0], np.zeros(n)) and not np.signbit(X[:, 0]).any()
        assert rep["iters"][1] == 1, rep["iters"]
        assert abs(X[k, 1] - 1.0 / lam[k]) <= 4.0 * np.spacing(1.0 / lam[k])
        assert rep["iters"][4] <= 9 < rep["iters"][2], rep["iters"]
        assert abs(int(rep["iters"][2]) - int(rep["iters"][3])) <= 2, rep["iters"]
        for early in (1, 4):
            Xs, rs = op.solve(B, tol=TOL, maxiter=int(rep["iters"][early]), strict=False, return_info=True, precond=pc)
            assert rs["iters"][early] == rep["iters"][early] and np.array_equal(Xs[:, early], X[:, early])
            assert rs["relres"][early] == rep["relres"][early]
        sc.check_solve("pcg special columns", np.diag(lam), X[:, 1:], B[:, 1:],
                       {**rep, "converged": rep["converged"] - 1, "iters": rep["iters"][1:], "relres": rep["relres"][1:]})
    finally:
        pc.close()
        op.close()


def budget(gsi, ctx, path):
    op, d, A, _ = operator_inputs(gsi, ctx, "pointcov2")
    pc = gsi.lowrank_preconditioner(op, basis=eig_basis(A, 8), diag=d)
    try:
        B = sc.rhs(300, 3, seed=8)
        X3, r3 = op.solve(B, diag=d, tol=TOL, maxiter=3, strict=False, return_info=True, precond=pc)
        assert r3["path"] == path and r3["converged"] == 0 and r3["breakdown"] == 0
        assert (r3["iters"] == 3).all() and r3["products"] == 3
        assert np.isfinite(r3["relres"]).all() and (r3["relres"] > TOL).all()
        try:
            op.solve(B, diag=d, tol=TOL, maxiter=3, precond=pc)
        except RuntimeError as e:
            assert "3 of 3 columns" in str(e), str(e)
        else:
            raise AssertionError("strict=True must raise for unconverged columns")
    finally:
        pc.close()
        op.close()


def determinism(gsi, ctx, path):
    op, d, A = dense_inputs(gsi, ctx, 257, "vec")
    pc = gsi.lowrank_preconditioner(op, basis=eig_basis(A, 16), diag=d)
    try:
        B = sc.rhs(257, 17, seed=4)
        B[:, 5] = 0.0
        a = op.solve(B, diag=d, tol=TOL, return_info=True, precond=pc)
        b = op.solve(B, diag=d, tol=TOL, return_info=True, precond=pc)
        assert a[1]["path"] == path
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["relres"], b[1]["relres"])
        assert np.array_equal(a[1]["iters"], b[1]["iters"]) and a[1]["products"] == b[1]["products"]
    finally:
        pc.close()
        op.close()


def breakdown(gsi, ctx, path):
    """sc.breakdown's indefinite operator under P = I: kind 1 in column 3."""
    n = 40
    rng = np.random.default_rng(6)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.linspace(1.0, 4.0, n)
    lam[7] = -1.0
    M = (Q * lam) @ Q.T
    M = 0.5 * (M + M.T)
    op = gsi.dense_operator(ctx, M)
    pc = gsi.lowrank_preconditioner(op, basis=np.zeros((n, 1)), shift=1.0)
    try:
        B = np.asfortranarray(np.column_stack([Q[:, 3], np.zeros(n), Q[:, 7], Q[:, 11]]))
        info = (C.c_int64 * 6)()
        relres, iters = np.zeros(4), np.zeros(4, dtype=np.int64)
        X = np.zeros((n, 4), order="F")
        dp = C.POINTER(C.c_double)
        st = ctx.lib.gsi_op_solve_pcg_host(ctx.h, op.h, None, pc.h, B.ctypes.data_as(dp), n, 4, X.ctypes.data_as(dp), n, TOL,
                                           100, info, relres.ctypes.data_as(dp), iters.ctypes.data_as(C.POINTER(C.c_int64)))
        assert st == 7, st
        assert b"column 3" in ctx.lib.gsi_last_error()
        assert info[3] == 3 and info[4] == 1 and info[5] == 1 and info[2] == {"fused": 1, "composed": 3}[path]
        assert np.isfinite(X).all()
        try:
            op.solve(B, precond=pc)
        except gsi.GsiError as e:
            assert e.code == 7
        else:
            raise AssertionError("an indefinite operator must raise")
    finally:
        pc.close()
        op.close()
    dense_solve(gsi, ctx, 63, 3, None, 2, path)             # the context is as good as before


def refusals(gsi, ctx, other_ctx, path):
    """Every refusal of the preconditioner, its apply and the preconditioned solve, by message fragment, with nothing
    allocated on the way; `other_ctx`: a second context of the same library."""
    n = 12
    A = sc.expcov(sc.points(n)) + 0.1 * np.eye(n)
    op = gsi.dense_operator(ctx, A)
    rect = gsi.dense_operator(ctx, np.ones((n, n + 1)))
    op13 = gsi.dense_operator(ctx, np.eye(n + 1))
    Zd = gsi.DeviceMatrix.from_host(ctx, eig_basis(A, 3))
    Zwide = gsi.DeviceMatrix(ctx, 4, 6)
    Zbig = gsi.DeviceMatrix(ctx, 2050, 2049)
    Zother = gsi.DeviceMatrix.from_host(other_ctx, eig_basis(A, 3))
    Bm = gsi.DeviceMatrix.from_host(ctx, sc.rhs(n, 2))
    Bad = gsi.DeviceMatrix(ctx, n + 1, 2)
    Xbad = gsi.DeviceMatrix(ctx, n, 3)
    Xok = gsi.DeviceMatrix(ctx, n, 2)
    pc = gsi.lowrank_preconditioner(op, basis=Zd, shift=0.1)
    opo = gsi.dense_operator(other_ctx, A)
    pco = gsi.lowrank_preconditioner(opo, basis=Zother, shift=0.1)
    lib = ctx.lib
    dp = C.POINTER(C.c_double)

    def create(Z, K, diag=None, shift=0.1, cx=ctx):
        h = C.c_void_p()
        d = np.ascontiguousarray(diag, dtype=np.float64) if diag is not None else None
        st = lib.gsi_precond_lowrank_create(cx.h, C.byref(h), Z.h, int(K), d.ctypes.data_as(dp) if d is not None else None,
                                            float(shift), None)
        if st != 0:
            assert not h.value
            raise gsi.GsiError(st, lib.gsi_last_error().decode())
        lib.gsi_precond_destroy(h)

    def raw(o, p, B, X, tol=TOL, maxiter=50, diag=None):
        d = np.ascontiguousarray(diag, dtype=np.float64) if diag is not None else None
        st = lib.gsi_op_solve_pcg(ctx.h, o.h, d.ctypes.data_as(dp) if d is not None else None, p.h, B.h, X.h, float(tol),
                                  int(maxiter), None, None, None)
        if st != 0:
            raise gsi.GsiError(st, lib.gsi_last_error().decode())

    def apply(p, R, Zo):
        st = lib.gsi_precond_apply(ctx.h, p.h, R.h, Zo.h)
        if st != 0:
            raise gsi.GsiError(st, lib.gsi_last_error().decode())
    try:
        before = ctx.device_bytes()
        for K in (0, -1):
            sc.refused(gsi, lambda: create(Zd, K), "K must be at least 1")
        sc.refused(gsi, lambda: create(Zd, 4), "K exceeds the columns of Z")
        sc.refused(gsi, lambda: create(Zwide, 5), "K exceeds the rows of Z")
        sc.refused(gsi, lambda: create(Zbig, 2049), "K exceeds 2048")
        sc.refused(gsi, lambda: create(Zother, 3), "Z belongs to another context")
        for bad in (-1e-300, float("nan"), float("inf")):
            sc.refused(gsi, lambda: create(Zd, 3, shift=bad), "shift")
        sc.refused(gsi, lambda: create(Zd, 3, shift=0.0), "diag + shift is not positive")
        for bad in (-0.1, 0.0, float("nan"), float("inf")):
            d = np.full(n, 0.1)
            d[5] = bad
            sc.refused(gsi, lambda: create(Zd, 3, diag=d, shift=0.0), "diag[5] + shift")
        # the solve: whatever block_cg_check refuses, and a pc that does not fit
        sc.refused(gsi, lambda: raw(rect, pc, Bm, Xok), "op")
        sc.refused(gsi, lambda: raw(op, pc, Bad, Xok), "B")
        sc.refused(gsi, lambda: raw(op, pc, Bm, Xbad), "X")
        sc.refused(gsi, lambda: raw(op, pc, Bm, Bm), "X must not be B")
        for t in (0.0, 1.0, -1e-3, float("nan")):
            sc.refused(gsi, lambda: raw(op, pc, Bm, Xok, tol=t), "tol")
        sc.refused(gsi, lambda: raw(op, pc, Bm, Xok, maxiter=0), "maxiter")
        d = np.full(n, 0.1)
        d[5] = -1.0
        sc.refused(gsi, lambda: raw(op, pc, Bm, Xok, diag=d), "diag[5]")
        sc.refused(gsi, lambda: raw(op, pco, Bm, Xok), "pc belongs to another context")
        sc.refused(gsi, lambda: raw(op13, pc, Bad, Bad), "rows")
        # apply
        sc.refused(gsi, lambda: apply(pc, Bad, Bad), "R must have the preconditioner's rows")
        sc.refused(gsi, lambda: apply(pc, Bm, Xbad), "Zout must have the shape of R")
        sc.refused(gsi, lambda: apply(pc, Bm, Bm), "Zout must not be R")
        assert ctx.device_bytes() == before                      # nothing was allocated on the way to a refusal
        # a NaN in Z: the Cholesky fails
        Zn = eig_basis(A, 3)
        Zn[4, 1] = float("nan")
        Znd = gsi.DeviceMatrix.from_host(ctx, Zn)
        try:
            create(Znd, 3)
        except gsi.GsiError as e:
            assert e.code == 7, e
        else:
            raise AssertionError("a NaN in Z must fail the Cholesky")
        finally:
            Znd.close()
        raw(op, pc, Bm, Xok)                                    # a following valid call succeeds
        assert (sc.true_relres(A, Xok.to_host(), Bm.to_host()) <= 2 * TOL).all()
    finally:
        for h in (pc, pco, op, opo, rect, op13, Zd, Zwide, Zbig, Zother, Bm, Bad, Xbad, Xok):
            h.close()


def kriging_drift(gsi, ctx, op, P, noise, pc, name):
    """sc.kriging_drift restated with `precond=pc`: M xi + G beta = y and G' xi = 0 to the same bars."""
    m = P.shape[1]
    rng = np.random.default_rng(12)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([2.0, -1.0, 0.5]) + rng.standard_normal(m)
    d = np.full(m, float(noise))
    xi, beta = gsi.kriging_weights(op, y, noise=noise, drift=G, tol=TOL, precond=pc)
    M = sc.dense_of(op, d)
    Ms = 0.5 * (M + M.T)
    Kd = np.block([[Ms, G], [G.T, np.zeros((3, 3))]])
    rhs_ = np.concatenate([y, np.zeros(3)])
    ref = np.linalg.solve(Kd, rhs_)
    z = np.concatenate([xi, beta])
    Kl = np.block([[M, G], [G.T, np.zeros((3, 3))]]).astype(LD)
    rho = float(np.linalg.norm(rhs_.astype(LD) - Kl @ z.astype(LD)) / np.linalg.norm(rhs_))
    rref = float(np.linalg.norm(rhs_.astype(LD) - Kl @ ref.astype(LD)) / np.linalg.norm(rhs_))
    kappa = np.linalg.cond(Kd)
    err = np.linalg.norm(z - ref) / np.linalg.norm(ref)
    print(f"{name}: saddle kappa {kappa:.3e}, rho {rho:.3e}, rho_ref {rref:.3e}, error {err:.3e}, bound {kappa * (rho + rref):.3e}")
    assert err <= kappa * (rho + rref)
    assert np.abs(G.T @ xi).max() <= 10 * TOL * np.linalg.norm(G, 2) * np.linalg.norm(xi)
    xi0, beta0 = gsi.kriging_weights(op, y, noise=noise, tol=TOL, precond=pc)
    assert beta0.size == 0 and (sc.true_relres(M, xi0[:, None], y[:, None]) <= 2 * TOL).all()
    # precond= reaches the solve: the report of the same right-hand side says so
    _, rep = gsi.solve(op, np.column_stack([y, G]), diag=noise, tol=TOL, return_info=True, precond=pc)
    assert rep["rank"] == pc.rank
