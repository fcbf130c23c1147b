"""Kriging on any covariance operator: `(A + D) X = B` by conjugate gradients with all columns advanced together on the
device (`gsi_op_solve_cg`, csrc/block_cg.hip), and what geostatistics builds on that solve -- kriging weights with a
drift, the kriged field on the grid of an `FFTOperatorAt`, and conditional simulation, which turns the unconditional
samplers of this package (`GridCovSampler.fields`, the FFTRF samplers) into fields that honour data.  Nothing here has a
counterpart in the reference: its only solver is `lsqr` on a `LowRankCovMatrix`."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import randmatfact as RMF
from . import fftrf as FFTRF
from .context import DeviceMatrix, _Handle

PATHS = {1: "fused", 3: "composed"}


def _diag_arg(diag, n):
    if diag is None:
        return None
    d = np.asarray(diag, dtype=np.float64)
    d = np.full(n, float(d)) if d.ndim == 0 else np.ascontiguousarray(d.reshape(-1))
    if d.shape != (n,):
        raise ValueError(f"diag must be a scalar or hold one entry per row of the operator, {n}")
    return d


class Preconditioner(_Handle):
    """P = Z Z' + diag(d + shift) for the solves of this module (`gsi_precond`): e = 1 / (d + shift)
    and W with P^-1 = diag(e) - W W' resident on the device.  Made by `lowrank_preconditioner`; pass it as `precond=` to
    `solve`, `Operator.solve`, `kriging_weights`, `condition_fields`.  `close()` (or a `with` block) frees it."""

    _destroy = "gsi_precond_destroy"

    def __init__(self, ctx, h, info):
        super().__init__(ctx, h)
        self.rank, self.n = int(info[0]), int(info[1])
        self.info = {"rank": self.rank, "n": self.n, "diag_min": float(info[2]), "diag_max": float(info[3])}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def logdet(self):
        """log det P = sum log(d + shift) + 2 sum log R_kk (`gsi_precond_logdet`), computed when the handle was made."""
        v = C.c_double()
        L.check(self.ctx.lib.gsi_precond_logdet(self.h, C.byref(v)), self.ctx.lib)
        return float(v.value)

    def sample(self, G1, G2):
        """`Z G1 + sqrt(d + shift) .* G2` (`gsi_precond_sample`): with standard normals in `G1` (rank x s) and `G2` (n x s) the
        columns are draws of N(0, P).  Two `DeviceMatrix` give a `DeviceMatrix`, two host arrays a host array."""
        ctx, lib = self.ctx, self.ctx.lib
        if isinstance(G1, DeviceMatrix) and isinstance(G2, DeviceMatrix):
            Z = DeviceMatrix(ctx, *G2.shape)
            try:
                L.check(lib.gsi_precond_sample(ctx.h, self.h, G1.h, G2.h, Z.h), lib)
            except Exception:
                Z.close()
                raise
            return Z
        G1f, G2f = L.fmat(G1, "G1"), L.fmat(G2, "G2")
        if G2f.shape[0] != self.n or G1f.shape != (self.rank, G2f.shape[1]):
            raise ValueError(f"G1 must be {self.rank} x s and G2 {self.n} x s")
        handles = [DeviceMatrix.from_host(ctx, G1f)]
        try:
            handles.append(DeviceMatrix.from_host(ctx, G2f))
            handles.append(self.sample(handles[0], handles[1]))
            return handles[2].to_host()
        finally:
            for h in handles:
                h.close()

    def apply(self, R):
        """`P^-1 R` (`gsi_precond_apply`): a host vector or matrix, or a `DeviceMatrix`; the result is of the same kind."""
        ctx, lib = self.ctx, self.ctx.lib
        if isinstance(R, DeviceMatrix):
            Z = DeviceMatrix(ctx, *R.shape)
            try:
                L.check(lib.gsi_precond_apply(ctx.h, self.h, R.h, Z.h), lib)
            except Exception:
                Z.close()
                raise
            return Z
        Rf = L.fmat(R, "R")
        if Rf.shape[0] != self.n:
            raise ValueError(f"dimension mismatch: the preconditioner has {self.n} rows, R has {Rf.shape[0]}")
        Rd = DeviceMatrix.from_host(ctx, Rf)
        try:
            Z = self.apply(Rd)
            try:
                out = Z.to_host()
            finally:
                Z.close()
        finally:
            Rd.close()
        return out[:, 0].copy() if np.ndim(R) == 1 else out


def lowrank_preconditioner(op, rank=None, basis=None, diag=None, shift=0.0, p=None, q=2, seed=None, *, method="randsvd",
                           tol=0.0):
    """A `Preconditioner` P = Z Z' + diag(diag + shift) for solves with `op` (`gsi_precond_lowrank_create`).  `basis`: a
    `DeviceMatrix` or a host n x K array whose first `rank` columns (all of them by default) are Z; otherwise `rank` runs the
    device randsvd of `op` (`gsi_randsvd_dev`: Z Z' ~ A, oversampling `p` -- min(rank, 64) by default, at most n - rank --
    and `q` power steps, Omega from `gsi_mat_randn` with `seed`) and the basis is dropped once the preconditioner is built.
    `method="pivoted_cholesky"` factors `op` by `RandMatFact.pivoted_cholesky` instead -- no operator product; for dense,
    implicit grid-covariance and implicit point-covariance operators -- to `rank`, or to fewer columns where the trace of
    the remainder has fallen to `tol` times the trace of `op`; `Preconditioner.rank` is the rank that was reached.
    `diag`: None, a scalar or n values, normally the solve's; every diag + shift must be positive."""
    if method not in ("randsvd", "pivoted_cholesky"):
        raise ValueError("method must be 'randsvd' or 'pivoted_cholesky'")
    op, _ = RMF._as_operator(op)
    ctx, lib = op.ctx, op.ctx.lib
    n = op.shape[0]
    d = _diag_arg(diag, n)
    owned = []
    try:
        if basis is None and method == "pivoted_cholesky":
            if rank is None:
                raise ValueError("lowrank_preconditioner needs rank or basis")
            Z, piv, _ = RMF._pivoted_cholesky_dev(op, min(int(rank), n), tol)
            owned.append(Z)
            K = len(piv)
            if K == 0:
                raise ValueError("pivoted_cholesky found rank 0: op has no positive diagonal entry")
        elif basis is not None:
            Z = basis
            if not isinstance(Z, DeviceMatrix):
                Z = DeviceMatrix.from_host(ctx, basis)
                owned.append(Z)
            K = Z.shape[1] if rank is None else int(rank)
        else:
            if rank is None:
                raise ValueError("lowrank_preconditioner needs rank or basis")
            K = int(rank)
            pp = max(0, min(min(K, 64) if p is None else int(p), n - K))
            Om = DeviceMatrix(ctx, n, K + pp)
            owned.append(Om)
            Om.randn(0 if seed is None else int(seed))
            Z = DeviceMatrix(ctx, n, K + pp)
            owned.append(Z)
            L.check(lib.gsi_randsvd_dev(ctx.h, op.h, Om.h, K, pp, int(q), Z.h, None), lib)
        h = C.c_void_p()
        info = (C.c_double * 4)()
        L.check(lib.gsi_precond_lowrank_create(ctx.h, C.byref(h), Z.h, K, L.dptr(d) if d is not None else None, float(shift),
                                               info), lib)
        return Preconditioner(ctx, h, info)
    finally:
        for m in owned:
            m.close()


def solve(op, B, diag=None, tol=1e-10, maxiter=None, strict=True, return_info=False, precond=None):
    """`(A + diag) X = B` for a square, symmetric positive semidefinite operator `op` by conjugate gradients, every column
    of `B` at once (`gsi_op_solve_cg` / `gsi_op_solve`).  `B`: a host vector or matrix, or a `DeviceMatrix`; the result
    is of the same kind.  `diag`: None, a scalar, or n values >= 0.  A column stops when its recurred residual is below
    `tol` times the column's norm; `maxiter` defaults to 10 n.  `strict`: a column that has not converged within
    `maxiter` raises RuntimeError with the counts (otherwise it is only reported).  `return_info`: also a dict with
    `products`, `converged`, `path` ("fused" / "composed"), `breakdown`, `relres` and `iters` per column.  An operator
    that is not positive definite along a search direction raises `GsiError` (GSI_ERR_NOT_POSDEF) naming the column.
    `precond`: a `Preconditioner` -- the preconditioned solver (`gsi_op_solve_pcg` / `gsi_op_solve_pcg_host`) with the
    same stopping rule; the report then also has `breakdown_kind` (1: p'(A + D)p, 2: r'z) and `rank`."""
    op, _ = RMF._as_operator(op)
    ctx, lib = op.ctx, op.ctx.lib
    n = op.shape[0]
    d = _diag_arg(diag, n)
    dp = L.dptr(d) if d is not None else None
    maxiter = 10 * n if maxiter is None else int(maxiter)
    info = (C.c_int64 * (4 if precond is None else 6))()
    if isinstance(B, DeviceMatrix):
        b = B.shape[1]
        relres, iters = np.zeros(b), np.zeros(b, dtype=np.int64)
        X = DeviceMatrix(ctx, B.shape[0], b)
        ip = iters.ctypes.data_as(C.POINTER(C.c_int64))
        if precond is None:
            status = lib.gsi_op_solve_cg(ctx.h, op.h, dp, B.h, X.h, float(tol), maxiter, info, L.dptr(relres), ip)
        else:
            status = lib.gsi_op_solve_pcg(ctx.h, op.h, dp, precond.h, B.h, X.h, float(tol), maxiter, info, L.dptr(relres), ip)
        if status != 0:
            X.close()
        out = X
    else:
        Bf = L.fmat(B, "B")
        b = Bf.shape[1]
        if Bf.shape[0] != n:
            raise ValueError(f"dimension mismatch: operator is {op.shape[0]}x{op.shape[1]}, B has {Bf.shape[0]} rows")
        relres, iters = np.zeros(b), np.zeros(b, dtype=np.int64)
        Xh = np.zeros((n, b), order="F")
        ip = iters.ctypes.data_as(C.POINTER(C.c_int64))
        if precond is None:
            status = lib.gsi_op_solve(ctx.h, op.h, dp, L.dptr(Bf), n, b, L.dptr(Xh), n, float(tol), maxiter, info,
                                      L.dptr(relres), ip)
        else:
            status = lib.gsi_op_solve_pcg_host(ctx.h, op.h, dp, precond.h, L.dptr(Bf), n, b, L.dptr(Xh), n, float(tol), maxiter,
                                               info, L.dptr(relres), ip)
        out = Xh[:, 0] if np.ndim(B) == 1 else Xh
    L.check(status, lib)
    rep = {"products": int(info[0]), "converged": int(info[1]), "path": PATHS.get(int(info[2]), int(info[2])),
           "breakdown": int(info[3]), "relres": relres, "iters": iters, "columns": b}
    if precond is not None:
        rep["breakdown_kind"], rep["rank"] = int(info[4]), int(info[5])
    if strict and rep["converged"] < b:
        if isinstance(out, DeviceMatrix):
            out.close()
        raise RuntimeError(f"conjugate gradients: {b - rep['converged']} of {b} columns did not reach tol = {tol:g} within "
                           f"maxiter = {maxiter} iterations (largest relative residual {np.max(relres):.3e})")
    return (out, rep) if return_info else out


def mat_axpy(alpha, X, Y):
    """`Y += alpha X` for two `DeviceMatrix` of one shape (`gsi_mat_axpy`); returns Y."""
    L.check(Y.ctx.lib.gsi_mat_axpy(Y.ctx.h, float(alpha), X.h, Y.h), Y.ctx.lib)
    return Y


def mat_rowdot_acc(A, B, acc):
    """`acc[i] += sum_c A[i, c] B[i, c]` for two `DeviceMatrix` of one shape and `acc` of rows x 1 (`gsi_mat_rowdot_acc`);
    returns acc.  Every product is rounded on its own and added in ascending c, so the result is a pure function of the
    operands' bits; `B is A` sums the squares and reads each entry once."""
    L.check(acc.ctx.lib.gsi_mat_rowdot_acc(acc.ctx.h, A.h, B.h, acc.h), acc.ctx.lib)
    return acc


def kriging_weights(op, y, noise=None, drift=None, **cg):
    """The weights of (universal) kriging: with M = A + diag(noise) and the drift matrix G (m x p, e.g. [1, x, y]),
    `xi, beta` such that  M xi + G beta = y,  G' xi = 0  -- from ONE solve of the 1 + p columns [y, G]:
    beta = (G' M^-1 G)^-1 G' M^-1 y on the host, xi = M^-1 y - M^-1 G beta.  Without `drift`, xi = M^-1 y and beta is
    empty.  `cg`: `tol`, `maxiter`, `strict`, `precond` of `solve`."""
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    m = yv.size
    if drift is None:
        return solve(op, yv, diag=noise, **cg), np.zeros(0)
    G = np.asarray(drift, dtype=np.float64).reshape(m, -1)
    S = solve(op, np.column_stack([yv, G]), diag=noise, **cg)
    My, MG = S[:, 0], S[:, 1:]
    beta = np.linalg.solve(G.T @ MG, G.T @ My)
    return My - MG @ beta, beta


def _probe_matrix(op, precond, probes, seed):
    """The n x s host matrix of probes z with E[zz'] = P (P = I without a preconditioner)."""
    ctx, n = op.ctx, op.shape[0]
    if isinstance(probes, (int, np.integer)):
        s = int(probes)
        if s < 1:
            raise ValueError("probes must be at least 1")
        handles = [DeviceMatrix(ctx, n, s)]
        try:
            handles[0].randn(int(seed) + 1)
            if precond is None:
                return handles[0].to_host()
            handles.append(DeviceMatrix(ctx, precond.rank, s))
            handles[1].randn(int(seed))
            handles.append(precond.sample(handles[1], handles[0]))
            return handles[2].to_host()
        finally:
            for h in handles:
                h.close()
    Z = probes.to_host() if isinstance(probes, DeviceMatrix) else L.fmat(probes, "probes")
    if Z.shape[0] != n or Z.shape[1] < 1:
        raise ValueError(f"probes must have one row per row of the operator, {n}, and at least one column; got {Z.shape}")
    return Z


def solve_trace(op, B, nquad, diag=None, precond=None, tol=1e-8, maxiter=None, qmax=512):
    """`gsi_op_solve_trace` on a host matrix `B` (n x b): `(A + diag) X = B` as `solve` computes it, and the Gauss rule of
    stochastic Lanczos quadrature for the last `nquad` columns.  Returns X and a dict: what `solve` reports, `quad` and `rho0`
    per column, `truncated` (the columns that went beyond `qmax` iterations)."""
    op, _ = RMF._as_operator(op)
    ctx, lib = op.ctx, op.ctx.lib
    n = op.shape[0]
    d = _diag_arg(diag, n)
    Bf = L.fmat(B, "B")
    b = Bf.shape[1]
    maxiter = 10 * n if maxiter is None else int(maxiter)
    info = (C.c_int64 * 7)()
    relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)
    handles = [DeviceMatrix.from_host(ctx, Bf)]
    try:
        handles.append(DeviceMatrix(ctx, n, b))
        L.check(lib.gsi_op_solve_trace(ctx.h, op.h, L.dptr(d) if d is not None else None, precond.h if precond is not None else None,
                                       handles[0].h, handles[1].h, int(nquad), int(qmax), float(tol), maxiter, info,
                                       L.dptr(relres), iters.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(quad)), lib)
        X = handles[1].to_host()
    finally:
        for h in handles:
            h.close()
    rep = {"products": int(info[0]), "converged": int(info[1]), "path": PATHS.get(int(info[2]), int(info[2])),
           "breakdown": int(info[3]), "breakdown_kind": int(info[4]), "rank": int(info[5]), "truncated": int(info[6]),
           "relres": relres, "iters": iters, "columns": b, "quad": quad[:b].copy(), "rho0": quad[b:].copy()}
    return X, rep


def _slq_report(rep, s, logdet_P):
    q = rep["quad"][-s:]
    return {"values": q, "rho0": rep["rho0"][-s:], "stderr": float(np.std(q, ddof=1) / np.sqrt(s)) if s > 1 else float("nan"),
            "iters": rep["iters"], "relres": rep["relres"], "products": rep["products"], "converged": rep["converged"],
            "truncated": rep["truncated"], "logdet_P": logdet_P, "path": rep["path"], "probes": s}


def logdet(op, diag=None, precond=None, probes=16, seed=0, tol=1e-8, maxiter=None, qmax=512, return_info=False):
    """log det(A + diag) by stochastic Lanczos quadrature from the coefficients of one (preconditioned) multi-column CG run
    on the probes (`gsi_op_solve_trace`): `precond.logdet` + the mean over the probes z of
    (z'P^-1 z) e1' log(T_z) e1.  `probes`: a count -- G1, G2 are drawn by `gsi_mat_randn` with `seed` and `seed + 1` and
    nothing else, so the same seed gives the same normals whatever the parameters of `op` are --, or an n x s host array /
    `DeviceMatrix` of probes with E[zz'] = P (the identity without `precond`).  `qmax`: the coefficients kept per probe.
    `return_info`: also a dict with the per-probe `values` and `rho0`, `stderr` = std / sqrt(s), `iters`, `products`,
    `truncated`, `logdet_P`."""
    op, _ = RMF._as_operator(op)
    Z = _probe_matrix(op, precond, probes, seed)
    s = Z.shape[1]
    _, rep = solve_trace(op, Z, s, diag=diag, precond=precond, tol=tol, maxiter=maxiter, qmax=qmax)
    ldP = precond.logdet if precond is not None else 0.0
    val = ldP + float(np.mean(rep["quad"]))
    return (val, _slq_report(rep, s, ldP)) if return_info else val


def log_likelihood(op, y, noise=None, drift=None, restricted=True, precond=None, probes=16, seed=0, tol=1e-8, maxiter=None,
                   qmax=512, return_info=False):
    """The Gaussian log-likelihood of the data `y` under M = A + diag(noise) with the drift G (m x p) profiled out, from ONE
    traced solve of the columns [y, G, probes]: with r = y - G beta the generalised-least-squares residual (`kriging_weights`)
        ML    -1/2 [r'M^-1 r + log det M + m log 2 pi]
        REML  -1/2 [r'M^-1 r + log det M + log det(G'M^-1 G) + (m - p) log 2 pi]        (`restricted`, the default)
    log det M as `logdet` estimates it; `probes`, `seed`, `tol`, `maxiter`, `qmax`, `precond` as there.  A data column that
    does not reach `tol` raises RuntimeError.  `return_info`: also a dict with `xi`, `beta` (the kriging weights), `quadform`,
    `logdet`, `logdet_GMG` and what `logdet` reports."""
    op, _ = RMF._as_operator(op)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    m = yv.size
    if op.shape[0] != m:
        raise ValueError(f"y must hold one value per row of the operator, {op.shape[0]}")
    G = np.zeros((m, 0)) if drift is None else np.asarray(drift, dtype=np.float64).reshape(m, -1)
    p = G.shape[1]
    Z = _probe_matrix(op, precond, probes, seed)
    s = Z.shape[1]
    X, rep = solve_trace(op, np.column_stack([yv, G, Z]), s, diag=noise, precond=precond, tol=tol, maxiter=maxiter, qmax=qmax)
    val, info, _ = _likelihood_value(yv, G, X, rep, s, precond, restricted, tol, "log_likelihood")
    return (val, info) if return_info else val


def _likelihood_value(yv, G, X, rep, s, precond, restricted, tol, who):
    """The value and the report of `log_likelihood` from the solved columns: X (m x b host array, column-major) needs its
    first 1 + p columns only.  One body for `log_likelihood` and `log_likelihood_grad`: the two values agree bit for bit.  Also
    returns G'M^-1 G (p x p)."""
    m, p = yv.size, G.shape[1]
    if (rep["relres"][:1 + p] > tol).any():
        raise RuntimeError(f"{who}: a data column did not reach tol = {tol:g} (largest relative residual "
                           f"{rep['relres'][:1 + p].max():.3e})")
    My, MG = X[:, 0], X[:, 1:1 + p]
    if p:
        GMG = G.T @ MG
        beta = np.linalg.solve(GMG, G.T @ My)
        xi = My - MG @ beta
        ld_gmg = float(np.linalg.slogdet(0.5 * (GMG + GMG.T))[1])
    else:
        GMG, beta, xi, ld_gmg = np.zeros((0, 0)), np.zeros(0), My, 0.0
    quadform = float((yv - G @ beta) @ xi)
    ldP = precond.logdet if precond is not None else 0.0
    ld = ldP + float(np.mean(rep["quad"][-s:]))
    if restricted:
        val = -0.5 * (quadform + ld + ld_gmg + (m - p) * np.log(2.0 * np.pi))
    else:
        val = -0.5 * (quadform + ld + m * np.log(2.0 * np.pi))
    info = _slq_report(rep, s, ldP)
    info.update({"xi": xi, "beta": beta, "quadform": quadform, "logdet": ld, "logdet_GMG": ld_gmg, "restricted": bool(restricted)})
    return val, info, GMG


def mat_bilinear(L_, Y, R=None, dd=None, g=0):
    """The bilinear reduction of the likelihood gradient on resident matrices (`gsi_mat_bilinear`):
    with V = Y + dd .* R (`dd`: n host values, `R` a `DeviceMatrix`; both None: V = Y), returns `(gram, t)` with
    gram[a, c] = sum_i L[i, a] V[i, c] for a, c < g and t[j - g] = sum_i L[i, j] V[i, j] for g <= j < b.  Every product is
    rounded on its own, chunks of 2048 rows are summed in row order and then added in chunk order: the result is a pure
    function of the operands' bits."""
    ctx, lib = L_.ctx, L_.ctx.lib
    b = L_.shape[1]
    g = int(g)
    d = None if dd is None else np.ascontiguousarray(np.asarray(dd, dtype=np.float64).reshape(-1))
    if d is not None and d.shape != (L_.shape[0],):
        raise ValueError(f"dd must hold one value per row, {L_.shape[0]}")
    gram, t = np.zeros(max(g, 0) ** 2), np.zeros(max(b - g, 0))
    L.check(lib.gsi_mat_bilinear(ctx.h, L_.h, Y.h, R.h if R is not None else None, L.dptr(d) if d is not None else None, g,
                                 L.dptr(gram) if gram.size else None, L.dptr(t) if t.size else None), lib)
    return gram.reshape((g, g), order="F"), t


def op_bilinear_terms(dop, ddiag, X, g, Wz):
    """One parameter's terms of the likelihood gradient (`gsi_op_bilinear_terms`): with dM = `dop` + diag(`ddiag`) (either may
    be None), X the resident solution M^-1 [y, G, Z] and Wz = P^-1 Z resident, returns `(S, t)`: S = X0' dM X0 for the first
    `g` columns X0 and t[i] = x_{g+i}' dM w_i.  R = [X0, Wz] and dop R are formed on the device."""
    ctx, lib = X.ctx, X.ctx.lib
    n, b = X.shape
    g = int(g)
    d = _diag_arg(ddiag, n)
    gram, t = np.zeros(max(g, 0) ** 2), np.zeros(max(b - g, 0))
    L.check(lib.gsi_op_bilinear_terms(ctx.h, dop.h if dop is not None else None, L.dptr(d) if d is not None else None, X.h, g,
                                      Wz.h if Wz is not None else None, L.dptr(gram) if gram.size else None,
                                      L.dptr(t) if t.size else None), lib)
    return gram.reshape((g, g), order="F"), t


def _probe_device(op, precond, probes, seed):
    """`_probe_matrix`'s probes as a `DeviceMatrix` (the same bits), made on the device where `probes` is a count."""
    ctx, n = op.ctx, op.shape[0]
    if isinstance(probes, DeviceMatrix):
        if probes.shape[0] != n or probes.shape[1] < 1:
            raise ValueError(f"probes must have one row per row of the operator, {n}, and at least one column; got {probes.shape}")
        return probes, False
    if isinstance(probes, (int, np.integer)):
        s = int(probes)
        if s < 1:
            raise ValueError("probes must be at least 1")
        G2 = DeviceMatrix(ctx, n, s)
        try:
            G2.randn(int(seed) + 1)
            if precond is None:
                out, G2 = G2, None
                return out, True
            G1 = DeviceMatrix(ctx, precond.rank, s)
            try:
                G1.randn(int(seed))
                return precond.sample(G1, G2), True
            finally:
                G1.close()
        finally:
            if G2 is not None:
                G2.close()
    return DeviceMatrix.from_host(ctx, _probe_matrix(op, precond, probes, seed)), True


def log_likelihood_grad(op, dops, y, noise=None, dnoise=None, drift=None, restricted=True, precond=None, probes=16, seed=0,
                        tol=1e-8, maxiter=None, qmax=512, return_info=False):
    """`log_likelihood` and its gradient with respect to K covariance parameters, from the ONE traced solve the value needs
    (DESIGN.md section 4.6n).  `dops`: a list of K operators dA/dtheta_k (e.g. from `fft_gridcov_derivative` through
    `fft_operator_at` / `linear_data_operator`; an entry None is the zero operator), or None; `dnoise`: a list of K vectors
    d noise / d theta_k (entries None: zero), or None; so d_k M = dops[k] + diag(dnoise[k]).  With X = M^-1 [y, G, Z],
    c = [1; -beta] and W_z = P^-1 Z,
        S_k = X0' (d_k M) X0,    t_ki = x_{1+p+i}' (d_k M) w_i    (E t_ki = tr(M^-1 d_k M)),
        REML  dL/dtheta_k = -1/2 [mean_i t_ki - tr((G'M^-1 G)^-1 S_k[1:, 1:]) - c' S_k c]      (ML: without the middle term).
    The solution X and the probes stay on the device: one `gsi_op_bilinear_terms` call per parameter, of which only
    (1 + p)^2 + s numbers come back.  The value equals `log_likelihood` with the same arguments bit for bit.  Returns
    `(value, grad)`; `return_info`: also a dict with `t` (K x s), `grad_stderr` (K: std(t_k) / (2 sqrt(s)), the standard error of
    grad[k]; `stderr` stays that of the log-determinant), `S` (K matrices) and what `log_likelihood` reports.  One GPU only."""
    op, _ = RMF._as_operator(op)
    ctx, lib = op.ctx, op.ctx.lib
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    m = yv.size
    if op.shape[0] != m:
        raise ValueError(f"y must hold one value per row of the operator, {op.shape[0]}")
    G = np.zeros((m, 0)) if drift is None else np.asarray(drift, dtype=np.float64).reshape(m, -1)
    p = G.shape[1]
    K = max(len(dops) if dops is not None else 0, len(dnoise) if dnoise is not None else 0)
    dops = [None] * K if dops is None else list(dops)
    dnoise = [None] * K if dnoise is None else list(dnoise)
    if len(dops) != K or len(dnoise) != K:
        raise ValueError("dops and dnoise must have one entry per parameter")
    d = _diag_arg(noise, m)
    maxit = 10 * m if maxiter is None else int(maxiter)
    owned = []
    try:
        Zd, mine = _probe_device(op, precond, probes, seed)
        if mine:
            owned.append(Zd)
        s = Zd.shape[1]
        b = 1 + p + s
        B = DeviceMatrix(ctx, m, b)
        owned.append(B)
        head = DeviceMatrix.from_host(ctx, np.column_stack([yv, G]))
        owned.append(head)
        L.check(lib.gsi_mat_copy_cols(ctx.h, B.h, 0, head.h, 0, 1 + p), lib)
        L.check(lib.gsi_mat_copy_cols(ctx.h, B.h, 1 + p, Zd.h, 0, s), lib)
        X = DeviceMatrix(ctx, m, b)
        owned.append(X)
        info7 = (C.c_int64 * 7)()
        relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)
        L.check(lib.gsi_op_solve_trace(ctx.h, op.h, L.dptr(d) if d is not None else None, precond.h if precond is not None else None,
                                       B.h, X.h, s, int(qmax), float(tol), maxit, info7, L.dptr(relres),
                                       iters.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(quad)), lib)
        rep = {"products": int(info7[0]), "converged": int(info7[1]), "path": PATHS.get(int(info7[2]), int(info7[2])),
               "breakdown": int(info7[3]), "breakdown_kind": int(info7[4]), "rank": int(info7[5]), "truncated": int(info7[6]),
               "relres": relres, "iters": iters, "columns": b, "quad": quad[:b].copy(), "rho0": quad[b:].copy()}
        # the 1 + p data and drift columns, into an array laid out as `solve_trace` lays out its whole solution
        Xh = np.empty((m, b), order="F")
        for c in range(1 + p):
            L.check(lib.gsi_mat_download_col(ctx.h, X.h, c, L.dptr(Xh[:, c])), lib)
        val, info, GMG = _likelihood_value(yv, G, Xh, rep, s, precond, restricted, tol, "log_likelihood_grad")
        Wz = Zd
        if precond is not None:
            Wz = precond.apply(Zd)
            owned.append(Wz)
        cvec = np.concatenate([[1.0], -info["beta"]])
        grad, T, S = np.zeros(K), np.zeros((K, s)), []
        for k in range(K):
            Sk, tk = op_bilinear_terms(dops[k], dnoise[k], X, 1 + p, Wz)
            mid = float(np.trace(np.linalg.solve(GMG, Sk[1:, 1:]))) if (restricted and p) else 0.0
            grad[k] = -0.5 * (float(np.mean(tk)) - mid - float(cvec @ Sk @ cvec))
            T[k] = tk
            S.append(Sk)
    finally:
        for h in owned:
            h.close()
    if not return_info:
        return val, grad
    info.update({"t": T, "S": S, "grad_stderr": (np.std(T, axis=1, ddof=1) / (2.0 * np.sqrt(s))) if s > 1 else np.full(K, np.nan)})
    return val, grad, info


COV_PARAMS = ("log_sigma2", "log_ell", "log_ell0", "log_ell1", "log_ell2", "theta", "nugget")


class CovarianceFamily:
    """`covariance_family`'s result: the covariance functions of `fft_gridcov_operator` on one grid, read on the grid, at
    scattered points (`fft_operator_at`) or through a linear forward model (`linear_data_operator`), as a function of the
    parameters.  `params`: a dict with `log_sigma2` (default 0), `log_ell` (all axes) and / or `log_ell0`, `log_ell1`,
    `log_ell2` (added to `log_ell`), `theta` (default 0) and `nugget` (default 0); other keys (`log_noise`) are ignored here.
    Operators made here are the caller's to `release`; the points plan of the first point operator is kept (and with it the
    FFT plan of the grid operator it was made on) and shared by every later one until `close()`."""

    def __init__(self, ctx, Ns, kind, points=None, box=None, model=None):
        if points is not None and model is not None:
            raise ValueError("a family reads the grid at points or through a model, not both")
        self.ctx, self.Ns, self.kind = ctx, tuple(int(v) for v in Ns), kind
        self.points, self.box, self.model = points, box, model
        self._base = None                    # the FFTOperatorAt whose points plan the others share

    def cov_args(self, params):
        d = len(self.Ns)
        le = float(params.get("log_ell", 0.0))
        ell = [float(np.exp(le + float(params.get(f"log_ell{a}", 0.0)))) for a in range(d)]
        return dict(kind=self.kind, ell=ell, theta=float(params.get("theta", 0.0)), sigma2=float(np.exp(params.get("log_sigma2", 0.0))))

    def _wrap(self, gop):
        try:
            if self.points is not None:
                if self._base is None:              # the one operator that plans and uploads the points
                    self._base = FFTRF.fft_operator_at(self.ctx, gop, self.points, box=self.box)
                return FFTRF.fft_operator_at(self.ctx, gop, like=self._base)
            if self.model is not None:
                from .pcga import linear_data_operator
                return linear_data_operator(gop, self.model)
            return gop
        except Exception:
            gop.close()
            raise

    def operator(self, params):
        """The covariance operator at `params`."""
        from .context import fft_gridcov_operator
        return self._wrap(fft_gridcov_operator(self.ctx, self.Ns, nugget=float(params.get("nugget", 0.0)), **self.cov_args(params)))

    def derivatives(self, params, wrt):
        """The operators dA / d wrt[k] at `params`, one per name in `wrt` (`COV_PARAMS`); None for a name that is not a
        covariance parameter (`log_noise`)."""
        from .context import fft_gridcov_derivative
        out = []
        try:
            for name in wrt:
                out.append(self._wrap(fft_gridcov_derivative(self.ctx, self.Ns, name, **self.cov_args(params)))
                           if name in COV_PARAMS else None)
        except Exception:
            for o in out:
                self.release(o)
            raise
        return out

    @staticmethod
    def release(op):
        """Close an operator of `operator` / `derivatives` and the grid operator under it."""
        if op is None:
            return
        gop = getattr(op, "grid_op", None)
        op.close()
        if gop is not None:
            gop.close()

    def close(self):
        if self._base is not None:
            self._base.close()          # (its grid operator was released with the operator that was built beside it)
            self._base = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def covariance_family(ctx, Ns, kind, *, points=None, box=None, model=None):
    """The family of covariance operators `fit_covariance` searches: `fft_gridcov_operator(ctx, Ns, kind, ...)` itself, read
    at `points` (ndims x m, with `box`) by `fft_operator_at`, or seen through `model` (a `LinearForwardModel`) by
    `linear_data_operator`.  See `CovarianceFamily`."""
    return CovarianceFamily(ctx, Ns, kind, points=points, box=box, model=model)


def fit_covariance(family, params0, y, noise, drift=None, wrt=("log_sigma2", "log_ell"), restricted=True, precond=None, probes=16,
                   seed=0, tol=1e-8, maxiter=50, gtol=1e-4, cg_maxiter=None, qmax=512, armijo=1e-4, max_backtracks=20):
    """Maximise the (restricted) log-likelihood of `y` over the parameters named in `wrt` by BFGS on `log_likelihood_grad`
    (DESIGN.md section 4.6n).  `family`: a `CovarianceFamily`; `params0`: its parameter dict at the start (the names not in
    `wrt` stay fixed); `wrt`: names of `COV_PARAMS` and / or "log_noise", which scales the noise vector by exp(log_noise), so
    that its derivative of M is diag(exp(log_noise) noise).  `probes` (a count: drawn once with `seed`; or a matrix), the seed
    and `precond` stay the same at every evaluation, so the objective is one deterministic function.  BFGS in numpy with a
    backtracking Armijo search (first step 1 after the first iteration, 1 / max(1, |g|) at the start).  Stops when
    max|grad| <= `gtol` ("gtol"), after `maxiter` iterations ("maxiter"), or when the search finds no sufficient increase
    within `max_backtracks` halvings ("linesearch").  Returns `(params, report)`: report["stop"], report["trace"] = one dict
    (params, value, grad, stderr) per accepted point, report["evaluations"]."""
    wrt = tuple(wrt)
    for name in wrt:
        if name not in COV_PARAMS and name != "log_noise":
            raise ValueError(f"unknown parameter {name!r}")
    base = dict(params0)
    for name in wrt:
        base.setdefault(name, 0.0)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    nz = _diag_arg(noise, yv.size)
    if nz is None:
        if "log_noise" in wrt:
            raise ValueError("log_noise needs a noise vector")
        nz = np.zeros(yv.size)
    state = {"evals": 0, "probes": probes}

    def evaluate(x):
        prm = dict(base)
        prm.update({name: float(v) for name, v in zip(wrt, x)})
        nv = nz * np.exp(float(prm.get("log_noise", 0.0)))
        op = family.operator(prm)
        dops = []
        try:
            dops = family.derivatives(prm, wrt)
            if isinstance(state["probes"], (int, np.integer)):          # drawn once, then the same matrix at every evaluation
                state["probes"] = _probe_matrix(op, precond, state["probes"], seed)
            dn = [nv if name == "log_noise" else None for name in wrt]
            val, grad, info = log_likelihood_grad(op, dops, yv, noise=nv, dnoise=dn, drift=drift, restricted=restricted,
                                                  precond=precond, probes=state["probes"], seed=seed, tol=tol,
                                                  maxiter=cg_maxiter, qmax=qmax, return_info=True)
        finally:
            for o in dops:
                family.release(o)
            family.release(op)
        state["evals"] += 1
        return prm, val, grad, info["grad_stderr"]

    x0 = np.array([float(base[name]) for name in wrt])
    prm, stop, trace = _bfgs_maximize(evaluate, x0, gtol, maxiter, armijo, max_backtracks)
    return prm, {"stop": stop, "trace": trace, "evaluations": state["evals"], "wrt": wrt}


def _bfgs_maximize(evaluate, x0, gtol=1e-4, maxiter=50, armijo=1e-4, max_backtracks=20):
    """BFGS ascent with a backtracking Armijo search, in numpy.  `evaluate(x)` -> (params, value, grad, stderr); a point where
    it raises `GsiError` or `RuntimeError`, or whose value is not finite, counts as a failed trial step.  Returns (params of
    the last accepted point, "gtol" | "maxiter" | "linesearch", trace of accepted points)."""
    x = np.asarray(x0, dtype=np.float64).copy()
    prm, val, grad, se = evaluate(x)
    trace = [{"params": prm, "value": val, "grad": np.array(grad, dtype=np.float64), "stderr": se}]
    H = np.eye(x.size)
    stop = "maxiter"
    for it in range(int(maxiter)):
        if np.max(np.abs(grad)) <= gtol:
            break
        direction = H @ grad                                   # ascent on the likelihood
        if direction @ grad <= 0.0:
            H = np.eye(x.size)
            direction = np.array(grad, dtype=np.float64)
        step = 1.0 if it > 0 else 1.0 / max(1.0, float(np.linalg.norm(grad)))
        slope = float(direction @ grad)
        found = False
        for _ in range(int(max_backtracks) + 1):
            xn = x + step * direction
            try:
                prm_n, val_n, grad_n, se_n = evaluate(xn)
            except (L.GsiError, RuntimeError):
                step *= 0.5                                    # outside the family's domain, or no convergence there
                continue
            if np.isfinite(val_n) and val_n >= val + armijo * step * slope:
                found = True
                break
            step *= 0.5
        if not found:
            stop = "linesearch"
            break
        sk, yk = xn - x, -(np.asarray(grad_n) - grad)          # BFGS on f = -L
        sy = float(sk @ yk)
        if sy > 1e-12 * float(np.linalg.norm(sk) * np.linalg.norm(yk)):
            rho = 1.0 / sy
            I = np.eye(x.size)
            H = (I - rho * np.outer(sk, yk)) @ H @ (I - rho * np.outer(yk, sk)) + rho * np.outer(sk, sk)
        x, prm, val, grad, se = xn, prm_n, val_n, np.array(grad_n, dtype=np.float64), se_n
        trace.append({"params": prm, "value": val, "grad": grad.copy(), "stderr": se})
    if stop == "maxiter" and np.max(np.abs(grad)) <= gtol:
        stop = "gtol"
    return prm, stop, trace


def _grid_product(at_op, G):
    """C G on the grid of `at_op` for a DeviceMatrix G (n_grid x b): a new DeviceMatrix."""
    ctx = at_op.ctx
    H = DeviceMatrix(ctx, *G.shape)
    try:
        L.check(ctx.lib.gsi_op_mul_dev(ctx.h, at_op.grid_op.h, 0, G.h, H.h), ctx.lib)
    except Exception:
        H.close()
        raise
    return H


def krige_to_grid(at_op, xi, beta=None, drift_grid=None):
    """The kriged field on the grid of an `FFTOperatorAt`: C W' xi (+ drift_grid beta), from `FFTRF.spread` and the grid
    operator's device product.  `xi`: m weights (or m x k); `drift_grid`: n_grid x p, the drift functions at the nodes.
    Returns a host array of n_grid values (or n_grid x k), vec() order."""
    ctx = at_op.ctx
    xv = np.asarray(xi, dtype=np.float64)
    G = FFTRF.spread(ctx, at_op._P, xv.reshape(xv.shape[0], -1), at_op.Ns, box=at_op._B)
    try:
        H = _grid_product(at_op, G)
        try:
            out = H.to_host()
        finally:
            H.close()
    finally:
        G.close()
    if beta is not None and np.size(beta) > 0:
        if drift_grid is None:
            raise ValueError("beta needs drift_grid, the drift functions at the grid nodes")
        out = out + (np.asarray(drift_grid, dtype=np.float64).reshape(out.shape[0], -1) @ np.asarray(beta, dtype=np.float64)
                     ).reshape(out.shape[0], -1)
    return out[:, 0].copy() if xv.ndim == 1 else out


def _prior_adjoint(op, xi):
    """C H' xi for a `LinearDataOperator` and a DeviceMatrix xi (nobs x b): a new DeviceMatrix (n_grid x b)."""
    G = op.model.adjoint(xi)
    try:
        return _grid_product(op, G)
    finally:
        G.close()


def estimate_field(op, xi, beta=None, drift_grid=None):
    """The best estimate on the grid of a `LinearDataOperator` (`linear_data_operator`): X beta + C H' xi, from the model's
    adjoint and the grid operator's device product.  `xi`: nobs weights (or nobs x k); `drift_grid`: n_grid x p, the drift
    functions X at the cells.  Returns a host array of n_grid values (or n_grid x k), vec() order."""
    xv = np.asarray(xi, dtype=np.float64)
    Xi = DeviceMatrix.from_host(op.ctx, L.fmat(xv, "xi"))
    try:
        S = _prior_adjoint(op, Xi)
        try:
            out = S.to_host()
        finally:
            S.close()
    finally:
        Xi.close()
    if beta is not None and np.size(beta) > 0:
        if drift_grid is None:
            raise ValueError("beta needs drift_grid, the drift functions at the grid cells")
        out = out + (np.asarray(drift_grid, dtype=np.float64).reshape(out.shape[0], -1) @ np.asarray(beta, dtype=np.float64)
                     ).reshape(out.shape[0], -1)
    return out[:, 0].copy() if xv.ndim == 1 else out


def _prior_adjoint_any(op, V):
    """C H' V for a `LinearDataOperator` (H the model's matrix) or an `FFTOperatorAt` (H the interpolation W) and a
    DeviceMatrix V (nobs x b): a new DeviceMatrix (n_grid x b)."""
    if hasattr(op, "model"):
        return _prior_adjoint(op, V)
    G = FFTRF.spread(op.ctx, op._P, V, op.Ns, box=op._B)
    try:
        return _grid_product(op, G)
    finally:
        G.close()


def _posterior_finish(c00, acc, U, X, S):
    """v_i = C_00 - acc_i + |Ls^-1 (x_i - u_i)|^2 with S = Ls Ls' (p x p); p = 0: the first two terms."""
    v = c00 - acc
    if X.shape[1]:
        z = np.linalg.solve(np.linalg.cholesky(0.5 * (S + S.T)), (X - U).T)
        v = v + np.sum(z * z, axis=0)
    return v


POSTX_INFO = ("column", "path", "batches", "batch", "adjoint_columns", "trapezoid_bytes")


def posterior_variance_exact(op, noise=None, drift_grid=None, *, method="cholesky", batch=None, precond=None, return_info=False,
                             **cg):
    """The exact posterior (estimation) variance of every grid cell for the data y = H s + v of `op` = H C H', a
    `LinearDataOperator` (`linear_data_operator`) or an `FFTOperatorAt` (H = the interpolation W): with M = H C H' +
    diag(noise), the prior s ~ N(X beta, C), beta unknown, X = `drift_grid` (n_grid x p; None: no drift) and g_i the rows of
    C H',
        v_i = C_ii - g_i' M^-1 g_i + (x_i - Phi' M^-1 g_i)' (Phi' M^-1 Phi)^-1 (x_i - Phi' M^-1 g_i),   Phi = H X
    -- the universal-kriging variance, with no rank-K basis and no sampling.  Returns n_grid host
    values in vec() order; they do not depend on the data.
    `method="cholesky"` (`gsi_op_posterior_variance`, nobs <= 32768): M is formed by nobs products of `op`, factored once on
    the device, and the columns of C H' L^-T are squared and summed row by row in batches of `batch` columns (None: the rule of
    the operator's own products).  `method="cg"`: no dense factor -- per batch J of unit columns E_J the solve
    U_J = M^-1 E_J (`solve` with `precond` and `cg` = `tol`, `maxiter`, `strict`), T_J = C H' U_J, G_J = C H' E_J and
    acc += rowdot(T_J, G_J) (`mat_rowdot_acc`); the drift terms come from one solve of the p columns of Phi.  `precond` and
    `cg` belong to `method="cg"` only.  `return_info`: also a dict -- `path` ("fused": the device kernels, "composed": the host
    path), `batches`, `batch`, `adjoint_columns`, `trapezoid_bytes` and, for "cg", `products` and `iters`."""
    if method not in ("cholesky", "cg"):
        raise ValueError("method must be 'cholesky' or 'cg'")
    if not (hasattr(op, "model") or hasattr(op, "_P")):
        raise TypeError("posterior_variance_exact needs a LinearDataOperator or an FFTOperatorAt")
    ctx, lib = op.ctx, op.ctx.lib
    nobs = op.shape[0]
    n = int(np.prod(op.grid_op.Ns))
    d = _diag_arg(noise, nobs)
    X = np.zeros((n, 0), order="F") if drift_grid is None else L.fmat(np.asarray(drift_grid, dtype=np.float64).reshape(n, -1),
                                                                       "drift_grid")
    p = X.shape[1]
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be at least 1 (None: the operator's own rule)")
    if method == "cholesky":
        if precond is not None or cg:
            raise ValueError("precond and the solver's keywords (tol, maxiter, strict) apply to method='cg' only: "
                             "method='cholesky' runs no iterative solve")
        var = np.zeros(n)
        info = (C.c_int64 * 8)()
        L.check(lib.gsi_op_posterior_variance(ctx.h, op.h, L.dptr(d) if d is not None else None, L.dptr(X) if p else None, n, p,
                                              0 if batch is None else int(batch), L.dptr(var), info), lib)
        rep = {k: int(v) for k, v in zip(POSTX_INFO, info)}
        rep["path"] = PATHS.get(rep["path"], rep["path"])
        rep["method"] = method
        return (var, rep) if return_info else var
    if batch is None:
        bw = max(2, ((2 << 30) // 8) // (2 * max(n, 1)))
        bw += bw & 1
    else:
        bw = int(batch)
    bw = max(1, min(bw, nobs))
    rep = {"method": method, "path": "composed", "batches": 0, "batch": bw, "adjoint_columns": 0, "products": 0, "iters": 0}
    acc = DeviceMatrix.from_host(ctx, np.zeros((n, 1)))
    try:
        for c0 in range(0, nobs, bw):
            b = min(bw, nobs - c0)
            Eh = np.zeros((nobs, b), order="F")
            Eh[np.arange(c0, c0 + b), np.arange(b)] = 1.0
            handles = [DeviceMatrix.from_host(ctx, Eh)]
            try:
                Uj, srep = solve(op, handles[0], diag=d, precond=precond, return_info=True, **cg)
                handles.append(Uj)
                handles.append(_prior_adjoint_any(op, Uj))
                handles.append(_prior_adjoint_any(op, handles[0]))
                mat_rowdot_acc(handles[2], handles[3], acc)
            finally:
                for h in handles:
                    h.close()
            rep["batches"] += 1
            rep["adjoint_columns"] += 2 * b
            rep["products"] += srep["products"]
            rep["iters"] = max(rep["iters"], int(srep["iters"].max()))
        acch = acc.to_host()[:, 0]
    finally:
        acc.close()
    U, S = np.zeros((n, 0)), np.zeros((0, 0))
    if p:
        Phi = op.model.apply_dev(X) if hasattr(op, "model") else FFTRF.interpolate(ctx, op._P, X, op.Ns, box=op._B)
        if isinstance(Phi, DeviceMatrix):
            Pd, Phi = Phi, Phi.to_host()
            Pd.close()
        MPhi, srep = solve(op, Phi, diag=d, precond=precond, return_info=True, **cg)
        rep["products"] += srep["products"]
        S = Phi.T @ MPhi
        Md = DeviceMatrix.from_host(ctx, MPhi)
        try:
            Ud = _prior_adjoint_any(op, Md)
            try:
                U = Ud.to_host()
            finally:
                Ud.close()
        finally:
            Md.close()
        rep["adjoint_columns"] += p
    e0 = np.zeros(n)
    e0[0] = 1.0
    c00 = float(op.grid_op.matmul(e0)[0])
    var = _posterior_finish(c00, acch, U, X, S)
    return (var, rep) if return_info else var


def linear_inversion(grid_op, model, y, noise, drift_grid=None, precond=None, return_info=False, variance=False,
                     variance_method="cholesky", **cg):
    """The exact linear geostatistical inversion of the data `y` = H s + v of a `LinearForwardModel` (identity link), with the
    prior s ~ N(X beta, C), C the covariance of the FFT operator `grid_op`, beta unknown, and v ~ N(0, diag(noise)):
        (H C H' + R) xi + H X beta = y,   (H X)' xi = 0,   s_hat = X beta + C H' xi.
    No rank-K basis, no finite differences, no sampling: the operator is `linear_data_operator(grid_op, model)` and the
    system is solved as `kriging_weights` solves it, by ONE solve of the 1 + p columns [y, H X]; H X is `model.apply_dev` of
    `drift_grid` (n_grid x p, the drift functions at the cells; None: no drift, beta empty).  `precond`: a `Preconditioner`
    built on such an operator; `cg`: `tol`, `maxiter`, `strict` of `solve`.  Returns `s_hat` (n_grid, host), `xi`, `beta`;
    with `return_info` also the report of `solve`.  `variance=True` appends the exact posterior variance of every cell
    (`posterior_variance_exact` with `method=variance_method`; "cg" reuses `precond` and `cg`) to the returned tuple."""
    from .pcga import linear_data_operator
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    if yv.size != model.nobs:
        raise ValueError(f"y must hold one value per observation of the model, {model.nobs}")
    op = linear_data_operator(grid_op, model)
    try:
        X = None if drift_grid is None else L.fmat(np.asarray(drift_grid, dtype=np.float64).reshape(model.n, -1), "drift_grid")
        B = yv[:, None] if X is None else np.column_stack([yv, model.apply_dev(X)])
        S, rep = solve(op, B, diag=noise, precond=precond, return_info=True, **cg)
        My, MG = S[:, 0], S[:, 1:]
        if X is None:
            xi, beta = My.copy(), np.zeros(0)
        else:
            HX = B[:, 1:]
            beta = np.linalg.solve(HX.T @ MG, HX.T @ My)
            xi = My - MG @ beta
        s_hat = estimate_field(op, xi, beta, X)
        out = (s_hat, xi, beta, rep) if return_info else (s_hat, xi, beta)
        if variance:
            kw = dict(precond=precond, **cg) if variance_method == "cg" else {}
            out = out + (posterior_variance_exact(op, noise, X, method=variance_method, **kw),)
    finally:
        op.close()
    return out


def condition_on_linear_data(op, F, y, noise, eps=None, seed=None, **cg):
    """Conditional simulation on the data of a linear forward model, by residual kriging.  `op`: a `LinearDataOperator`
    H C H'; `F`: a `DeviceMatrix` of n_grid x b holding zero-mean unconditional fields with the grid operator's covariance
    C; `y`: the nobs data; `noise`: their error variances D (a scalar or nobs values).  Returns
        F + C H' (H C H' + D)^-1 (y 1' + sqrt(D) .* eps - H F)
    as a new `DeviceMatrix`; `F` is not modified.  `eps`: nobs x b standard normals, given, or drawn by `RandMatFact.randn`
    (after `RandMatFact.seed(seed)` if `seed` is given).  Forward product, solve, adjoint, grid product, axpy -- all on the
    device: only the nobs x b right-hand side crosses the host link, nothing of the grid's size."""
    ctx = op.ctx
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    m, b = yv.size, F.shape[1]
    if op.shape[0] != m:
        raise ValueError(f"y must hold one value per observation of op, {op.shape[0]}")
    d = _diag_arg(noise, m)
    if d is None:
        d = np.zeros(m)
    if eps is None:
        if seed is not None:
            RMF.seed(seed)
        eps = RMF.randn(m, b)
    E = np.asarray(eps, dtype=np.float64).reshape(m, -1)
    if E.shape != (m, b):
        raise ValueError(f"eps must be nobs x b = {m} x {b}")
    handles = []
    try:
        rhs = DeviceMatrix.from_host(ctx, yv[:, None] + np.sqrt(d)[:, None] * E)
        handles.append(rhs)
        HF = op.model.apply_dev(F)
        handles.append(HF)
        mat_axpy(-1.0, HF, rhs)
        xi = solve(op, rhs, diag=d, **cg)
        handles.append(xi)
        out = _prior_adjoint(op, xi)
        try:
            mat_axpy(1.0, F, out)
        except Exception:
            out.close()
            raise
        return out
    finally:
        for h in handles:
            h.close()


def condition_fields(at_op, F, y, noise, eps=None, seed=None, **cg):
    """Conditional simulation by residual kriging.  `F`: a `DeviceMatrix` of n_grid x b holding zero-mean unconditional
    fields with the grid operator's covariance C (e.g. `GridCovSampler.fields` of the same kind, ell and sigma2);
    `y`: the m data at the points of `at_op` = W C W'; `noise`: their error variances D (a scalar or m values).  Returns
        F + C W' (A + D)^-1 (y 1' + sqrt(D) .* eps - W F)
    as a new `DeviceMatrix`; `F` is not modified.  `eps`: m x b standard normals, given, or drawn by `RandMatFact.randn`
    (after `RandMatFact.seed(seed)` if `seed` is given).  Interpolate, solve, spread, grid product, axpy -- all on the
    device: only the m x b right-hand side crosses the host link, nothing of the grid's size."""
    ctx = at_op.ctx
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    m, b = yv.size, F.shape[1]
    if at_op.shape[0] != m:
        raise ValueError(f"y must hold one value per point of at_op, {at_op.shape[0]}")
    d = _diag_arg(noise, m)
    if d is None:
        d = np.zeros(m)
    if eps is None:
        if seed is not None:
            RMF.seed(seed)
        eps = RMF.randn(m, b)
    E = np.asarray(eps, dtype=np.float64).reshape(m, -1)
    if E.shape != (m, b):
        raise ValueError(f"eps must be m x b = {m} x {b}")
    handles = []
    try:
        rhs = DeviceMatrix.from_host(ctx, yv[:, None] + np.sqrt(d)[:, None] * E)
        handles.append(rhs)
        WF = FFTRF.interpolate(ctx, at_op._P, F, at_op.Ns, box=at_op._B)
        handles.append(WF)
        mat_axpy(-1.0, WF, rhs)
        xi = solve(at_op, rhs, diag=d, **cg)
        handles.append(xi)
        G = FFTRF.spread(ctx, at_op._P, xi, at_op.Ns, box=at_op._B)
        handles.append(G)
        out = _grid_product(at_op, G)
        try:
            mat_axpy(1.0, F, out)
        except Exception:
            out.close()
            raise
        return out
    finally:
        for h in handles:
            h.close()
