"""Shared cases and numpy models of the log-determinant by stochastic Lanczos quadrature (`gsi_op_solve_trace`,
`gsi_slq_quadrature`, `gsi_precond_sample`, `gsi_precond_logdet`, `logdet`, `log_likelihood`) for
tests/test_op_logdet_cpu.py (the CPU reference library, composed path, the quadrature on the host) and
tests/test_op_logdet_gpu.py (csrc/block_slq.hip).  Not a test module.  Inputs come from tests/solve_cases.py and
tests/pcg_cases.py: dense exponential covariances with `eig_basis` preconditioners.

The models.  `pcg_trace`: the recurrences of cg_state.hpp per column in float64 with alpha_k, beta_k kept.  `gauss_eigh`:
the quadrature of a trace by numpy.linalg.eigh on the tridiagonal.  `ql_f64`: the float64 restatement of slq_state.hpp's
implicit QL on the first row.  `dense_form`: u' log(L^-1 M L^-T) u with P = L L' and u = L^-1 z, from eigh of the dense
matrix -- any factor of P gives the same number, the Lanczos process sees P^-1/2 M P^-1/2 up to an orthogonal change of basis.
"""
import ctypes as C

import numpy as np

import pcg_cases as pg
import solve_cases as sc

LD = np.longdouble
RATIOS = {}


# ---------------------------------------------------------------- the numpy models
def pcg_trace(M, z, pinv, tol, maxiter):
    """alpha, beta (one entry per applied iteration; beta[k] is nan where the column stopped at k), rho0 of one column."""
    bn = np.linalg.norm(z)
    if bn == 0.0:
        return np.zeros(0), np.zeros(0), 0.0
    x, r = np.zeros_like(z), z.copy()
    zz = pinv(r) if pinv is not None else r
    p, rho = zz.copy(), r @ zz
    rho0 = rho
    al, be = [], []
    for _ in range(maxiter):
        w = M @ p
        a = rho / (p @ w)
        x += a * p
        r -= a * w
        al.append(a)
        if np.sqrt(r @ r) <= tol * bn:
            be.append(np.nan)
            break
        zz = pinv(r) if pinv is not None else r
        rz = r @ zz
        be.append(rz / rho)
        p = zz + (rz / rho) * p
        rho = rz
    return np.array(al), np.array(be), float(rho0)


def tridiagonal(al, be, m):
    d = 1.0 / al[:m]
    d[1:] += be[:m - 1] / al[:m - 1]
    e = np.sqrt(be[:m - 1]) / al[:m - 1]
    return d, e


def gauss_eigh(al, be, m, rho0):
    """(value, scale): rho0 sum tau_i^2 log lambda_i and rho0 sum tau_i^2 |log lambda_i| from eigh of T."""
    if m == 0:
        return 0.0, 0.0
    d, e = tridiagonal(al, be, m)
    lam, V = np.linalg.eigh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
    t2 = V[0] ** 2
    return float(rho0 * (t2 @ np.log(lam))), float(rho0 * (t2 @ np.abs(np.log(lam))))


def ql_f64(al, be, m, rho0):
    """slq_state.hpp's quadrature_log restated: the implicit QL of EISPACK's imtql2 with the rotations applied to e1' only."""
    if m == 0:
        return 0.0
    d, e0 = tridiagonal(al, be, m)
    d = [float(v) for v in d]
    e = [float(v) for v in e0] + [0.0]
    z = [1.0] + [0.0] * (m - 1)
    hyp = np.hypot
    for l in range(m):
        sweeps = 0
        while True:
            mm = l
            while mm < m - 1:
                dd = abs(d[mm]) + abs(d[mm + 1])
                if abs(e[mm]) + dd == dd:
                    break
                mm += 1
            if mm == l:
                break
            sweeps += 1
            assert sweeps <= 60
            g = (d[l + 1] - d[l]) / (2.0 * e[l])
            r = float(hyp(g, 1.0))
            g = d[mm] - d[l] + e[l] / (g + (r if g >= 0.0 else -r))
            s = c = 1.0
            p = 0.0
            i = mm - 1
            broke = False
            while i >= l:
                f = s * e[i]
                bb = c * e[i]
                r = float(hyp(f, g))
                e[i + 1] = r
                if r == 0.0:
                    d[i + 1] -= p
                    e[mm] = 0.0
                    broke = True
                    break
                s = f / r
                c = g / r
                g = d[i + 1] - p
                r = (d[i] - g) * s + 2.0 * c * bb
                p = s * r
                d[i + 1] = g + p
                g = c * r - bb
                f = z[i + 1]
                z[i + 1] = s * z[i] + c * f
                z[i] = c * z[i] - s * f
                i -= 1
            if broke:
                continue
            d[l] -= p
            e[l] = g
            e[mm] = 0.0
    acc = 0.0
    for k in range(m):
        acc += z[k] * z[k] * float(np.log(d[k]))
    return rho0 * acc


def chol_ld(P):
    """The lower Cholesky factor of P in np.longdouble."""
    A = np.array(P, dtype=LD)
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for k in range(n):
        Lm[k, k] = np.sqrt(A[k, k] - Lm[k, :k] @ Lm[k, :k])
        if k + 1 < n:
            Lm[k + 1:, k] = (A[k + 1:, k] - Lm[k + 1:, :k] @ Lm[k, :k]) / Lm[k, k]
    return Lm


def logdet_ld(P):
    return float(2.0 * np.log(np.diag(chol_ld(P))).sum())


def precond_factor(Z, K, d, shift, n):
    """L (float64) with L L' = P, the identity without a basis."""
    if Z is None:
        return np.eye(n)
    return chol_ld(pg.dense_P(Z, K, d, shift)).astype(float)


def dense_form(M, Lp, Zp):
    """Per column z of Zp: u' log(Lp^-1 M Lp^-T) u and rho0 = u'u with u = Lp^-1 z."""
    S = np.linalg.solve(Lp, np.linalg.solve(Lp, 0.5 * (M + M.T)).T)
    lam, V = np.linalg.eigh(0.5 * (S + S.T))
    U = np.linalg.solve(Lp, Zp)
    Wt = V.T @ U
    return (Wt ** 2 * np.log(lam)[:, None]).sum(axis=0), (U ** 2).sum(axis=0)


def interleave(cols, qmax):
    """alpha, beta (qmax x b, C order: step k of column j at [k * b + j]), steps, rho0 from a list of (al, be, rho0)."""
    b = len(cols)
    A, Bt = np.zeros((qmax, b)), np.zeros((qmax, b))
    steps, rho0 = np.zeros(b, dtype=np.int64), np.zeros(b)
    for j, (al, be, r0) in enumerate(cols):
        m = min(len(al), qmax)
        A[:m, j] = al[:m]
        Bt[:m, j] = np.nan_to_num(be[:m], nan=0.0)
        steps[j], rho0[j] = m, r0
    return np.ascontiguousarray(A), np.ascontiguousarray(Bt), steps, rho0


def raw_quadrature(ctx, A, Bt, steps, rho0, qmax):
    b = steps.size
    out = np.zeros(b)
    dp = C.POINTER(C.c_double)
    st = ctx.lib.gsi_slq_quadrature(ctx.h, A.ctypes.data_as(dp), Bt.ctypes.data_as(dp), steps.ctypes.data_as(C.POINTER(C.c_int64)),
                                    rho0.ctypes.data_as(dp), int(qmax), int(b), out.ctypes.data_as(dp))
    return st, out


# ---------------------------------------------------------------- 1. the quadrature alone
_TRACES = {}


def long_trace(steps):
    """A numpy PCG trace of at least `steps` iterations (plain CG on the n = 1000 covariance with diag 1e-4 runs to several
    hundred; the shorter ones come from its front: a truncated trace is a valid Lanczos tridiagonal)."""
    if "long" not in _TRACES:
        A = sc.expcov(sc.points(1000, 2, seed=1000))
        M = A + 1e-4 * np.eye(1000)
        z = sc.rhs(1000, 1, seed=5)[:, 0]
        _TRACES["long"] = pcg_trace(M, z, None, 1e-10, 400)
    al, be, r0 = _TRACES["long"]
    assert len(al) >= steps, len(al)
    return al[:steps], be[:steps], r0


def short_trace(seed):
    """A preconditioned trace that converges in a few dozen iterations, a different one per seed."""
    key = ("short", seed)
    if key not in _TRACES:
        n = 257
        A = sc.expcov(sc.points(n, 2, seed=n))
        d = np.full(n, 0.01)
        Z = pg.eig_basis(A, 32)
        z = sc.rhs(n, 1, seed=300 + seed)[:, 0]
        _TRACES[key] = pcg_trace(A + np.diag(d), z, pg.numpy_pinv(Z, 32, d, 0.0), 1e-10, 2570)
    return _TRACES[key]


def quadrature_bar(cols, qmax):
    """Per column: eigh's value, and the bar max(4 x |ql_f64 - eigh|, 1e-13 x scale) -- the scale is rho0 sum tau^2 |log|."""
    ref, bar = [], []
    for al, be, r0 in cols:
        m = min(len(al), qmax)
        v, scale = gauss_eigh(al, be, m, r0)
        ref.append(v)
        bar.append(max(4.0 * abs(ql_f64(al, be, m, r0) - v), 1e-13 * scale))
    return np.array(ref), np.array(bar)


def quadrature_case(ctx, name, cols, qmax):
    A, Bt, steps, rho0 = interleave(cols, qmax)
    st, out = raw_quadrature(ctx, A, Bt, steps, rho0, qmax)
    assert st == 0, ctx.lib.gsi_last_error()
    ref, bar = quadrature_bar(cols, qmax)
    err = np.abs(out - ref)
    ratio = float(np.max(err / np.where(bar > 0, bar, 1.0)))
    print(f"quadrature {name}: b={len(cols)} qmax={qmax} steps {steps.min()}..{steps.max()}, largest error {err.max():.3e}, "
          f"largest ratio to the bar {ratio:.3f}")
    RATIOS[f"quadrature {name}"] = ratio
    assert (err <= bar).all(), (name, ratio)
    return out, steps, rho0


def quadrature_cases(ctx):
    # b = 1, 64, 65 at 49 steps: windows of the long trace (any window of CG coefficients is the L D L' form of a positive
    # definite tridiagonal) and the short traces, which end before 49
    for b in (1, 64, 65):
        cols = []
        al, be, r0 = long_trace(49 + 64)
        for j in range(b):
            cols.append((al[j:j + 49], be[j:j + 49], r0 * (1.0 + j)) if j % 3 != 1 else short_trace(j % 5))
        quadrature_case(ctx, f"49 steps b={b}", cols, 64)
    # steps 1, 2, about 190, and exactly qmax
    one = long_trace(1)
    out, _, _ = quadrature_case(ctx, "1 step", [one], 8)
    want = one[2] * np.log(1.0 / one[0][0])
    assert abs(out[0] - want) <= 2.0 * np.spacing(abs(want)), (out[0], want)
    sh = short_trace(0)
    quadrature_case(ctx, "2 steps", [long_trace(2), (sh[0][:2], sh[1][:2], 3.0)], 4)
    quadrature_case(ctx, "190 steps", [long_trace(190), long_trace(187)], 256)
    quadrature_case(ctx, "exactly qmax", [long_trace(96), long_trace(96)], 96)
    # columns of different lengths, a zero-step column among them
    empty = (np.zeros(0), np.zeros(0), 0.0)
    cols = [long_trace(49), empty, short_trace(1), long_trace(1), long_trace(120), short_trace(2), empty, long_trace(2)]
    out, steps, _ = quadrature_case(ctx, "mixed lengths", cols, 128)
    assert steps[1] == 0 and out[1] == 0.0 and out[6] == 0.0 and not np.signbit(out[1])


# ---------------------------------------------------------------- 2. sampling and logdet_P
def sample_case(gsi, ctx, n, K, b):
    """`Preconditioner.sample` against Z G1 + sqrt(d + shift) G2 in longdouble, and `Preconditioner.logdet` against the
    longdouble Cholesky of the dense P: 4 x the float64 restatement's error, floor 1e-13, as pg.apply_case builds its bar."""
    rng = np.random.default_rng(100 * n + K)
    Z = np.asfortranarray(rng.standard_normal((n, K)))
    d = 0.05 + 0.1 * rng.random(n)
    shift = 0.01
    G1 = np.asfortranarray(rng.standard_normal((K, b)))
    G2 = np.asfortranarray(rng.standard_normal((n, b)))
    dl = (d + shift).astype(LD)
    ref = Z.astype(LD) @ G1.astype(LD) + np.sqrt(dl)[:, None] * G2.astype(LD)
    refn = np.sqrt((ref ** 2).sum(axis=0)).astype(float)
    # the float64 restatement of what the library computes: (W (R G1)) ./ e + G2 ./ sqrt(e)
    e = 1.0 / (d + shift)
    U = np.linalg.cholesky(np.eye(K) + Z.T @ (e[:, None] * Z)).T
    W = np.linalg.solve(U.T, (e[:, None] * Z).T).T
    f64 = (W @ (U @ G1)) / e[:, None] + G2 / np.sqrt(e)[:, None]
    e64 = np.sqrt(((f64.astype(LD) - ref) ** 2).sum(axis=0)).astype(float) / refn
    bar = np.maximum(4.0 * e64, 1e-13)
    ld_ref = logdet_ld(pg.dense_P(Z, K, d, shift))
    ld64 = float(np.log(d + shift).sum() + 2.0 * np.log(np.diag(U)).sum())
    ld_bar = max(4.0 * abs(ld64 - ld_ref), 1e-13 * abs(ld_ref))
    op = gsi.dense_operator(ctx, np.eye(n))
    try:
        pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d, shift=shift)
    finally:
        op.close()
    try:
        got = pc.sample(G1, G2)
        err = np.sqrt(((got.astype(LD) - ref) ** 2).sum(axis=0)).astype(float) / refn
        print(f"sample n={n} K={K} b={b}: error {err.max():.3e}, float64 restatement {e64.max():.3e}, largest ratio "
              f"{(err / bar).max():.3f}; logdet_P {pc.logdet:.15g}, reference {ld_ref:.15g}, bar {ld_bar:.3e}")
        RATIOS[f"sample n={n} K={K} b={b}"] = float((err / bar).max())
        RATIOS[f"logdet_P n={n} K={K}"] = float(abs(pc.logdet - ld_ref) / ld_bar)
        assert (err <= bar).all(), (err / bar).max()
        assert abs(pc.logdet - ld_ref) <= ld_bar, (pc.logdet, ld_ref, ld_bar)
        G1d, G2d = gsi.DeviceMatrix.from_host(ctx, G1), gsi.DeviceMatrix.from_host(ctx, G2)
        Zd = pc.sample(G1d, G2d)
        assert isinstance(Zd, gsi.DeviceMatrix) and np.array_equal(Zd.to_host(), got)
        for h in (Zd, G1d, G2d):
            h.close()
    finally:
        pc.close()


def sample_beyond_grid(gsi, ctx):
    """n = 1024 * 256 + 3: a second trip of the panel pass's row loop, K = 1, against the formula in longdouble."""
    n = 1024 * 256 + 3
    rng = np.random.default_rng(17)
    Z = np.asfortranarray(rng.standard_normal((n, 1)))
    d = 0.05 + 0.1 * rng.random(n)
    G1 = np.array([[0.75, -1.5]])
    G2 = np.asfortranarray(rng.standard_normal((n, 2)))
    Zd = gsi.DeviceMatrix.from_host(ctx, Z)
    h = C.c_void_p()
    try:
        st = ctx.lib.gsi_precond_lowrank_create(ctx.h, C.byref(h), Zd.h, 1, d.ctypes.data_as(C.POINTER(C.c_double)), 0.0, None)
        assert st == 0, ctx.lib.gsi_last_error()
        pc = gsi.Preconditioner(ctx, h, [1, n, d.min(), d.max()])
    finally:
        Zd.close()
    try:
        got = pc.sample(G1, G2)
        ref = Z.astype(LD) @ G1.astype(LD) + np.sqrt(d.astype(LD))[:, None] * G2.astype(LD)
        err = float(np.abs(got.astype(LD) - ref).max() / np.abs(ref).max())
        print(f"sample n={n}: largest error {err:.3e} of the largest entry")
        assert err <= 16 * np.finfo(float).eps          # Z g1: e z / r * r g1 / e, four roundings each way, and the sum
        want = float(np.log(d.astype(LD)).sum() + np.log(LD(1.0) + ((Z[:, 0].astype(LD) ** 2) / d.astype(LD)).sum()))
        assert abs(pc.logdet - want) <= 1e-13 * abs(want), (pc.logdet, want)
    finally:
        pc.close()


# ---------------------------------------------------------------- 3. the trace is passive
def raw_trace(ctx, op, d, pc, Bh, nquad, qmax, tol, maxiter=None):
    """gsi_op_solve_trace on a host B: status, X, info (7), relres, iters, quad (2 b)."""
    import gsi_amd as gsi
    n, b = Bh.shape
    Bd, Xd = gsi.DeviceMatrix.from_host(ctx, Bh), gsi.DeviceMatrix(ctx, n, b)
    info = (C.c_int64 * 7)()
    relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)
    dp = C.POINTER(C.c_double)
    dd = np.ascontiguousarray(d, dtype=np.float64) if d is not None else None
    try:
        st = ctx.lib.gsi_op_solve_trace(ctx.h, op.h, dd.ctypes.data_as(dp) if dd is not None else None,
                                        pc.h if pc is not None else None, Bd.h, Xd.h, int(nquad), int(qmax), float(tol),
                                        int(10 * n if maxiter is None else maxiter), info, relres.ctypes.data_as(dp),
                                        iters.ctypes.data_as(C.POINTER(C.c_int64)), quad.ctypes.data_as(dp))
        X = Xd.to_host()
    finally:
        Bd.close()
        Xd.close()
    return st, X, list(info), relres, iters, quad


def passive_case(gsi, ctx, n, b, diag, K, path):
    """X, relres and iters of the traced solve are those of gsi_op_solve_cg / gsi_op_solve_pcg bit for bit, plain and
    preconditioned, with a zero column and columns that stop at different iterations; a repeat is bit-identical."""
    op, d, A = pg.dense_inputs(gsi, ctx, n, diag)
    pc = gsi.lowrank_preconditioner(op, basis=pg.eig_basis(A, K), diag=d, shift=pg.shift_for(d))
    try:
        B = sc.rhs(n, b, seed=n + b)
        if b > 2:
            B[:, 1] = 0.0
            M = A + (np.diag(d) if d is not None else 0.0)
            B[:, 2] = np.linalg.eigh(M)[1][:, -3:].sum(axis=1)   # three eigenvectors: plain CG stops after three iterations
        for p_ in (None, pc):
            X0, rep0 = op.solve(B, diag=d, tol=sc.TOL, return_info=True, precond=p_)
            assert rep0["path"] == path
            st, X1, info, relres, iters, quad = raw_trace(ctx, op, d, p_, B, min(b, 2), 64, sc.TOL)
            assert st == 0, ctx.lib.gsi_last_error()
            assert np.array_equal(X1, X0.reshape(n, b)) and np.array_equal(relres, rep0["relres"])
            assert np.array_equal(iters, rep0["iters"]) and info[0] == rep0["products"] and info[1] == rep0["converged"]
            assert info[2] == {"fused": 1, "composed": 3}[path] and info[3] == 0
            assert info[5] == (pc.rank if p_ is not None else 0)
            assert info[6] == int((iters > 64).sum())
            assert (quad[:b - min(b, 2)] == 0.0).all() and np.isfinite(quad).all()
            st2, X2, info2, relres2, iters2, quad2 = raw_trace(ctx, op, d, p_, B, min(b, 2), 64, sc.TOL)
            assert st2 == 0 and np.array_equal(X2, X1) and np.array_equal(quad2, quad) and info2 == info
            assert np.array_equal(relres2, relres) and np.array_equal(iters2, iters)
            if b > 2:
                assert iters[1] == 0 and len(set(iters.tolist())) >= (3 if p_ is None else 2), iters
    finally:
        pc.close()
        op.close()


# ---------------------------------------------------------------- 4. per-probe values against the dense matrix
PROBE_CASES = [(64, 0.1, 0), (64, 0.1, 32), (257, 0.01, 0), (257, 0.01, 32), (257, 0.01, 64), (1000, "u", 0), (1000, "u", 64)]


def probe_setup(gsi, ctx, n, diag, K, s=16, seed=0):
    """op, d, pc (or None), M, the factor L of P, explicit probes L g."""
    op, d, A = pg.dense_inputs(gsi, ctx, n, diag)
    M = A + np.diag(d)
    Z = pg.eig_basis(A, K) if K else None
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d) if K else None
    Lp = precond_factor(Z, K, d, 0.0, n)
    Zp = np.asfortranarray(Lp @ sc.rhs(n, s, seed=900 + seed))
    return op, d, pc, M, Z, Lp, Zp


def probe_values(gsi, ctx, n, diag, K, path, s=16, qmax=512):
    """16 explicit probes L_P g at tol 1e-10: each value within max(4 x the numpy restatement's error on that probe, 1e-12)
    rho0 of u' log(L^-1 M L^-T) u."""
    op, d, pc, M, Z, Lp, Zp = probe_setup(gsi, ctx, n, diag, K, s=s)
    try:
        val, info = gsi.logdet(op, diag=d, precond=pc, probes=Zp, tol=1e-10, qmax=qmax, return_info=True)
        assert info["path"] == path and info["truncated"] == 0 and info["converged"] == s, info
        want, rho0 = dense_form(M, Lp, Zp)
        pinv = pg.numpy_pinv(Z, K, d, 0.0) if K else None
        model = np.zeros(s)
        for j in range(s):
            al, be, r0 = pcg_trace(M, Zp[:, j].copy(), pinv, 1e-10, 10 * n)
            model[j] = gauss_eigh(al, be, len(al), r0)[0]
        e_model = np.abs(model - want) / rho0
        bar = np.maximum(4.0 * e_model, 1e-12) * rho0
        err = np.abs(info["values"] - want)
        ratio = float((err / bar).max())
        print(f"probes n={n} diag={diag} K={K} s={s}: iterations {info['iters'].min()}..{info['iters'].max()}, largest error / rho0 "
              f"{(err / rho0).max():.3e}, numpy restatement {e_model.max():.3e}, largest ratio to the bar {ratio:.3f}")
        RATIOS[f"probes n={n} diag={diag} K={K}" + ("" if s == 16 else f" s={s}")] = ratio
        assert np.allclose(info["rho0"], rho0, rtol=1e-10)
        assert (err <= bar).all(), ratio
        ldP = pc.logdet if pc is not None else 0.0
        assert info["logdet_P"] == ldP and val == ldP + float(np.mean(info["values"]))
        assert abs(info["stderr"] - np.std(info["values"], ddof=1) / np.sqrt(s)) <= 1e-12 * abs(info["stderr"])
    finally:
        if pc is not None:
            pc.close()
        op.close()


# ---------------------------------------------------------------- 5. the exact log-determinant
def exact_logdet(gsi, ctx, K, path):
    """n = 48 with the n scaled unit vectors as probes (sqrt(n) e_i, or sqrt(n) L_P e_i): the mean is the trace, the estimate
    is log det M itself, to 1e-11 |slogdet|."""
    n = 48
    op, d, A = pg.dense_inputs(gsi, ctx, n, 0.1)
    M = A + np.diag(d)
    Z = pg.eig_basis(A, K) if K else None
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d) if K else None
    try:
        Lp = precond_factor(Z, K, d, 0.0, n)
        val = gsi.logdet(op, diag=d, precond=pc, probes=np.sqrt(n) * Lp, tol=1e-12, qmax=64)
        want = float(np.linalg.slogdet(M)[1])
        print(f"exact logdet n={n} K={K}: {val:.15g}, slogdet {want:.15g}, difference {abs(val - want):.3e}")
        RATIOS[f"exact logdet K={K}"] = abs(val - want) / (1e-11 * abs(want))
        assert abs(val - want) <= 1e-11 * abs(want)
    finally:
        if pc is not None:
            pc.close()
        op.close()


# ---------------------------------------------------------------- 6. truncation
def truncation(gsi, ctx, path):
    """qmax = 5 on plain CG that needs about 40 iterations: the values are the numpy model's 5-step rule to the bar of
    probe_values (the model is the reference here, so its floor: 1e-12 rho0), info counts the truncated columns, and the
    data columns still converge."""
    n = 257
    op, d, A = pg.dense_inputs(gsi, ctx, n, 0.7)
    M = A + np.diag(d)
    try:
        B = sc.rhs(n, 6, seed=61)
        st, X, info, relres, iters, quad = raw_trace(ctx, op, d, None, B, 4, 5, sc.TOL)
        assert st == 0, ctx.lib.gsi_last_error()
        print(f"truncation: iterations {iters}")
        assert 30 <= iters.min() and iters.max() <= 50 and info[6] == 6 and info[1] == 6
        assert (sc.true_relres(M, X, B) <= 2 * sc.TOL).all()
        cols = [pcg_trace(M, B[:, j].copy(), None, sc.TOL, 10 * n) for j in range(6)]
        ref = np.array([gauss_eigh(al, be, 5, r0)[0] for al, be, r0 in cols])
        bar = 1e-12 * np.array([c[2] for c in cols])             # the bar of probe_values with the model as the reference
        err = np.abs(quad[2:6] - ref[2:])
        print(f"truncation: largest error {err.max():.3e}, bars {bar[2:]}")
        RATIOS["truncation"] = float((err / bar[2:]).max())
        assert (quad[:2] == 0.0).all() and (err <= bar[2:]).all(), err / bar[2:]
        assert np.allclose(quad[6:], [c[2] for c in cols], rtol=1e-13)
    finally:
        op.close()


# ---------------------------------------------------------------- 7. log_likelihood
def dense_likelihood(M, G, y, logdet_M, restricted):
    Ms = 0.5 * (M + M.T)
    m, p = G.shape
    My, MG = np.linalg.solve(Ms, y), np.linalg.solve(Ms, G)
    beta = np.linalg.solve(G.T @ MG, G.T @ My) if p else np.zeros(0)
    xi = My - MG @ beta
    q = float((y - G @ beta) @ xi)
    if restricted:
        return -0.5 * (q + logdet_M + (float(np.linalg.slogdet(G.T @ MG)[1]) if p else 0.0) + (m - p) * np.log(2 * np.pi)), xi, beta
    return -0.5 * (q + logdet_M + m * np.log(2 * np.pi)), xi, beta


def likelihood_case(gsi, ctx, op, P, noise, pc, Lp, name):
    """ML and REML with drift [1, x, y] and explicit probes: the dense formula with log det M replaced by logdet_P + the mean
    of the exact per-probe forms, to 1e-10 relative; xi, beta to kriging_weights' own bar (pg.kriging_drift)."""
    m = P.shape[1]
    rng = np.random.default_rng(12)
    G = np.column_stack([np.ones(m), P[0], P[1]])
    y = G @ np.array([2.0, -1.0, 0.5]) + rng.standard_normal(m)
    d = np.full(m, float(noise))
    M = sc.dense_of(op, d)
    Zp = np.asfortranarray(Lp @ sc.rhs(m, 16, seed=77))
    want_q, _ = dense_form(M, Lp, Zp)
    ldP = pc.logdet if pc is not None else 0.0
    for restricted in (False, True):
        val, info = gsi.log_likelihood(op, y, noise=noise, drift=G, restricted=restricted, precond=pc, probes=Zp, tol=1e-12,
                                       return_info=True)
        want, xi_ref, beta_ref = dense_likelihood(M, G, y, ldP + float(np.mean(want_q)), restricted)
        print(f"{name} restricted={restricted}: {val:.15g}, dense {want:.15g}, relative difference {abs(val - want) / abs(want):.3e}")
        RATIOS[f"{name} restricted={restricted}"] = abs(val - want) / (1e-10 * abs(want))
        assert abs(val - want) <= 1e-10 * abs(want)
        Kd = np.block([[0.5 * (M + M.T), G], [G.T, np.zeros((3, 3))]])
        rhs_ = np.concatenate([y, np.zeros(3)])
        ref = np.linalg.solve(Kd, rhs_)
        z = np.concatenate([info["xi"], info["beta"]])
        Kl = np.block([[M, G], [G.T, np.zeros((3, 3))]]).astype(LD)
        rho = float(np.linalg.norm(rhs_.astype(LD) - Kl @ z.astype(LD)) / np.linalg.norm(rhs_))
        rref = float(np.linalg.norm(rhs_.astype(LD) - Kl @ ref.astype(LD)) / np.linalg.norm(rhs_))
        err = np.linalg.norm(z - ref) / np.linalg.norm(ref)
        assert err <= np.linalg.cond(Kd) * (rho + rref), (err, rho, rref)
    xi, beta = gsi.kriging_weights(op, y, noise=noise, drift=G, tol=1e-12, precond=pc)
    assert np.allclose(info["xi"], xi, rtol=0, atol=1e-9 * np.abs(xi).max()) and np.allclose(info["beta"], beta, rtol=1e-8)


def likelihood_pivchol(gsi, ctx):
    """The same on an implicit point covariance with the basis from the pivoted Cholesky factorization: the factor is a
    function of the entries alone, so a second factorization gives the P the preconditioner was built from."""
    m, K = 150, 16
    P = sc.points(m, 2, seed=21)
    op = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=0.3)
    pc = gsi.lowrank_preconditioner(op, rank=K, diag=0.1, method="pivoted_cholesky")
    try:
        assert pc.rank == K
        Ld, piv = gsi.pivoted_cholesky(op, K)
        Zh = Ld.to_host()
        Ld.close()
        Lp = precond_factor(Zh, K, np.full(m, 0.1), 0.0, m)
        likelihood_case(gsi, ctx, op, P, 0.1, pc, Lp, f"log_likelihood pointcov m={m}, pivoted Cholesky K={K}")
    finally:
        pc.close()
        op.close()


def same_normals(gsi, ctx):
    """Two parameter sets with the same seed use identical normals: the probes of a count are G2 (and Z G1 + sqrt(d) G2 with
    the same G1, G2 under a preconditioner) from gsi_mat_randn(seed + 1) and (seed) alone."""
    n, s = 63, 5
    P = sc.points(n, 2, seed=3)
    G2 = gsi.DeviceMatrix(ctx, n, s)
    G2.randn(8)
    G1 = gsi.DeviceMatrix(ctx, 4, s)
    G1.randn(7)
    g1, g2 = G1.to_host(), G2.to_host()
    G1.close()
    G2.close()
    vals = []
    for ell in (0.2, 0.4):
        A = sc.expcov(P, ell)
        op = gsi.dense_operator(ctx, A)
        Z = pg.eig_basis(A, 4)
        pc = gsi.lowrank_preconditioner(op, basis=Z, diag=0.1)
        try:
            kriging = gsi.Kriging
            assert np.array_equal(kriging._probe_matrix(op, None, s, 7), g2)
            got = kriging._probe_matrix(op, pc, s, 7)
            assert np.array_equal(got, pc.sample(g1, g2))
            assert np.allclose(got, Z @ g1 + np.sqrt(0.1) * g2, rtol=1e-12, atol=1e-12)
            a = gsi.logdet(op, diag=0.1, precond=pc, probes=s, seed=7, tol=1e-10)
            assert a == gsi.logdet(op, diag=0.1, precond=pc, probes=s, seed=7, tol=1e-10)
            vals.append(a)
        finally:
            pc.close()
            op.close()
    assert vals[0] != vals[1]


# ---------------------------------------------------------------- 8. refusals
def refusals(gsi, ctx, path):
    n = 12
    A = sc.expcov(sc.points(n)) + 0.1 * np.eye(n)
    op = gsi.dense_operator(ctx, A)
    op13 = gsi.dense_operator(ctx, np.eye(n + 1))
    pc13 = gsi.lowrank_preconditioner(op13, basis=np.ones((n + 1, 1)), shift=1.0)
    B = sc.rhs(n, 3)
    try:
        def call(**kw):
            a = dict(op=op, pc=None, nquad=2, qmax=8)
            a.update(kw)
            st = raw_trace(ctx, a["op"], None, a["pc"], B, a["nquad"], a["qmax"], sc.TOL)[0]
            if st != 0:
                raise gsi.GsiError(st, ctx.lib.gsi_last_error().decode())
        sc.refused(gsi, lambda: call(qmax=0), "qmax")
        sc.refused(gsi, lambda: call(qmax=4097), "qmax")
        sc.refused(gsi, lambda: call(nquad=4), "nquad")
        sc.refused(gsi, lambda: call(nquad=-1), "nquad")
        sc.refused(gsi, lambda: call(pc=pc13), "pc was built for")
        for q in (0, 4097):
            st, _ = raw_quadrature(ctx, np.ones((1, 1)), np.ones((1, 1)), np.ones(1, dtype=np.int64), np.ones(1), q)
            assert st == 1 and b"qmax" in ctx.lib.gsi_last_error()
        try:
            gsi.logdet(op, probes=np.ones((n + 1, 2)))
        except ValueError as e:
            assert "probes" in str(e)
        else:
            raise AssertionError("probes of the wrong row count must be refused")
        call()                                                  # a following valid call succeeds
    finally:
        pc13.close()
        op13.close()
        op.close()
    # an indefinite operator: GSI_ERR_NOT_POSDEF, naming the column
    rng = np.random.default_rng(6)
    Q, _ = np.linalg.qr(rng.standard_normal((40, 40)))
    lam = np.linspace(1.0, 4.0, 40)
    lam[7] = -1.0
    Mi = (Q * lam) @ Q.T
    opi = gsi.dense_operator(ctx, 0.5 * (Mi + Mi.T))
    try:
        Bi = np.asfortranarray(np.column_stack([Q[:, 3], np.zeros(40), Q[:, 7], Q[:, 11]]))
        st, X, info, relres, iters, quad = raw_trace(ctx, opi, None, None, Bi, 2, 8, sc.TOL, maxiter=100)
        assert st == 7 and b"column 3" in ctx.lib.gsi_last_error(), (st, ctx.lib.gsi_last_error())
        assert info[3] == 3 and (quad == 0.0).all() and np.isfinite(X).all()
        try:
            gsi.logdet(opi, probes=Bi)
        except gsi.GsiError as e:
            assert e.code == 7
        else:
            raise AssertionError("an indefinite operator must raise")
    finally:
        opi.close()
