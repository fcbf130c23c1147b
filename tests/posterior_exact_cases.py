"""Shared cases and checks of the exact posterior variance (`gsi_op_posterior_variance`, `posterior_variance_exact`,
`gsi_mat_rowdot_acc`) for tests/test_posterior_exact_cpu.py (the CPU reference library: the host path, C a
power-law FFT operator) and tests/test_posterior_exact_gpu.py (the kernels, C a grid covariance function).  Not a test module.

H: `fwd_cov_cases`' rays (40 rays of 64 samples, 20 point samples, a repeated row, an empty row) with its noise 0.01, and
random sparse rows (`sparse_csr`: 1 to 6 cells per row, weights in [0.5, 1.5]) with nobs on both sides of the Cholesky's
64-column blocks.  For the sparse rows and the scattered points the noise is `fair_noise`: the largest eigenvalue of H C H'
over 1000, at least 0.01, so that cond(M) is of order 10^3; tests/test_posterior_exact_cpu.py asserts `fwd_cov_cases.fair` for
every case of both files from the dense matrices.

The bar (`check`): |v - v_ref| <= max(4 x the float64 restatement's own error against the longdouble reference, 1e-12 C_00),
both from tests/posterior_exact_model.py; the references are computed once per case and shared."""
import numpy as np

import fwd_cov_cases as fc
import posterior_exact_model as pm

SPARSE_NOBS = (1, 63, 64, 65, 129, 200)
DRIFTS = ("none", "constant", "linear")
_REFS = {}


def sparse_csr(n, nobs, seed=0):
    """Random rows: 1 to 6 distinct cells each, weights in [0.5, 1.5]; row 0 of nobs == 1 is one point sample of weight 1."""
    rng = np.random.default_rng([n, nobs, seed])
    indptr, indices, data = [0], [], []
    for r in range(nobs):
        k = 1 if nobs == 1 else int(rng.integers(1, 7))
        cells = np.sort(rng.choice(n, size=k, replace=False))
        indices.extend(int(c) for c in cells)
        data.extend([1.0] if nobs == 1 else list(0.5 + rng.random(k)))
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(data)


def dense_of(csr, n):
    indptr, indices, data = csr
    H = np.zeros((len(indptr) - 1, n))
    for r in range(len(indptr) - 1):
        for t in range(indptr[r], indptr[r + 1]):
            H[r, indices[t]] += data[t]
    return H


def fair_noise(A):
    """A scalar noise variance with cond(A + noise I) of order 10^3."""
    lam = float(np.linalg.eigvalsh(0.5 * (A + A.T)).max())
    return max(1e-2, float(f"{lam / 1e3:.2g}"))


def drift(Ns, which):
    """n x p: none (p = 0), constant, or [1, x, y]."""
    Xg = fc.drift_grid(Ns)
    return np.asfortranarray({"none": Xg[:, :0], "constant": Xg[:, :1], "linear": Xg[:, :3]}[which])


def references(key, Cm, H, d, X):
    """(v_ref as float64, the bar) for the dense operands, computed once per key."""
    if key not in _REFS:
        ref = pm.reference(Cm, H, d, X)
        rest = pm.restatement(Cm, H, d, X)
        own = float(np.abs(rest.astype(pm.LD) - ref).max())
        _REFS[key] = (ref.astype(np.float64), max(4.0 * own, 1e-12 * Cm[0, 0]), own)
    return _REFS[key]


def check(key, v, Cm, H, d, X, extra=0.0):
    """|v - v_ref| <= bar (+ extra, per cell); without a drift also v <= C_00 exactly and v >= -bar.  Returns the worst ratio."""
    ref, bar, own = references(key, Cm, H, d, X)
    err = np.abs(v - ref)
    ratio = float((err / (bar + extra)).max())
    print(f"{key}: max|v - v_ref| = {err.max():.3e}, restatement's own error {own:.3e}, bar {bar:.3e}, worst ratio {ratio:.3e}")
    assert v.shape == ref.shape and np.isfinite(v).all()
    assert (err <= bar + extra).all(), (key, ratio)
    if X.shape[1] == 0:
        assert (v <= Cm[0, 0]).all() and (v >= -(bar + extra)).all(), key
    return ratio


def at_dense(Ns, m):
    """(points, box, dense W) of the `FFTOperatorAt` cases: m scattered points in an inner box of the grid."""
    import fftrf_interp_model as im
    import interp_adjoint_model as am
    P = im.scattered_points(Ns, m, seed=19)
    box = im.inner_box(P, shrink=0.05)
    base, frac = im.plan(P, Ns, box)
    return P, box, am.weights_matrix(Ns, base, frac)


def cg_extra(Cm, H, d, tol):
    """The solver's share of the bar of `method="cg"`, per cell: 2 tol |g_i|_1 |g_i|_2 / lambda_min(M), the 2 tol true-residual
    guarantee of every unit column carried through g_i' M^-1 g_i."""
    M = H @ Cm @ H.T + np.diag(d)
    G = Cm @ H.T
    return 2 * tol * np.abs(G).sum(axis=1) * np.linalg.norm(G, axis=1) / np.linalg.eigvalsh(0.5 * (M + M.T)).min()


def full_noise(d, nobs):
    return np.full(nobs, float(d)) if np.ndim(d) == 0 else np.asarray(d, dtype=np.float64)


def refusals(gsi, ctx, op, n, make_ctx, other_op):
    """Every GSI_ERR_ARG of gsi_op_posterior_variance by message, with nothing allocated on the way; `other_op`: an operator
    of another kind on ctx."""
    import ctypes as C
    import solve_cases as sc
    L = gsi._lib
    var = np.zeros(n)
    X = np.ones((n, 1), order="F")

    def raw(cx, o, Xp, ldx, p, batch, diag=None, out=var):
        st = cx.lib.gsi_op_posterior_variance(cx.h, o.h if o is not None else None, L.dptr(diag) if diag is not None else None,
                                              L.dptr(Xp) if Xp is not None else None, ldx, p, batch,
                                              L.dptr(out) if out is not None else None, None)
        if st != 0:
            raise gsi.GsiError(st, cx.lib.gsi_last_error().decode())
    ctx.release_cache()
    before = ctx.device_bytes()
    sc.refused(gsi, lambda: raw(ctx, other_op, None, n, 0, 0), "op must be an operator H C H'")
    sc.refused(gsi, lambda: raw(ctx, op, None, n, -1, 0), "p must be >= 0")
    sc.refused(gsi, lambda: raw(ctx, op, None, n, 1, 0), "X is NULL with p > 0")
    sc.refused(gsi, lambda: raw(ctx, op, X, n - 1, 1, 0), "ldx")
    sc.refused(gsi, lambda: raw(ctx, op, None, n, 0, -1), "batch must be >= 0")
    sc.refused(gsi, lambda: raw(ctx, op, None, n, 0, 0, out=None), "NULL")
    bad = np.full(op.shape[0], np.nan)
    sc.refused(gsi, lambda: raw(ctx, op, None, n, 0, 0, diag=bad), "non-finite")
    other = make_ctx()
    try:
        sc.refused(gsi, lambda: raw(other, op, None, n, 0, 0), "op belongs to another context")
    finally:
        other.close()
    big = 32769                                            # one row beyond the dense factor's limit: one cell per row
    rows = (np.arange(big + 1, dtype=np.int64), np.arange(big, dtype=np.int64) % n, np.ones(big), (big, n))
    bigm = gsi.LinearForwardModel(rows, ctx=ctx)
    bigop = gsi.linear_data_operator(op.grid_op, bigm)
    try:
        held = ctx.device_bytes()
        sc.refused(gsi, lambda: raw(ctx, bigop, None, n, 0, 0), "nobs = 32769")
        assert ctx.device_bytes() == held
    finally:
        bigop.close()
        bigm.close()
    try:
        gsi.posterior_variance_exact(op, 0.1, method="cholesky", tol=1e-8)
    except ValueError as e:
        assert "method='cg' only" in str(e)
    else:
        raise AssertionError("a solver keyword with method='cholesky' was accepted")
    ctx.release_cache()
    assert ctx.device_bytes() == before
