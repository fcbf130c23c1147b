"""Shared cases of the direct saddle-point solver (gsi_pcgamat_solve, gsi_chol_lower) for
tests/test_saddle_solve_cpu.py (CPU reference library: the host path) and tests/test_saddle_solve_gpu.py (the kernels), with
a scipy restatement of the algebra: cho_factor, two solve_triangular, the Schur scalar.

The bar of the manufactured systems: the relative forward error against x_true is at most BAR = 8 times the larger of two
forward errors on the same system, the restatement's and np.linalg.solve's.  A blocked, differently ordered summation moves a
forward error by a small factor; a lost update or a wrong edge tile is orders of magnitude above it."""
import ctypes as C
import functools

import numpy as np

BAR = 8.0
EXACT_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 200]
# (nobs, K, sigma2, dense R, b[-1])
MANUFACTURED = [(300, 16, 1e-2, False, 0.0), (300, 16, 1e-2, True, 0.0), (300, 16, 1e-8, False, 0.0), (300, 16, 1e-8, True, 0.0),
                (257, 3, 1.0, False, 0.0), (257, 3, 1.0, True, 0.0), (300, 16, 1e-2, False, 0.75)]


def case_id(c):
    return f"nobs{c[0]}-K{c[1]}-s{c[2]:g}-{'dense' if c[3] else 'diag'}" + ("-b2" if c[4] else "")


# ---- exact factors --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_factor(n):
    """(A, L0): L0 integer lower triangular, diagonal from {1, 2, 4}, off-diagonals from {-3 .. 3}; A = L0 L0'.  Every Schur
    complement of A is an integer matrix, every division is by a power of two and every square root is of 1, 4 or 16, so any
    correct Cholesky in fp64 returns L0 bit for bit, whatever its blocking or summation order."""
    rng = np.random.default_rng(1000 + n)
    L0 = np.tril(rng.integers(-3, 4, size=(n, n)).astype(np.float64), -1)
    L0[np.arange(n), np.arange(n)] = rng.choice([1.0, 2.0, 4.0], size=n)
    A = L0 @ L0.T
    assert np.array_equal(A, np.round(A)) and np.abs(A).max() < 2.0 ** 40
    A.setflags(write=False)
    L0.setflags(write=False)
    return A, L0


def failing_matrix(n, j):
    """exact_factor(n)'s A with the pivot of column j (0-based) made exactly -1"""
    A, L0 = exact_factor(n)
    B = A.copy()
    B[j, j] -= L0[j, j] ** 2 + 1.0
    return B


def failure_columns(n):
    return sorted({j for j in (0, 63, 64, 65, n - 1) if 0 <= j < n})


def chol_lower(gsi, ctx, A, lda=None):
    """gsi_chol_lower through the C ABI: (status, L, [column, path], message).  lda > n: A is embedded in a taller array whose
    other rows hold NaN."""
    n = A.shape[0]
    lda = lda or n
    buf = np.full((lda, n), np.nan, order="F")
    buf[:n, :] = A
    Lout = np.full((n, n), np.nan, order="F")
    info = (C.c_int64 * 2)(-7, -7)
    st = ctx.lib.gsi_chol_lower(ctx.h, gsi._lib.dptr(buf), n, lda, gsi._lib.dptr(Lout), info)
    msg = (ctx.lib.gsi_last_error() or b"").decode() if st else ""
    return st, Lout, [int(info[0]), int(info[1])], msg


def dpotrf_info(A):
    import scipy.linalg.lapack as lapack
    return int(lapack.dpotrf(np.asfortranarray(A), lower=1)[1])


# ---- manufactured systems -------------------------------------------------------------------------------------------
def restatement(E, HX, Rdense, b):
    """The algebra of PcgaLowRank::solve with scipy: Cholesky of E E' + R, w = L^-1 HX, v = L^-1 b1,
    beta = (w'v - b2) / (w'w), xi = L^-T (v - beta w)."""
    from scipy.linalg import cho_factor, solve_triangular
    A = E @ E.T + Rdense
    Lf = np.tril(cho_factor(A, lower=True)[0])
    w = solve_triangular(Lf, HX, lower=True)
    v = solve_triangular(Lf, b[:-1], lower=True)
    beta = (w @ v - b[-1]) / (w @ w)
    xi = solve_triangular(Lf, v - beta * w, lower=True, trans="T")
    return np.concatenate([xi, [beta]])


def relerr(x, x_true):
    x_true = np.asarray(x_true, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(x) - x_true) / np.linalg.norm(x_true))


@functools.lru_cache(maxsize=None)
def manufactured(nobs, K, sigma2, dense, b_last, seed=0):
    """E = randn(nobs, K), HX = randn, x_true = randn, b = bigA x_true formed in np.longdouble.  b_last false: x_true's first
    nobs entries are made orthogonal to HX, so b[-1] = 0 as in pcgadirect; b_last true: x_true as drawn, b[-1] = HX'xi != 0."""
    rng = np.random.default_rng(7919 * nobs + 31 * K + seed)
    E = rng.standard_normal((nobs, K))
    HX = rng.standard_normal(nobs)
    x_true = rng.standard_normal(nobs + 1)
    Rdense = sigma2 * np.eye(nobs)
    if dense:                                   # a full SPD R with the same scale: sigma2 (I + G G' / nobs)
        G = rng.standard_normal((nobs, nobs))
        Rdense = sigma2 * (np.eye(nobs) + G @ G.T / nobs)
        Rdense = 0.5 * (Rdense + Rdense.T)
    El, Rl, hl = E.astype(np.longdouble), Rdense.astype(np.longdouble), HX.astype(np.longdouble)

    def big_times(xl):                          # bigA x in long double, by matrix-vector products (E E' is never rounded)
        xi, beta = xl[:nobs], xl[nobs]
        top = El @ (El.T @ xi) + (Rl @ xi if dense else np.longdouble(sigma2) * xi) + hl * beta
        return np.concatenate([top, [hl @ xi]])

    xl = x_true.astype(np.longdouble)
    if not b_last:
        # pcgadirect's right-hand side ends in 0 (direct.jl:56): xi is made orthogonal to HX in long double, so that
        # b[-1] = HX'xi is 0 to long double rounding (1e-19 of |HX||xi|, far below every error compared here)
        xl[:nobs] -= hl * ((hl @ xl[:nobs]) / (hl @ hl))
        x_true = np.asarray(xl, dtype=np.float64)
    b = np.asarray(big_times(xl), dtype=np.float64)
    if not b_last:
        b[-1] = 0.0
    bigd = np.zeros((nobs + 1, nobs + 1))
    bigd[:nobs, :nobs] = E @ E.T + Rdense
    bigd[:nobs, nobs] = bigd[nobs, :nobs] = HX
    refs = (relerr(restatement(E, HX, Rdense, b), x_true), relerr(np.linalg.solve(bigd, b), x_true))
    out = dict(nobs=nobs, K=K, E=E, HX=HX, Rdense=Rdense, R=(Rdense if dense else None), sigma2=sigma2, dense=dense, b=b,
               x_true=x_true, ref_errors=refs, bound=BAR * max(refs))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def make_matrix(gsi, ctx, case):
    """PCGALowRankMatrix of a manufactured case: a scipy sparse diagonal R (stored as its diagonal) or a dense R."""
    import scipy.sparse as sp
    R = case["Rdense"] if case["dense"] else case["sigma2"] * sp.identity(case["nobs"], format="csc")
    etas = [np.ascontiguousarray(case["E"][:, i]) for i in range(case["K"])]
    return gsi.PCGALowRankMatrix(etas, case["HX"], R, ctx=ctx)


def solve_case(gsi, ctx, case):
    A = make_matrix(gsi, ctx, case)
    try:
        x, info = A.solve(case["b"], return_info=True)
    finally:
        A.close()
    return x, info


# ---- end to end -------------------------------------------------------------------------------------------------------
def device_inversion(gsi, ctx):
    """pcgadirect with a DeviceBasis and a LinearForwardModel at n = 4096, K = 16, nobs = 300 (block averages over runs of
    1 .. 200 cells with weights, noise 1e-4, R = 1e-8 I, truth = mean + a combination of six xi): (cholesky, pinv, truth,
    fallbacks of the cholesky run)."""
    import scipy.sparse as sp
    from helpers import gaussian_cov
    rng = np.random.default_rng(4096)
    n, M, p, nobs = 4096, 16, 4, 300
    Qc = gaussian_cov(64, 64, 6.0)
    Om = rng.standard_normal((n, M + p))
    lengths = np.linspace(1, 200, nobs).astype(np.int64)
    starts = np.array([rng.integers(0, n - ln + 1) for ln in lengths], dtype=np.int64)
    indptr = np.zeros(nobs + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lengths)
    indices = np.concatenate([np.arange(a, a + ln) for a, ln in zip(starts, lengths)]).astype(np.int64)
    data = np.concatenate([np.full(ln, 1.0 / ln) for ln in lengths])
    w = 1.0 + 0.1 * rng.standard_normal(n)
    H = sp.csr_matrix((data, indices, indptr), shape=(nobs, n))
    coef = np.concatenate([rng.standard_normal(6), np.zeros(M - 6)])
    basis = gsi.getxis_device(Qc, M, p, 3, Omega=Om, ctx=ctx)
    fwd = gsi.LinearForwardModel(H, weights=w, ctx=ctx)
    try:
        xis = np.stack([basis[i] for i in range(M)], axis=1)
        X = np.full(n, 10.0)
        truth = X + xis @ coef
        y = H @ (w * truth) + 1e-4 * rng.standard_normal(nobs)
        R = 1e-8 * sp.identity(nobs, format="csc")
        before = fwd.info()[7]
        chol = gsi.pcgadirect(fwd, X.copy(), X, basis, R, y, solver="cholesky")
        fallbacks = gsi.pcgadirect.last_fallbacks
        assert fwd.info()[7] > before, "the forward model left the device entry point"
        pinv = gsi.pcgadirect(fwd, X.copy(), X, basis, R, y, solver="pinv")
        return chol, pinv, truth, fallbacks
    finally:
        fwd.close()
        basis.close()


def check_inversion(chol, pinv, truth, fallbacks):
    """Bars of tests/test_gpu_parity.py::test_device_resident_basis_gpu for two correct runs: 1e-3 between them, 2e-2 to the
    truth; and the Cholesky path took no fallback."""
    agree = np.linalg.norm(chol - pinv) / np.linalg.norm(pinv)
    rec = np.linalg.norm(chol - truth) / np.linalg.norm(truth)
    print(f"cholesky vs pinv {agree:.3g}, cholesky vs truth {rec:.3g}, pinv vs truth "
          f"{np.linalg.norm(pinv - truth) / np.linalg.norm(truth):.3g}, fallbacks {fallbacks}")
    assert agree < 1e-3, agree
    assert rec < 2e-2, rec
    assert fallbacks == 0
