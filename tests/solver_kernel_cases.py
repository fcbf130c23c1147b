"""Shared cases, references and checks of the solver-side kernels (csrc/misc.hip: gemv_n, gemv_t, project_out, colnorms,
dot_dev, chol_upper, trsm_right_upper, center_rows; csrc/lsqr_dev.hip) for tests/test_solver_kernels_cpu.py (the CPU reference
library) and tests/test_solver_kernels_gpu.py (the HIP library).  Not a test module.  Every check takes `(gsi, ctx)`.

Three public entry points, inputs whose references are exact or well conditioned:

A  `PCGALowRankMatrix.matvec` with integer data in [-3, 3]: five bare gemv calls, every partial sum an integer far below
   2^53, so the result is the same in any summation order and must equal the int64 formula bit for bit.
B  `eig_nystrom` on A = W diag(linspace(1, 4, n)) W' (kappa(Q'AQ) <= 4): U diag(Sigma^2) U' = (A Q)(Q'AQ)^-1 (A Q)' against the
   same product in np.longdouble, in the max norm relative to max |ref|.  Bar: NYSTROM_C j eps kappa_2(Q'AQ).
C  the adaptive `rangefinder(A; epsilon, r)` against the oracle on the same Gaussian stream.  Bar: 100 times the distance
   between the oracle in float64 and the oracle with its products accumulated in np.longdouble, at least 1e-13.
D  `PCGALowRankMatrix.lsqr` on a well-conditioned saddle system: the oracle's iteration count exactly, the iterate within
   100 times the distance between the oracle in float64 and with long-double products and norms (at least 1e-13).

The measured reference errors the bars rest on are printed by tests/test_solver_kernels_cpu.py and recorded in the docstring
of tests/test_solver_kernels_gpu.py.
"""
import functools
import re

import numpy as np

from oracle import oracle as orc
from helpers import exact_rank_matrix

LD = np.longdouble
EPS = np.finfo(np.float64).eps
ERR_ARG, ERR_NOT_POSDEF = 1, 7
MEASURED = {}      # name -> figures behind a bar, printed by the CPU module


def _ld_mm(X, Y):
    """X @ Y accumulated in long double, rounded once to float64."""
    return (np.asarray(X, dtype=LD) @ np.asarray(Y, dtype=LD)).astype(np.float64)


def _ld_norm(x):
    x = np.asarray(x, dtype=LD)
    return float(np.sqrt((x * x).sum()))


# ================================================================ A. PCGALowRankMatrix.matvec, exact
# (nobs, K, dense R): the edge each one crosses is named in tests/test_solver_kernels_gpu.py
MATVEC = [(1, 1, True), (31, 2, True), (255, 3, True), (257, 4, True), (1025, 5, True), (2049, 6, True), (2051, 1030, False),
          (8193, 7, False)]


def matvec_inputs(nobs, K, dense):
    """Integer entries in [-3, 3]; a diagonal R has no zero on its diagonal (the constructor would take it for dense)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(100003 * nobs + K)
    E = rng.integers(-3, 4, size=(nobs, K))
    HX = rng.integers(-3, 4, size=nobs)
    x = rng.integers(-3, 4, size=nobs + 1)
    if dense:
        Ri = rng.integers(-3, 4, size=(nobs, nobs))
        R = Ri.astype(np.float64)
    else:
        d = rng.integers(1, 4, size=nobs) * rng.choice([-1, 1], size=nobs)
        Ri = d
        R = sp.diags(d.astype(np.float64), format="csc")
    return E, HX, Ri, R, x


def matvec_want(E, HX, Ri, x):
    """[(E E' + R) xs + HX x_end; HX' xs] in int64; the largest partial sum of any order is below the asserted 2^50."""
    E, HX, Ri, x = (np.asarray(a, dtype=np.int64) for a in (E, HX, Ri, x))
    xs = x[:-1]
    t = E.T @ xs
    Rx = Ri @ xs if Ri.ndim == 2 else Ri * xs
    want = np.concatenate([E @ t + Rx + HX * x[-1], [HX @ xs]])
    # the sum of the absolute values of every term that enters any entry bounds every partial sum in any order
    aE, ax = np.abs(E), np.abs(xs)
    bound = aE @ (aE.T @ ax) + (np.abs(Ri) @ ax if Ri.ndim == 2 else np.abs(Ri) * ax) + np.abs(HX) * abs(x[-1])
    assert max(int(bound.max()), int(np.abs(HX) @ ax), int(np.abs(want).max())) < 2 ** 50
    return want


def _matvec_equal(gsi, ctx, E, HX, Ri, R, x):
    want = matvec_want(E, HX, Ri, x)
    A = gsi.PCGALowRankMatrix([E[:, i].astype(np.float64) for i in range(E.shape[1])], HX.astype(np.float64), R, ctx=ctx)
    try:
        got = A.matvec(x.astype(np.float64))
    finally:
        A.close()
    bad = np.flatnonzero(got != want.astype(np.float64))
    assert np.array_equal(got, want.astype(np.float64)), (bad[:8], got[bad[:8]], want[bad[:8]])


def check_matvec(gsi, ctx, nobs, K, dense):
    _matvec_equal(gsi, ctx, *matvec_inputs(nobs, K, dense))


def check_matvec_planted(gsi, ctx):
    """nobs = 1025, dense R with ones in column 1024 only, x = e_1024: y = [ones(nobs); 0].  The one element of the second x
    chunk reaches every row exactly once; a dropped or doubled element gives 0 or 2, which no sum of other terms hides (the
    etas and HX are integers with a zero row 1024, so they contribute exact zeros)."""
    nobs, K = 1025, 5
    rng = np.random.default_rng(11)
    E = rng.integers(-3, 4, size=(nobs, K))
    HX = rng.integers(-3, 4, size=nobs)
    E[1024, :] = 0
    HX[1024] = 0
    Ri = np.zeros((nobs, nobs), dtype=np.int64)
    Ri[:, 1024] = 1
    x = np.zeros(nobs + 1, dtype=np.int64)
    x[1024] = 1
    want = matvec_want(E, HX, Ri, x)
    assert np.array_equal(want, np.concatenate([np.ones(nobs, dtype=np.int64), [0]]))
    _matvec_equal(gsi, ctx, E, HX, Ri, Ri.astype(np.float64), x)


# ================================================================ B. eig_nystrom
NYSTROM = [(40, 1), (40, 2), (300, 17), (600, 256), (600, 257), (600, 258), (700, 300)]
# bar = NYSTROM_C j eps kappa_2(B2).  test_solver_kernels_cpu.py asserts LAPACK and the CPU library within a quarter of it on
# every case of the table: at j = 1 the CPU library's 3.7 eps (40-term inner products, not j, set the error there) needs
# c >= 14.7, at j = 2 LAPACK's 6.3 eps needs c >= 10.2; 16 is the next power of two.
NYSTROM_C = 16.0


def nystrom_bar(j, kappa):
    return NYSTROM_C * j * EPS * kappa


@functools.lru_cache(maxsize=None)
def nystrom_inputs(n, j):
    rng = np.random.default_rng(7000 + 31 * n + j)
    W, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (W * np.linspace(1.0, 4.0, n)) @ W.T
    A = np.asfortranarray(0.5 * (A + A.T))
    Q, _ = np.linalg.qr(rng.standard_normal((n, j)))
    A.setflags(write=False)
    Q.setflags(write=False)
    return A, Q


def _ld_chol_upper(B):
    """The upper Cholesky factor of the symmetric long-double B, by columns."""
    j = B.shape[0]
    U = np.zeros((j, j), dtype=LD)
    for k in range(j):
        d = B[k, k] - (U[:k, k] * U[:k, k]).sum()
        assert d > 0
        U[k, k] = np.sqrt(d)
        if k + 1 < j:
            U[k, k + 1:] = (B[k, k + 1:] - U[:k, k] @ U[:k, k + 1:]) / U[k, k]
    return U


def _ld_solve_right_upper(F, U):
    """F U^-1 in long double."""
    X = np.zeros_like(F)
    for c in range(U.shape[0]):
        X[:, c] = (F[:, c] - X[:, :c] @ U[:c, c]) / U[c, c]
    return X


@functools.lru_cache(maxsize=None)
def nystrom_reference(n, j):
    """(F F' in long double rounded to float64, kappa_2(B2), Sigma of orc.eig_nystrom, max-norm error of orc.eig_nystrom)."""
    A, Q = nystrom_inputs(n, j)
    B1 = A.astype(LD) @ Q.astype(LD)
    B2 = Q.astype(LD).T @ B1
    B2 = np.triu(B2) + np.triu(B2, 1).T                     # Hermitian(B2) reads the upper triangle
    F = _ld_solve_right_upper(B1, _ld_chol_upper(B2))
    ref = (F @ F.T).astype(np.float64)
    ref.setflags(write=False)
    kappa = float(np.linalg.cond(B2.astype(np.float64)))
    Uo, So = orc.eig_nystrom(A, Q)
    err_lapack = float(np.abs((Uo * So ** 2) @ Uo.T - ref).max() / np.abs(ref).max())
    MEASURED[f"nystrom n={n} j={j}"] = {"kappa": kappa, "bar": nystrom_bar(j, kappa), "lapack": err_lapack}
    return ref, kappa, So, err_lapack


def nystrom_error(U, S, ref):
    return float(np.abs((U * S ** 2) @ U.T - ref).max() / np.abs(ref).max())


def check_nystrom(gsi, ctx, n, j, name="library"):
    A, Q = nystrom_inputs(n, j)
    ref, kappa, So, err_lapack = nystrom_reference(n, j)
    U, S = gsi.eig_nystrom(A, Q, ctx=ctx)
    assert U.shape == (n, j) and S.shape == (j,) and np.isfinite(U).all() and np.isfinite(S).all()
    err = nystrom_error(U, S, ref)
    serr = float(np.abs(S - So).max() / So[0])
    bar = nystrom_bar(j, kappa)
    MEASURED[f"nystrom n={n} j={j}"][name] = err
    print(f"eig_nystrom n={n} j={j}: kappa(B2) {kappa:.3f}, bar {bar:.3e}, LAPACK {err_lapack:.3e}, {name} {err:.3e}, "
          f"Sigma {serr:.3e}")
    assert err <= bar, (n, j, err, bar)
    assert serr <= bar, (n, j, serr, bar)
    return err


# ---- beyond one sweep of the 4096-workgroup grids: a LowRankCovMatrix operator
BIG_N, BIG_SAMPLES, BIG_J = 1048576 + 3, 4, 2


BIG_STRIDE = 257


@functools.lru_cache(maxsize=None)
def nystrom_big_inputs():
    """N = 4 integer fields (sums, means -- multiples of 1/4 -- and centred values are exact in any order), sample i scaled by
    i + 1 so that the two singular values of F are well apart, and an orthonormal n x 2 Q.

    The fields are non-zero on every 257th row (257 is prime to the 256 lanes: every lane, 4080 of the 4096 workgroups) and on
    the three rows 2^20 .. 2^20 + 2 that only the second trip of a 4096 x 256 grid reaches.  The bar has no n in it and is
    relative to max |ref|; with all 2^20 rows non-zero every entry of U is ~1e-3 and carries the accumulation error of
    million-term inner products (measured on the CPU library: Sigma 1e-13, U diag(Sigma) 8e-11 at row 0, where its Householder
    QR leaves an absolute eps), which says nothing about a loop edge.  With 4084 non-zero rows those sums are short, the rows
    between must come back as exact zeros, and a row that a grid-stride loop skips, repeats or shifts still shows."""
    rng = np.random.default_rng(2024)
    S = np.zeros((BIG_SAMPLES, BIG_N))
    rows = np.concatenate([np.arange(0, 1 << 20, BIG_STRIDE), np.arange(1 << 20, BIG_N)])
    S[:, rows] = rng.integers(-4, 5, size=(BIG_SAMPLES, rows.size)) * np.arange(1.0, BIG_SAMPLES + 1.0)[:, None]
    Q, _ = np.linalg.qr(rng.standard_normal((BIG_N, BIG_J)))
    return S, np.asfortranarray(Q)


@functools.lru_cache(maxsize=None)
def nystrom_big_reference():
    """(F_ref V, Sigma, kappa_2(B2)) from the centred samples on the host, through the 2 x 2 F_ref'F_ref."""
    S, Q = nystrom_big_inputs()
    Sc = (S - S.mean(axis=0)[None, :]).astype(LD)            # exact
    T = Sc @ Q.astype(LD)                                    # N x j
    B1 = (Sc.T @ T) / LD(BIG_SAMPLES - 1)                    # A Q, n x j
    B2 = Q.astype(LD).T @ B1
    B2 = np.triu(B2) + np.triu(B2, 1).T
    F = _ld_solve_right_upper(B1, _ld_chol_upper(B2))
    G = (F.T @ F).astype(np.float64)
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1], V[:, ::-1]
    return (F @ V.astype(LD)).astype(np.float64), np.sqrt(lam), float(np.linalg.cond(B2.astype(np.float64))), lam


def check_nystrom_big(gsi, ctx):
    S, Q = nystrom_big_inputs()
    FV, Sref, kappa, lam = nystrom_big_reference()
    bar = nystrom_bar(BIG_J, kappa)
    lr = gsi.LowRankCovMatrix(S, ctx=ctx)
    try:
        U, Sig = gsi.eig_nystrom(lr, Q, ctx=ctx)
    finally:
        lr.close()
    serr = float(np.abs(Sig - Sref).max() / Sref[0])
    US = U * Sig
    US = US * np.sign((US * FV).sum(axis=0))[None, :]        # singular vectors up to sign
    # the singular vectors answer a perturbation delta of F'F with a rotation of delta / gap: the gap is asserted below
    gap = float((lam[0] - lam[1]) / lam[0])
    err = float(np.abs(US - FV).max() / np.abs(FV).max())
    print(f"eig_nystrom lowrank n={BIG_N} j={BIG_J}: kappa(B2) {kappa:.3f}, relative gap of Sigma^2 {gap:.3f}, bar {bar:.3e}, "
          f"Sigma {serr:.3e}, U diag(Sigma) {err:.3e}")
    MEASURED[f"nystrom lowrank n={BIG_N}"] = {"kappa": kappa, "gap": gap, "bar": bar, "sigma": serr, "usigma": err}
    assert gap >= 0.25, gap                                  # a condition on the inputs: the two directions are well separated
    assert serr <= bar and err <= bar, (serr, err, bar)


def check_nystrom_not_posdef(gsi, ctx):
    A = np.diag([1.0, 1.0, -1.0, 1.0, 1.0])
    Q = np.asfortranarray(np.eye(5)[:, :4])
    try:
        gsi.eig_nystrom(A, Q, ctx=ctx)
    except gsi.GsiError as e:
        assert e.code == ERR_NOT_POSDEF, (e.code, str(e))
        assert "not positive definite" in str(e) and re.search(r"\b3\b", str(e).split("PosDefException")[-1]), str(e)
    else:
        raise AssertionError("an indefinite Q'AQ must raise")
    check_nystrom(gsi, ctx, 40, 2, name="after the refusal")  # the flag was cleared: the next call succeeds and meets the bar


# ================================================================ C. adaptive rangefinder
RANGEFINDER = [(1100, 9, 10), (1030, 70, 64), (300, 5, 1), (300, 5, 2)]
STREAM_SEED = 77


def rangefinder_hooked(A, randn, mm, norm, epsilon=1e-8, r=10):
    """orc.rangefinder_adaptive with its products (`mm`) and its norm replaceable: with `np.matmul` and `np.linalg.norm` it
    is that routine operation for operation (test_solver_kernels_cpu.py asserts equal bits)."""
    m, n = A.shape
    kmax = min(n, m)
    Yfull = np.zeros((n, r + kmax))
    Yfull[:m, :r] = mm(A, randn((n, r)))
    Qfull = np.zeros((m, kmax))
    j = 0
    thresh = epsilon / np.sqrt(200.0 / np.pi)
    while orc.colnorms(Yfull[:, j:j + r]).max() > thresh:
        if j >= kmax:
            break
        j += 1
        Yj = Yfull[:m, j - 1].copy()
        Q = Qfull[:, :j - 1]
        Yj = Yj - mm(Q, mm(Q.T, Yj))
        Qfull[:, j - 1] += Yj / norm(Yj)
        Q = Qfull[:, :j]
        Aomega = mm(A, randn((n,)))
        Yfull[:m, r + j - 1] = Aomega - mm(Q, mm(Q.T, Aomega))
        Qj = Qfull[:, j - 1]
        for i in range(j + 1, j + r):
            Yi = Yfull[:m, i - 1]
            Yi -= mm(Qj, Yi) * Qj
    return Qfull[:, :j].copy()


def _stream():
    rng = np.random.default_rng(STREAM_SEED)
    return lambda shape: rng.standard_normal(int(np.prod(shape))).reshape(shape, order="F")


@functools.lru_cache(maxsize=None)
def rangefinder_reference(n, m, r):
    """(A, the oracle's Q, the bar: 100 |Q - Q with long-double products| over columns [: m - 1], at least 1e-13)."""
    A = exact_rank_matrix(np.random.default_rng(5 * n + m), n, m)
    Qref = orc.rangefinder_adaptive(A, _stream(), r=r)
    Qld = rangefinder_hooked(A, _stream(), _ld_mm, _ld_norm, r=r)
    assert Qld.shape == Qref.shape
    diff = float(np.abs(Qref[:, :m - 1] - Qld[:, :m - 1]).max())
    bar = max(100.0 * diff, 1e-13)
    MEASURED[f"rangefinder n={n} m={m} r={r}"] = {"float64_vs_longdouble": diff, "bar": bar, "columns": Qref.shape[1]}
    A.setflags(write=False)
    Qref.setflags(write=False)
    return A, Qref, bar


def check_rangefinder(gsi, ctx, n, m, r, name="library"):
    A, Qref, bar = rangefinder_reference(n, m, r)
    gsi.RandMatFact.seed(STREAM_SEED)
    Q = gsi.rangefinder(A, r=r, ctx=ctx)
    assert Q.shape == Qref.shape, (Q.shape, Qref.shape)
    res = float(np.linalg.norm(A - Q @ (Q.T @ A)))
    err = float(np.abs(Q[:, :m - 1] - Qref[:, :m - 1]).max())
    MEASURED[f"rangefinder n={n} m={m} r={r}"][name] = err
    print(f"rangefinder n={n} m={m} r={r}: {Q.shape[1]} columns, |A - QQ'A| {res:.3e}, columns vs oracle {err:.3e}, bar {bar:.3e}")
    assert res < 1e-8, res
    assert err <= bar, (err, bar)


def check_rangefinder_refuses_r65(gsi, ctx):
    A, _, _ = rangefinder_reference(300, 5, 1)
    try:
        gsi.rangefinder(A, r=65, ctx=ctx)
    except gsi.GsiError as e:
        assert e.code == ERR_ARG and "r <= 64" in str(e), str(e)
    else:
        raise AssertionError("r = 65 must be refused")


# ================================================================ D. PCGALowRankMatrix.lsqr
LSQR = [(300, 4), (32768, 3), (65539, 3)]
# At nobs = 300 the Krylov space is nearly exhausted when the stopping rule fires (R has three distinct values, K + 1 = 5 more
# directions), and how much rounding the last iterations amplify depends on the draw: over seeds 0 .. 7 the oracle in float64
# and with long-double accumulation differ by 4e-15 .. 4e-12.  Seed 1 is the draw with the smallest difference, so the tightest bar.
LSQR_SEED = {300: 1}


def lsqr_hooked(matvec, b, ncols, norm):
    """orc.lsqr for a symmetric operator with IterativeSolvers' defaults (damp = 0) and a replaceable norm: with
    `np.linalg.norm` it is that routine operation for operation (test_solver_kernels_cpu.py asserts equal bits)."""
    b = np.asarray(b, dtype=np.float64)
    tol = np.sqrt(EPS)
    maxiter = max(b.shape[0], ncols)
    x = np.zeros(ncols)
    u = b.copy()
    beta = norm(u)
    u /= beta
    v = matvec(u)
    alpha = norm(v)
    v = v / alpha
    w = v.copy()
    rhobar, phibar, bnorm = alpha, beta, beta
    Anorm = ddnorm = xxnorm = z = 0.0
    cs2, sn2 = -1.0, 0.0
    it = 0
    while it < maxiter:
        it += 1
        u = matvec(v) - alpha * u
        beta = norm(u)
        if beta > 0:
            u /= beta
            Anorm = np.sqrt(Anorm ** 2 + alpha ** 2 + beta ** 2)
            v = matvec(u) - beta * v
            alpha = norm(v)
            if alpha > 0:
                v /= alpha
        rho = np.sqrt(rhobar ** 2 + beta ** 2)
        cs, sn = rhobar / rho, beta / rho
        theta = sn * alpha
        rhobar = -cs * alpha
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1, t2 = phi / rho, -theta / rho
        ddnorm += (norm(w) / rho) ** 2
        x = x + t1 * w
        w = v + t2 * w
        delta, gambar = sn2 * rho, -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = np.sqrt(xxnorm + zbar ** 2)
        gamma = np.sqrt(gambar ** 2 + theta ** 2)
        cs2, sn2 = gambar / gamma, theta / gamma
        z = rhs / gamma
        xxnorm += z ** 2
        Acond = Anorm * np.sqrt(ddnorm)
        rnorm = np.sqrt(phibar ** 2)
        Arnorm = alpha * abs(tau)
        test1 = rnorm / bnorm
        test2 = Arnorm / (Anorm * rnorm) if Anorm * rnorm > 0 else 0.0
        test3 = 1.0 / Acond if Acond > 0 else 0.0
        t1c = test1 / (1.0 + Anorm * xnorm / bnorm)
        rtol = tol + tol * Anorm * xnorm / bnorm
        if (1 + test3 <= 1) or (1 + test2 <= 1) or (1 + t1c <= 1):
            break
        if test3 <= 1e-8 or test2 <= tol or test1 <= rtol:
            break
    return x, it


def lsqr_inputs(nobs, K):
    """R = diag(1 + (i mod 3) / 4), etas and HX integers in [-2, 2] over sqrt(nobs), b = [integers in [-3, 3]; 0]."""
    import scipy.sparse as sp
    rng = np.random.default_rng(LSQR_SEED.get(nobs, 500 + nobs + K))
    s = 1.0 / np.sqrt(nobs)
    E = rng.integers(-2, 3, size=(nobs, K)) * s
    HX = rng.integers(-2, 3, size=nobs) * s
    d = 1.0 + 0.25 * (np.arange(nobs) % 3)
    b = np.concatenate([rng.integers(-3, 4, size=nobs).astype(np.float64), [0.0]])
    return E, HX, d, sp.diags(d, format="csc"), b


def _ld_saddle_matvec(E, HX, d):
    El, Hl, dl = E.astype(LD), HX.astype(LD), d.astype(LD)

    def mv(x):
        xl = np.asarray(x, dtype=LD)
        xs = xl[:-1]
        top = dl * xs + El @ (El.T @ xs) + Hl * xl[-1]
        return np.concatenate([top, [Hl @ xs]]).astype(np.float64)
    return mv


@functools.lru_cache(maxsize=None)
def lsqr_reference(nobs, K):
    """(x of orc.lsqr, its iteration count, its true residual, the bar: 100 |x - x with long-double products and norms| /
    |x|, at least 1e-13)."""
    E, HX, d, R, b = lsqr_inputs(nobs, K)
    ref = orc.PCGALowRankMatrix([E[:, i] for i in range(K)], HX, R)
    x, it = orc.lsqr(ref.matvec, ref.matvec, b, nobs + 1)
    mv = _ld_saddle_matvec(E, HX, d)
    xl, itl = lsqr_hooked(mv, b, nobs + 1, _ld_norm)
    assert itl == it, (itl, it)
    diff = float(np.linalg.norm(x - xl) / np.linalg.norm(x))
    bar = max(100.0 * diff, 1e-13)
    res = _ld_norm(mv(x) - b)
    MEASURED[f"lsqr nobs={nobs} K={K}"] = {"float64_vs_longdouble": diff, "bar": bar, "iterations": it,
                                           "oracle_residual_over_b": res / float(np.linalg.norm(b))}
    x.setflags(write=False)
    return x, it, res, bar


def lsqr_run(gsi, ctx, nobs, K):
    E, HX, d, R, b = lsqr_inputs(nobs, K)
    A = gsi.PCGALowRankMatrix([E[:, i] for i in range(K)], HX, R, ctx=ctx)
    try:
        return A.lsqr(b, return_iterations=True)
    finally:
        A.close()


def check_lsqr(gsi, ctx, nobs, K, name="library"):
    xr, itr, resr, bar = lsqr_reference(nobs, K)
    E, HX, d, R, b = lsqr_inputs(nobs, K)
    x, it = lsqr_run(gsi, ctx, nobs, K)
    err = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    res = _ld_norm(_ld_saddle_matvec(E, HX, d)(x) - b)
    MEASURED[f"lsqr nobs={nobs} K={K}"][name] = err
    print(f"lsqr nobs={nobs} K={K}: {it} iterations (oracle {itr}), |x - x_oracle| / |x_oracle| {err:.3e}, bar {bar:.3e}, "
          f"residual {res:.3e} (oracle {resr:.3e})")
    assert it == itr, (it, itr)
    assert err <= bar, (err, bar)
    assert res <= 2.0 * resr, (res, resr)


def check_lsqr_beta_zero(gsi, ctx):
    """[[I, e_0], [e_0', 0]] x = e_1: u = A v - alpha u is exactly zero in the first iteration (beta == 0: neither u nor v is
    rescaled), and x = b after it, bit for bit."""
    nobs = 6
    e0, b = np.zeros(nobs), np.zeros(nobs + 1)
    e0[0], b[1] = 1.0, 1.0
    A = gsi.PCGALowRankMatrix([np.zeros(nobs)], e0, np.eye(nobs), ctx=ctx)
    try:
        x, it = A.lsqr(b, return_iterations=True)
    finally:
        A.close()
    ref = orc.PCGALowRankMatrix([np.zeros(nobs)], e0, np.eye(nobs))
    xo, ito = orc.lsqr(ref.matvec, ref.matvec, b, nobs + 1)
    assert ito == 1 and np.array_equal(xo, b)
    assert it == 1 and np.array_equal(x, b), (it, x)


# the child of the poll-invariance test: argv = [out.npz, "cpu" | "gpu"]; GSI_LSQR_POLL is read once per process
POLL_CHILD = r"""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gsi_amd as gsi
import solver_kernel_cases as sk
if sys.argv[2] == "cpu":
    import cpuref
    ctx = gsi.Context(0, lib=cpuref.load_cpuref())
else:
    ctx = gsi.Context(0)
x, it = sk.lsqr_run(gsi, ctx, 300, 4)
np.savez(sys.argv[1], x=x, it=np.int64(it))
ctx.close()
print("lsqr-ok")
"""


def check_lsqr_poll_invariance(which, tmp_path, root):
    """x and the iteration count of the nobs = 300 case with GSI_LSQR_POLL = 1, 8 and 64, one child process each: equal bits
    (with 64, some fifty iterations are enqueued after the stop; on the device they must be no-ops)."""
    import os
    import subprocess
    import sys
    outs = []
    for poll in (1, 8, 64):
        out = str(tmp_path / f"poll{poll}.npz")
        env = dict(os.environ, GSI_LSQR_POLL=str(poll))
        r = subprocess.run([sys.executable, "-c", POLL_CHILD, out, which], capture_output=True, text=True, timeout=300, env=env,
                           cwd=root)
        assert r.returncode == 0 and "lsqr-ok" in r.stdout, f"poll {poll}\n" + r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(np.load(out))
    xr, itr, _, _ = lsqr_reference(300, 4)
    assert int(outs[0]["it"]) == itr
    for o in outs[1:]:
        assert int(o["it"]) == int(outs[0]["it"]) and np.array_equal(o["x"], outs[0]["x"])
