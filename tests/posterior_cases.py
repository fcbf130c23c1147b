"""Cases, extended-precision references and bounds for the posterior variance, shared by the CPU
tests (host path of the CPU reference library) and the GPU tests (posterior_var.hip).

Kernel cases: a[i] = |W' z_i|^2, q[i] = |z_i|^2, t[i] = u' z_i in np.longdouble from the values the basis stores, with bounds
that hold for any summation order and any use of FMA (u = 2^-53), so they are fixed here and not measured:
    |a - a_ref|_i <= 4 (max(K, ncols) + 2) u sum_j (sum_k |z_ik| |W_kj|)^2
    |q - q_ref|_i <= 2 (K + 1) u sum_k z_ik^2
    |t - t_ref|_i <= (K + 1) u sum_k |z_ik| |u_k|
Feature cases: the four shapes of the section, deterministic, and the dense saddle-point formula
    V = Q - [Q H' X] [E E' + R  w; w' 0]^-1 [H Q; X'],   Q = Z Z',
in np.longdouble (Gaussian elimination with partial pivoting written out below: numpy's solvers are float64)."""
import numpy as np

U = 2.0 ** -53
ROW_TILE = 64        # posterior_var.hip: PV_ROWS
COL_CHUNK = 128      # posterior_var.hip: 16 NB columns of W per chunk (NB = 8); ncols <= 64 take NB = 4
N_LIST = sorted({1, 15, 16, 17, 63, 64, 65, 1000, ROW_TILE + 1})
K_LIST = sorted({1, 3, 4, 5, 16, 17, 37, 64, 65, 130, 257, COL_CHUNK + 1})
N_LIST_CPU = [1, 17, 65, 200]
K_LIST_CPU = [1, 4, 5, 37, 130, 257]
VARIANCE_BAR = 1e-12
LD = np.longdouble


def make_basis(gsi, ctx, Z, precision):
    """(basis, the n x K values it stores): an fp32 basis is compared through what it holds, column by column."""
    Z = np.asfortranarray(Z, dtype=np.float64)
    basis = gsi.DeviceBasis(gsi.DeviceMatrix.from_host(ctx, Z), Z.shape[1], precision=precision)
    return basis, np.stack([basis[i] for i in range(Z.shape[1])], axis=1)


def close_basis(basis):
    Zm = basis.Zmat
    basis.close()
    if Zm is not None:
        Zm.close()


def kernel_inputs(n, K, integer, seed=0):
    """Z (n x K) and u (K): Gaussian, or integers in [-3, 3] (every partial sum is then an integer below 2^53)."""
    rng = np.random.default_rng(1000003 * n + 101 * K + seed)
    if integer:
        return rng.integers(-3, 4, (n, K)).astype(np.float64), rng.integers(-3, 4, K).astype(np.float64)
    return rng.standard_normal((n, K)), rng.standard_normal(K)


def w_variants(K, integer, seed=0):
    """(name, the array to pass, upper, the clean K x ncols matrix it stands for): dense K x K; upper triangular with the lower
    part of the passed array NaN; K x ncols for ncols in {1, K - 1, K + 3} inside a parent with a larger leading dimension."""
    rng = np.random.default_rng(77 * K + seed)
    draw = (lambda *s: rng.integers(-3, 4, s).astype(np.float64)) if integer else (lambda *s: rng.standard_normal(s))
    out = []
    W = np.asfortranarray(draw(K, K))
    out.append(("dense", W, False, W))
    Wu = np.triu(draw(K, K))
    Wp = np.asfortranarray(Wu + np.tril(np.full((K, K), np.nan), -1))
    out.append(("upper", Wp, True, Wu))
    for ncols in sorted({1, K - 1, K + 3}):
        if ncols < 1:
            continue
        parent = np.full((K + 5, ncols), np.nan, order="F")
        parent[:K, :] = draw(K, ncols)
        out.append((f"ncols{ncols}", parent[:K, :], False, np.array(parent[:K, :])))
    return out


def kernel_reference(Zs, W, u):
    """a, q, t in extended precision and the three bounds, from the stored basis values."""
    Zl, Wl = Zs.astype(LD), W.astype(LD)
    K, ncols = W.shape
    P = Zl @ Wl
    a = (P * P).sum(axis=1)
    q = (Zl * Zl).sum(axis=1)
    Pa = np.abs(Zl) @ np.abs(Wl)
    ba = 4.0 * (max(K, ncols) + 2) * U * (Pa * Pa).sum(axis=1)
    bq = 2.0 * (K + 1) * U * q
    t = bt = None
    if u is not None:
        t = Zl @ u.astype(LD)
        bt = (K + 1) * U * (np.abs(Zl) @ np.abs(u).astype(LD))
    return dict(a=a, q=q, t=t, ba=ba, bq=bq, bt=bt)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the rows (0 / 0 counts as 0, x / 0 as inf)."""
    err = np.abs(got.astype(LD) - ref)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def check_kernel_case(basis, Zs, integer, label, expect_path):
    """All W variants, with and without u, on one basis; returns the largest error / bound ratio."""
    K = Zs.shape[1]
    _, u = kernel_inputs(Zs.shape[0], K, integer, seed=1)
    worst = 0.0
    for name, Wpass, upper, Wclean in w_variants(K, integer):
        for uu in (u, None):
            a, q, t, info = basis.quadform(Wpass, uu, upper=upper, return_info=True)
            assert info == [0, expect_path], (label, name, info)
            ref = kernel_reference(Zs, Wclean, uu)
            assert (t is None) == (uu is None)
            if integer:
                assert np.array_equal(a, ref["a"].astype(np.float64)), (label, name, "a")
                assert np.array_equal(q, ref["q"].astype(np.float64)), (label, name, "q")
                if uu is not None:
                    assert np.array_equal(t, ref["t"].astype(np.float64)), (label, name, "t")
                continue
            ra, rq = worst_ratio(a, ref["a"], ref["ba"]), worst_ratio(q, ref["q"], ref["bq"])
            rt = worst_ratio(t, ref["t"], ref["bt"]) if uu is not None else 0.0
            worst = max(worst, ra, rq, rt)
            assert ra <= 1.0 and rq <= 1.0 and rt <= 1.0, (label, name, ra, rq, rt)
    return worst


# ---- extended-precision linear algebra ------------------------------------------------------------------------------
def solve_ld(M, B):
    """M^-1 B in np.longdouble by Gaussian elimination with partial pivoting."""
    A = np.array(M, dtype=LD)
    X = np.array(B, dtype=LD)
    if X.ndim == 1:
        X = X[:, None]
    m = A.shape[0]
    for j in range(m):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]] = A[[p, j]]
            X[[j, p]] = X[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:, j:] -= f[:, None] * A[j, j:][None, :]
        X[j + 1:] -= f[:, None] * X[j][None, :]
    for j in range(m - 1, -1, -1):
        X[j] = (X[j] - A[j, j + 1:] @ X[j + 1:]) / A[j, j]
    return X if np.ndim(B) == 2 else X[:, 0]


def chol_ld(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    Lo = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - Lo[j, :j] @ Lo[j, :j]
        Lo[j, j] = np.sqrt(d)
        Lo[j + 1:, j] = (A[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    return Lo


def dense_reference(Zs, E, w, Rfull, X, full=False):
    """The dense saddle-point formula in extended precision: diag(V) for the low-rank prior and c_i' M^-1 c_i (what is
    subtracted from any prior variance); with full=True also V itself."""
    Zl, El, wl, Xl = Zs.astype(LD), E.astype(LD), w.astype(LD), X.astype(LD)
    nobs = E.shape[0]
    M = np.zeros((nobs + 1, nobs + 1), dtype=LD)
    M[:nobs, :nobs] = El @ El.T + Rfull.astype(LD)
    M[:nobs, nobs] = wl
    M[nobs, :nobs] = wl
    Cm = np.vstack([El @ Zl.T, Xl[None, :]])                  # (nobs + 1) x n: [H Q; X'] = [E Z'; X']
    S = solve_ld(M, Cm)
    red = (Cm * S).sum(axis=0)
    q = (Zl * Zl).sum(axis=1)
    out = dict(var=q - red, reduction=red, q=q)
    if full:
        out["V"] = Zl @ Zl.T - Cm.T @ S
    return out


def factor_reference(E, w, Rfull):
    """N = I + B'B, u and gamma of the capacitance form in extended precision."""
    LR = chol_ld(Rfull)
    B = solve_ld(LR, E.astype(LD))
    wt = solve_ld(LR, w.astype(LD))
    N = np.eye(E.shape[1], dtype=LD) + B.T @ B
    r = B.T @ wt
    u = solve_ld(N, r)
    return dict(N=N, u=u, gamma=wt @ wt - r @ u)


# ---- the four feature cases ---------------------------------------------------------------------------------------------
FEATURE_CASES = ["n777_diag", "n777_dense", "n500_points", "n300_K130"]


def feature_case(name):
    """Z, X, R (scipy sparse diagonal, or dense), a forward model description and the linearisation point."""
    import scipy.sparse as sp
    shapes = {"n777_diag": (777, 40, 24, 11), "n777_dense": (777, 40, 24, 11), "n500_points": (500, 60, 37, 12),
              "n300_K130": (300, 10, 130, 13)}
    n, nobs, K, seed = shapes[name]
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, K)) * (1.0 / np.sqrt(1.0 + np.arange(K)))[None, :]
    X = np.ones(n)
    prior = (Z * Z).sum(axis=1) + rng.uniform(0.1, 0.5, n)     # a "true" prior variance above the low-rank one
    if name == "n500_points":
        idx = np.sort(rng.choice(n, nobs, replace=False))
        H = sp.csr_matrix((np.ones(nobs), (np.arange(nobs), idx)), shape=(nobs, n))
        Rdiag = rng.uniform(1e-4, 2e-4, nobs)
        R = sp.diags(Rdiag, format="csc")
        Rfull = np.diag(Rdiag)
        return dict(name=name, n=n, nobs=nobs, K=K, Z=Z, X=X, prior=prior, H=H, idx=idx, R=R, Rfull=Rfull, Rdiag=Rdiag,
                    s=np.zeros(n))
    H = rng.standard_normal((nobs, n)) / np.sqrt(n)
    if name == "n777_dense":
        A = rng.standard_normal((nobs, nobs))
        Rfull = A @ A.T / nobs + 0.5 * np.eye(nobs)
        R = Rfull
    else:
        Rdiag = rng.uniform(0.5, 1.5, nobs)
        R = sp.diags(Rdiag, format="csc")
        Rfull = np.diag(Rdiag)
    return dict(name=name, n=n, nobs=nobs, K=K, Z=Z, X=X, prior=prior, H=H, R=R, Rfull=Rfull, s=np.zeros(n))


def forward_model(gsi, ctx, case):
    """The case's model: a LinearForwardModel for the point samples (linearised on the device beside a DeviceBasis), a host
    callable otherwise."""
    if case["name"] == "n500_points":
        return gsi.LinearForwardModel(case["H"], ctx=ctx)
    H = case["H"]
    return lambda s: H @ s


def linearisation(gsi, fwd, basis, case):
    """E (nobs x K) and HX exactly as posterior_variance computes them: the same call with the same inputs."""
    import sys
    mod = sys.modules[gsi.__name__ + ".pcga"]          # the module: the package's attribute `pcga` is the function
    etas, HX, _, _ = mod._iteration_head(fwd, basis, case["s"], case["X"], mod.SQRT_EPS)
    return np.stack(etas, axis=1), HX


# ---- feature checks, run by both test files on their own context ------------------------------------------------------------
def check_variance(gsi, ctx, name, precision, with_prior, expect_path):
    """posterior_variance against the dense formula; returns max |v - v_ref| / max |v_ref|."""
    case = feature_case(name)
    basis, Zs = make_basis(gsi, ctx, case["Z"], precision)
    fwd = forward_model(gsi, ctx, case)
    try:
        E, w = linearisation(gsi, fwd, basis, case)
        ref = dense_reference(Zs, E, w, case["Rfull"], case["X"])
        prior = case["prior"] if with_prior else None
        want = (case["prior"].astype(LD) - ref["reduction"]) if with_prior else ref["var"]
        v, info = gsi.posterior_variance(fwd, case["s"], case["X"], basis, case["R"], prior_variance=prior, return_info=True)
        assert info == [0, expect_path], info
        ratio = float(np.abs(v.astype(LD) - want).max() / np.abs(want).max())
        if not with_prior:
            assert np.all(v >= 0.0)
    finally:
        if hasattr(fwd, "close"):
            fwd.close()
        close_basis(basis)
    return ratio


def check_factor(gsi, ctx, name, expect_path):
    """W upper triangular with W' N W = I, u and gamma against extended precision; returns the three ratios."""
    case = feature_case(name)
    basis, Zs = make_basis(gsi, ctx, case["Z"], 64)
    fwd = forward_model(gsi, ctx, case)
    try:
        E, w = linearisation(gsi, fwd, basis, case)
        A = gsi.PCGALowRankMatrix([E[:, i].copy() for i in range(E.shape[1])], w, case["R"], ctx=ctx)
        W, u, gamma, info = A.posterior_factor(return_info=True)
        A.close()
    finally:
        if hasattr(fwd, "close"):
            fwd.close()
        close_basis(basis)
    assert info == [0, expect_path], info
    K = case["K"]
    assert W.shape == (K, K) and np.array_equal(np.tril(W, -1), np.zeros((K, K)))
    ref = factor_reference(E, w, case["Rfull"])
    Wl = W.astype(LD)
    r_id = float(np.abs(Wl.T @ ref["N"] @ Wl - np.eye(K, dtype=LD)).max())
    r_u = float(np.sqrt(((u.astype(LD) - ref["u"]) ** 2).sum()) / np.sqrt((ref["u"] ** 2).sum()))
    r_g = float(abs(LD(gamma) - ref["gamma"]) / abs(ref["gamma"]))
    assert r_id <= 1e-12 * K and r_u <= 1e-12 and r_g <= 1e-12, (name, r_id, r_u, r_g)
    return r_id, r_u, r_g


def check_observed_points(gsi, ctx, precision, expect_path):
    """60 point samples of a field of 500 with R_jj in [1, 2] 1e-4: the measurement itself is an unbiased estimator with
    variance R_jj, so the posterior variance at every observed point is at most R_jj; and every variance is >= 0."""
    case = feature_case("n500_points")
    basis, _ = make_basis(gsi, ctx, case["Z"], precision)
    fwd = forward_model(gsi, ctx, case)
    try:
        v, info = gsi.posterior_variance(fwd, case["s"], case["X"], basis, case["R"], return_info=True)
    finally:
        fwd.close()
        close_basis(basis)
    assert info == [0, expect_path]
    ratio = v[case["idx"]] / case["Rdiag"]
    assert np.all(v >= 0.0)
    assert np.all(ratio <= 1.0), float(ratio.max())
    return float(ratio.max())


def check_realizations(gsi, ctx, xis_on_device):
    """posterior_realizations with a given omega against the numpy formula, and Z W W' Z' + d d' / gamma against the dense V
    at n = 300; returns the two ratios."""
    case = feature_case("n300_K130")
    n, K = case["n"], case["K"]
    basis, Zs = make_basis(gsi, ctx, case["Z"], 64)
    fwd = forward_model(gsi, ctx, case)
    try:
        E, w = linearisation(gsi, fwd, basis, case)
        A = gsi.PCGALowRankMatrix([E[:, i].copy() for i in range(K)], w, case["R"], ctx=ctx)
        W, u, gamma = A.posterior_factor()
        A.close()
        rng = np.random.default_rng(21)
        omega = rng.standard_normal((K + 1, 3))
        s_hat = rng.standard_normal(n)
        xis = basis if xis_on_device else [np.ascontiguousarray(case["Z"][:, i]) for i in range(K)]
        got = gsi.posterior_realizations(fwd, s_hat, case["X"], xis, case["R"], 3, omega=omega, ctx=ctx)
        again = gsi.posterior_realizations(fwd, s_hat, case["X"], xis, case["R"], 3, omega=omega, ctx=ctx)
    finally:
        close_basis(basis)
    assert got.shape == (n, 3) and np.array_equal(got, again)
    # the factor at s_hat: the model is linear, but the finite differences are taken there
    case2 = dict(case, s=s_hat)
    basis2, _ = make_basis(gsi, ctx, case["Z"], 64)
    try:
        E2, w2 = linearisation(gsi, fwd, basis2, case2)
        A2 = gsi.PCGALowRankMatrix([E2[:, i].copy() for i in range(K)], w2, case["R"], ctx=ctx)
        W2, u2, g2 = A2.posterior_factor()
        A2.close()
    finally:
        close_basis(basis2)
    w2s = omega[K] / np.sqrt(g2)
    want = s_hat[:, None] + Zs @ (W2 @ omega[:K] + np.outer(u2, w2s)) - np.outer(case["X"], w2s)
    r_real = float(np.abs(got - want).max() / np.abs(want).max())
    ref = dense_reference(Zs, E, w, case["Rfull"], case["X"], full=True)
    Zl = Zs.astype(LD)
    d = Zl @ u.astype(LD) - case["X"].astype(LD)
    ZW = Zl @ W.astype(LD)
    V = ZW @ ZW.T + np.outer(d, d) / LD(gamma)
    r_cov = float(np.abs(V - ref["V"]).max() / np.abs(ref["V"]).max())
    assert r_real <= 1e-12 and r_cov <= 1e-12, (r_real, r_cov)
    return r_real, r_cov
