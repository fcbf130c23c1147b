"""Cases, bars and checks of the likelihood gradient, shared by tests/test_loglik_grad_cpu.py (the CPU
reference library: dense A and dense dA) and tests/test_loglik_grad_gpu.py (the same, plus the FFT operators).

The bar of S_k and t_{k,i} is a first-order bound formed here from the dense matrices and the solver's reported `relres`,
doubled:
  * a solved column x_a = M^-1 b_a is off by at most  e_a = relres_a |b_a| / lambda_min(M);
  * S_k[a, c] = x_a' dM x_c moves by at most  |dM|_2 (e_a |x_c| + |x_a| e_c),  t_{k,i} = x_i' dM w_i by  e_i |dM w_i|;
  * the product Y = dM R has the project's bar for an operator product, 1e-12 max|Y_ref| per entry, so the sum over the rows
    moves by at most that times |x_a|_1.
The gradient's bar sums these through its formula, with the first-order movement of beta and G'M^-1 G."""
import numpy as np

import loglik_grad_model as lm

N_DENSE, S_PROBES, RANK = 37, 5, 6
NOISE = 0.05
TOL = 1e-11
PRODUCT_BAR = 1e-12
PARAMS = ("log_sigma2", "log_ell", "log_noise")


def dense_case(p, seed=3):
    """37 scattered points in the unit square under sigma2 exp(-d / ell) + noise: M, the three dM, y, G, and A."""
    rng = np.random.default_rng([seed, p])
    n = N_DENSE
    P = rng.random((2, n))
    D = np.sqrt(((P[:, :, None] - P[:, None, :]) ** 2).sum(axis=0))
    sigma2, ell = 1.4, 0.35
    A = sigma2 * np.exp(-D / ell)
    noise = NOISE * (1.0 + rng.random(n))
    dA = [A.copy(), A * (D / ell), np.zeros((n, n))]
    dn = [None, None, noise.copy()]
    dMs = [dA[0], dA[1], np.diag(noise)]
    G = np.column_stack([np.ones(n), P[0]])[:, :p]
    Lc = np.linalg.cholesky(A + np.diag(noise))
    y = Lc @ rng.standard_normal(n) + (G @ np.array([0.7, -0.4])[:p] if p else 0.0)
    return {"A": A, "noise": noise, "M": A + np.diag(noise), "dA": dA, "dnoise": dn, "dMs": dMs, "y": y, "G": G, "points": P,
            "D": D, "x0": np.array([np.log(sigma2), np.log(ell), 0.0])}


def dense_M(case, x):
    """M at the parameters x = (log sigma2, log ell, log noise) of a `dense_case`."""
    return np.exp(x[0]) * np.exp(-case["D"] / np.exp(x[1])) + np.diag(case["noise"] * np.exp(x[2]))


def precond_parts(A, noise, rank=RANK):
    """A rank-`rank` basis (leading eigenpairs of A) and the dense P = Zb Zb' + diag(noise)."""
    w, V = np.linalg.eigh(A)
    Zb = V[:, -rank:] * np.sqrt(w[-rank:])
    return Zb, Zb @ Zb.T + np.diag(noise)


def probes(n, s, P=None, seed=11):
    """Host-given probes: standard normals (coloured by chol(P) with a preconditioner, so that E[zz'] = P)."""
    Z = np.random.default_rng([seed, n, s]).standard_normal((n, s))
    return Z if P is None else np.linalg.cholesky(P) @ Z


def column_errors(M, B, relres):
    """e_a = relres_a |b_a| / lambda_min(M) per solved column."""
    lam = float(np.linalg.eigvalsh(0.5 * (M + M.T))[0])
    return np.asarray(relres) * np.linalg.norm(B, axis=0) / lam


def term_bars(M, dM, B, X, W, relres, g):
    """(bar_S (g x g), bar_t (s)) for one parameter, doubled; X = the dense M^-1 B, W = the dense P^-1 Z."""
    e = column_errors(M, B, relres)
    nx = np.linalg.norm(X, axis=0)
    dn = float(np.linalg.norm(dM, 2))
    R = np.column_stack([X[:, :g], W])
    Yref = dM @ R
    pb = PRODUCT_BAR * max(float(np.abs(Yref).max()), np.finfo(float).tiny)
    l1 = np.abs(X).sum(axis=0)
    bS = dn * (e[:g, None] * nx[None, :g] + nx[:g, None] * e[None, :g]) + pb * l1[:g, None]
    bt = e[g:] * np.linalg.norm(dM @ W, axis=0) + pb * l1[g:]
    return 2.0 * bS, 2.0 * bt


def grad_bar(M, dM, y, G, B, X, W, relres, restricted):
    """The summed first-order bound of one gradient entry -1/2 [mean t - tr(GMG^-1 S11) - c'Sc], doubled terms included."""
    g = 1 + G.shape[1]
    bS, bt = term_bars(M, dM, B, X, W, relres, g)
    e = column_errors(M, B, relres)
    S = X[:, :g].T @ dM @ X[:, :g]
    if g > 1:
        GMG = G.T @ X[:, 1:g]
        Gi = np.linalg.inv(GMG)
        beta = Gi @ (G.T @ X[:, 0])
        gn, gin = float(np.linalg.norm(G, 2)), float(np.linalg.norm(Gi, 2))
        dGMG = gn * float(np.linalg.norm(e[1:g]))
        dbeta = 2.0 * gin * (gn * e[0] + dGMG * float(np.linalg.norm(beta)))
        c = np.concatenate([[1.0], -beta])
        dc = np.concatenate([[0.0], np.full(g - 1, dbeta)])
        quad = np.abs(c) @ bS @ np.abs(c) + 2.0 * dc @ np.abs(S) @ np.abs(c)
        mid = 0.0
        if restricted:
            mid = np.sum(np.abs(Gi) * bS[1:, 1:].T) + 2.0 * gin * gin * dGMG * float(np.linalg.norm(S[1:, 1:])) * np.sqrt(g - 1.0)
    else:
        quad, mid = bS[0, 0], 0.0
    return 0.5 * (float(np.mean(bt)) + mid + quad)


def dense_terms(case, Z, P=None):
    """The dense same-probe S, T, X, W and B of a case."""
    S, T, X = lm.same_probe_terms(case["M"], case["dMs"], case["y"], case["G"], Z, P)
    W = Z if P is None else np.linalg.solve(P, Z)
    return S, T, X, W, np.column_stack([case["y"], case["G"], Z])


def check_terms(case, info, Z, P, record=None, what=""):
    """Assert S_k and t_{k,i} of a `log_likelihood_grad` report against the dense same-probe quantities; returns the worst
    ratio to the bar."""
    S, T, X, W, B = dense_terms(case, Z, P)
    g = 1 + case["G"].shape[1]
    worst = 0.0
    for k, dM in enumerate(case["dMs"]):
        bS, bt = term_bars(case["M"], dM, B, X, W, info["relres"], g)
        rS = float((np.abs(info["S"][k] - S[k]) / bS).max())
        rt = float((np.abs(info["t"][k] - T[k]) / bt).max())
        print(f"{what} param {k}: S ratio {rS:.3e}, t ratio {rt:.3e}")
        worst = max(worst, rS, rt)
        assert rS <= 1.0 and rt <= 1.0, (what, k, rS, rt)
    if record is not None:
        record(what, worst)
    return worst


def write_errors(section, values, bars=None):
    """LOGLIK_GRAD_ERRORS=<path>: merge `values` (and `bars`) under `section` into that JSON file
    (profiles/loglik_grad_errors.json is such a run of the CPU files and of the GPU file)."""
    import json
    import os
    path = os.environ.get("LOGLIK_GRAD_ERRORS")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[section] = {"values": values}
    if bars is not None:
        doc[section]["bars"] = bars
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True, default=float)
        f.write("\n")


# ---- the runs shared by the CPU reference and the GPU file (dense A, dense dA) -----------------------------------------------
def _dense_ops(gsi, ctx, case):
    op = gsi.dense_operator(ctx, case["A"])
    dops = [gsi.dense_operator(ctx, case["dA"][0]), gsi.dense_operator(ctx, case["dA"][1]), None]
    return op, dops


def _close(ops):
    for o in ops:
        if o is not None:
            o.close()


def run_dense_terms(gsi, ctx, p, with_precond, record, where):
    case = dense_case(p)
    n = N_DENSE
    Zb, P = precond_parts(case["A"], case["noise"]) if with_precond else (None, None)
    Z = probes(n, S_PROBES, P)
    op, dops = _dense_ops(gsi, ctx, case)
    pc = gsi.lowrank_preconditioner(op, basis=Zb, diag=case["noise"]) if with_precond else None
    try:
        drift = case["G"] if p else None
        val, grad, info = gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=drift,
                                                  precond=pc, probes=Z, tol=TOL, return_info=True)
        check_terms(case, info, Z, P, record, f"{where} dense p={p} precond={with_precond}")
        # the value is log_likelihood's, bit for bit; the gradient is what the model forms from the reported terms
        for restricted in (True, False):
            v1, g1 = gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=drift,
                                             precond=pc, probes=Z, tol=TOL, restricted=restricted)
            v0 = gsi.log_likelihood(op, case["y"], noise=case["noise"], drift=drift, precond=pc, probes=Z, tol=TOL,
                                    restricted=restricted)
            assert v1 == v0, (v1, v0)
            assert np.isfinite(g1).all() and g1.shape == (3,)
        assert info["t"].shape == (3, S_PROBES) and info["grad_stderr"].shape == (3,) and len(info["S"]) == 3
        assert np.allclose(info["grad_stderr"], np.std(info["t"], axis=1, ddof=1) / (2.0 * np.sqrt(S_PROBES)), rtol=1e-14)
        # NULL dop with dnoise is the noise derivative alone; dops=None with dnoise only gives the same entry
        _, g2 = gsi.log_likelihood_grad(op, None, case["y"], noise=case["noise"], dnoise=[case["noise"]], drift=drift,
                                        precond=pc, probes=Z, tol=TOL)
        assert g2.shape == (1,) and g2[0] == grad[2]
    finally:
        if pc is not None:
            pc.close()
        _close([op] + dops)


def run_dense_gradient(gsi, ctx, p, restricted, record, where):
    """Z = sqrt(m) I, no preconditioner: the trace is exact, and the gradient is the analytic dense gradient within the
    summed bound."""
    case = dense_case(p)
    n = N_DENSE
    Z = np.sqrt(n) * np.eye(n)
    op, dops = _dense_ops(gsi, ctx, case)
    try:
        drift = case["G"] if p else None
        val, grad, info = gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=drift,
                                                  probes=Z, tol=TOL, restricted=restricted, return_info=True)
        want = lm.loglik_grad(case["M"], case["dMs"], case["y"], case["G"], restricted)
        S, T, X, W, B = dense_terms(case, Z)
        worst = 0.0
        for k, dM in enumerate(case["dMs"]):
            bar = grad_bar(case["M"], dM, case["y"], case["G"], B, X, W, info["relres"], restricted)
            ratio = abs(grad[k] - want[k]) / bar
            print(f"{where} p={p} restricted={restricted} param {k}: grad {grad[k]:.12e}, dense {want[k]:.12e}, ratio to bar {ratio:.3e}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (k, grad[k], want[k], bar)
        record(f"{where} gradient p={p} {'reml' if restricted else 'ml'}", worst)
        # with unit probes the log-determinant is exact as well: the value is the dense one to the solver's tolerance
        dense_val = lm.loglik(case["M"], case["y"], case["G"], restricted)
        assert abs(val - dense_val) <= 1e-6 * abs(dense_val)
    finally:
        _close([op] + dops)


def run_term_refusals(gsi, ctx):
    import solve_cases as sc
    case = dense_case(0)
    n = N_DENSE
    X, Wz, bad = gsi.DeviceMatrix(ctx, n, 20), gsi.DeviceMatrix(ctx, n, 19), gsi.DeviceMatrix(ctx, n, 5)
    Xw = gsi.DeviceMatrix(ctx, n, 18)
    op = gsi.dense_operator(ctx, case["A"])
    small = gsi.dense_operator(ctx, case["A"][:5, :5].copy())
    try:
        sc.refused(gsi, lambda: gsi.op_bilinear_terms(op, None, X, 17, Wz), "min(b, 16)")
        sc.refused(gsi, lambda: gsi.op_bilinear_terms(op, None, X, 1, bad), "Wz is")
        sc.refused(gsi, lambda: gsi.op_bilinear_terms(op, None, X, 1, None), "Wz is NULL")
        sc.refused(gsi, lambda: gsi.op_bilinear_terms(small, None, X, 1, Wz), "dop is")
        sc.refused(gsi, lambda: gsi.op_bilinear_terms(op, np.full(n, np.inf), X, 1, Wz), "non-finite")
        with np.testing.assert_raises(ValueError):
            gsi.op_bilinear_terms(op, np.ones(n - 1), X, 1, Wz)
        with np.testing.assert_raises(ValueError):
            gsi.log_likelihood_grad(op, [None, None], case["y"], noise=case["noise"], dnoise=[None])
        with np.testing.assert_raises(ValueError):
            gsi.log_likelihood_grad(op, [None], case["y"][:-1], noise=case["noise"][:-1])
    finally:
        for h in (X, Wz, bad, Xw, op, small):
            h.close()


# ---- FFT covariances read at points or through a linear model (GPU; the dense side is checked on the CPU) -------------------
FFT_NS, FFT_KIND, FFT_ELL, FFT_SIGMA2 = (8, 6), 1, 2.5, 1.4


def sparse_rows(n, nobs, seed):
    """CSR (indptr, indices, data) of `nobs` rows of 5 positive weights each, and the dense H."""
    rng = np.random.default_rng([seed, n, nobs])
    H = np.zeros((nobs, n))
    indptr, indices, data = [0], [], []
    for r in range(nobs):
        cols = np.sort(rng.choice(n, size=5, replace=False))
        vals = 0.5 + rng.random(5)
        H[r, cols] = vals
        indices += cols.tolist()
        data += vals.tolist()
        indptr.append(len(indices))
    return (np.array(indptr), np.array(indices), np.array(data)), H


def fft_geometry(which, Ns=FFT_NS):
    """("at": 30 scattered points; "linear": 20 sparse rows) -> (dense observation matrix Hm, points, box, csr)"""
    import fftrf_interp_model as im
    import interp_adjoint_model as am
    n = int(np.prod(Ns))
    if which == "at":
        m = 30 if Ns == FFT_NS else 60
        P = im.scattered_points(Ns, m, seed=23)
        box = im.inner_box(P, shrink=0.05)
        base, frac = im.plan(P, Ns, box)
        return am.weights_matrix(Ns, base, frac), P, box, None
    csr, H = sparse_rows(n, 20, 29)
    return H, None, None, csr


def fft_M(Hm, noise, x, Ns=FFT_NS, kind=FFT_KIND):
    """(M, [dM]) at x = (log sigma2, log ell, log noise): ell in grid spacings, the same on every axis."""
    ell = [float(np.exp(x[1]))] * len(Ns)
    s2 = float(np.exp(x[0]))
    Cm = lm.cov_entries(Ns, kind, ell, 0.0, s2, 0.0).astype(np.float64)
    dC = [lm.dk_entries(Ns, kind, ell, 0.0, s2, prm).astype(np.float64) for prm in ("log_sigma2", "log_ell")]
    nz = noise * np.exp(x[2])
    A = Hm @ Cm @ Hm.T
    dA = [Hm @ d @ Hm.T for d in dC] + [np.zeros_like(A)]
    return A, dA, nz


def fft_case(which, p):
    Hm, P, box, csr = fft_geometry(which)
    m = Hm.shape[0]
    rng = np.random.default_rng([41, m, p])
    noise = NOISE * (1.0 + rng.random(m))
    x0 = np.array([np.log(FFT_SIGMA2), np.log(FFT_ELL), 0.0])
    A, dA, nz = fft_M(Hm, noise, x0)
    M = A + np.diag(nz)
    G = np.column_stack([np.ones(m), np.linspace(-1.0, 1.0, m)])[:, :p]
    y = np.linalg.cholesky(M) @ rng.standard_normal(m) + (G @ np.array([0.7, -0.4])[:p] if p else 0.0)
    return {"A": A, "noise": nz, "M": M, "dA": dA, "dnoise": [None, None, nz.copy()], "dMs": dA[:2] + [np.diag(nz)], "y": y, "G": G,
            "points": P, "box": box, "csr": csr, "which": which}


def fft_family(gsi, ctx, case, Ns=FFT_NS, kind="exponential"):
    if case["which"] == "at":
        return gsi.covariance_family(ctx, Ns, kind, points=case["points"], box=case["box"]), None
    indptr, indices, data = case["csr"]
    mdl = gsi.LinearForwardModel((indptr, indices, data, (len(indptr) - 1, int(np.prod(Ns)))), link="identity", ctx=ctx)
    return gsi.covariance_family(ctx, Ns, kind, model=mdl), mdl


def run_fft_terms(gsi, ctx, which, p, with_precond, record):
    case = fft_case(which, p)
    m = case["y"].size
    Zb, P = precond_parts(case["A"], case["noise"]) if with_precond else (None, None)
    Z = probes(m, S_PROBES, P)
    fam, mdl = fft_family(gsi, ctx, case)
    prm = {"log_sigma2": np.log(FFT_SIGMA2), "log_ell": np.log(FFT_ELL)}
    op = fam.operator(prm)
    dops = fam.derivatives(prm, PARAMS)
    assert dops[2] is None
    pc = gsi.lowrank_preconditioner(op, basis=Zb, diag=case["noise"]) if with_precond else None
    try:
        drift = case["G"] if p else None
        val, grad, info = gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=drift,
                                                  precond=pc, probes=Z, tol=TOL, return_info=True)
        check_terms(case, info, Z, P, record, f"gpu fft-{which} p={p} precond={with_precond}")
        v0 = gsi.log_likelihood(op, case["y"], noise=case["noise"], drift=drift, precond=pc, probes=Z, tol=TOL)
        assert val == v0
        # probes drawn on the device (a count): the same value as log_likelihood with the same seed, bit for bit
        v1, _ = gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=drift, precond=pc,
                                        probes=4, seed=5, tol=TOL)
        assert v1 == gsi.log_likelihood(op, case["y"], noise=case["noise"], drift=drift, precond=pc, probes=4, seed=5, tol=TOL)
    finally:
        if pc is not None:
            pc.close()
        for o in dops + [op]:
            fam.release(o)
        fam.close()
        if mdl is not None:
            mdl.close()


# ---- the fit ---------------------------------------------------------------------------------------------------------------
FIT_NS, FIT_M = (16, 12), 60
FIT_TRUE = {"log_sigma2": np.log(2.0), "log_ell": np.log(4.0)}
FIT_START = {"log_sigma2": 0.0, "log_ell": np.log(1.5)}
FIT_NOISE = 0.05
FIT_GTOL = 1e-3
FIT_SEED = 4


def fit_case():
    """16 x 12 exponential grid read at 60 points; data drawn at ell = 4, sigma2 = 2 with noise 0.05."""
    Hm, P, box, _ = fft_geometry("at", FIT_NS)
    m = Hm.shape[0]
    noise = np.full(m, FIT_NOISE)
    xt = np.array([FIT_TRUE["log_sigma2"], FIT_TRUE["log_ell"], 0.0])
    A, _, nz = fft_M(Hm, noise, xt, FIT_NS)
    y = np.linalg.cholesky(A + np.diag(nz)) @ np.random.default_rng(FIT_SEED).standard_normal(m)
    return {"Hm": Hm, "points": P, "box": box, "noise": noise, "y": y, "which": "at"}


def fit_dense_evaluate(fc):
    """The dense model's (params, value, gradient, None) at x = (log sigma2, log ell): what `fit_covariance` maximises when
    its probes are Z = sqrt(m) I."""
    G0 = np.zeros((fc["y"].size, 0))

    def evaluate(x):
        A, dA, nz = fft_M(fc["Hm"], fc["noise"], np.array([x[0], x[1], 0.0]), FIT_NS)
        M = A + np.diag(nz)
        return ({"log_sigma2": float(x[0]), "log_ell": float(x[1])}, lm.loglik(M, fc["y"], G0, True),
                lm.loglik_grad(M, dA[:2], fc["y"], G0, True), None)

    return evaluate


def check_fit(report, params, fc):
    """The conditions of the fit: the value never decreases, the stop reason is gtol, and the dense gradient at the result
    is at most 1e-3 of that at the start (largest entry)."""
    vals = [t["value"] for t in report["trace"]]
    assert all(b >= a for a, b in zip(vals, vals[1:])), vals
    assert report["stop"] == "gtol", report["stop"]
    ev = fit_dense_evaluate(fc)
    g0 = ev([FIT_START["log_sigma2"], FIT_START["log_ell"]])[2]
    g1 = ev([params["log_sigma2"], params["log_ell"]])[2]
    ratio = float(np.abs(g1).max() / np.abs(g0).max())
    print(f"fit: {len(vals)} accepted points, value {vals[0]:.6f} -> {vals[-1]:.6f}, params {params}, dense |g| ratio {ratio:.3e}")
    assert ratio <= 1e-3, (g0, g1)
    return ratio
