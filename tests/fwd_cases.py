"""Shared inputs and references of the sparse-forward-model tests (test_pcga_forward_cpu.py, test_pcga_forward_gpu.py).

Everything here is numpy on the host; references are computed once per configuration and handed out read-only."""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
ROW_LENGTHS = [0, 1, 3, 63, 64, 65, 200, 1000]


def csr_rows(n, lengths, rng, values="randn"):
    """CSR arrays with the given row lengths: unsorted indices, and in every row of 3 or more a repeated one."""
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lengths)
    idx, val = [], []
    for ln in lengths:
        j = rng.choice(n, size=ln, replace=False).astype(np.int64)
        if ln >= 3:
            j[-1] = j[0]
        idx.append(j)
        val.append(rng.integers(-3, 4, size=ln).astype(np.float64) if values == "int" else rng.standard_normal(ln))
    return indptr, np.concatenate(idx) if idx else np.zeros(0, np.int64), np.concatenate(val) if val else np.zeros(0)


def dense_of(indptr, indices, data, n):
    """(H, |H|) as dense matrices; repeated indices add."""
    nobs = len(indptr) - 1
    rows = np.repeat(np.arange(nobs), np.diff(indptr))
    H = np.zeros((nobs, n))
    A = np.zeros((nobs, n))
    np.add.at(H, (rows, indices), data)
    np.add.at(A, (rows, indices), np.abs(data))
    return H, A


def paramstorun(Zs, s, X, delta):
    """direct.jl:39-45 from the STORED basis columns Zs (n x K)."""
    return np.concatenate([s[:, None] + delta * Zs, (s + delta * X)[:, None], (s + delta * s)[:, None], s[:, None]], axis=1)


def reference(indptr, indices, data, n, w, link, P):
    """(ref, bound): ref = H g(w .* P); bound = 8 eps (nnz_r + 8) (|H| |g|), times (1 + max|w P|) for the exp link --
    the standard rounding bound of a dot product with slack for FMA contraction and exp, none for a lost nonzero."""
    H, A = dense_of(indptr, indices, data, n)
    wv = np.ones(n) if w is None else w
    arg = wv[:, None] * P
    g = np.exp(arg) if link else arg
    ref = H @ g
    nnz_r = np.diff(indptr).astype(np.float64)
    bound = 8 * EPS * (nnz_r[:, None] + 8) * (A @ np.abs(g))
    if link:
        bound = bound * (1.0 + np.abs(arg).max())
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def planned_segments(indptr, limit):
    """(segments, split rows) the planner must report for this limit."""
    ln = np.diff(indptr)
    return int(np.maximum(1, -(-ln // limit)).sum()), int((ln > limit).sum())


@functools.lru_cache(maxsize=None)
def product_case(K, link, n=1000, nobs=40):
    """The product problem of the issue: n = 1000, nobs = 40, row lengths cycling through ROW_LENGTHS.  Arguments of the
    exp link are scaled so that max |w P| <= 10."""
    rng = np.random.default_rng(1000 * K + link)
    lengths = [ROW_LENGTHS[r % len(ROW_LENGTHS)] for r in range(nobs)]
    indptr, indices, data = csr_rows(n, lengths, rng)
    w = 1.0 + 0.1 * rng.standard_normal(n)
    Z = rng.standard_normal((n, K + 2))                # the matrix behind the basis has spare columns
    s = rng.standard_normal(n)
    X = rng.standard_normal(n)
    delta = 0.25
    if link:
        Z, s, X = 0.5 * Z, 0.5 * s, 0.5 * X
    for a in (indptr, indices, data, w, Z, s, X):
        a.setflags(write=False)
    return dict(n=n, nobs=nobs, K=K, link=link, indptr=indptr, indices=indices, data=data, w=w, Z=Z, s=s, X=X, delta=delta)


def check_product(got, case, Zs):
    """got (nobs x (K+3)) against the reference on the stored columns Zs, componentwise; empty rows exactly zero.
    Returns the largest error / bound ratio."""
    P = paramstorun(Zs, case["s"], case["X"], case["delta"])
    if case["link"]:
        assert np.abs(case["w"][:, None] * P).max() <= 10.0
    ref, bound = reference(case["indptr"], case["indices"], case["data"], case["n"], case["w"], case["link"], P)
    assert got.shape == ref.shape
    empty = np.diff(case["indptr"]) == 0
    assert empty.any() and np.all(got[empty] == 0.0)
    err = np.abs(got - ref)
    bad = err > bound
    ratio = float((err[~empty] / bound[~empty]).max())
    assert not bad.any(), f"{int(bad.sum())} entries beyond the bound; largest error / bound = {ratio:.3g}"
    return ratio


@functools.lru_cache(maxsize=None)
def inversion_case(link):
    """The end-to-end problem of the issue: n = 1000, M = 12, p = 4, nobs = 96, rows = runs of 1 .. 1000 consecutive cells
    (block averages), w = 1 + 0.1 randn, noise 1e-4, truth = mean + a combination of six xi."""
    import scipy.sparse as sp
    from helpers import gaussian_cov
    rng = np.random.default_rng(77 + link)
    n, M, p, nobs = 1000, 12, 4, 96
    Qc = gaussian_cov(40, 25, 6.0)
    Om = rng.standard_normal((n, M + p))
    lengths = np.linspace(1, n, nobs).astype(np.int64)
    starts = np.array([rng.integers(0, n - ln + 1) for ln in lengths], dtype=np.int64)
    indptr = np.zeros(nobs + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lengths)
    indices = np.concatenate([np.arange(a, a + ln) for a, ln in zip(starts, lengths)]).astype(np.int64)
    data = np.concatenate([np.full(ln, 1.0 / ln) for ln in lengths])
    w = 1.0 + 0.1 * rng.standard_normal(n)
    H = sp.csr_matrix((data, indices, indptr), shape=(nobs, n))
    mu = 1.0 if link else 10.0
    coef = np.concatenate([rng.standard_normal(6), np.zeros(M - 6)]) * (0.3 if link else 1.0)
    noise = 1e-4 * rng.standard_normal(nobs)
    S = rng.standard_normal((48, nobs))
    return dict(n=n, M=M, p=p, nobs=nobs, Qc=Qc, Om=Om, H=H, w=w, mu=mu, coef=coef, noise=noise, S=S, link=link)


def host_lambda(case):
    H, w, link = case["H"], case["w"], case["link"]
    return (lambda pv: H @ np.exp(w * pv)) if link else (lambda pv: H @ (w * pv))


def run_inversions(gsi, ctx, link, precision=64):
    """pcgadirect, pcgalsqr and rga with the LinearForwardModel against the same calls with the host lambda, on one basis.
    Bars (tests/test_gpu_parity.py:606-609): the two solutions agree within 1e-3 relative, both recover the truth within
    2e-2.  Returns the model's info() at the end and the figures."""
    import scipy.sparse as sp
    c = inversion_case(link)
    basis = gsi.getxis_device(c["Qc"], c["M"], c["p"], 3, Omega=c["Om"], ctx=ctx, precision=precision)
    fwd = gsi.LinearForwardModel(c["H"], weights=c["w"], link="exp" if link else "identity", ctx=ctx)
    lam = host_lambda(c)
    try:
        xis = np.stack([basis[i] for i in range(c["M"])], axis=1)
        X = np.full(c["n"], c["mu"])
        truth = X + xis @ c["coef"]
        y = lam(truth) + c["noise"]
        R = 1e-8 * sp.identity(c["nobs"], format="csc")
        figures = {}
        before = fwd.info()[7]
        for name, solve in (("pcgadirect", gsi.pcgadirect), ("pcgalsqr", gsi.pcgalsqr)):
            got = solve(fwd, X.copy(), X, basis, R, y)
            ref = solve(lam, X.copy(), X, basis, R, y)
            figures[name] = (np.linalg.norm(got - ref) / np.linalg.norm(ref), np.linalg.norm(got - truth) / np.linalg.norm(truth),
                             np.linalg.norm(ref - truth) / np.linalg.norm(truth))
        assert fwd.info()[7] > before
        before = fwd.info()[7]
        got = gsi.rga(fwd, X.copy(), X, basis, R, y, c["S"])
        assert fwd.info()[7] > before, "rga left the device path"
        ref = gsi.rga(lam, X.copy(), X, basis, R, y, c["S"])
        figures["rga"] = (np.linalg.norm(got - ref) / np.linalg.norm(ref), np.linalg.norm(got - truth) / np.linalg.norm(truth),
                          np.linalg.norm(ref - truth) / np.linalg.norm(truth))
        print(f"link {link} precision {precision}: (model vs lambda, model vs truth, lambda vs truth) = {figures}")
        for name, (agree, rec_model, rec_lambda) in figures.items():
            assert agree < 1e-3, (name, agree)
            assert rec_model < 2e-2 and rec_lambda < 2e-2, (name, rec_model, rec_lambda)
        return fwd.info(), figures
    finally:
        fwd.close()
        basis.close()
