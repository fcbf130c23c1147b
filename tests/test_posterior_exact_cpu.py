"""The exact posterior variance of linear inversion on the CPU reference library: the host path of
`gsi_op_posterior_variance` and `gsi_mat_rowdot_acc` (csrc/posterior_exact_host.hpp, saddle_host.hpp's factorization) under
pcga.cpp's driver, with `fft_powerlaw_operator` as C (that backend has no grid-covariance plan and no resident interpolation
plan, so the grid-covariance cases and the `FFTOperatorAt` cases run in tests/test_posterior_exact_gpu.py only).  Cases, bars
and checks: tests/posterior_exact_cases.py, tests/posterior_exact_model.py.  The inputs of both files are checked for
fairness here, from the dense matrices."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import fwd_cov_cases as fc
import posterior_exact_cases as pc
import posterior_exact_model as pm
import solve_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


@pytest.fixture(scope="module", params=list(fc.POWERLAW))
def case(gsi, cx, request):
    """(name, Ns, grid operator, its dense matrix, dense H)"""
    Ns, beta = fc.POWERLAW[request.param]
    gop = gsi.fft_powerlaw_operator(cx, list(Ns), beta)
    n = int(np.prod(Ns))
    Cm = gop.matmul(np.eye(n))                     # existing code, not under test here
    yield request.param, Ns, gop, 0.5 * (Cm + Cm.T), fc.dense_H(Ns)
    gop.close()


def test_exported(gsi):
    for name in ("posterior_variance_exact", "mat_rowdot_acc"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    for name in ("gsi_op_posterior_variance", "gsi_mat_rowdot_acc"):
        assert name in gsi._lib.SIGNATURES, name


# ---- the numpy models themselves ---------------------------------------------------------------------------------------
def test_model_rowdot_is_sequential():
    """The model rounds after every product and every sum: a case where fused or pairwise evaluation gives other bits."""
    A = np.array([[1.0 + 2.0 ** -30, 1.0, 1.0]])
    B = np.array([[1.0 - 2.0 ** -30, 2.0 ** -53, 2.0 ** -53]])
    out = pm.rowdot_acc(A, B, np.array([-1.0]))
    # -1 + fl((1 + e)(1 - e)) = -1 + 1 = 0 (the product rounds to 1); then 2^-53 twice, one at a time
    assert out[0] == 2.0 ** -52
    assert pm.rowdot_acc(A[:, :0], B[:, :0], np.array([3.0]))[0] == 3.0


def test_model_restatement_against_the_reference():
    """The float64 restatement agrees with the longdouble reference to rounding, with and without a drift, and for one
    point sample without a drift v_j = C_00 - C_00^2 / (C_00 + d)."""
    Ns = (6, 5)
    n = 30
    Cm = fc.dense_matrix(Ns, 1, (2.0, 2.0), 0.0, 1.3, 0.0)
    H = pc.dense_of(pc.sparse_csr(n, 7), n)
    d = np.full(7, 0.05)
    for which in pc.DRIFTS:
        X = pc.drift(Ns, which)
        ref = pm.reference(Cm, H, d, X)
        assert np.abs(pm.restatement(Cm, H, d, X).astype(pm.LD) - ref).max() < 1e-13
        # the defining formula through the full inverse, in float64
        M = H @ Cm @ H.T + np.diag(d)
        G = Cm @ H.T
        v = np.diag(Cm) - np.einsum("ij,ij->i", G @ np.linalg.inv(M), G)
        if X.shape[1]:
            Phi = H @ X
            Mi = np.linalg.inv(M)
            R = X - G @ Mi @ Phi
            v = v + np.einsum("ij,ij->i", R @ np.linalg.inv(Phi.T @ Mi @ Phi), R)
        assert np.abs(v - ref.astype(np.float64)).max() < 1e-11
    H1 = pc.dense_of(pc.sparse_csr(n, 1), n)
    j = int(np.argmax(H1[0]))
    ref = pm.reference(Cm, H1, np.array([0.05]), pc.drift(Ns, "none"))
    assert abs(float(ref[j]) - (1.3 - 1.3 ** 2 / (1.3 + 0.05))) < 1e-15


# ---- fairness of the inputs of this file and of the GPU file -----------------------------------------------------------
def test_inputs_are_fair(case):
    name, Ns, _, Cm, H = case
    fc.fair(name, H @ Cm @ H.T + fc.NOISE * np.eye(H.shape[0]))


@pytest.mark.parametrize("gname", list(fc.GRIDCOV))
def test_inputs_of_the_gpu_file_are_fair(gname):
    """The rays with noise 0.01, the sparse rows and the scattered points with `fair_noise`: cond(M) of order 10^3 and numpy's
    own CG ends within 1 tol."""
    Ns = fc.GRIDCOV[gname][0]
    n = int(np.prod(Ns))
    Cm = fc.gridcov_dense(gname)
    H = fc.dense_H(Ns)
    fc.fair(gname, H @ Cm @ H.T + fc.NOISE * np.eye(H.shape[0]))
    for m in (20, 65):
        W = pc.at_dense(Ns, m)[2]
        A = W @ Cm @ W.T
        M = A + pc.fair_noise(A) * np.eye(m)
        assert np.linalg.cond(M) < 5e3
        fc.fair(f"{gname} at {m} points", M)
    if gname == "exp-24x20":
        for nobs in pc.SPARSE_NOBS:
            Hs = pc.dense_of(pc.sparse_csr(n, nobs), n)
            A = Hs @ Cm @ Hs.T
            M = A + pc.fair_noise(A) * np.eye(nobs)
            assert np.linalg.cond(M) < 5e3
            fc.fair(f"{gname} sparse nobs={nobs}", M)


# ---- the row pass through gsi_mat_rowdot_acc (the host implementation) ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_rowdot_bits(gsi, cx, n):
    rng = np.random.default_rng([5, n])
    for b in (1, 7, 8, 9, 17):
        Ah, Bh, a0 = rng.standard_normal((n, b)), rng.standard_normal((n, b)), rng.standard_normal((n, 1))
        A, B = gsi.DeviceMatrix.from_host(cx, Ah), gsi.DeviceMatrix.from_host(cx, Bh)
        try:
            for same in (False, True):
                acc = gsi.DeviceMatrix.from_host(cx, a0)
                assert gsi.mat_rowdot_acc(A, A if same else B, acc) is acc
                got = acc.to_host()[:, 0]
                acc.close()
                assert np.array_equal(got, pm.rowdot_acc(Ah, Ah if same else Bh, a0)), (n, b, same)
        finally:
            A.close()
            B.close()


def test_rowdot_refusals(gsi, cx):
    A, B, acc, wide = (gsi.DeviceMatrix(cx, 5, 3), gsi.DeviceMatrix(cx, 5, 2), gsi.DeviceMatrix(cx, 5, 1), gsi.DeviceMatrix(cx, 5, 2))
    try:
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(A, B, acc), "same shape")
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(B, B, wide), "acc is 5 x 2")
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(acc, acc, acc), "acc must not be A or B")
    finally:
        for h in (A, B, acc, wide):
            h.close()


# ---- the feature on the host path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pc.DRIFTS)
def test_variance_against_the_reference(gsi, cx, case, which):
    name, Ns, gop, Cm, H = case
    nobs = H.shape[0]
    X = pc.drift(Ns, which)
    d = pc.full_noise(fc.NOISE, nobs)
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        got = {}
        for batch in (2, 50, None):
            v, rep = gsi.posterior_variance_exact(op, fc.NOISE, X if which != "none" else None, batch=batch, return_info=True)
            assert rep["path"] == "composed" and rep["column"] == 0                      # the host path: info_out[1] = 3
            bw = nobs if batch is None else min(batch, nobs)
            assert rep["batch"] == bw and rep["batches"] == -(-nobs // bw), rep
            assert rep["adjoint_columns"] == nobs + X.shape[1] and rep["trapezoid_bytes"] == 8 * (2 * nobs + X.shape[1]) * nobs
            pc.check(f"{name} {which} batch={batch}", v, Cm, H, d, X)
            got[batch] = v
        v2 = gsi.posterior_variance_exact(op, fc.NOISE, X if which != "none" else None, batch=2)
        assert np.array_equal(v2, got[2])                                                # a repeat returns the same bits
    finally:
        op.close()
        mdl.close()


@pytest.fixture(scope="module")
def sparse_grid(gsi, cx):
    """(Ns, grid operator, its dense matrix) of the sparse-row cases: the 12 x 10 power-law grid."""
    Ns, beta = fc.POWERLAW["powerlaw-12x10"]
    gop = gsi.fft_powerlaw_operator(cx, list(Ns), beta)
    Cm = gop.matmul(np.eye(int(np.prod(Ns))))
    yield Ns, gop, 0.5 * (Cm + Cm.T)
    gop.close()


@pytest.mark.parametrize("nobs", pc.SPARSE_NOBS)
def test_sparse_rows_across_the_cholesky_blocks(gsi, cx, sparse_grid, nobs):
    """Random sparse H with nobs on both sides of the 64-column blocks, on the host path: the assembly and the factorization
    of the doubled trapezoid on the host, the upload back; every drift that is not singular; batch 50 is ragged at
    nobs = 129.  nobs = 1: one point sample, v_j = C_00 - C_00^2 / (C_00 + d)."""
    Ns, gop, Cm = sparse_grid
    n = int(np.prod(Ns))
    csr = pc.sparse_csr(n, nobs)
    H = pc.dense_of(csr, n)
    noise = pc.fair_noise(H @ Cm @ H.T)
    d = pc.full_noise(noise, nobs)
    mdl = gsi.LinearForwardModel((csr[0], csr[1], csr[2], (nobs, n)), ctx=cx)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        for which in pc.DRIFTS:
            X = pc.drift(Ns, which)
            if nobs < X.shape[1]:
                continue                                               # fewer observations than drift functions: singular
            key = f"powerlaw sparse nobs={nobs} {which}"
            for batch in (50, None):
                v, rep = gsi.posterior_variance_exact(op, noise, X if X.shape[1] else None, batch=batch, return_info=True)
                bw = nobs if batch is None else min(batch, nobs)
                assert rep["path"] == "composed" and rep["batch"] == bw and rep["batches"] == -(-nobs // bw), rep
                pc.check(key, v, Cm, H, d, X)
            if nobs == 1 and which == "none":                          # one point sample of cell j
                j, c00 = int(np.argmax(H[0])), Cm[0, 0]
                assert abs(v[j] - (c00 - c00 ** 2 / (c00 + noise))) <= pc.references(key, Cm, H, d, X)[1]
    finally:
        op.close()
        mdl.close()


def test_sparse_inputs_are_fair(sparse_grid):
    Ns, _, Cm = sparse_grid
    n = int(np.prod(Ns))
    for nobs in pc.SPARSE_NOBS:
        H = pc.dense_of(pc.sparse_csr(n, nobs), n)
        A = H @ Cm @ H.T
        fc.fair(f"powerlaw sparse nobs={nobs}", A + pc.fair_noise(A) * np.eye(nobs))


def test_linear_inversion_with_variance(gsi, cx, case):
    name, Ns, gop, Cm, H = case
    Xg = fc.drift_grid(Ns)
    y = np.random.default_rng(12).standard_normal(H.shape[0])
    mdl = fc.model(gsi, cx, Ns)
    try:
        plain = gsi.linear_inversion(gop, mdl, y, fc.NOISE, drift_grid=Xg, tol=sc.TOL)
        withv = gsi.linear_inversion(gop, mdl, y, fc.NOISE, drift_grid=Xg, tol=sc.TOL, variance=True)
        assert len(plain) == 3 and len(withv) == 4
        for a, b in zip(plain, withv[:3]):
            assert np.array_equal(a, b)
        op = gsi.linear_data_operator(gop, mdl)
        try:
            assert np.array_equal(withv[3], gsi.posterior_variance_exact(op, fc.NOISE, Xg))
        finally:
            op.close()
        info = gsi.linear_inversion(gop, mdl, y, fc.NOISE, tol=sc.TOL, variance=True, return_info=True)
        assert len(info) == 5 and isinstance(info[3], dict) and info[4].shape == (Cm.shape[0],)
    finally:
        mdl.close()


def test_cg_method(gsi, cx):
    """`method="cg"` at tol = 1e-12: |v - v_ref| <= 2 tol |g_i|_1 |g_i|_2 / lambda_min(M) + the direct bar -- the solver's
    2 tol true-residual guarantee per unit column carried through g_i'M^-1 g_i, from the dense matrices (`posterior_exact_cases.cg_extra`), without a drift and
    with a constant one.  12 sparse rows on a 6 x 5 grid: this library's solver runs column by
    column on the host."""
    Ns, nobs, tol = (6, 5), 12, 1e-12
    n = int(np.prod(Ns))
    gop = gsi.fft_powerlaw_operator(cx, list(Ns), -3.5)
    Cm = gop.matmul(np.eye(n))
    Cm = 0.5 * (Cm + Cm.T)
    csr = pc.sparse_csr(n, nobs)
    H = pc.dense_of(csr, n)
    noise = pc.fair_noise(H @ Cm @ H.T)
    d = pc.full_noise(noise, nobs)
    M = H @ Cm @ H.T + np.diag(d)
    fc.fair("cg case", M)
    extra = pc.cg_extra(Cm, H, d, tol)
    mdl = gsi.LinearForwardModel((csr[0], csr[1], csr[2], (nobs, n)), ctx=cx)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        for which in ("none", "constant"):
            X = pc.drift(Ns, which)
            v, rep = gsi.posterior_variance_exact(op, noise, X if X.shape[1] else None, method="cg", batch=5, tol=tol,
                                                  return_info=True)
            assert rep["method"] == "cg" and rep["batches"] == 3 and rep["products"] > 0
            pc.check(f"cg 6x5 {which}", v, Cm, H, d, X, extra=extra)
        with pytest.raises(ValueError, match="method='cg' only"):
            gsi.posterior_variance_exact(op, noise, method="cholesky", tol=tol)
        with pytest.raises(ValueError, match="method must be"):
            gsi.posterior_variance_exact(op, noise, method="lu")
    finally:
        op.close()
        mdl.close()
        gop.close()


def test_failures(gsi, cx, case):
    name, Ns, gop, Cm, H = case
    nobs = H.shape[0]
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        d = np.full(nobs, fc.NOISE)
        d[0] = -10.0 * np.diag(H @ Cm @ H.T).max()
        with pytest.raises(gsi.GsiError) as e:
            gsi.posterior_variance_exact(op, d)
        assert e.value.code == 7 and "Cholesky failed at 1" in str(e.value)
        Xg = fc.drift_grid(Ns)
        with pytest.raises(gsi.GsiError) as e:
            gsi.posterior_variance_exact(op, fc.NOISE, np.column_stack([Xg[:, 1], Xg[:, 1]]))
        assert e.value.code == 3 and "linearly dependent" in str(e.value)
    finally:
        op.close()
        mdl.close()


def test_refusals_and_memory(gsi, cx):
    Ns = (6, 5)
    gop = gsi.fft_powerlaw_operator(cx, list(Ns), -3.5)
    mdl = fc.model(gsi, cx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        op.matmul(np.ones(mdl.nobs))                       # the model's inverted index is built by the first product
        pc.refusals(gsi, cx, op, 30, lambda: gsi.Context(0, lib=cx.lib), gop)
        cx.release_cache()
        before = cx.device_bytes()
        v = gsi.posterior_variance_exact(op, 0.01, fc.drift_grid(Ns)[:, :1])
        cx.release_cache()
        assert cx.device_bytes() == before and np.isfinite(v).all()
    finally:
        op.close()
        mdl.close()
        gop.close()


_KEEP = []


def test_refuses_a_communicator(gsi, monkeypatch):
    """An operator made before its context got a communicator: the variance is refused by name."""
    lib = cpuref.load_cpuref()
    cbs = (cpuref.ALLREDUCE_FN(lambda buf, count: None),
           cpuref.ALLGATHER_FN(lambda send, recv, count: [recv.__setitem__(i, send[i]) for i in range(count)] and None))
    _KEEP.extend(cbs)                      # the library keeps the pointers
    lib.gsi_cpuref_set_collectives(*cbs)
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0, lib=lib)
    try:
        gop = gsi.fft_powerlaw_operator(cc, [6, 5], -3.5)
        mdl = fc.model(gsi, cc, (6, 5))
        op = gsi.linear_data_operator(gop, mdl)
        cc.comm_init(1, 0, b"\0" * 128)
        sc.refused(gsi, lambda: gsi.posterior_variance_exact(op, 0.01), "communicator")
        op.close()
        mdl.close()
        gop.close()
    finally:
        cc.close()


def test_lifetimes(gsi, cx):
    """The operator, the model and the grid operator destroyed in any order after the call."""
    import itertools
    Ns = (6, 5)
    for order in itertools.permutations(range(3)):
        gop = gsi.fft_powerlaw_operator(cx, list(Ns), -3.5)
        mdl = fc.model(gsi, cx, Ns)
        op = gsi.linear_data_operator(gop, mdl)
        v = gsi.posterior_variance_exact(op, 0.01)
        hs = [gop, mdl, op]
        for k in order:
            hs[k].close()
        assert np.isfinite(v).all()


def test_host_code_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host-path check"
    exe = str(tmp_path / "posterior_exact_host_check")
    src = os.path.join(ROOT, "tests", "posterior_exact_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "posterior exact host ok" in r.stdout
