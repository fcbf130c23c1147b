"""The exact posterior variance of linear inversion and kriging on the GPU: the row pass of
csrc/posterior_exact.hip through `gsi_mat_rowdot_acc`, bit for bit against tests/posterior_exact_model.py, and
`gsi_op_posterior_variance` / `posterior_variance_exact` against the longdouble reference from the dense matrices.  Cases,
bars and checks: tests/posterior_exact_cases.py; the inputs' fairness is asserted in
tests/test_posterior_exact_cpu.py::test_inputs_of_the_gpu_file_are_fair.
`POSTERIOR_EXACT_ERRORS=<path>`: the worst ratio to its bar per case is written there as JSON
(profiles/posterior_exact_errors.json)."""
import itertools
import json
import os

import numpy as np
import pytest

import fwd_cov_cases as fc
import posterior_exact_cases as pc
import posterior_exact_model as pm
import solve_cases as sc

pytestmark = pytest.mark.gpu

RATIOS = {}
BAR = "max |v - v_ref| <= max(4 x the float64 restatement's own error against the longdouble reference, 1e-12 C_00)"
# one sweep of the row pass's capped grid: 1024 workgroups of 256 lanes, two rows per lane with 16-byte loads (even n), one
# with 8-byte loads (odd n)
SWEEP_VEC, SWEEP_SCALAR = 1024 * 256 * 2, 1024 * 256


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("POSTERIOR_EXACT_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"bar": BAR, "largest_ratio_to_the_bar": RATIOS}, f, indent=1, sort_keys=True, default=float)
            f.write("\n")


@pytest.fixture(scope="module", params=list(fc.GRIDCOV))
def case(gsi, ctx, request):
    """(name, Ns, grid operator, dense C, dense H)"""
    name = request.param
    Ns = fc.GRIDCOV[name][0]
    gop = fc.gridcov_operator(gsi, ctx, name)
    yield name, Ns, gop, fc.gridcov_dense(name), fc.dense_H(Ns)
    gop.close()


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def _none(X):
    return X if X.shape[1] else None


# ---- the row pass alone, bit for bit -------------------------------------------------------------------------------------
def _rowdot_case(gsi, ctx, n, b, rng):
    Ah, Bh, a0 = rng.standard_normal((n, b)), rng.standard_normal((n, b)), rng.standard_normal((n, 1))
    A, B = gsi.DeviceMatrix.from_host(ctx, Ah), gsi.DeviceMatrix.from_host(ctx, Bh)
    try:
        for same in (False, True):
            want = pm.rowdot_acc(Ah, Ah if same else Bh, a0)
            for _ in range(2):                                          # two calls return the same bits
                acc = gsi.DeviceMatrix.from_host(ctx, a0)               # pre-filled with non-zeros
                assert gsi.mat_rowdot_acc(A, A if same else B, acc) is acc
                got = acc.to_host()[:, 0]
                acc.close()
                assert np.array_equal(got, want), (n, b, same, np.abs(got - want).max())
        assert np.array_equal(A.to_host(), Ah) and np.array_equal(B.to_host(), Bh)   # the panels are not written
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 1001])
def test_rowdot_bits(gsi, ctx, n, monkeypatch):
    """Every n at b below, at and above the column unroll of 8, B == A and B != A; even n: 16-byte loads, odd n: 8-byte."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    rng = np.random.default_rng([7, n])
    for b in (1, 7, 8, 9, 16, 17):
        _rowdot_case(gsi, ctx, n, b, rng)


@pytest.mark.parametrize("n", [SWEEP_VEC + 2, SWEEP_VEC + 514, SWEEP_SCALAR + 1, SWEEP_SCALAR + 257])
def test_rowdot_beyond_one_sweep_of_the_grid(gsi, ctx, n, monkeypatch):
    """n just beyond what the capped grid covers in one sweep, on both load widths: the grid-strided rows."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    _rowdot_case(gsi, ctx, n, 3, np.random.default_rng([8, n]))


def test_rowdot_is_exact_on_small_integers(gsi, ctx):
    rng = np.random.default_rng(9)
    for n, b in ((66, 9), (65, 17)):
        Ah = rng.integers(-8, 9, size=(n, b)).astype(np.float64)
        Bh = rng.integers(-8, 9, size=(n, b)).astype(np.float64)
        a0 = rng.integers(-8, 9, size=(n, 1)).astype(np.float64)
        A, B, acc = (gsi.DeviceMatrix.from_host(ctx, M) for M in (Ah, Bh, a0))
        try:
            gsi.mat_rowdot_acc(A, B, acc)
            gsi.mat_rowdot_acc(A, A, acc)                               # accumulates on top
            assert np.array_equal(acc.to_host()[:, 0], a0[:, 0] + (Ah * Bh).sum(axis=1) + (Ah * Ah).sum(axis=1))
        finally:
            for h in (A, B, acc):
                h.close()


def test_rowdot_refusals(gsi, ctx):
    A, B, acc, wide = (gsi.DeviceMatrix(ctx, 5, 3), gsi.DeviceMatrix(ctx, 5, 2), gsi.DeviceMatrix(ctx, 5, 1),
                       gsi.DeviceMatrix(ctx, 5, 2))
    try:
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(A, B, acc), "same shape")
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(B, B, wide), "acc is 5 x 2")
        sc.refused(gsi, lambda: gsi.mat_rowdot_acc(acc, acc, acc), "acc must not be A or B")
    finally:
        for h in (A, B, acc, wide):
            h.close()


# ---- the feature: a LinearDataOperator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pc.DRIFTS)
def test_variance_against_the_reference(gsi, ctx, case, which, monkeypatch):
    """The rays of fwd_cov_cases (nobs = 62) with noise 0.01: batch 2, 50 (a ragged last batch) and the default; a repeat
    returns the same bits; the host path agrees to the bar and reports path 3."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    name, Ns, gop, Cm, H = case
    nobs = H.shape[0]
    X = pc.drift(Ns, which)
    d = pc.full_noise(fc.NOISE, nobs)
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        key = f"{name} rays {which}"
        got = {}
        for batch in (2, 50, None):
            v, rep = gsi.posterior_variance_exact(op, fc.NOISE, _none(X), batch=batch, return_info=True)
            assert rep["path"] == "fused" and rep["column"] == 0, rep
            bw = nobs if batch is None else min(batch, nobs)
            assert rep["batch"] == bw and rep["batches"] == -(-nobs // bw), rep
            assert rep["adjoint_columns"] == nobs + X.shape[1] and rep["trapezoid_bytes"] == 8 * (2 * nobs + X.shape[1]) * nobs
            _record(key, pc.check(key, v, Cm, H, d, X))
            got[batch] = v
        assert np.array_equal(gsi.posterior_variance_exact(op, fc.NOISE, _none(X), batch=2), got[2])
        assert mdl.adjoint_info()["host_products"] == 0 and mdl.info()[6] == 0            # the kernels, not the host paths
        monkeypatch.setenv("GSI_POSTX_HOST", "1")
        vh, rep = gsi.posterior_variance_exact(op, fc.NOISE, _none(X), batch=50, return_info=True)
        assert rep["path"] == "composed", rep
        _record(key + " host path", pc.check(key, vh, Cm, H, d, X))
    finally:
        op.close()
        mdl.close()


@pytest.mark.parametrize("nobs", pc.SPARSE_NOBS)
def test_sparse_rows_across_the_cholesky_blocks(gsi, ctx, nobs, monkeypatch):
    """Random sparse H on (24, 20): nobs on both sides of the 64-column blocks of the factorization inside the doubled
    trapezoid; every drift; batch 50 is ragged at nobs = 129.  nobs = 1: one point sample, v_j = C_00 - C_00^2 / (C_00 + d)."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    gname = "exp-24x20"
    Ns = fc.GRIDCOV[gname][0]
    n = int(np.prod(Ns))
    Cm = fc.gridcov_dense(gname)
    csr = pc.sparse_csr(n, nobs)
    H = pc.dense_of(csr, n)
    noise = pc.fair_noise(H @ Cm @ H.T)
    d = pc.full_noise(noise, nobs)
    gop = fc.gridcov_operator(gsi, ctx, gname)
    mdl = gsi.LinearForwardModel((csr[0], csr[1], csr[2], (nobs, n)), ctx=ctx)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        for which in pc.DRIFTS:
            X = pc.drift(Ns, which)
            if nobs < X.shape[1]:
                continue                                               # fewer observations than drift functions: singular
            key = f"{gname} sparse nobs={nobs} {which}"
            for batch in (50, None):
                v, rep = gsi.posterior_variance_exact(op, noise, _none(X), batch=batch, return_info=True)
                assert rep["path"] == "fused"
                _record(key, pc.check(key, v, Cm, H, d, X))
            if nobs == 1 and which == "none":
                j, c00 = int(np.argmax(H[0])), Cm[0, 0]
                assert abs(v[j] - (c00 - c00 ** 2 / (c00 + noise))) <= pc.references(key, Cm, H, d, X)[1]
    finally:
        op.close()
        mdl.close()
        gop.close()


# ---- the feature: an FFTOperatorAt ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [20, 65])
def test_points_operator(gsi, ctx, case, m, monkeypatch):
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    name, Ns, gop, Cm, _ = case
    P, box, W = pc.at_dense(Ns, m)
    noise = pc.fair_noise(W @ Cm @ W.T)
    d = pc.full_noise(noise, m)
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    try:
        for which in pc.DRIFTS:
            X = pc.drift(Ns, which)
            key = f"{name} at {m} points {which}"
            for batch in (2, 50, None):
                v, rep = gsi.posterior_variance_exact(op, noise, _none(X), batch=batch, return_info=True)
                assert rep["path"] == "fused" and rep["batch"] == (m if batch is None else min(batch, m))
                _record(key, pc.check(key, v, Cm, W, d, X))
        monkeypatch.setenv("GSI_POSTX_HOST", "1")
        vh, rep = gsi.posterior_variance_exact(op, noise, _none(X), return_info=True)
        assert rep["path"] == "composed"
        _record(key + " host path", pc.check(key, vh, Cm, W, d, X))
    finally:
        op.close()


# ---- method="cg" -----------------------------------------------------------------------------------------------------------
def _cg_case(gsi, op, key, Cm, H, noise, Ns, batch, batches, with_precond):
    """`method="cg"` at tol = 1e-12 without a drift and with a constant one, against the dense matrices: the issue's bar,
    |v - v_ref| <= 2 tol |g_i|_1 |g_i|_2 / lambda_min(M) + the direct bar (`posterior_exact_cases.cg_extra`, `check`)."""
    tol = 1e-12
    d = pc.full_noise(noise, H.shape[0])
    extra = pc.cg_extra(Cm, H, d, tol)
    # (rank 16 with the default oversampling would sketch all 20 dimensions of the 20-point operator, and the range
    # finder's LU of a square panel meets a zero pivot: no oversampling where fewer than 16 dimensions are left)
    over = None if H.shape[0] >= 32 else 0
    pre = gsi.lowrank_preconditioner(op, rank=16, diag=noise, seed=3, p=over) if with_precond else None
    try:
        for which in ("none", "constant"):
            X = pc.drift(Ns, which)
            v, rep = gsi.posterior_variance_exact(op, noise, _none(X), method="cg", batch=batch, precond=pre, tol=tol,
                                                  return_info=True)
            assert rep["method"] == "cg" and rep["batches"] == batches and rep["products"] > 0
            _record(f"{key} {which} cg precond={with_precond}", pc.check(f"{key} {which}", v, Cm, H, d, X, extra=extra))
        with pytest.raises(ValueError, match="method='cg' only"):
            gsi.posterior_variance_exact(op, noise, method="cholesky", precond=pre, tol=tol)
    finally:
        if pre is not None:
            pre.close()


@pytest.mark.parametrize("with_precond", [False, True])
def test_cg_method(gsi, ctx, case, with_precond, monkeypatch):
    """The rays (a `LinearDataOperator`): the prior adjoint is the model's adjoint and the grid product, Phi the model's
    forward product; with and without a rank-16 preconditioner."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        _cg_case(gsi, op, f"{name} rays", Cm, H, fc.NOISE, Ns, 32, 2, with_precond)
    finally:
        op.close()
        mdl.close()


@pytest.mark.parametrize("with_precond", [False, True])
@pytest.mark.parametrize("m", [20, 65])
def test_cg_method_on_a_points_operator(gsi, ctx, case, m, with_precond, monkeypatch):
    """The same for an `FFTOperatorAt` with 20 and 65 points against the dense W C W': the prior adjoint is `FFTRF.spread` and
    the grid product, Phi the interpolation of the drift; batch 16 is ragged at both sizes."""
    monkeypatch.delenv("GSI_POSTX_HOST", raising=False)
    name, Ns, gop, Cm, _ = case
    P, box, W = pc.at_dense(Ns, m)
    noise = pc.fair_noise(W @ Cm @ W.T)
    op = gsi.fft_operator_at(ctx, gop, P, box=box)
    try:
        _cg_case(gsi, op, f"{name} at {m} points", Cm, W, noise, Ns, 16, -(-m // 16), with_precond)
    finally:
        op.close()


# ---- linear_inversion(..., variance=True) --------------------------------------------------------------------------------
def test_linear_inversion_with_variance(gsi, ctx, case):
    name, Ns, gop, Cm, H = case
    Xg = fc.drift_grid(Ns)
    y = np.random.default_rng(12).standard_normal(H.shape[0])
    mdl = fc.model(gsi, ctx, Ns)
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
    finally:
        mdl.close()


# ---- failures, refusals, lifetimes, memory ---------------------------------------------------------------------------------
def test_failures(gsi, ctx, case):
    name, Ns, gop, Cm, H = case
    nobs = H.shape[0]
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        d = np.full(nobs, fc.NOISE)
        d[0] = -10.0 * np.diag(H @ Cm @ H.T).max()
        with pytest.raises(gsi.GsiError) as e:
            gsi.posterior_variance_exact(op, d)
        assert e.value.code == 7 and "Cholesky failed at 1" in str(e.value)
        info = (gsi._lib.c_i64 * 8)()
        var = np.zeros(Cm.shape[0])
        st = ctx.lib.gsi_op_posterior_variance(ctx.h, op.h, gsi._lib.dptr(d), None, Cm.shape[0], 0, 0, gsi._lib.dptr(var), info)
        assert st == 7 and info[0] == 1 and info[1] == 1
        Xg = fc.drift_grid(Ns)
        with pytest.raises(gsi.GsiError) as e:
            gsi.posterior_variance_exact(op, fc.NOISE, np.column_stack([Xg[:, 1], Xg[:, 1]]))
        assert e.value.code == 3 and "linearly dependent" in str(e.value)
        assert np.isfinite(gsi.posterior_variance_exact(op, fc.NOISE)).all()             # a following valid call succeeds
    finally:
        op.close()
        mdl.close()


def test_refusals_and_memory(gsi, ctx):
    Ns = (6, 5)
    gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=[2.0, 2.0])
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        op.matmul(np.ones(mdl.nobs))                       # the model's inverted index is uploaded by the first product
        pc.refusals(gsi, ctx, op, 30, lambda: gsi.Context(0), gop)
        ctx.release_cache()
        before = ctx.device_bytes()
        v = gsi.posterior_variance_exact(op, 0.01, fc.drift_grid(Ns)[:, :1])
        ctx.release_cache()
        assert ctx.device_bytes() == before and np.isfinite(v).all()
    finally:
        op.close()
        mdl.close()
        gop.close()


def test_lifetimes(gsi, ctx):
    """The operator, the model and the grid operator destroyed in any order after the call."""
    Ns = (6, 5)
    for order in itertools.permutations(range(3)):
        gop = gsi.fft_gridcov_operator(ctx, list(Ns), kind="exponential", ell=[2.0, 2.0])
        mdl = fc.model(gsi, ctx, Ns)
        op = gsi.linear_data_operator(gop, mdl)
        v = gsi.posterior_variance_exact(op, 0.01)
        hs = [gop, mdl, op]
        for k in order:
            hs[k].close()
        assert np.isfinite(v).all()
