"""The operator H C H' of a linear forward model on the GPU (`gsi_op_fwd_cov`, `linear_data_operator`) and the linear
inversion built on it (`linear_inversion`, `estimate_field`, `condition_on_linear_data`); DESIGN.md 4.6l.  Cases, bars and
checks: tests/fwd_cov_cases.py; the inputs' fairness (numpy's own CG ends within 1 tol on every solve case here) is asserted
in tests/test_fwd_cov_cpu.py::test_inputs_of_the_gpu_file_are_fair.
`FWD_COV_ERRORS=<path>`: the measured ratios to the bars are written there as JSON (profiles/fwd_cov_errors.json)."""
import json
import os

import numpy as np
import pytest

import fftrf_interp_model as im
import fwd_adjoint_model as fm
import fwd_cov_cases as fc
import interp_adjoint_model as am
import logdet_cases as lc
import solve_cases as sc

pytestmark = pytest.mark.gpu

PATH = "fused"
RATIOS = {}
BARS = {"operator_err_over_1e-12_scale": "max |Y - H C H' X| <= 1e-12 max |Y_ref| against the dense matrix",
        "interp_as_csr_err_over_2e-12_scale": "H = W as CSR: max |Y - Y_fft_operator_at| <= 2e-12 max |Y|",
        "solve": "solve_cases.check_solve: true relative residual <= 2 tol, solution error <= kappa (rho + rho_ref)",
        "log_likelihood_probe_over_bar": "logdet_cases.probe_values' bar per probe"}


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("FWD_COV_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"bars": BARS, "largest_ratio_to_its_bar": RATIOS, "solves": sc.RATIOS}, f, indent=1, sort_keys=True, default=float)
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


def test_operator_products(gsi, ctx, case, monkeypatch):
    name, Ns, gop, Cm, H = case
    monkeypatch.delenv("GSI_FWD_HOST", raising=False)
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        assert isinstance(op, gsi.LinearDataOperator) and H.shape[0] == 62
        _record("operator_err_over_1e-12_scale", fc.products(gsi, op, H @ Cm @ H.T, name, monkeypatch))
        ai = mdl.adjoint_info()
        assert ai["built"] and ai["host_products"] == 0 and mdl.info()[6] == 0          # the kernels, not the host paths
    finally:
        op.close()
        mdl.close()


def test_operator_with_weights_and_phases(gsi, ctx, case):
    name, Ns, gop, Cm, _ = case
    w = fm.weights(int(np.prod(Ns)))
    H = fc.dense_H(Ns, w)
    mdl = fc.model(gsi, ctx, Ns, w)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        X = np.random.default_rng(9).standard_normal((H.shape[0], 5))
        ctx.profile(1)
        ctx.phase_reset()
        Y = op.matmul(X)
        ph = ctx.phase_times()
        ctx.profile(0)
        _record("operator_err_over_1e-12_scale", fc.close(Y, H @ (Cm @ (H.T @ X)), f"{name} weighted"))
        for phase in ("gemm_t", "gemm_n", "other"):                                       # adjoint, grid product, forward
            assert ph[phase][1] >= 1 and ph[phase][0] > 0.0, ph
    finally:
        ctx.profile(0)
        op.close()
        mdl.close()


@pytest.mark.parametrize("Ns", [(24, 20), (6, 4, 5)], ids=im.gid)
def test_interpolation_as_a_csr_model(gsi, ctx, Ns):
    """H = W, the interpolation matrix of `fft_operator_at`, as CSR (weights from interp_adjoint_model): the two operators
    agree within 2e-12 max|Y| -- each is within 1e-12 of the exact product."""
    import scipy.sparse as sp
    m = 257
    P = im.scattered_points(Ns, m, seed=19)
    box = im.inner_box(P, shrink=0.05)
    base, frac = im.plan(P, Ns, box)
    W = sp.csr_matrix(am.weights_matrix(Ns, base, frac))
    name = "exp-24x20" if len(Ns) == 2 else "exp-6x4x5"
    gop = fc.gridcov_operator(gsi, ctx, name)
    at = gsi.fft_operator_at(ctx, gop, P, box=box)
    mdl = gsi.LinearForwardModel(W, ctx=ctx)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        for l in (1, 8):
            X = np.random.default_rng([m, l]).standard_normal((m, l))
            Y, Yat = op.matmul(X), at.matmul(X)
            ratio = np.abs(Y - Yat).max() / np.abs(Yat).max() / 2e-12
            print(f"{im.gid(Ns)} l={l}: max|Y - Y_at| / max|Y| = {ratio * 2e-12:.2e}")
            _record("interp_as_csr_err_over_2e-12_scale", ratio)
            assert ratio < 1.0
    finally:
        for h in (op, mdl, at, gop):
            h.close()


def test_solve_plain_and_preconditioned(gsi, ctx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        A = H @ Cm @ H.T
        rep = fc.solve_case(gsi, op, A, f"fwd_cov {name}", PATH)
        pc = gsi.lowrank_preconditioner(op, rank=16, diag=fc.NOISE, seed=3)
        try:
            assert pc.rank == 16
            rep_pc = fc.solve_case(gsi, op, A, f"fwd_cov {name} rank 16", PATH, precond=pc)
            print(f"{name}: iterations {rep['iters'].max()} plain, {rep_pc['iters'].max()} with a rank-16 preconditioner")
        finally:
            pc.close()
    finally:
        op.close()
        mdl.close()


def test_log_likelihood_probe_values(gsi, ctx, case):
    """`log_likelihood` on the operator with 8 explicit probes at tol 1e-10: each probe's value within logdet_cases' bar,
    max(4 x the numpy restatement's error on that probe, 1e-12) rho0, of u' log(M) u from eigh of the dense M."""
    name, Ns, gop, Cm, H = case
    nobs = H.shape[0]
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        M = H @ Cm @ H.T + fc.NOISE * np.eye(nobs)
        Zp = sc.rhs(nobs, 8, seed=900)
        y = np.random.default_rng(12).standard_normal(nobs)
        val, info = gsi.log_likelihood(op, y, noise=fc.NOISE, probes=Zp, tol=1e-10, return_info=True)
        assert np.isfinite(val) and info["path"] == PATH and info["truncated"] == 0
        want, rho0 = lc.dense_form(M, np.eye(nobs), Zp)
        model = np.zeros(8)
        for j in range(8):
            al, be, r0 = lc.pcg_trace(0.5 * (M + M.T), Zp[:, j].copy(), None, 1e-10, 10 * nobs)
            model[j] = lc.gauss_eigh(al, be, len(al), r0)[0]
        bar = np.maximum(4.0 * np.abs(model - want) / rho0, 1e-12) * rho0
        err = np.abs(info["values"] - want)
        print(f"{name}: per-probe error / bar = {(err / bar).max():.3f}")
        _record("log_likelihood_probe_over_bar", (err / bar).max())
        assert (err <= bar).all(), err / bar
        # the value: the dense formula with the exact per-probe forms; the quadratic form y'M^-1 y from a column whose true
        # residual is at most 2 tol |y| is off by at most |y| |M^-1| 2 tol |y|
        ref, _, _ = lc.dense_likelihood(M, np.zeros((nobs, 0)), y, float(np.mean(want)), True)
        qbar = 2e-10 * float(y @ y) * np.linalg.norm(np.linalg.inv(M), 2)
        assert abs(val - ref) <= 0.5 * (qbar + float(np.mean(bar))) + 1e-13 * abs(ref)
    finally:
        op.close()
        mdl.close()


def test_linear_inversion(gsi, ctx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, ctx, Ns)
    try:
        fc.inversion(gsi, gop, mdl, H, Cm, f"linear_inversion {name}")
    finally:
        mdl.close()


def test_condition_on_linear_data(gsi, ctx, case):
    name, Ns, gop, Cm, H = case
    mdl = fc.model(gsi, ctx, Ns)
    op = gsi.linear_data_operator(gop, mdl)
    try:
        fc.conditioning(gsi, op, H, Cm, f"conditioning {name}")
    finally:
        op.close()
        mdl.close()


def test_refusals(gsi, ctx, monkeypatch):
    gop = gsi.fft_gridcov_operator(ctx, [6, 5], kind="gaussian", ell=2.0)
    try:
        fc.refusals(gsi, ctx, gop, lambda: gsi.Context(0))
    finally:
        gop.close()
    # a context with a communicator (one rank, threads-of-one-process communicator)
    monkeypatch.setenv("GSI_LOCAL_COMM", "1")
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0)
    try:
        cc.comm_init(1, 0, cc.unique_id())
        g2 = gsi.fft_gridcov_operator(cc, [6, 5], kind="gaussian", ell=2.0)
        m2 = fc.model(gsi, cc, (6, 5))
        sc.refused(gsi, lambda: gsi.linear_data_operator(g2, m2), "communicator")
        m2.close()
        g2.close()
    finally:
        cc.close()


def test_lifetimes(gsi, ctx):
    make = lambda: gsi.fft_gridcov_operator(ctx, [6, 5], kind="gaussian", ell=2.0)
    g, m = make(), fc.model(gsi, ctx, (6, 5))                  # (a first cycle: whatever workspace the products cache exists from here on)
    o = gsi.linear_data_operator(g, m)
    o.matmul(np.ones(m.nobs))
    for h in (o, m, g):
        h.close()
    ctx.release_cache()
    before = ctx.device_bytes()
    fc.lifetimes(gsi, ctx, make, (6, 5))
    ctx.release_cache()
    assert ctx.device_bytes() == before           # plan, model, inverted index: all returned
