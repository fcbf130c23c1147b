"""`gsi_op_solve_trace` / `gsi_slq_quadrature` / `gsi_precond_sample` / `logdet` / `log_likelihood` on the device: the trace
kernels beside csrc/block_cg.hip and csrc/block_pcg.hip (path 1, "fused"), the quadrature kernel and the sampling pass of
csrc/block_slq.hip, under the checks of tests/logdet_cases.py; more columns than one block of the trace kernel has threads,
one size beyond a sweep of the sampling pass's grid, the composed leg in the same process, and the device memory account.
OP_LOGDET_ERRORS=<path>: the largest ratios seen, as profiles/op_logdet_errors.json."""
import json
import os

import numpy as np
import pytest

import logdet_cases as lc
import pcg_cases as pg
import solve_cases as sc

pytestmark = pytest.mark.gpu

PATH = "fused"


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    path = os.environ.get("OP_LOGDET_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"library": "device kernels (csrc/block_slq.hip), fused path",
                       "bars": {"quadrature": "max(4 x |float64 QL restatement - eigh|, 1e-13 x rho0 sum tau^2 |log lambda|)",
                                "sample, logdet_P": "4 x the float64 restatement's error, floor 1e-13",
                                "probes": "max(4 x the numpy restatement's error, 1e-12) x rho0",
                                "exact logdet": "1e-11 |slogdet|", "log_likelihood": "1e-10 relative"},
                       "largest_probe_ratio": max((v for k, v in lc.RATIOS.items() if k.startswith("probes")), default=0.0),
                       "ratios_to_the_bar": lc.RATIOS}, f, indent=1, sort_keys=True)
            f.write("\n")


def test_quadrature_alone(ctx):
    lc.quadrature_cases(ctx)


@pytest.mark.parametrize("n,K,b", pg.APPLY)
def test_sample_and_logdet_P(gsi, ctx, n, K, b):
    lc.sample_case(gsi, ctx, n, K, b)


def test_sample_beyond_one_sweep_of_the_grid(gsi, ctx):
    lc.sample_beyond_grid(gsi, ctx)


@pytest.mark.parametrize("n,b,diag,K", pg.DENSE)
def test_trace_is_passive(gsi, ctx, n, b, diag, K):
    lc.passive_case(gsi, ctx, n, b, diag, K, PATH)


@pytest.mark.parametrize("n,diag,K", lc.PROBE_CASES)
def test_probe_values(gsi, ctx, n, diag, K):
    lc.probe_values(gsi, ctx, n, diag, K, PATH)


def test_more_columns_than_threads_of_the_trace_block(gsi, ctx):
    """300 probes: the trace kernels' column loop makes a second trip (256 threads), the quadrature runs on 5 blocks."""
    lc.probe_values(gsi, ctx, 64, 0.1, 0, PATH, s=300, qmax=64)


@pytest.mark.parametrize("K", [0, 8])
def test_exact_logdet(gsi, ctx, K):
    lc.exact_logdet(gsi, ctx, K, PATH)


def test_truncation(gsi, ctx):
    lc.truncation(gsi, ctx, PATH)


@pytest.mark.parametrize("K", [0, 32])
def test_log_likelihood_dense(gsi, ctx, K):
    n = 257
    P = sc.points(n, 2, seed=n)
    op, d, A = pg.dense_inputs(gsi, ctx, n, 0.1)
    Z = pg.eig_basis(A, K) if K else None
    pc = gsi.lowrank_preconditioner(op, basis=Z, diag=d) if K else None
    try:
        lc.likelihood_case(gsi, ctx, op, P, 0.1, pc, lc.precond_factor(Z, K, d, 0.0, n), f"log_likelihood dense n={n} K={K}")
    finally:
        if pc is not None:
            pc.close()
        op.close()


def test_log_likelihood_pointcov_pivoted_cholesky(gsi, ctx):
    lc.likelihood_pivchol(gsi, ctx)


def test_same_seed_same_normals(gsi, ctx):
    lc.same_normals(gsi, ctx)


def test_composed_leg_and_poll_interval(gsi, ctx, monkeypatch):
    """The in-process A/B legs: the poll interval changes no bit of what the traced fused path returns, the quadrature values
    included; the composed path (trace kept on the host, the same quadrature kernel) passes the same bar."""
    op, d, pc, M, Z, Lp, Zp = lc.probe_setup(gsi, ctx, 257, 0.01, 32, s=5)
    try:
        st, X, info, relres, iters, quad = lc.raw_trace(ctx, op, d, pc, Zp, 5, 128, 1e-10)
        assert st == 0 and info[2] == 1
        for poll in ("1", "7"):
            monkeypatch.setenv("GSI_CG_POLL", poll)
            st2, X2, info2, relres2, iters2, quad2 = lc.raw_trace(ctx, op, d, pc, Zp, 5, 128, 1e-10)
            assert st2 == 0 and np.array_equal(X2, X) and np.array_equal(quad2, quad) and np.array_equal(iters2, iters)
    finally:
        pc.close()
        op.close()
    monkeypatch.setenv("GSI_CG_COMPOSED", "1")
    lc.probe_values(gsi, ctx, 257, 0.01, 32, "composed")


def test_refusals(gsi, ctx):
    lc.refusals(gsi, ctx, PATH)


def test_device_memory_returns(gsi, ctx):
    """After close() of everything the context holds what it held before (the second cycle is measured: the first fills the
    backend's cache of released blocks)."""
    def cycle():
        op, d, A = pg.dense_inputs(gsi, ctx, 257, "vec")
        pc = gsi.lowrank_preconditioner(op, rank=16, diag=d, seed=4)
        gsi.logdet(op, diag=d, precond=pc, probes=4, seed=1, qmax=32)
        gsi.log_likelihood(op, sc.rhs(257, 1)[:, 0], noise=d, precond=pc, probes=3)
        for h in (pc, op):
            h.close()
    cycle()
    before = ctx.device_bytes()
    cycle()
    assert ctx.device_bytes() == before
