"""`log_likelihood_grad`, `covariance_family` and `fit_covariance` on the MI355X.  Cases, bars and
checks: tests/loglik_grad_cases.py (the bars are first-order bounds formed from dense matrices and the reported `relres`).
  * dense A and dense dA (37 points, p = 0 and 2, 5 host-given probes, with and without a rank-6 preconditioner): S_k and
    t_{k,i} against the dense same-probe quantities; the value equals `log_likelihood` bit for bit; a NULL operator with
    `dnoise` is the noise derivative;
  * the same through `fft_operator_at` (8 x 6 grid read at 30 points) and `linear_data_operator` (20 rows), with the operators
    of a `covariance_family`;
  * Z = sqrt(m) I: the gradient against the analytic dense REML and ML gradients under the summed bound;
  * one fit: a 16 x 12 exponential grid at 60 points, data drawn at ell = 4, sigma2 = 2, started at ell = 1.5, sigma2 = 1.
LOGLIK_GRAD_ERRORS=<path>: the ratios to the bars are merged into that JSON file (profiles/loglik_grad_errors.json)."""
import numpy as np
import pytest

import loglik_grad_cases as lc

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module")
def ctx(gsi):
    yield gsi.default_context()
    lc.write_errors("gpu_ratio_to_bar", RATIOS)


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("with_precond", [False, True])
def test_dense_terms(gsi, ctx, p, with_precond, monkeypatch):
    monkeypatch.delenv("GSI_BILINEAR_HOST", raising=False)
    lc.run_dense_terms(gsi, ctx, p, with_precond, _record, "gpu")


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("restricted", [True, False])
def test_dense_gradient_with_unit_probes(gsi, ctx, p, restricted):
    lc.run_dense_gradient(gsi, ctx, p, restricted, _record, "gpu")


@pytest.mark.parametrize("which", ["at", "linear"])
@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("with_precond", [False, True])
def test_fft_terms(gsi, ctx, which, p, with_precond):
    lc.run_fft_terms(gsi, ctx, which, p, with_precond, _record)


def test_host_path_of_the_reduction_gives_the_same_gradient_bits(gsi, ctx, monkeypatch):
    case = lc.dense_case(2)
    Z = lc.probes(lc.N_DENSE, lc.S_PROBES)
    op, dops = lc._dense_ops(gsi, ctx, case)
    try:
        out = []
        for host in (False, True):
            if host:
                monkeypatch.setenv("GSI_BILINEAR_HOST", "1")
            else:
                monkeypatch.delenv("GSI_BILINEAR_HOST", raising=False)
            out.append(gsi.log_likelihood_grad(op, dops, case["y"], noise=case["noise"], dnoise=case["dnoise"], drift=case["G"],
                                               probes=Z, tol=lc.TOL))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    finally:
        lc._close([op] + dops)


def test_refusals(gsi, ctx):
    lc.run_term_refusals(gsi, ctx)


def test_fit(gsi, ctx):
    fc = lc.fit_case()
    m = fc["y"].size
    fam = gsi.covariance_family(ctx, lc.FIT_NS, "exponential", points=fc["points"], box=fc["box"])
    try:
        before = None
        params, report = gsi.fit_covariance(fam, dict(lc.FIT_START), fc["y"], fc["noise"], wrt=("log_sigma2", "log_ell"),
                                            probes=np.sqrt(m) * np.eye(m), gtol=lc.FIT_GTOL, tol=1e-10)
        ratio = lc.check_fit(report, params, fc)
        _record("fit dense |g| ratio (bar 1e-3)", ratio)
        assert report["evaluations"] >= len(report["trace"]) and set(params) >= {"log_sigma2", "log_ell"}
        for t in report["trace"]:
            assert set(t) == {"params", "value", "grad", "stderr"}
    finally:
        fam.close()
