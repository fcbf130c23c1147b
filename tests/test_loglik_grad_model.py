"""The dense models of the likelihood gradient check themselves, without a GPU: the analytic
derivative entries of tests/loglik_grad_model.py (the formulas of csrc/pointcov.hpp's `dkernel`) and the analytic REML / ML
gradient agree with Richardson-extrapolated central differences of the existing kernels and of the dense `slogdet`
likelihood; the same-probe estimator with Z = sqrt(m) I is the analytic gradient.

The bars are 10 x the agreement that was measured here (profiles/loglik_grad_errors.json, "model"; LOGLIK_GRAD_ERRORS=<path>
writes it): entries 9.8e-16 of max|entry| (longdouble, h = 2^-8), gradient 4.2e-13 of max|grad| (float64 `slogdet`, h = 2^-5), the estimator with unit probes 5.8e-15 of max|grad|."""
import numpy as np
import pytest

import loglik_grad_cases as lc
import loglik_grad_model as lm

LD = lm.LD
ENTRY_BAR = 1e-14          # 10 x 9.8e-16
GRAD_BAR = 5e-12           # 10 x 4.2e-13 (rounded up)
ESTIMATOR_BAR = 6e-14      # 10 x 5.8e-15
SHAPES = [((5,), (2.0,), 0.0), ((7, 5), (3.0, 1.5), 0.0), ((7, 5), (3.0, 1.5), 0.4), ((3, 4, 5), (3.0, 2.0, 4.0), 0.0),
          ((7, 5), (1.0, 0.8), 0.3)]
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _feature_present(gsi):
    """These files restate product code (csrc/pointcov.hpp's `dprofile`, csrc/bilinear_terms_host.hpp's order, the formulas of
    `log_likelihood_grad`): beside a library without it they check nothing, so they fail there."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "geostatinversion.jl_amd", "csrc")
    assert "dprofile" in open(os.path.join(csrc, "pointcov.hpp")).read()
    assert os.path.exists(os.path.join(csrc, "bilinear_terms_host.hpp"))
    for name in ("log_likelihood_grad", "fit_covariance", "mat_bilinear", "fft_gridcov_derivative"):
        assert name in gsi.__all__, name


def applicable(param, ndims):
    if param == "theta":
        return ndims == 2
    if param in ("log_ell0", "log_ell1", "log_ell2"):
        return int(param[-1]) < ndims
    return True


@pytest.fixture(scope="module", autouse=True)
def _write():
    yield
    lc.write_errors("model", MEASURED, {"entries_rel": ENTRY_BAR, "gradient_rel": GRAD_BAR, "estimator_rel": ESTIMATOR_BAR})


@pytest.mark.parametrize("kind", range(4))
def test_entries_against_differences_of_the_kernel(kind):
    worst = 0.0
    for Ns, ell, theta in SHAPES:
        for param in lm.PARAMS:
            if param == "nugget" or not applicable(param, len(Ns)):
                continue
            a = lm.dk_entries(Ns, kind, ell, theta, 1.7, param)
            f = lm.fd_entries(Ns, kind, ell, theta, 1.7, param, h=LD(1) / 256)
            scale = float(np.abs(a).max())
            if scale == 0.0:                 # theta with equal lengths and the like: identically zero
                assert float(np.abs(f).max()) < 1e-17
                continue
            worst = max(worst, float(np.abs(a - f).max()) / scale)
    print(f"kind {kind}: entries against Richardson differences, worst relative {worst:.2e}")
    MEASURED[f"entries_rel_kind{kind}"] = worst
    assert worst <= ENTRY_BAR


def test_nugget_and_special_entries():
    Ns, ell = (4, 3), (2.0, 2.0)
    n = 12
    for kind in range(4):
        assert np.array_equal(lm.dk_entries(Ns, kind, ell, 0.3, 1.7, "nugget"), np.eye(n))
        # equal lengths: the rotation does nothing, d / d theta = 0
        assert float(np.abs(lm.dk_entries(Ns, kind, ell, 0.3, 1.7, "theta")).max()) == 0.0
        # log_ell is the sum of the per-axis derivatives; log_sigma2 is the covariance
        tot = lm.dk_entries(Ns, kind, (2.0, 3.0), 0.3, 1.7, "log_ell")
        parts = sum(lm.dk_entries(Ns, kind, (2.0, 3.0), 0.3, 1.7, f"log_ell{a}") for a in range(2))
        assert float(np.abs(tot - parts).max()) <= 4 * np.finfo(LD).eps * float(np.abs(tot).max())
        assert np.array_equal(lm.dk_entries(Ns, kind, (2.0, 3.0), 0.3, 1.7, "log_sigma2"),
                              lm.cov_entries(Ns, kind, (2.0, 3.0), 0.3, 1.7, 0.0))
        # the entry at r = 0 is finite (0 for the length and angle derivatives)
        for param in ("log_ell", "log_ell0", "log_ell1", "theta"):
            d = np.diag(lm.dk_entries(Ns, kind, (2.0, 3.0), 0.3, 1.7, param))
            assert np.all(d == 0.0), (kind, param)


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("restricted", [True, False])
def test_gradient_against_differences_of_the_slogdet_likelihood(p, restricted):
    c = lc.dense_case(p)
    ga = lm.loglik_grad(c["M"], c["dMs"], c["y"], c["G"], restricted)
    gf = []
    for k in range(3):
        def f(v, k=k):
            x = c["x0"].copy()
            x[k] = v
            return lm.loglik(lc.dense_M(c, x), c["y"], c["G"], restricted)
        gf.append(lm.richardson(f, c["x0"][k], 1.0 / 32))
    rel = float(np.abs(np.array(gf) - ga).max() / np.abs(ga).max())
    print(f"p = {p}, restricted = {restricted}: analytic against differenced gradient, relative {rel:.2e}")
    MEASURED[f"gradient_rel_p{p}_{'reml' if restricted else 'ml'}"] = rel
    assert rel <= GRAD_BAR


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("restricted", [True, False])
def test_same_probe_estimator_with_unit_probes_is_the_gradient(p, restricted):
    c = lc.dense_case(p)
    m = c["y"].size
    S, T, X = lm.same_probe_terms(c["M"], c["dMs"], c["y"], c["G"], np.sqrt(m) * np.eye(m))
    got = lm.grad_from_terms(S, T, X, c["y"], c["G"], restricted)
    want = lm.loglik_grad(c["M"], c["dMs"], c["y"], c["G"], restricted)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"p = {p}, restricted = {restricted}: estimator with Z = sqrt(m) I against the analytic gradient, relative {rel:.2e}")
    MEASURED[f"estimator_rel_p{p}_{'reml' if restricted else 'ml'}"] = rel
    assert rel <= ESTIMATOR_BAR


def test_random_probes_estimate_the_trace_within_their_standard_error():
    c = lc.dense_case(2)
    m = c["y"].size
    Z = np.random.default_rng(5).standard_normal((m, 400))
    _, T, _ = lm.same_probe_terms(c["M"], c["dMs"], c["y"], c["G"], Z)
    for k, dM in enumerate(c["dMs"]):
        tr = float(np.trace(np.linalg.solve(c["M"], dM)))
        se = float(np.std(T[k], ddof=1) / np.sqrt(T.shape[1]))
        assert abs(float(np.mean(T[k])) - tr) <= 4.0 * se, (k, tr, float(np.mean(T[k])), se)
