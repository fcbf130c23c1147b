"""`log_likelihood_grad` on the CPU reference library: dense A and dense dA (37 scattered points,
p = 0 and 2, 5 host-given probes, with and without a rank-6 preconditioner) through `gsi_op_solve_trace`,
`gsi_precond_apply` and `gsi_op_bilinear_terms` on the host path.  S_k and t_{k,i} against the dense same-probe quantities,
the gradient with Z = sqrt(m) I against the analytic dense gradient, the value against `log_likelihood` bit for bit.  Cases
and bars: tests/loglik_grad_cases.py.  Also the argument checks of the new operator entry points, which end in this backend's
"not supported" where they are valid."""
import numpy as np
import pytest

import cpuref
import loglik_grad_cases as lc
import loglik_grad_model as lm
import solve_cases as sc

RATIOS = {}


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


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()
    lc.write_errors("cpu_reference_ratio_to_bar", RATIOS)


def _record(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


def test_exported(gsi):
    for name in ("log_likelihood_grad", "covariance_family", "fit_covariance", "fft_gridcov_derivative", "CovarianceFamily"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    for name in ("gsi_op_fft_gridcov_deriv", "gsi_op_fft_at_like"):
        assert name in gsi._lib.SIGNATURES, name


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("with_precond", [False, True])
def test_terms_against_the_dense_same_probe_quantities(gsi, cx, p, with_precond):
    lc.run_dense_terms(gsi, cx, p, with_precond, _record, "cpuref")


@pytest.mark.parametrize("p", [0, 2])
@pytest.mark.parametrize("restricted", [True, False])
def test_gradient_with_unit_probes_is_the_analytic_gradient(gsi, cx, p, restricted):
    lc.run_dense_gradient(gsi, cx, p, restricted, _record, "cpuref")


def test_refusals(gsi, cx):
    lc.run_term_refusals(gsi, cx)


@pytest.mark.parametrize("kwargs,word", [
    (dict(Ns=[8, 6], param=7), "param"),
    (dict(Ns=[8, 6], param=-1), "param"),
    (dict(Ns=[12], param="theta"), "THETA"),
    (dict(Ns=[4, 5, 6], param="theta"), "THETA"),
    (dict(Ns=[12], param="log_ell1"), "LOG_ELL"),
    (dict(Ns=[8, 6], param="log_ell2"), "LOG_ELL"),
    (dict(Ns=[8, 6], param="log_ell", ell=0.0), "ell"),
    (dict(Ns=[8, 6], param="log_ell", sigma2=0.0), "sigma2"),
    (dict(Ns=[8, 6], param="log_ell", kind=4), "kind"),
    (dict(Ns=[4, 5, 6], param="log_ell", theta=0.3), "theta"),
    (dict(Ns=[5000], param="log_ell"), "4096 grid points per axis"),
])
def test_derivative_operator_refusals(gsi, cx, kwargs, word):
    kw = dict(kwargs)
    Ns, param = kw.pop("Ns"), kw.pop("param")
    try:
        gsi.fft_gridcov_derivative(cx, Ns, param, **kw)
    except gsi.GsiError as e:
        assert e.code == 1 and word in str(e) and "not supported by this backend" not in str(e), str(e)
    else:
        raise AssertionError("not refused")


def test_valid_derivative_calls_reach_the_backend(gsi, cx):
    for param in lm.PARAMS:
        if param == "log_ell2":            # refused on a 2-D grid (above)
            continue
        sc.refused(gsi, lambda: gsi.fft_gridcov_derivative(cx, [8, 6], param, kind="matern32", ell=[2.0, 3.0], theta=0.2),
                   "not supported by this backend")


def test_a_dense_bfgs_from_the_same_start_meets_the_conditions_of_the_gpu_fit(gsi):
    """The fit case of tests/test_loglik_grad_gpu.py, with the dense model as the objective and the package's own BFGS: the
    seed of the data (FIT_SEED) was fixed after this held."""
    fc = lc.fit_case()
    prm, stop, trace = gsi.Kriging._bfgs_maximize(lc.fit_dense_evaluate(fc), [lc.FIT_START["log_sigma2"], lc.FIT_START["log_ell"]],
                                                  gtol=lc.FIT_GTOL)
    ratio = lc.check_fit({"stop": stop, "trace": trace}, prm, fc)
    _record("dense fit |g| ratio (bar 1e-3)", ratio)


@pytest.mark.parametrize("which", ["at", "linear"])
def test_inputs_of_the_gpu_file_are_well_conditioned(which):
    for p in (0, 2):
        c = lc.fft_case(which, p)
        assert np.linalg.cond(c["M"]) < 5e3
        # the dense dM of the case are the derivatives of its M: differences of the dense matrix
        x0 = np.array([np.log(lc.FFT_SIGMA2), np.log(lc.FFT_ELL), 0.0])
        Hm = lc.fft_geometry(which)[0]
        base = c["noise"]
        for k in range(3):
            def f(v, k=k):
                x = x0.copy()
                x[k] = v
                A, _, nz = lc.fft_M(Hm, base, x)
                return A + np.diag(nz)
            fd = lm.richardson(f, x0[k], 1.0 / 64)
            assert np.abs(fd - c["dMs"][k]).max() <= 1e-9 * np.abs(c["dMs"][k]).max(), (which, p, k)
