"""The posterior variance (gsi_basis_quadform, gsi_pcgamat_posterior, gsi_pcga_posterior_variance, posterior_variance,
posterior_realizations) without a GPU: on the CPU reference library the backend declines, so this is
the host path of pcga.cpp (posterior_host.hpp) and the whole API around it, with info[1] == 3 -- the row sums to the bounds
of posterior_cases.py and exactly on integers, the variance against the dense saddle-point formula in extended precision, the
factor, the observed-point property, the realisations, the errors, and the host path as a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import posterior_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = 3


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("K", pc.K_LIST_CPU)
def test_row_sums_within_the_bounds(gsi, cx, K, precision):
    worst = 0.0
    for n in pc.N_LIST_CPU:
        Z, _ = pc.kernel_inputs(n, K, False)
        basis, Zs = pc.make_basis(gsi, cx, Z, precision)
        worst = max(worst, pc.check_kernel_case(basis, Zs, False, (n, K, precision), HOST))
        pc.close_basis(basis)
    print(f"K={K} fp{precision}: largest error / bound {worst:.3g}")


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("K", pc.K_LIST_CPU)
def test_row_sums_exact_on_integers(gsi, cx, K, precision):
    for n in pc.N_LIST_CPU:
        Z, _ = pc.kernel_inputs(n, K, True)
        basis, Zs = pc.make_basis(gsi, cx, Z, precision)
        assert np.array_equal(Zs, Z)
        pc.check_kernel_case(basis, Zs, True, (n, K, precision), HOST)
        pc.close_basis(basis)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", pc.FEATURE_CASES)
def test_variance_against_the_dense_formula(gsi, cx, name, precision, with_prior):
    ratio = pc.check_variance(gsi, cx, name, precision, with_prior, HOST)
    print(f"{name} fp{precision} prior={with_prior}: max |v - v_ref| / max |v_ref| = {ratio:.3g}")
    assert ratio <= pc.VARIANCE_BAR


@pytest.mark.parametrize("name", pc.FEATURE_CASES)
def test_factor_and_scalars(gsi, cx, name):
    r = pc.check_factor(gsi, cx, name, HOST)
    print(f"{name}: |W'NW - I| {r[0]:.3g}, u {r[1]:.3g}, gamma {r[2]:.3g}")


@pytest.mark.parametrize("precision", [64, 32])
def test_observed_points_are_no_worse_than_their_measurement(gsi, cx, precision):
    print(f"fp{precision}: max v / R_jj = {pc.check_observed_points(gsi, cx, precision, HOST):.4f}")


@pytest.mark.parametrize("on_device", [True, False])
def test_realizations_and_the_covariance_identity(gsi, cx, on_device):
    r = pc.check_realizations(gsi, cx, on_device)
    print(f"realisations {r[0]:.3g}, covariance identity {r[1]:.3g}")


def test_host_xis_take_a_temporary_basis(gsi, cx):
    case = pc.feature_case("n777_diag")
    fwd = pc.forward_model(gsi, cx, case)
    basis, _ = pc.make_basis(gsi, cx, case["Z"], 64)
    a = gsi.posterior_variance(fwd, case["s"], case["X"], basis, case["R"])
    xis = [np.ascontiguousarray(case["Z"][:, i]) for i in range(case["K"])]
    b = gsi.posterior_variance(fwd, case["s"], case["X"], xis, case["R"], ctx=cx)
    pc.close_basis(basis)
    assert np.array_equal(a, b)


def test_sharded_basis_is_not_implemented(gsi, cx):
    case = pc.feature_case("n300_K130")
    Zm = gsi.DeviceMatrix.from_host(cx, case["Z"])
    basis = gsi.ShardedDeviceBasis(Zm, case["K"], gather=lambda rows: rows)
    with pytest.raises(NotImplementedError):
        gsi.posterior_variance(lambda s: s[:3], case["s"], case["X"], basis, np.eye(3))
    basis.close()
    Zm.close()


# ---- errors ---------------------------------------------------------------------------------------------------------
def _matrix(gsi, ctx, nobs=6, K=3, hx=None, rdiag=None, seed=4):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rd = np.full(nobs, 0.5) if rdiag is None else rdiag
    return gsi.PCGALowRankMatrix([rng.standard_normal(nobs) for _ in range(K)],
                                 rng.standard_normal(nobs) if hx is None else hx, sp.diags(rd, format="csc"), ctx=ctx)


def test_zero_pivot_of_a_dense_r_reports_the_column(gsi, cx):
    rd = np.full(6, 0.5)
    rd[4] = 0.0
    rng = np.random.default_rng(4)
    A = gsi.PCGALowRankMatrix([rng.standard_normal(6) for _ in range(3)], rng.standard_normal(6), np.diag(rd), ctx=cx)
    W, u, g = np.empty((3, 3), order="F"), np.empty(3), C.c_double()
    info = (C.c_int64 * 2)()
    dp = gsi._lib.dptr
    st = cx.lib.gsi_pcgamat_posterior(cx.h, A.h, dp(W), dp(u), C.byref(g), info)
    assert st == 7 and info[0] == 5, (st, list(info))
    with pytest.raises(gsi.GsiError) as ei:
        A.posterior_factor()
    assert ei.value.code == 7 and "5" in str(ei.value)
    A.close()


def test_diagonal_r_with_a_zero_entry(gsi, cx):
    """The diagonal storage (r_is_diag = 1) through the C ABI directly."""
    rng = np.random.default_rng(4)
    nobs, K = 6, 3
    E = np.asfortranarray(rng.standard_normal((nobs, K)))
    hx = rng.standard_normal(nobs)
    rd = np.full(nobs, 0.5)
    rd[2] = 0.0
    dp = gsi._lib.dptr
    h = C.c_void_p()
    assert cx.lib.gsi_pcgamat_create(cx.h, C.byref(h), dp(E), nobs, K, dp(hx), dp(rd), 1) == 0
    W, u, g = np.empty((K, K), order="F"), np.empty(K), C.c_double()
    info = (C.c_int64 * 2)()
    st = cx.lib.gsi_pcgamat_posterior(cx.h, h, dp(W), dp(u), C.byref(g), info)
    assert st == 7 and info[0] == 3 and b"3" in cx.lib.gsi_last_error()
    cx.lib.gsi_pcgamat_destroy(h)


def test_hx_zero_is_singular(gsi, cx):
    A = _matrix(gsi, cx, hx=np.zeros(6))
    with pytest.raises(gsi.GsiError) as ei:
        A.posterior_factor()
    assert ei.value.code == 3
    A.close()


def test_objects_of_another_context_are_refused(gsi, cx):
    other = gsi.Context(0, lib=cx.lib)
    try:
        Z = np.random.default_rng(1).standard_normal((9, 3))
        basis, _ = pc.make_basis(gsi, cx, Z, 64)
        A = _matrix(gsi, other)
        X, v = np.ones(9), np.empty(9)
        dp = gsi._lib.dptr
        st = cx.lib.gsi_pcga_posterior_variance(cx.h, basis.h, A.h, dp(X), None, dp(v), None)
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        W, u, g = np.empty((3, 3), order="F"), np.empty(3), C.c_double()
        st = cx.lib.gsi_pcgamat_posterior(cx.h, A.h, dp(W), dp(u), C.byref(g), None)
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        a = np.empty(9)
        st = other.lib.gsi_basis_quadform(other.h, basis.h, dp(W), 3, 3, 0, None, dp(a), None, None, None)
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        A.close()
        pc.close_basis(basis)
    finally:
        other.close()


def test_null_arguments_are_refused(gsi, cx):
    dp = gsi._lib.dptr
    Z = np.random.default_rng(2).standard_normal((9, 3))
    basis, _ = pc.make_basis(gsi, cx, Z, 64)
    A = _matrix(gsi, cx)
    W, u, g = np.asfortranarray(np.eye(3)), np.ones(3), C.c_double()
    a, q, t, X, v = (np.empty(9) for _ in range(5))
    X[:] = 1.0
    info = (C.c_int64 * 2)()
    lib = cx.lib
    for args in ((None, basis.h, dp(W), 3, 3, 0, dp(u), dp(a), dp(q), dp(t), info),
                 (cx.h, None, dp(W), 3, 3, 0, dp(u), dp(a), dp(q), dp(t), info),
                 (cx.h, basis.h, None, 3, 3, 0, dp(u), dp(a), dp(q), dp(t), info),
                 (cx.h, basis.h, dp(W), 3, 3, 0, dp(u), None, dp(q), dp(t), info)):
        assert lib.gsi_basis_quadform(*args) == 1 and b"NULL" in lib.gsi_last_error()
    assert lib.gsi_basis_quadform(cx.h, basis.h, dp(W), 3, 3, 0, dp(u), dp(a), dp(q), None, info) == 1      # u without t_out
    assert lib.gsi_basis_quadform(cx.h, basis.h, dp(W), 3, 3, 0, None, dp(a), dp(q), dp(t), info) == 1
    assert lib.gsi_basis_quadform(cx.h, basis.h, dp(W), 2, 3, 0, None, dp(a), None, None, info) == 1 and b"ldw" in lib.gsi_last_error()
    assert lib.gsi_basis_quadform(cx.h, basis.h, dp(W), 3, 0, 0, None, dp(a), None, None, info) == 1
    assert lib.gsi_basis_quadform(cx.h, basis.h, dp(W), 3, 3, 0, None, dp(a), None, None, None) == 0         # the optional ones
    Wo, uo = np.empty((3, 3), order="F"), np.empty(3)
    for args in ((None, A.h, dp(Wo), dp(uo), C.byref(g), info), (cx.h, None, dp(Wo), dp(uo), C.byref(g), info),
                 (cx.h, A.h, None, dp(uo), C.byref(g), info), (cx.h, A.h, dp(Wo), None, C.byref(g), info),
                 (cx.h, A.h, dp(Wo), dp(uo), None, info)):
        assert lib.gsi_pcgamat_posterior(*args) == 1 and b"NULL" in lib.gsi_last_error()
    for args in ((None, basis.h, A.h, dp(X), None, dp(v), info), (cx.h, None, A.h, dp(X), None, dp(v), info),
                 (cx.h, basis.h, None, dp(X), None, dp(v), info), (cx.h, basis.h, A.h, None, None, dp(v), info),
                 (cx.h, basis.h, A.h, dp(X), None, None, info)):
        assert lib.gsi_pcga_posterior_variance(*args) == 1 and b"NULL" in lib.gsi_last_error()
    assert lib.gsi_pcga_posterior_variance(cx.h, basis.h, A.h, dp(X), None, dp(v), None) == 0
    A.close()
    pc.close_basis(basis)


def test_a_diagonal_r_has_no_limit_on_nobs(gsi, cx):
    """The 32768 limit is the factorization's and concerns a dense R only: a diagonal R is scaled entry by entry."""
    nobs = 32769
    dp = gsi._lib.dptr
    E, hx = np.ones((nobs, 1), order="F"), np.ones(nobs)
    basis, _ = pc.make_basis(gsi, cx, np.ones((4, 1)), 64)
    h = C.c_void_p()
    assert cx.lib.gsi_pcgamat_create(cx.h, C.byref(h), dp(E), nobs, 1, dp(hx), dp(hx), 1) == 0
    X, v = np.zeros(4), np.empty(4)
    assert cx.lib.gsi_pcga_posterior_variance(cx.h, basis.h, h, dp(X), None, dp(v), None) == 0
    assert np.all(np.isfinite(v))
    cx.lib.gsi_pcgamat_destroy(h)
    pc.close_basis(basis)


# ---- the host path as a program of its own, under sanitizers ----------------------------------------------------------
def test_host_path_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host-path check"
    exe = str(tmp_path / "posterior_host_check")
    src = os.path.join(ROOT, "tests", "posterior_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "posterior host ok" in r.stdout
