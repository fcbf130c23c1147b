"""The direct saddle-point solver (gsi_pcgamat_solve, gsi_chol_lower, pcgadirect(solver="cholesky"))
without a GPU: on the CPU reference library the backend declines, so this is the host path of pcga.cpp
(saddle_host.hpp) and the whole API around it -- argument checks, exact factors and failure columns, the singular system,
manufactured systems against the bar of saddle_cases.py, pcgadirect end to end and with a forced fallback, and the host path
as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import saddle_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def _small_matrix(gsi, ctx, nobs=5, K=2):
    import scipy.sparse as sp
    rng = np.random.default_rng(3)
    return gsi.PCGALowRankMatrix([rng.standard_normal(nobs) for _ in range(K)], rng.standard_normal(nobs),
                                 0.5 * sp.identity(nobs, format="csc"), ctx=ctx)


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_null_arguments_are_refused(gsi, cx):
    dp = gsi._lib.dptr
    A = _small_matrix(gsi, cx)
    b, x = np.ones(6), np.empty(6)
    info = (C.c_int64 * 2)()
    lib = cx.lib
    for args in ((None, A.h, dp(b), dp(x), info), (cx.h, None, dp(b), dp(x), info), (cx.h, A.h, None, dp(x), info),
                 (cx.h, A.h, dp(b), None, info)):
        assert lib.gsi_pcgamat_solve(*args) == 1
        assert b"NULL" in lib.gsi_last_error()
    assert lib.gsi_pcgamat_solve(cx.h, A.h, dp(b), dp(x), None) == 0          # info_out may be NULL
    M = np.eye(3, order="F")
    Lo = np.empty((3, 3), order="F")
    for args in ((None, dp(M), 3, 3, dp(Lo), info), (cx.h, None, 3, 3, dp(Lo), info), (cx.h, dp(M), 3, 3, None, info)):
        assert lib.gsi_chol_lower(*args) == 1
        assert b"NULL" in lib.gsi_last_error()
    assert lib.gsi_chol_lower(cx.h, dp(M), 0, 3, dp(Lo), info) == 1 and b"n >= 1" in lib.gsi_last_error()
    assert lib.gsi_chol_lower(cx.h, dp(M), 3, 2, dp(Lo), info) == 1 and b"lda" in lib.gsi_last_error()
    assert lib.gsi_chol_lower(cx.h, dp(M), 3, 3, dp(Lo), None) == 0 and np.array_equal(Lo, np.eye(3))
    A.close()


def test_matrix_of_another_context_is_refused(gsi, cx):
    other = gsi.Context(0, lib=cx.lib)
    try:
        A = _small_matrix(gsi, other)
        b, x = np.ones(6), np.empty(6)
        st = cx.lib.gsi_pcgamat_solve(cx.h, A.h, gsi._lib.dptr(b), gsi._lib.dptr(x), None)
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        assert np.all(np.isfinite(A.solve(b)))                      # and on its own context it solves
        A.close()
    finally:
        other.close()


def test_nobs_beyond_the_limit_is_refused_before_allocation(gsi, cx):
    import scipy.sparse as sp
    nobs = 32769
    A = gsi.PCGALowRankMatrix([np.ones(nobs)], np.ones(nobs), sp.identity(nobs, format="csc"), ctx=cx)
    used = C.c_int64()
    assert cx.lib.gsi_ctx_device_bytes(cx.h, C.byref(used)) == 0
    before = used.value
    b, x = np.ones(nobs + 1), np.empty(nobs + 1)
    info = (C.c_int64 * 2)(-1, -1)
    st = cx.lib.gsi_pcgamat_solve(cx.h, A.h, gsi._lib.dptr(b), gsi._lib.dptr(x), info)
    msg = cx.lib.gsi_last_error()
    assert st == 1 and b"32769" in msg and b"32768" in msg, msg
    assert list(info) == [0, 0]
    assert cx.lib.gsi_ctx_device_bytes(cx.h, C.byref(used)) == 0 and used.value == before
    A.close()


# ---- exact factors and failure columns ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.EXACT_SIZES)
def test_exact_factor(gsi, cx, n):
    A, L0 = sc.exact_factor(n)
    st, Lout, info, msg = sc.chol_lower(gsi, cx, A)
    assert st == 0, msg
    assert info == [0, 3]                                           # the CPU library has the host path only
    assert np.array_equal(Lout, L0)
    assert np.array_equal(np.triu(Lout, 1), np.zeros((n, n)))


def test_exact_factor_with_a_leading_dimension(gsi, cx):
    A, L0 = sc.exact_factor(129)
    st, Lout, info, msg = sc.chol_lower(gsi, cx, A, lda=140)
    assert st == 0, msg
    assert np.array_equal(Lout, L0)


def test_upper_triangle_is_not_read(gsi, cx):
    A, L0 = sc.exact_factor(65)
    B = np.tril(A) + np.triu(np.full((65, 65), np.nan), 1)
    st, Lout, info, msg = sc.chol_lower(gsi, cx, B)
    assert st == 0 and np.array_equal(Lout, L0)


@pytest.mark.parametrize("n", [129, 200])
def test_exact_failure_column(gsi, cx, n):
    for j in sc.failure_columns(n):
        B = sc.failing_matrix(n, j)
        st, _, info, msg = sc.chol_lower(gsi, cx, B)
        assert st == 7 and info[0] == j + 1 == sc.dpotrf_info(B), (j, st, info, msg)
        assert str(j + 1) in msg and "PosDefException" in msg


def test_non_finite_pivot_is_a_failure(gsi, cx):
    A, _ = sc.exact_factor(70)
    B = A.copy()
    B[66, 3] = np.nan                        # stays in row 66 and reaches the pivot of column 67 (1-based) through the updates
    st, _, info, _ = sc.chol_lower(gsi, cx, B)
    assert st == 7 and info[0] == 67


# ---- the saddle-point system ----------------------------------------------------------------------------------------
def test_hx_zero_is_singular(gsi, cx):
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    nobs = 40
    A = gsi.PCGALowRankMatrix([rng.standard_normal(nobs) for _ in range(3)], np.zeros(nobs),
                              sp.identity(nobs, format="csc"), ctx=cx)
    with pytest.raises(gsi.GsiError) as ei:
        A.solve(np.ones(nobs + 1))
    assert ei.value.code == 3 and "singular" in str(ei.value)
    A.close()


def test_not_positive_definite_reports_the_column(gsi, cx):
    """E E' - I with K < nobs has negative eigenvalues: status 7, and the column is dpotrf's."""
    rng = np.random.default_rng(6)
    nobs, K = 90, 4
    E = rng.standard_normal((nobs, K))
    A = gsi.PCGALowRankMatrix([E[:, i].copy() for i in range(K)], rng.standard_normal(nobs), -np.eye(nobs), ctx=cx)
    b, x = np.ones(nobs + 1), np.empty(nobs + 1)
    info = (C.c_int64 * 2)()
    st = cx.lib.gsi_pcgamat_solve(cx.h, A.h, gsi._lib.dptr(b), gsi._lib.dptr(x), info)
    want = sc.dpotrf_info(E @ E.T - np.eye(nobs))
    assert st == 7 and want > 0 and info[0] == want and info[1] == 3
    assert str(want).encode() in cx.lib.gsi_last_error()
    A.close()


@pytest.mark.parametrize("case", sc.MANUFACTURED, ids=sc.case_id)
def test_manufactured_system(gsi, cx, case):
    c = sc.manufactured(*case)
    x, info = sc.solve_case(gsi, cx, c)
    err = sc.relerr(x, c["x_true"])
    print(f"{sc.case_id(case)}: error {err:.3g}; restatement {c['ref_errors'][0]:.3g}, dgesv {c['ref_errors'][1]:.3g}, "
          f"bound {c['bound']:.3g}")
    assert info == [0, 3]
    assert (c["b"][-1] != 0.0) == bool(case[4])
    assert err <= c["bound"]


# ---- pcgadirect -----------------------------------------------------------------------------------------------------
def _inversion_setup():
    """The setup of tests/test_gpu_parity.py::test_device_resident_basis_gpu with the xis on the host."""
    import scipy.sparse as sp
    from oracle import oracle as orc
    rng = np.random.default_rng(43)
    M, N, mu = 16, 512, 10.0
    x = rng.standard_normal(N)
    Q0 = rng.standard_normal((M, N))
    Qc = Q0.T @ Q0
    w, V = np.linalg.eigh(Qc)
    truep = (V * np.sqrt(np.clip(w, 0, None))) @ V.T @ rng.standard_normal(N) + mu
    forward = lambda pv: pv * x
    Om = rng.standard_normal((N, M + 2))
    xis = orc.getxis_dense(Qc, M, 2, 3, Om)
    X = np.full(N, mu)
    y = forward(truep) + 1e-4 * rng.standard_normal(N)
    return forward, X, xis, sp, N, y, truep


def test_pcgadirect_cholesky_against_pinv(gsi, cx):
    forward, X, xis, sp, N, y, truep = _inversion_setup()
    R = 1e-8 * sp.identity(N, format="csc")
    chol = gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx, solver="cholesky")
    fallbacks = gsi.pcgadirect.last_fallbacks
    pinv = gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx, solver="pinv")
    sc.check_inversion(chol, pinv, truep, fallbacks)
    default = gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx)
    assert np.array_equal(default, pinv)                       # the default is the pseudo-inverse, as before
    with pytest.raises(ValueError):
        gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx, solver="lu")


def test_rga_takes_the_keyword_through_partial(gsi, cx):
    import functools
    forward, X, xis, sp, N, y, truep = _inversion_setup()
    R = 1e-8 * sp.identity(N, format="csc")
    S = np.random.default_rng(9).standard_normal((64, N))
    # rga passes no ctx: the partial carries it with the solver
    chol = gsi.rga(forward, X.copy(), X, xis, R, y, S, maxiters=2,
                   pcgafunc=functools.partial(gsi.pcgadirect, solver="cholesky", ctx=cx))
    assert gsi.pcgadirect.last_fallbacks == 0
    pinv = gsi.rga(forward, X.copy(), X, xis, R, y, S, maxiters=2, pcgafunc=functools.partial(gsi.pcgadirect, ctx=cx))
    assert np.linalg.norm(chol - pinv) < 1e-3 * np.linalg.norm(pinv)


def test_forced_fallback_returns_what_pinv_returns(gsi, cx):
    forward, X, xis, sp, N, y, truep = _inversion_setup()
    R = -1.0 * sp.identity(N, format="csc")                    # HQH + R = E E' - I is not positive definite (K = 16 < 512)
    calls = []
    chol = gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx, solver="cholesky", maxiters=3,
                          callback=lambda s, o: calls.append(1))
    assert gsi.pcgadirect.last_fallbacks == len(calls) > 0
    pinv = gsi.pcgadirect(forward, X.copy(), X, xis, R, y, ctx=cx, solver="pinv", maxiters=3)
    assert gsi.pcgadirect.last_fallbacks == 0
    assert np.array_equal(chol, pinv)


# ---- the host path as a program of its own, under sanitizers ----------------------------------------------------------
def test_host_path_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host-path check"
    exe = str(tmp_path / "saddle_host_check")
    src = os.path.join(ROOT, "tests", "saddle_host_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "saddle host ok" in r.stdout
