"""The direct saddle-point solver on the MI355X (csrc/chol_saddle.hip): the cases of
tests/test_saddle_solve_cpu.py on the HIP backend -- info[1] == 1 shows that the kernels ran -- and what only the device path
has: many block steps and workgroups per trailing update (n = 1500), a ragged k in the formation (K = 259), the device path
beside GSI_SADDLE_HOST=1 in one process, run-to-run bit equality, recovery after a failed factorization, and pcgadirect with
a DeviceBasis and a LinearForwardModel.  Bars: tests/saddle_cases.py."""
import os

import numpy as np
import pytest

import saddle_cases as sc

pytestmark = pytest.mark.gpu

BIG = (1500, 259, 1e-2, False, 0.0)


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


@pytest.mark.parametrize("n", sc.EXACT_SIZES + [1500])
def test_exact_factor(gsi, ctx, n):
    A, L0 = sc.exact_factor(n)
    st, Lout, info, msg = sc.chol_lower(gsi, ctx, A)
    assert st == 0, msg
    assert info == [0, 1]
    assert np.array_equal(Lout, L0)
    assert np.array_equal(np.triu(Lout, 1), np.zeros((n, n)))


def test_exact_factor_with_a_leading_dimension_and_unread_upper_triangle(gsi, ctx):
    A, L0 = sc.exact_factor(129)
    B = np.tril(A) + np.triu(np.full((129, 129), np.nan), 1)
    st, Lout, info, msg = sc.chol_lower(gsi, ctx, B, lda=140)
    assert st == 0 and info == [0, 1], msg
    assert np.array_equal(Lout, L0)


@pytest.mark.parametrize("n", [129, 200])
def test_exact_failure_column(gsi, ctx, n):
    for j in sc.failure_columns(n):
        B = sc.failing_matrix(n, j)
        st, _, info, msg = sc.chol_lower(gsi, ctx, B)
        assert st == 7 and info == [j + 1, 1] and j + 1 == sc.dpotrf_info(B), (j, st, info, msg)
        assert str(j + 1) in msg


def test_non_finite_pivot_is_a_failure(gsi, ctx):
    A, _ = sc.exact_factor(70)
    B = A.copy()
    B[66, 3] = np.nan
    st, _, info, _ = sc.chol_lower(gsi, ctx, B)
    assert st == 7 and info == [67, 1]


def test_hx_zero_is_singular(gsi, ctx):
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    nobs = 40
    A = gsi.PCGALowRankMatrix([rng.standard_normal(nobs) for _ in range(3)], np.zeros(nobs),
                              sp.identity(nobs, format="csc"), ctx=ctx)
    with pytest.raises(gsi.GsiError) as ei:
        A.solve(np.ones(nobs + 1))
    assert ei.value.code == 3
    A.close()


@pytest.mark.parametrize("case", sc.MANUFACTURED + [BIG], ids=sc.case_id)
def test_manufactured_system(gsi, ctx, case):
    c = sc.manufactured(*case)
    x, info = sc.solve_case(gsi, ctx, c)
    err = sc.relerr(x, c["x_true"])
    print(f"{sc.case_id(case)}: error {err:.3g}; restatement {c['ref_errors'][0]:.3g}, dgesv {c['ref_errors'][1]:.3g}, "
          f"bound {c['bound']:.3g}")
    assert info == [0, 1]
    assert err <= c["bound"]


def test_device_path_beside_the_host_path(gsi, ctx):
    c = sc.manufactured(*sc.MANUFACTURED[0])
    x_dev, info_dev = sc.solve_case(gsi, ctx, c)
    old = os.environ.get("GSI_SADDLE_HOST")
    os.environ["GSI_SADDLE_HOST"] = "1"                    # read at each call
    try:
        x_host, info_host = sc.solve_case(gsi, ctx, c)
        A, L0 = sc.exact_factor(65)
        st, Lout, info_chol, _ = sc.chol_lower(gsi, ctx, A)
    finally:
        if old is None:
            del os.environ["GSI_SADDLE_HOST"]
        else:
            os.environ["GSI_SADDLE_HOST"] = old
    e_dev, e_host = sc.relerr(x_dev, c["x_true"]), sc.relerr(x_host, c["x_true"])
    print(f"device {e_dev:.3g}, host {e_host:.3g}, bound {c['bound']:.3g}")
    assert info_dev == [0, 1] and info_host == [0, 3]
    assert e_dev <= c["bound"] and e_host <= c["bound"]
    assert st == 0 and info_chol == [0, 3] and np.array_equal(Lout, L0)
    assert sc.solve_case(gsi, ctx, c)[1] == [0, 1]          # and the device path again once the variable is gone


def test_two_calls_return_the_same_bits(gsi, ctx):
    c = sc.manufactured(*BIG)
    A = sc.make_matrix(gsi, ctx, c)
    x1 = A.solve(c["b"])
    x2 = A.solve(c["b"])
    A.close()
    assert np.array_equal(x1, x2)


def test_good_system_after_a_failed_one(gsi, ctx):
    rng = np.random.default_rng(6)
    nobs, K = 200, 4
    E = rng.standard_normal((nobs, K))
    bad = gsi.PCGALowRankMatrix([E[:, i].copy() for i in range(K)], rng.standard_normal(nobs), -np.eye(nobs), ctx=ctx)
    with pytest.raises(gsi.GsiError) as ei:
        bad.solve(np.ones(nobs + 1))
    want = sc.dpotrf_info(E @ E.T - np.eye(nobs))
    assert ei.value.code == 7 and want > 0 and f"failed at {want}" in str(ei.value)
    bad.close()
    c = sc.manufactured(*sc.MANUFACTURED[4])
    x, info = sc.solve_case(gsi, ctx, c)
    assert info == [0, 1] and sc.relerr(x, c["x_true"]) <= c["bound"]


def test_pcgadirect_cholesky_with_device_basis_and_model(gsi, ctx):
    chol, pinv, truth, fallbacks = sc.device_inversion(gsi, ctx)
    sc.check_inversion(chol, pinv, truth, fallbacks)
