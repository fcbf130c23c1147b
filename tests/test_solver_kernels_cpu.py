"""The checks of tests/solver_kernel_cases.py on the CPU reference library: the inputs and bars are shown to be fair before a
GPU sees them (tests/test_solver_kernels_gpu.py runs the same checks on the HIP kernels).  Run with -s to see the measured
reference errors that the bars were set from."""
import os

import numpy as np
import pytest

import cpuref
import solver_kernel_cases as sk
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cx(gsi):
    c = gsi.Context(0, lib=cpuref.load_cpuref())
    yield c
    c.close()
    for name in sorted(sk.MEASURED):
        print(name, {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in sk.MEASURED[name].items()})


# ---- A
@pytest.mark.parametrize("nobs,K,dense", sk.MATVEC)
def test_matvec_exact(gsi, cx, nobs, K, dense):
    sk.check_matvec(gsi, cx, nobs, K, dense)


def test_matvec_planted_column(gsi, cx):
    sk.check_matvec_planted(gsi, cx)


def test_matvec_table_covers_every_residue_of_K():
    assert {K % 4 for _, K, _ in sk.MATVEC} == {0, 1, 2, 3}


# ---- B
@pytest.mark.parametrize("n,j", sk.NYSTROM)
def test_eig_nystrom(gsi, cx, n, j):
    """The bar is fair: LAPACK (orc.eig_nystrom) and the CPU library both sit at or below a quarter of it."""
    err = sk.check_nystrom(gsi, cx, n, j, name="cpu_library")
    ref, kappa, _, err_lapack = sk.nystrom_reference(n, j)
    assert kappa <= 4.0 * (1.0 + 1e-12)
    assert max(err, err_lapack) <= 0.25 * sk.nystrom_bar(j, kappa), (err, err_lapack, sk.nystrom_bar(j, kappa))


def test_eig_nystrom_lowrank_beyond_one_sweep(gsi, cx):
    sk.check_nystrom_big(gsi, cx)


def test_eig_nystrom_not_posdef_then_clean(gsi, cx):
    sk.check_nystrom_not_posdef(gsi, cx)


# ---- C
def test_hooked_restatements_are_the_oracle():
    """`rangefinder_hooked` and `lsqr_hooked` with float64 products and norms give the oracle's bits, so that their
    long-double runs differ from the oracle in the accumulation alone."""
    A = sk.exact_rank_matrix(np.random.default_rng(3), 120, 7)
    Q0 = orc.rangefinder_adaptive(A, sk._stream(), r=4)
    Q1 = sk.rangefinder_hooked(A, sk._stream(), np.matmul, np.linalg.norm, r=4)
    assert np.array_equal(Q0, Q1)
    E, HX, d, R, b = sk.lsqr_inputs(300, 4)
    ref = orc.PCGALowRankMatrix([E[:, i] for i in range(4)], HX, R)
    x0, it0 = orc.lsqr(ref.matvec, ref.matvec, b, 301)
    x1, it1 = sk.lsqr_hooked(ref.matvec, b, 301, np.linalg.norm)
    assert it0 == it1 and np.array_equal(x0, x1)


@pytest.mark.parametrize("n,m,r", sk.RANGEFINDER)
def test_rangefinder_adaptive(gsi, cx, n, m, r):
    sk.check_rangefinder(gsi, cx, n, m, r, name="cpu_library")


def test_rangefinder_refuses_r65(gsi, cx):
    sk.check_rangefinder_refuses_r65(gsi, cx)


# ---- D
@pytest.mark.parametrize("nobs,K", sk.LSQR)
def test_lsqr(gsi, cx, nobs, K):
    sk.check_lsqr(gsi, cx, nobs, K, name="cpu_library")


def test_lsqr_beta_zero(gsi, cx):
    sk.check_lsqr_beta_zero(gsi, cx)


def test_lsqr_poll_invariance(tmp_path):
    sk.check_lsqr_poll_invariance("cpu", tmp_path, ROOT)
