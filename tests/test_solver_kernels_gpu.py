"""The BLAS-2, Nystrom and LSQR kernels of csrc/misc.hip and csrc/lsqr_dev.hip at their loop edges, through three public entry
points (`PCGALowRankMatrix.matvec` / `.lsqr`, `eig_nystrom`, the adaptive `rangefinder`).  Cases, references and checks:
tests/solver_kernel_cases.py; tests/test_solver_kernels_cpu.py runs the same checks on the CPU reference library.

kernel -> edge -> case that reaches it
  gemv_n_kernel            x staged in LDS in chunks of 1024, two barriers per chunk, row + k0 * lda
    one chunk, tail loop (k % 4 = 1, 2, 3)        matvec (1, 1) (31, 2) (255, 3): gemv_n(nobs, K) and gemv_n(nobs, 1)
    k % 4 = 0, no tail                            matvec (257, 4)
    second workgroup holding one row              matvec (257, 4) dense: gemv_n(257, 257)
    second chunk of one element (k = 1025)        matvec (1025, 5) dense, and the planted column 1024 (every row = 1 exactly)
    three chunks (k = 2049)                       matvec (2049, 6) dense
    k > 1024 with a tail of 2 in the last chunk   matvec (2051, 1030) diagonal R: gemv_n(2051, 1030)
    k = 1100 > 1024 from the range finder         rangefinder (1100, 9, 10): gemv_n(m, n) with A itself
    beta = 0 and beta = 1                         every matvec case (the etas leg overwrites, the R and HX legs add)
  gemv_t_partial_kernel    m rows over 32 slabs of per = ceil(m / 32), 256 lanes per slab
    m < 32: per = 1, empty slabs with i0 > m      matvec (1, 1) (31, 2)
    per <= 256: one trip per slab                 matvec (255, 3) .. (2051, 1030)
    per = 257 > 256: a second trip per slab       matvec (8193, 7)
    more than 256 columns (gemv_t_final's grid)   matvec (2051, 1030)
  project_apply_kernel     dots in __shared__ double d[64], ncols = r - 1
    ncols = 0 (no launch), 1                      rangefinder (300, 5, 1), (300, 5, 2)
    ncols = 9                                     rangefinder (1100, 9, 10)
    ncols = 63, the most the caller allows        rangefinder (1030, 70, 64); j - 1 = 0 .. 69 passes every residue mod 4 in
                                                  gemv_n(m, j - 1) and gemv_t(m, j - 1)
    r = 65                                        refused with GSI_ERR_ARG before anything runs
  colnorms_sq_kernel       one workgroup per column, 256 lanes over m
    m = 300, 1030, 1100: two to five trips        the rangefinder cases (r = 1, 2, 10, 64 columns)
  chol_upper_kernel        one workgroup, columns c = k + 1 + tid, c += 256
    j = 1, 2                                      eig_nystrom (40, 1), (40, 2)
    odd width, one trip                           eig_nystrom (300, 17)
    j = 256, 257: last widths with one trip       eig_nystrom (600, 256), (600, 257)
    j = 258: first second trip (column 257, k = 0)  eig_nystrom (600, 258)
    ragged second trip (43 columns at k = 0)      eig_nystrom (700, 300)
    not positive definite at column 3 (d = 1.0 patched in, the kernel goes on)
                                                  diag(1, 1, -1, 1, 1) with Q = I[:, :4]: GSI_ERR_NOT_POSDEF naming column 3
    the error flag is cleared afterwards          the next eig_nystrom on the same context meets the bar
  trsm_right_upper_kernel  thread = one row, grid capped at 4096 workgroups
    j = 1 .. 300 as above, n = 40 .. 700          the eig_nystrom table
    second trip of the grid-stride loop           LowRankCovMatrix n = 2^20 + 3, j = 2: rows 2^20 .. 2^20 + 2
  center_rows_kernel       thread = one row, grid capped at 4096 workgroups
    second trip                                   the same case (the operator centres its N = 4 samples on creation)
  lsqr_*_kernel            128 workgroups of 256 lanes, grid-stride loops over m = n = nobs + 1
    one trip                                      lsqr (300, 4)
    second trip by one element (32 769)           lsqr (32768, 3)
    third trip (65 540)                           lsqr (65539, 3)
    beta == 0: lsqr_scale_u and lsqr_v skip       [[I, e_0], [e_0', 0]] x = e_1: x == b after one iteration
    iterations enqueued after the stop are no-ops GSI_LSQR_POLL = 1, 8, 64 in three child processes: equal bits
  dot_kernel / dot_partial_kernel + dot_final_kernel   (the two start-up norms of LSQR)
    single workgroup, n < 65 536                  lsqr (300, 4), (32768, 3)
    two-stage form, n >= 65 536                   lsqr (65539, 3)

Bars and what they rest on (measured by tests/test_solver_kernels_cpu.py; "CPU" is the CPU reference library, "HIP" what
this module measured on an MI355X):
  matvec        equal bits: integer data, every partial sum an integer below 2^50.
  eig_nystrom   | U diag(Sigma^2) U' - ref |max / |ref|max <= 16 j eps kappa_2(Q'AQ), ref in np.longdouble.
                (n, j): LAPACK / bar, CPU / bar:  (40, 1) 0.13, 0.23   (40, 2) 0.16, 0.05   (300, 17) 0.017, 0.043
                (600, 256) 0.0008, 0.023   (600, 257) 0.0007, 0.023   (600, 258) 0.0007, 0.023   (700, 300) 0.0007, 0.024.
                The two narrow cases set c = 16: their error comes from the 40-term inner products, not from j.
                HIP / bar in the same order: 0.13, 0.11, 0.024, 0.0030, 0.0048, 0.0034, 0.0032.
                n = 2^20 + 3: bar 7.4e-14 (kappa 10.4, relative gap of Sigma^2 0.43); CPU: Sigma 2.1e-15, U diag(Sigma) 5.1e-15;
                HIP: 3.6e-16, 4.3e-16, in 0.2 s.  Its fields are non-zero on every 257th row and on the last three
                (solver_kernel_cases.nystrom_big_inputs says why).
  rangefinder   columns [: m - 1] within 100 x |oracle float64 - oracle with long-double products|max, at least 1e-13.
                (n, m, r): that distance, bar, CPU:  (1100, 9, 10) 5.4e-16, 1e-13, 1.2e-15   (1030, 70, 64) 3.5e-15, 3.5e-13,
                6.8e-15   (300, 5, 1) 1.2e-16, 1e-13, 2.5e-16   (300, 5, 2) 8.3e-17, 1e-13, 3.1e-16.
                HIP: 6.8e-16, 4.0e-15, 1.9e-16, 1.9e-16.  (The float64 oracle runs on the host's BLAS, so the distance, and with
                it the bar, moves by some percent between hosts.)
  lsqr          the oracle's iteration count; |x - x_oracle| / |x_oracle| within 100 x the same distance, at least 1e-13; true
                residual <= 2 x the oracle's.  (nobs, K): iterations, distance, bar, CPU:  (300, 4) 13, 3.8e-15, 3.8e-13, 1.1e-14
                (32768, 3) 11, 1.9e-16, 1e-13, 4.3e-16   (65539, 3) 11, 2.4e-16, 1e-13, 2.2e-15.
                HIP: 2.5e-15, 2.2e-16, 2.7e-16, the same iteration counts.
"""
import os

import pytest

import solver_kernel_cases as sk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


# ---- A. PCGALowRankMatrix.matvec: gemv_n, gemv_t, bit for bit
@pytest.mark.parametrize("nobs,K,dense", sk.MATVEC)
def test_matvec_exact(gsi, ctx, nobs, K, dense):
    sk.check_matvec(gsi, ctx, nobs, K, dense)


def test_matvec_planted_column(gsi, ctx):
    sk.check_matvec_planted(gsi, ctx)


# ---- B. eig_nystrom: chol_upper, trsm_right_upper
@pytest.mark.parametrize("n,j", sk.NYSTROM)
def test_eig_nystrom(gsi, ctx, n, j):
    sk.check_nystrom(gsi, ctx, n, j, name="hip_library")


def test_eig_nystrom_lowrank_beyond_one_sweep(gsi, ctx):
    sk.check_nystrom_big(gsi, ctx)


def test_eig_nystrom_not_posdef_then_clean(gsi, ctx):
    sk.check_nystrom_not_posdef(gsi, ctx)


# ---- C. adaptive rangefinder: gemv_n at k > 1024, gemv_t, project_out, colnorms
@pytest.mark.parametrize("n,m,r", sk.RANGEFINDER)
def test_rangefinder_adaptive(gsi, ctx, n, m, r):
    sk.check_rangefinder(gsi, ctx, n, m, r, name="hip_library")


def test_rangefinder_refuses_r65(gsi, ctx):
    sk.check_rangefinder_refuses_r65(gsi, ctx)


# ---- D. PCGALowRankMatrix.lsqr: lsqr_dev.hip, dot_dev
@pytest.mark.parametrize("nobs,K", sk.LSQR)
def test_lsqr(gsi, ctx, nobs, K):
    sk.check_lsqr(gsi, ctx, nobs, K, name="hip_library")


def test_lsqr_beta_zero(gsi, ctx):
    sk.check_lsqr_beta_zero(gsi, ctx)


def test_lsqr_poll_invariance(tmp_path):
    sk.check_lsqr_poll_invariance("gpu", tmp_path, ROOT)
