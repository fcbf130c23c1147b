// fft_gridcov_plan.hip -- the front half of the FFT operator for covariance FUNCTIONS on a regular grid
// (gsi_op_fft_gridcov[_table]): the lags of the kernel over the box, their even / odd split for centrally
// symmetric 2-D kernels, the sine sibling of fft_cos_matrix and the step that turns the re-embedded sums into a plan.
// The passes that apply the plan are fft_cov.hip's, unchanged; the per-axis factors are applied by the contraction kernel
// (hip_backend.hip:fftcov_spectrum_of_lags).  Everything here runs once per plan: plain grid-stride kernels.
// gsi_op_fft_gridcov_deriv is the same plan from the lags of the covariance's derivative with respect to
// one parameter: fft_lag_table_deriv_kernel, a sibling of fft_lag_table_kernel; nothing behind it differs.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"

namespace gsi { namespace hipk {

static inline int plan_grid_for(int64_t total, int cap) {
  int64_t g = (total + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// cp[t0 + N0 (t1 + N1 t2)] = sigma2 k(r) at the lag t, t_a >= 0 (nugget NOT included: it is added to the spectrum);
// cm (2-D rotated kernels only, else null) = the same at (t0, -t1).  u = t except in the rotated 2-D case
// (u = (cs t0 + sn t1, -sn t0 + cs t1)); r^2 = sum_a (u_a inv_ell[a])^2; k = pointcov::kernel's family.
__global__ __launch_bounds__(256) void fft_lag_table_kernel(double* __restrict__ cp, double* __restrict__ cm, int64_t N0, int64_t N1,
                                                            int64_t N2, int kind, double ie0, double ie1, double ie2, double cs,
                                                            double sn, double sigma2) {
  const int64_t total = N0 * N1 * N2;
  pointcov::Params prm;
  prm.d = 3; prm.kind = kind; prm.inv_ell = 1.0; prm.sigma2 = sigma2; prm.nugget = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i0 = e % N0, r = e / N0, i1 = r % N1, i2 = r / N1;
    const double t0 = (double)i0, t1 = (double)i1, t2 = (double)i2;
    const double w = t2 * ie2;
    {
      const double u = (cs * t0 + sn * t1) * ie0, v = (-sn * t0 + cs * t1) * ie1;
      cp[e] = pointcov::kernel(prm, u * u + v * v + w * w, false);
    }
    if (cm != nullptr) {
      const double u = (cs * t0 - sn * t1) * ie0, v = (-sn * t0 - cs * t1) * ie1;
      cm[e] = pointcov::kernel(prm, u * u + v * v + w * w, false);
    }
  }
}
void fft_lag_table(hipStream_t st, double* cp, double* cm, const int64_t N[3], int kind, const double inv_ell[3], double cs,
                   double sn, double sigma2) {
  hipLaunchKernelGGL(fft_lag_table_kernel, dim3(plan_grid_for(N[0] * N[1] * N[2], 4096)), dim3(256), 0, st, cp, cm, N[0], N[1], N[2],
                     kind, inv_ell[0], inv_ell[1], inv_ell[2], cs, sn, sigma2);
}

// fft_lag_table_kernel's sibling for gsi_op_fft_gridcov_deriv: cp / cm <- d (sigma2 k(r)) / d param at the
// same lags, pointcov::dkernel's formulas.  A derivative is neither positive nor (for theta) even along the axes: cm is
// written whenever the caller passes it, and nothing behind this kernel clamps the spectrum.  rot = ell1/ell0 - ell0/ell1.
__global__ __launch_bounds__(256) void fft_lag_table_deriv_kernel(double* __restrict__ cp, double* __restrict__ cm, int64_t N0,
                                                                  int64_t N1, int64_t N2, int kind, int param, double ie0, double ie1,
                                                                  double ie2, double cs, double sn, double sigma2, double rot) {
  const int64_t total = N0 * N1 * N2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i0 = e % N0, r = e / N0, i1 = r % N1, i2 = r / N1;
    const double t0 = (double)i0, t1 = (double)i1, t2 = (double)i2;
    const double w = t2 * ie2;
    {
      const double u = (cs * t0 + sn * t1) * ie0, v = (-sn * t0 + cs * t1) * ie1;
      cp[e] = pointcov::dkernel(kind, param, sigma2, u, v, w, rot);
    }
    if (cm != nullptr) {
      const double u = (cs * t0 - sn * t1) * ie0, v = (-sn * t0 - cs * t1) * ie1;
      cm[e] = pointcov::dkernel(kind, param, sigma2, u, v, w, rot);
    }
  }
}
// param == D_LOG_SIGMA2 is the covariance itself without its nugget: fft_lag_table's own kernel, hence its bits
void fft_lag_table_deriv(hipStream_t st, double* cp, double* cm, const int64_t N[3], int kind, int param, const double inv_ell[3],
                         double cs, double sn, double sigma2) {
  if (param == pointcov::D_LOG_SIGMA2) { fft_lag_table(st, cp, cm, N, kind, inv_ell, cs, sn, sigma2); return; }
  const double rot = inv_ell[0] / inv_ell[1] - inv_ell[1] / inv_ell[0];
  hipLaunchKernelGGL(fft_lag_table_deriv_kernel, dim3(plan_grid_for(N[0] * N[1] * N[2], 4096)), dim3(256), 0, st, cp, cm, N[0], N[1],
                     N[2], kind, param, inv_ell[0], inv_ell[1], inv_ell[2], cs, sn, sigma2, rot);
}

// (c+, c-) -> (c_ee, c_oo) = ((c+ + c-) / 2, (c+ - c-) / 2), in place
__global__ __launch_bounds__(256) void fft_even_odd_kernel(double* __restrict__ cp, double* __restrict__ cm, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const double a = cp[e], b = cm[e];
    cp[e] = 0.5 * (a + b);
    cm[e] = 0.5 * (a - b);
  }
}
void fft_even_odd_split(hipStream_t st, double* cp, double* cm, int64_t total) {
  hipLaunchKernelGGL(fft_even_odd_kernel, dim3(plan_grid_for(total, 4096)), dim3(256), 0, st, cp, cm, total);
}

// fft_cos_matrix's sine sibling (always weighted): out[r + c rows] = (r > 0 ? 2 : 1) sin(2 pi r c / period)
__global__ __launch_bounds__(256) void fft_sin_matrix_kernel(double* __restrict__ out, int64_t rows, int64_t cols, int64_t period) {
  const int64_t total = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e % rows, c = e / rows;
    const int64_t a = (r * c) % period;                    // exact argument reduction
    const double v = sinpi(2.0 * (double)a / (double)period);
    out[e] = (r > 0) ? 2.0 * v : v;
  }
}
void fft_sin_matrix(hipStream_t st, double* out, int64_t rows, int64_t cols, int64_t period) {
  hipLaunchKernelGGL(fft_sin_matrix_kernel, dim3(plan_grid_for(rows * cols, 4096)), dim3(256), 0, st, out, rows, cols, period);
}

// a -= b
__global__ __launch_bounds__(256) void fft_subtract_kernel(double* __restrict__ a, const double* __restrict__ b, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) a[e] -= b[e];
}
void fft_subtract(hipStream_t st, double* a, const double* b, int64_t total) {
  hipLaunchKernelGGL(fft_subtract_kernel, dim3(plan_grid_for(total, 4096)), dim3(256), 0, st, a, b, total);
}

// lam <- (lam + nugget) / Mtot: the inverse transform's 1 / Mtot (a power of two: exact) and nugget * I on the box; NO
// normalisation to a unit diagonal (fft_finish_plan's division by sum(lambda) is that and the 1 / Mtot at once)
__global__ __launch_bounds__(256) void fft_scale_shift_kernel(double* __restrict__ lam, int64_t Mtot, double nugget, double inv_mtot) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < Mtot; e += (int64_t)gridDim.x * 256)
    lam[e] = (lam[e] + nugget) * inv_mtot;
}
void fft_finish_plan_lags(hipStream_t st, double* lam, const int64_t M[3], double nugget) {
  const int64_t Mtot = M[0] * M[1] * M[2];
  fft_plan_twiddles(st, lam, M);
  hipLaunchKernelGGL(fft_scale_shift_kernel, dim3(plan_grid_for(Mtot, 4096)), dim3(256), 0, st, lam, Mtot, nugget, 1.0 / (double)Mtot);
}

}}  // namespace gsi::hipk
