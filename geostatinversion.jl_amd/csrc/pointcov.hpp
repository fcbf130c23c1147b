// pointcov.hpp -- the stationary covariance kernels of the scattered-point implicit operator (SURVEY.md 8b "kernel-function
// covariance: coords + kernel id + params"), one definition for the device code (the generator table, tests of the in-loader entry) and the CPU reference
// backend of the tests.  r = |x_i - x_j| / ell.
#pragma once
#include <cmath>
#if defined(__HIPCC__)
#define GSI_PC_HD __host__ __device__
#else
#define GSI_PC_HD
#endif
namespace gsi { namespace pointcov {
enum { GAUSSIAN = 0, EXPONENTIAL = 1, MATERN32 = 2, MATERN52 = 3, NUM_KINDS = 4 };
struct Params { int d, kind; double inv_ell, sigma2, nugget; };
// exp(x) for x <= 0.  On the device: n = rint(x log2 e), r = x - n ln 2 (two-piece ln 2), the degree-12 Taylor polynomial
// of exp(r) on |r| <= ln(2)/2 (truncation 1.7e-16 relative) and one ldexp: ~20 instructions against the ~100 of the library
// exp with its special cases -- the generator evaluates it once per matrix entry (1e12 times per pass at n = 1e6).
GSI_PC_HD inline double exp_nonpos(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const bool under = x < -745.2;                   // (a select at the end, not an early return: no divergent branch per entry)
  x = under ? 0.0 : x;
  const double n = rint(x * 1.4426950408889634);
  double r = fma(-n, 6.93147180369123816490e-01, x);
  r = fma(-n, 1.90821492927058770002e-10, r);
  double p = 2.08767569878681e-09;                 // 1/12!
  p = fma(p, r, 2.505210838544172e-08);            // 1/11!
  p = fma(p, r, 2.755731922398589e-07);            // 1/10!
  p = fma(p, r, 2.7557319223985893e-06);           // 1/9!
  p = fma(p, r, 2.48015873015873e-05);             // 1/8!
  p = fma(p, r, 1.984126984126984e-04);            // 1/7!
  p = fma(p, r, 1.3888888888888889e-03);           // 1/6!
  p = fma(p, r, 8.333333333333333e-03);            // 1/5!
  p = fma(p, r, 4.1666666666666664e-02);           // 1/4!
  p = fma(p, r, 1.6666666666666666e-01);           // 1/3!
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const double e = ldexp(p, (int)n);
  return under ? 0.0 : e;
#else
  return exp(x);
#endif
}
// d2 = squared distance; same: i and j are the same point (the nugget sits on the diagonal)
GSI_PC_HD inline double kernel(const Params& p, double d2, bool same) {
  const double r2 = d2 * p.inv_ell * p.inv_ell;
  double v;
  if (p.kind == GAUSSIAN) v = exp_nonpos(-0.5 * r2);
  else {
    const double r = sqrt(r2);
    if (p.kind == EXPONENTIAL) v = exp_nonpos(-r);
    else if (p.kind == MATERN32) { const double a = 1.7320508075688772 * r; v = (1.0 + a) * exp_nonpos(-a); }
    else { const double a = 2.23606797749979 * r; v = (1.0 + a + a * a * (1.0 / 3.0)) * exp_nonpos(-a); }
  }
  v *= p.sigma2;
  return same ? v + p.nugget : v;
}
// ---- derivatives of sigma2 k(r) with respect to the covariance parameters (gsi_op_fft_gridcov_deriv) ----
// (the values of GSI_DPARAM_* in include/gsi_hip.h)
enum { D_LOG_SIGMA2 = 0, D_LOG_ELL = 1, D_LOG_ELL0 = 2, D_LOG_ELL1 = 3, D_LOG_ELL2 = 4, D_THETA = 5, D_NUGGET = 6, NUM_DPARAMS = 7 };
// The derivative profile g(r) = -k'(r) / r of the unit-variance kernel, at r2 = r^2: Gaussian k, exponential e^-r / r,
// Matern 3/2 3 e^(-sqrt3 r), Matern 5/2 (5/3)(1 + sqrt5 r) e^(-sqrt5 r).  The exponential kernel has a cusp at r = 0: every
// derivative below multiplies g by a factor that vanishes there, so g(0) is DEFINED as 0, by a select (never 0 * inf).
GSI_PC_HD inline double dprofile(int kind, double r2) {
  if (kind == GAUSSIAN) return exp_nonpos(-0.5 * r2);
  const double r = sqrt(r2);
  if (kind == EXPONENTIAL) {
    const bool zero = !(r > 0.0);
    const double e = exp_nonpos(-r) / (zero ? 1.0 : r);
    return zero ? 0.0 : e;
  }
  if (kind == MATERN32) return 3.0 * exp_nonpos(-1.7320508075688772 * r);
  const double a = 2.23606797749979 * r;
  return (5.0 / 3.0) * (1.0 + a) * exp_nonpos(-a);
}
// d (sigma2 k(r)) / d param off the diagonal at the SCALED lag (u, v, w) = (u_a / ell_a), r^2 = u^2 + v^2 + w^2 (in rotated
// 2-D: u, v along the rotated axes).  With q_a = (u_a / ell_a)^2:  log ell_a: sigma2 g q_a;  log ell (all axes): sigma2 g r^2;
// theta: -sigma2 g u v rot, rot = ell1 / ell0 - ell0 / ell1;  log sigma2: sigma2 k;  nugget: 0 (its derivative is the identity,
// which the plan adds to the spectrum as it adds the nugget itself).
GSI_PC_HD inline double dkernel(int kind, int param, double sigma2, double u, double v, double w, double rot) {
  const double q0 = u * u, q1 = v * v, q2 = w * w, r2 = q0 + q1 + q2;
  if (param == D_NUGGET) return 0.0;
  if (param == D_LOG_SIGMA2) {
    Params p;
    p.d = 3; p.kind = kind; p.inv_ell = 1.0; p.sigma2 = sigma2; p.nugget = 0.0;
    return kernel(p, r2, false);
  }
  const double g = sigma2 * dprofile(kind, r2);
  if (param == D_LOG_ELL) return g * r2;
  if (param == D_LOG_ELL0) return g * q0;
  if (param == D_LOG_ELL1) return g * q1;
  if (param == D_LOG_ELL2) return g * q2;
  return -(g * (u * v)) * rot;                      // D_THETA
}
}}  // namespace gsi::pointcov
