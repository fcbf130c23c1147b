// slq_state.hpp -- the Gauss quadrature of stochastic Lanczos quadrature, written ONCE and run by
// the device kernel (block_slq.hip, one thread per column) and by the host path of solvers.cpp, as cg_state.hpp and
// lsqr_state.hpp do for their recurrences.
//
// The coefficients alpha_k, beta_k of m steps of (preconditioned) CG started from z are the Lanczos tridiagonal T (m x m) of
// P^-1/2 (A + D) P^-1/2 started at u = P^-1/2 z:
//     T[k, k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1}          T[k, k+1] = sqrt(beta_k) / alpha_k
// and  rho0 * e1' f(T) e1 = rho0 * sum_i tau_i^2 f(lambda_i)  (rho0 = z'P^-1 z, lambda_i the eigenvalues of T, tau_i the first
// components of its eigenvectors) is the m-point Gauss rule for u' f(P^-1/2 (A + D) P^-1/2) u.  With f = log, its mean over
// z ~ N(0, P) is log det(A + D) - log det P.
//
// The eigenvalues and the tau_i come from the implicit QL iteration on T (EISPACK's imtql2) with the rotations applied to one
// row only, started at e1: 3 m numbers of work, m^2 rotations or so, no matrix.  All arrays are read with a stride, so that b
// columns can be interleaved (entry k of column j at k * stride + j) and neighbouring threads touch neighbouring words.
#pragma once
#include <cmath>
#include <cstdint>
#if defined(__HIPCC__)
#define GSI_HD __host__ __device__
#else
#define GSI_HD
#endif

namespace gsi { namespace slq {

constexpr int64_t QMAX_LIMIT = 4096;
constexpr int QL_SWEEPS = 60;          // per eigenvalue, as EISPACK allows 30: beyond it the value is NaN

GSI_HD inline size_t work_doubles(int64_t b, int64_t qmax) { return (size_t)3 * (size_t)qmax * (size_t)b; }

// d, e (m entries each, stride): T's diagonal and off-diagonal (e[m-1] = 0) from the trace
GSI_HD inline void tridiagonal(const double* alpha, const double* beta, int64_t m, int64_t stride, double* d, double* e) {
  for (int64_t k = 0; k < m; ++k) {
    const double a = alpha[k * stride];
    double t = 1.0 / a;
    if (k > 0) t += beta[(k - 1) * stride] / alpha[(k - 1) * stride];
    d[k * stride] = t;
    e[k * stride] = (k + 1 < m) ? std::sqrt(beta[k * stride]) / a : 0.0;
  }
}

// Implicit QL on (d, e), z <- e1' Q: on return d holds the eigenvalues and z the first components of the eigenvectors.
// false: an eigenvalue did not settle in QL_SWEEPS sweeps (or the input held a NaN).
GSI_HD inline bool ql_first_row(double* d, double* e, double* z, int64_t m, int64_t stride) {
#define GSI_SLQ_AT(a, i) a[(i) * stride]
  for (int64_t k = 0; k < m; ++k) GSI_SLQ_AT(z, k) = (k == 0) ? 1.0 : 0.0;
  for (int64_t l = 0; l < m; ++l) {
    int sweeps = 0;
    int64_t mm;
    do {
      for (mm = l; mm < m - 1; ++mm) {
        const double dd = std::fabs(GSI_SLQ_AT(d, mm)) + std::fabs(GSI_SLQ_AT(d, mm + 1));
        if (std::fabs(GSI_SLQ_AT(e, mm)) + dd == dd) break;
      }
      if (mm != l) {
        if (sweeps++ == QL_SWEEPS) return false;
        double g = (GSI_SLQ_AT(d, l + 1) - GSI_SLQ_AT(d, l)) / (2.0 * GSI_SLQ_AT(e, l));
        double r = std::hypot(g, 1.0);
        if (!(r <= 1.79769313486231570815e308)) return false;
        g = GSI_SLQ_AT(d, mm) - GSI_SLQ_AT(d, l) + GSI_SLQ_AT(e, l) / (g + (g >= 0.0 ? r : -r));
        double s = 1.0, c = 1.0, p = 0.0;
        int64_t i;
        for (i = mm - 1; i >= l; --i) {
          double f = s * GSI_SLQ_AT(e, i);
          const double bb = c * GSI_SLQ_AT(e, i);
          r = std::hypot(f, g);
          GSI_SLQ_AT(e, i + 1) = r;
          if (r == 0.0) {
            GSI_SLQ_AT(d, i + 1) -= p;
            GSI_SLQ_AT(e, mm) = 0.0;
            break;
          }
          s = f / r;
          c = g / r;
          g = GSI_SLQ_AT(d, i + 1) - p;
          r = (GSI_SLQ_AT(d, i) - g) * s + 2.0 * c * bb;
          p = s * r;
          GSI_SLQ_AT(d, i + 1) = g + p;
          g = c * r - bb;
          f = GSI_SLQ_AT(z, i + 1);
          GSI_SLQ_AT(z, i + 1) = s * GSI_SLQ_AT(z, i) + c * f;
          GSI_SLQ_AT(z, i) = c * GSI_SLQ_AT(z, i) - s * f;
        }
        if (r == 0.0 && i >= l) continue;
        GSI_SLQ_AT(d, l) -= p;
        GSI_SLQ_AT(e, l) = g;
        GSI_SLQ_AT(e, mm) = 0.0;
      }
    } while (mm != l);
  }
#undef GSI_SLQ_AT
  return true;
}

// rho0 * sum_i tau_i^2 log(lambda_i) for one column: alpha, beta point at the column's first step, d, e, z at its first
// work entry, all with the same stride.  m = 0: 0.  One step: rho0 * log(1 / alpha_0), no rotation.
GSI_HD inline double quadrature_log(const double* alpha, const double* beta, int64_t m, double rho0, int64_t stride,
                                    double* d, double* e, double* z) {
  if (m <= 0) return 0.0;
  tridiagonal(alpha, beta, m, stride, d, e);
  if (!ql_first_row(d, e, z, m, stride)) return std::nan("");
  double acc = 0.0;
  for (int64_t k = 0; k < m; ++k) {
    const double t = z[k * stride];
    acc += t * t * std::log(d[k * stride]);
  }
  return rho0 * acc;
}

}}  // namespace gsi::slq
