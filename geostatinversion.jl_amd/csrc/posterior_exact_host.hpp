// posterior_exact_host.hpp -- the host side of the exact posterior variance of linear inversion and kriging (DESIGN.md
// section 4.6m): the row pass of posterior_exact.hip, the assembly of the doubled trapezoid and the finishing formula as plain
// C++ on host arrays.  The row pass and the assembly run here when the backend declines (Backend::rowdot_acc, unit_panel,
// trapezoid_rows, carried_rows say "not mine") or GSI_POSTX_HOST=1; the small p x p algebra and the finish run here on every path.  It is what
// the CPU tests and tests/posterior_exact_host_check.cpp exercise.  Nothing here depends on a backend.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

// the row pass is stated product by product: no fused multiply-add may merge a product with the add behind it
#if defined(__clang__)
#define GSI_POSTX_NO_CONTRACT
#define GSI_POSTX_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define GSI_POSTX_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#define GSI_POSTX_NO_CONTRACT_BODY
#else
#define GSI_POSTX_NO_CONTRACT
#define GSI_POSTX_NO_CONTRACT_BODY
#endif

namespace gsi { namespace postx_host {

// acc[i] += sum over c < b of A[i, c] B[i, c] for column-major n x b panels: every product rounded on its own and added to
// the row's running sum in ascending c, starting from acc[i].  B == A: the sum of squares.
GSI_POSTX_NO_CONTRACT inline void rowdot_acc(int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb,
                                             double* acc) {
  GSI_POSTX_NO_CONTRACT_BODY
  for (int64_t c = 0; c < b; ++c) {
    const double* a = A + (size_t)c * (size_t)lda;
    const double* bb = B + (size_t)c * (size_t)ldb;
    for (int64_t i = 0; i < n; ++i) {
      const double prod = a[i] * bb[i];
      acc[i] = acc[i] + prod;
    }
  }
}

// E (nobs x b, ld): zeros with a one at (c0 + c, c)
inline void unit_panel(double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) {
  for (int64_t c = 0; c < b; ++c)
    for (int64_t r = 0; r < nobs; ++r) E[(size_t)r + (size_t)c * (size_t)ld] = (r == c0 + c) ? 1.0 : 0.0;
}

// The (2 nobs + p) x nobs trapezoid T (ld) whose top nobs x nobs holds H C H': diag (nobs values, or null) is added to the
// diagonal, rows [nobs, nobs + p) <- Phi' (Phi: nobs x p, ld ldphi), rows [nobs + p, 2 nobs + p) <- I.
inline void assemble(double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi, int64_t ldphi) {
  for (int64_t j = 0; j < nobs; ++j) {
    double* cj = T + (size_t)j * (size_t)ld;
    if (diag) cj[j] += diag[j];
    for (int64_t k = 0; k < p; ++k) cj[nobs + k] = Phi[(size_t)j + (size_t)k * (size_t)ldphi];
    for (int64_t i = 0; i < nobs; ++i) cj[nobs + p + i] = (i == j) ? 1.0 : 0.0;
  }
}

// Wd (nobs x p, ld nobs) <- the transpose of the p carried rows of the factored trapezoid, W_d = L^-1 Phi.  rows: the first of
// them (element (nobs, 0) of the trapezoid with its ld, or a p x nobs copy of the rows with ld = p).
inline void carried_rows(const double* rows, int64_t ld, int64_t nobs, int64_t p, double* Wd) {
  for (int64_t k = 0; k < p; ++k)
    for (int64_t j = 0; j < nobs; ++j) Wd[(size_t)j + (size_t)k * (size_t)nobs] = rows[(size_t)k + (size_t)j * (size_t)ld];
}

// Lower Cholesky factor of the p x p S (ld p, lower triangle read) in place.  Returns 0, or the 1-based column whose pivot is
// not finite or has fallen to 64 eps times the diagonal entry it started from: the drift columns H X are then linearly
// dependent to rounding (S = Phi' M^-1 Phi is singular exactly when Phi is rank deficient).
inline int64_t chol_small(double* S, int64_t p) {
  const double floor_rel = 64.0 * 2.220446049250313e-16;
  for (int64_t j = 0; j < p; ++j) {
    const double d0 = S[j + j * p];
    double d = d0;
    for (int64_t t = 0; t < j; ++t) d -= S[j + t * p] * S[j + t * p];
    if (!std::isfinite(d) || !(d > floor_rel * d0)) return j + 1;
    const double r = std::sqrt(d);
    S[j + j * p] = r;
    for (int64_t i = j + 1; i < p; ++i) {
      double v = S[i + j * p];
      for (int64_t t = 0; t < j; ++t) v -= S[i + t * p] * S[j + t * p];
      S[i + j * p] = v / r;
    }
  }
  return 0;
}

// var[i] = c00 - acc[i] + |Ls^-1 (x_i - u_i)|^2 with x_i the rows of X (n x p, ld ldx), u_i the rows of U (n x p, ld ldu) and
// Ls the p x p lower factor of chol_small (ld p).  p == 0: the first two terms.
inline void finish(int64_t n, int64_t p, double c00, const double* acc, const double* U, int64_t ldu, const double* X,
                   int64_t ldx, const double* Ls, double* var) {
  std::vector<double> z((size_t)(p > 0 ? p : 1));
  for (int64_t i = 0; i < n; ++i) {
    double q = 0.0;
    for (int64_t k = 0; k < p; ++k) {
      double v = X[(size_t)i + (size_t)k * (size_t)ldx] - U[(size_t)i + (size_t)k * (size_t)ldu];
      for (int64_t t = 0; t < k; ++t) v -= Ls[k + t * p] * z[(size_t)t];
      v /= Ls[k + k * p];
      z[(size_t)k] = v;
      q += v * v;
    }
    var[i] = (c00 - acc[i]) + q;
  }
}

}}  // namespace gsi::postx_host
