// saddle_host.hpp -- the host path of pcgadirect's saddle-point solve: the algebra of
// chol_saddle.hip as plain unblocked C++ on host arrays.  It runs when the backend declines (Backend::saddle_solve /
// chol_lower return -1) or GSI_SADDLE_HOST=1, and it is what the CPU tests and tests/saddle_host_check.cpp exercise.
// Nothing here depends on a backend.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace gsi { namespace saddle_host {

// The m x n column-major trapezoid A (m >= n, ld; lower triangle of the top n x n read) <- [L; (L^-1 B')'] in place, where B is
// rows n .. m-1.  Left-looking by columns.  Returns 0, or the 1-based column whose pivot is not a positive finite number
// (columns before it are factored, the rest is untouched past the updates of that column).
inline int64_t chol_lower(double* A, int64_t m, int64_t n, int64_t ld) {
  for (int64_t j = 0; j < n; ++j) {
    double* cj = A + j * ld;
    for (int64_t t = 0; t < j; ++t) {
      const double* ct = A + t * ld;
      const double a = ct[j];
      for (int64_t i = j; i < m; ++i) cj[i] -= a * ct[i];
    }
    const double d = cj[j];
    if (!(d > 0.0) || !std::isfinite(d)) return j + 1;
    const double r = std::sqrt(d);
    cj[j] = r;
    for (int64_t i = j + 1; i < m; ++i) cj[i] /= r;
  }
  return 0;
}

// W ((nobs + 2) x nobs, ld >= nobs + 2): lower triangle of E E' + R, then HX' and b1' as rows nobs, nobs + 1.
// E: nobs x K (ld nobs); R: nobs x nobs (ld nobs, lower triangle read) or, with r_diag, its nobs diagonal entries.
inline void form(double* W, int64_t ld, int64_t nobs, int64_t K, const double* E, const double* R, bool r_diag, const double* HX,
                 const double* b) {
  for (int64_t j = 0; j < nobs; ++j) {
    double* cj = W + j * ld;
    for (int64_t i = 0; i < j; ++i) cj[i] = 0.0;
    for (int64_t i = j; i < nobs; ++i) cj[i] = 0.0;
    for (int64_t t = 0; t < K; ++t) {
      const double* et = E + t * nobs;
      const double e = et[j];
      for (int64_t i = j; i < nobs; ++i) cj[i] += e * et[i];
    }
    if (r_diag) cj[j] += R[j];
    else for (int64_t i = j; i < nobs; ++i) cj[i] += R[i + j * nobs];
    cj[nobs] = HX[j];
    cj[nobs + 1] = b[j];
  }
}

// x (nobs + 1) = [(E E' + R) HX; HX' 0] \ b.  Returns 0, the 1-based column at which E E' + R stopped being positive
// definite, or -2: w'w is zero or beta is not finite (HX = 0 makes the saddle-point matrix singular).
inline int64_t solve(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag, const double* b,
                     double* x) {
  const int64_t ld = nobs + 2;
  std::vector<double> W((size_t)ld * (size_t)nobs);
  form(W.data(), ld, nobs, K, E, R, r_diag, HX, b);
  const int64_t col = chol_lower(W.data(), nobs + 2, nobs, ld);
  if (col != 0) return col;
  double ww = 0.0, wv = 0.0;                         // w = L^-1 HX, v = L^-1 b1: rows nobs, nobs + 1
  for (int64_t c = 0; c < nobs; ++c) {
    const double w = W[(size_t)(nobs + c * ld)], v = W[(size_t)(nobs + 1 + c * ld)];
    ww += w * w;
    wv += w * v;
  }
  const double beta = (wv - b[nobs]) / ww;
  if (!(ww > 0.0) || !std::isfinite(ww) || !std::isfinite(beta)) return -2;
  for (int64_t c = 0; c < nobs; ++c) x[c] = W[(size_t)(nobs + 1 + c * ld)] - beta * W[(size_t)(nobs + c * ld)];
  for (int64_t j = nobs - 1; j >= 0; --j) {          // L' xi = v - beta w
    const double* cj = W.data() + j * ld;
    double v = x[j];
    for (int64_t i = j + 1; i < nobs; ++i) v -= cj[i] * x[i];
    x[j] = v / cj[j];
  }
  x[nobs] = beta;
  return 0;
}

}}  // namespace gsi::saddle_host
