// posterior_host.hpp -- the host path of the PCGA posterior variance: the capacitance-form factor and
// the row pass of posterior_var.hip as plain C++ on host arrays.  It runs when the backend declines (Backend::chol_lower /
// basis_quadform say "not mine") or GSI_POST_HOST=1, and it is what the CPU tests and tests/posterior_host_check.cpp
// exercise.  Nothing here depends on a backend.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "saddle_host.hpp"

namespace gsi { namespace posterior_host {

// From E (nobs x K, ld nobs), w = HX (nobs) and R (nobs x nobs, ld nobs, lower triangle read; or its nobs diagonal entries):
//   B = L_R^-1 E, wt = L_R^-1 w, N = I + B'B = L_N L_N', W = L_N^-T (K x K, ld K, strictly lower part zero),
//   r = B'wt, u = N^-1 r, gamma = wt'wt - r'u.
// Returns 0; the 1-based column at which R stopped being positive definite (a diagonal entry that is not a positive finite
// number); or -2: w = 0, or gamma is not a positive finite number.  W, u, gamma are meaningful only on 0.
inline int64_t factor(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag, double* W,
                      double* u, double* gamma) {
  std::vector<double> B((size_t)nobs * (size_t)K), wt((size_t)nobs);
  if (r_diag) {
    for (int64_t i = 0; i < nobs; ++i)
      if (!(R[i] > 0.0) || !std::isfinite(R[i])) return i + 1;
    for (int64_t i = 0; i < nobs; ++i) {
      const double d = 1.0 / std::sqrt(R[i]);
      wt[(size_t)i] = d * HX[i];
      for (int64_t c = 0; c < K; ++c) B[(size_t)(i + c * nobs)] = d * E[i + c * nobs];
    }
  } else {
    // one factorization of the trapezoid [R; E'; w']: the carried rows come back as B' and wt'
    const int64_t ld = nobs + K + 1;
    std::vector<double> T((size_t)ld * (size_t)nobs);
    for (int64_t j = 0; j < nobs; ++j) {
      double* cj = T.data() + (size_t)j * (size_t)ld;
      for (int64_t i = 0; i < nobs; ++i) cj[i] = i >= j ? R[i + j * nobs] : 0.0;
      for (int64_t c = 0; c < K; ++c) cj[nobs + c] = E[j + c * nobs];
      cj[nobs + K] = HX[j];
    }
    const int64_t col = saddle_host::chol_lower(T.data(), ld, nobs, ld);
    if (col != 0) return col;
    for (int64_t j = 0; j < nobs; ++j) {
      const double* cj = T.data() + (size_t)j * (size_t)ld;
      for (int64_t c = 0; c < K; ++c) B[(size_t)(j + c * nobs)] = cj[nobs + c];
      wt[(size_t)j] = cj[nobs + K];
    }
  }
  // the 2K x K trapezoid [N; I]: chol_lower leaves [L_N; L_N^-T]
  const int64_t ld2 = 2 * K;
  std::vector<double> T2((size_t)ld2 * (size_t)K, 0.0), r((size_t)K), y((size_t)K);
  for (int64_t j = 0; j < K; ++j) {
    double* cj = T2.data() + (size_t)j * (size_t)ld2;
    const double* bj = B.data() + (size_t)j * (size_t)nobs;
    for (int64_t i = j; i < K; ++i) {
      const double* bi = B.data() + (size_t)i * (size_t)nobs;
      double s = 0.0;
      for (int64_t o = 0; o < nobs; ++o) s += bi[o] * bj[o];
      cj[i] = s;
    }
    cj[j] += 1.0;
    cj[K + j] = 1.0;
    double s = 0.0;
    for (int64_t o = 0; o < nobs; ++o) s += bj[o] * wt[(size_t)o];
    r[(size_t)j] = s;
  }
  const int64_t col2 = saddle_host::chol_lower(T2.data(), ld2, K, ld2);
  if (col2 != 0) return -2;                                  // N = I + B'B has eigenvalues >= 1: only non-finite input gets here
  for (int64_t j = 0; j < K; ++j)
    for (int64_t i = 0; i < K; ++i) W[i + j * K] = i <= j ? T2[(size_t)(K + i + j * ld2)] : 0.0;
  double ww = 0.0, ru = 0.0;
  for (int64_t o = 0; o < nobs; ++o) ww += wt[(size_t)o] * wt[(size_t)o];
  for (int64_t j = 0; j < K; ++j) {                          // y = W'r
    double s = 0.0;
    for (int64_t i = 0; i <= j; ++i) s += W[i + j * K] * r[(size_t)i];
    y[(size_t)j] = s;
  }
  for (int64_t i = 0; i < K; ++i) {                          // u = W y
    double s = 0.0;
    for (int64_t j = i; j < K; ++j) s += W[i + j * K] * y[(size_t)j];
    u[i] = s;
  }
  for (int64_t j = 0; j < K; ++j) ru += r[(size_t)j] * u[j];
  *gamma = ww - ru;
  if (!(ww > 0.0) || !std::isfinite(*gamma) || !(*gamma > 0.0)) return -2;
  return 0;
}

// a[i] = |W' z_i|^2, q[i] = |z_i|^2 (q may be null), t[i] = u' z_i (u, t null together) over the rows of Z (n x K, ld ldz,
// double or float); W: K x ncols, ld ldw; upper: W[k, j] with k > j is zero and not read.
template <typename T>
inline void quadform(const T* Z, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw, int64_t ncols, bool upper,
                     const double* u, double* a, double* q, double* t) {
  std::vector<double> z((size_t)K);
  for (int64_t i = 0; i < n; ++i) {
    double sq = 0.0, st = 0.0, sa = 0.0;
    for (int64_t k = 0; k < K; ++k) {
      const double v = (double)Z[(size_t)k * (size_t)ldz + (size_t)i];
      z[(size_t)k] = v;
      sq += v * v;
      if (u) st += v * u[k];
    }
    for (int64_t j = 0; j < ncols; ++j) {
      const double* wj = W + (size_t)j * (size_t)ldw;
      const int64_t kend = upper ? (j + 1 < K ? j + 1 : K) : K;
      double p = 0.0;
      for (int64_t k = 0; k < kend; ++k) p += z[(size_t)k] * wj[k];
      sa += p * p;
    }
    a[i] = sa;
    if (q) q[i] = sq;
    if (t) t[i] = st;
  }
}

// var[i] = a_i + (t_i - X_i)^2 / gamma, plus prior_i - q_i when the caller gives the true prior variances
inline void finish(int64_t n, const double* a, const double* q, const double* t, const double* X, const double* prior,
                   double gamma, double* var) {
  for (int64_t i = 0; i < n; ++i) {
    const double d = t[i] - X[i];
    const double v = a[i] + d * d / gamma;
    var[i] = prior ? (prior[i] - q[i]) + v : v;
  }
}

}}  // namespace gsi::posterior_host
