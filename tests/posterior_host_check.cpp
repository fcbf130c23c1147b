// The host path of the posterior variance (posterior_host.hpp) as a program of its own, for the address and undefined-behaviour
// sanitizers: every array is a heap block of exactly the size the interface promises, on the smallest and the odd shapes
// (K = 1, n = 1, nobs = 1, ncols != K, a leading dimension, a triangular W whose lower part is NaN), checked against long
// double restatements.  tests/test_posterior_cpu.py builds and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "posterior_host.hpp"

namespace ph = gsi::posterior_host;

static uint64_t g_state = 88172645463325252ull;
static double rnd() {                                  // xorshift: uniform in (-1, 1)
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

static int g_bad = 0;
static void expect(bool ok, const char* what, int64_t a, int64_t b, int64_t c) {
  if (!ok) { std::printf("FAILED %s (%lld, %lld, %lld)\n", what, (long long)a, (long long)b, (long long)c); ++g_bad; }
}

template <typename T>
static void check_quadform(int64_t n, int64_t K, int64_t ncols, int64_t ldw, bool upper, bool with_u) {
  std::vector<T> Z((size_t)(n * K));
  for (auto& z : Z) z = (T)rnd();
  std::vector<double> W((size_t)(ldw * (ncols - 1) + K)), u((size_t)K), a((size_t)n), q((size_t)n), t((size_t)n);
  for (int64_t j = 0; j < ncols; ++j)
    for (int64_t k = 0; k < K; ++k)
      W[(size_t)(k + j * ldw)] = (upper && k > j) ? std::numeric_limits<double>::quiet_NaN() : rnd();
  for (auto& v : u) v = rnd();
  ph::quadform(Z.data(), n, n, K, W.data(), ldw, ncols, upper, with_u ? u.data() : nullptr, a.data(), q.data(),
               with_u ? t.data() : nullptr);
  for (int64_t i = 0; i < n; ++i) {
    long double sa = 0, sq = 0, st = 0;
    for (int64_t k = 0; k < K; ++k) {
      const long double z = Z[(size_t)(i + k * n)];
      sq += z * z;
      st += z * u[(size_t)k];
    }
    for (int64_t j = 0; j < ncols; ++j) {
      long double p = 0;
      for (int64_t k = 0; k < K && (!upper || k <= j); ++k) p += (long double)Z[(size_t)(i + k * n)] * W[(size_t)(k + j * ldw)];
      sa += p * p;
    }
    const double tol = 1e-13 * (double)(K + ncols);
    expect(std::fabs((double)(a[(size_t)i] - sa)) <= tol * (1.0 + (double)sa), "a", n, K, ncols);
    expect(std::fabs((double)(q[(size_t)i] - sq)) <= tol * (1.0 + (double)sq), "q", n, K, ncols);
    if (with_u) expect(std::fabs((double)(t[(size_t)i] - st)) <= tol * (1.0 + std::fabs((double)st)), "t", n, K, ncols);
  }
}

static void check_factor(int64_t nobs, int64_t K, bool r_diag) {
  std::vector<double> E((size_t)(nobs * K)), HX((size_t)nobs), R(r_diag ? (size_t)nobs : (size_t)(nobs * nobs)), W((size_t)(K * K)),
      u((size_t)K);
  for (auto& v : E) v = rnd();
  for (auto& v : HX) v = 1.0 + 0.5 * rnd();
  if (r_diag) {
    for (auto& v : R) v = 1.0 + 0.5 * rnd();
  } else {
    for (int64_t j = 0; j < nobs; ++j)
      for (int64_t i = 0; i < nobs; ++i) R[(size_t)(i + j * nobs)] = (i == j ? 2.0 + (double)nobs * 0.1 : 0.1 * std::cos((double)(i + j)));
  }
  double gamma = 0.0;
  const int64_t st = ph::factor(E.data(), nobs, K, HX.data(), R.data(), r_diag, W.data(), u.data(), &gamma);
  expect(st == 0, "factor status", nobs, K, r_diag);
  expect(gamma > 0.0 && std::isfinite(gamma), "gamma", nobs, K, r_diag);
  // gamma = w' (E E' + R)^-1 w and u = E' (E E' + R)^-1 w, by a dense long double solve
  const int64_t m = nobs;
  std::vector<long double> M((size_t)(m * m)), x((size_t)m);
  for (int64_t j = 0; j < m; ++j)
    for (int64_t i = 0; i < m; ++i) {
      long double s = r_diag ? (i == j ? (long double)R[(size_t)i] : 0.0L) : (long double)R[(size_t)((i >= j ? i : j) + (i >= j ? j : i) * nobs)];
      for (int64_t k = 0; k < K; ++k) s += (long double)E[(size_t)(i + k * nobs)] * E[(size_t)(j + k * nobs)];
      M[(size_t)(i + j * m)] = s;
    }
  for (int64_t i = 0; i < m; ++i) x[(size_t)i] = HX[(size_t)i];
  for (int64_t j = 0; j < m; ++j) {                    // symmetric positive definite: elimination without pivoting
    for (int64_t i = j + 1; i < m; ++i) {
      const long double f = M[(size_t)(i + j * m)] / M[(size_t)(j + j * m)];
      for (int64_t c = j; c < m; ++c) M[(size_t)(i + c * m)] -= f * M[(size_t)(j + c * m)];
      x[(size_t)i] -= f * x[(size_t)j];
    }
  }
  for (int64_t j = m - 1; j >= 0; --j) {
    long double s = x[(size_t)j];
    for (int64_t c = j + 1; c < m; ++c) s -= M[(size_t)(j + c * m)] * x[(size_t)c];
    x[(size_t)j] = s / M[(size_t)(j + j * m)];
  }
  long double g = 0;
  for (int64_t i = 0; i < m; ++i) g += (long double)HX[(size_t)i] * x[(size_t)i];
  expect(std::fabs((double)(gamma - g)) <= 1e-11 * std::fabs((double)g), "gamma value", nobs, K, r_diag);
  for (int64_t k = 0; k < K; ++k) {
    long double s = 0;
    for (int64_t i = 0; i < m; ++i) s += (long double)E[(size_t)(i + k * nobs)] * x[(size_t)i];
    expect(std::fabs((double)(u[(size_t)k] - s)) <= 1e-11 * (1.0 + std::fabs((double)s)), "u value", nobs, K, k);
  }
  for (int64_t j = 0; j < K; ++j)
    for (int64_t i = j + 1; i < K; ++i) expect(W[(size_t)(i + j * K)] == 0.0, "W lower part", nobs, K, i);
}

int main() {
  const int64_t ns[] = {1, 2, 17}, Ks[] = {1, 2, 5, 17};
  for (int64_t n : ns)
    for (int64_t K : Ks)
      for (int64_t ncols : {(int64_t)1, K, K + 3})
        for (int pad = 0; pad < 2; ++pad)
          for (int up = 0; up < 2; ++up) {
            check_quadform<double>(n, K, ncols, K + 3 * pad, up != 0, true);
            check_quadform<float>(n, K, ncols, K + 3 * pad, up != 0, up == 0);
          }
  for (int64_t nobs : {(int64_t)1, (int64_t)2, (int64_t)9})
    for (int64_t K : Ks) {
      check_factor(nobs, K, true);
      check_factor(nobs, K, false);
    }
  // the failures: a zero diagonal entry, a dense R that is not positive definite, HX = 0
  {
    double E[2] = {1.0, 2.0}, HX[2] = {1.0, 1.0}, Rd[2] = {1.0, 0.0}, W[1], u[1], g = 0.0;
    expect(ph::factor(E, 2, 1, HX, Rd, true, W, u, &g) == 2, "zero diagonal entry", 2, 1, 0);
    double Rn[4] = {1.0, 2.0, 2.0, 1.0};
    expect(ph::factor(E, 2, 1, HX, Rn, false, W, u, &g) == 2, "indefinite dense R", 2, 1, 0);
    double Z0[2] = {0.0, 0.0}, R1[2] = {1.0, 1.0};
    expect(ph::factor(E, 2, 1, Z0, R1, true, W, u, &g) == -2, "HX = 0", 2, 1, 0);
  }
  if (g_bad != 0) return 1;
  std::printf("posterior host ok\n");
  return 0;
}
