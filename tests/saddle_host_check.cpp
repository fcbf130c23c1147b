// saddle_host_check.cpp -- the host path of the direct saddle-point solver (csrc/saddle_host.hpp) as a program of its own,
// built with -fsanitize=address,undefined by tests/test_saddle_solve_cpu.py.  The cases are those of tests/saddle_cases.py:
// exact integer factors (bit for bit, with and without a leading dimension), exact failure columns, rows carried through
// the factorization, the singular system, and a small saddle-point system against its residual.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "saddle_host.hpp"

namespace {
uint64_t g_state = 88172645463325252ull;
uint64_t next_u64() {                      // xorshift64
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return g_state;
}
double unit() { return (double)(next_u64() >> 11) / 9007199254740992.0 - 0.5; }

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                      \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

// L0: integer lower triangular, diagonal from {1, 2, 4}, off-diagonals from {-3 .. 3}; A = L0 L0' (ld lda, lower triangle
// only: the upper triangle holds NaN and must not be read)
void exact_case(int64_t n, int64_t lda, std::vector<double>& L0, std::vector<double>& A) {
  L0.assign((size_t)n * n, 0.0);
  for (int64_t j = 0; j < n; ++j) {
    L0[(size_t)(j + j * n)] = (double)(1 << (next_u64() % 3));
    for (int64_t i = j + 1; i < n; ++i) L0[(size_t)(i + j * n)] = (double)((int)(next_u64() % 7) - 3);
  }
  A.assign((size_t)lda * n, std::nan(""));
  for (int64_t j = 0; j < n; ++j)
    for (int64_t i = j; i < n; ++i) {
      double s = 0.0;
      for (int64_t t = 0; t <= j; ++t) s += L0[(size_t)(i + t * n)] * L0[(size_t)(j + t * n)];
      A[(size_t)(i + j * lda)] = s;
    }
}
}  // namespace

int main() {
  using namespace gsi::saddle_host;
  const int64_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 200};
  std::vector<double> L0, A;
  for (int64_t n : sizes) {
    for (int64_t lda : {n, n + 11}) {
      exact_case(n, lda, L0, A);
      CHECK(chol_lower(A.data(), n, n, lda) == 0);
      for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j; i < n; ++i) CHECK(A[(size_t)(i + j * lda)] == L0[(size_t)(i + j * n)]);
    }
    // the same matrix with the pivot of column j made exactly -1
    for (int64_t j : {(int64_t)0, (int64_t)63, (int64_t)64, (int64_t)65, n - 1}) {
      if (j >= n) continue;
      exact_case(n, n, L0, A);
      A[(size_t)(j + j * n)] -= L0[(size_t)(j + j * n)] * L0[(size_t)(j + j * n)] + 1.0;
      CHECK(chol_lower(A.data(), n, n, n) == j + 1);
    }
  }
  {  // two integer rows carried below the matrix come out as (L0^-1 B')': B = C L0' for an integer C gives C back exactly
    const int64_t n = 70, m = n + 2;
    exact_case(n, n, L0, A);
    std::vector<double> W((size_t)m * n), Cm((size_t)2 * n);
    for (auto& v : Cm) v = (double)((int)(next_u64() % 5) - 2);
    for (int64_t j = 0; j < n; ++j) {
      for (int64_t i = 0; i < n; ++i) W[(size_t)(i + j * m)] = A[(size_t)(i + j * n)];
      for (int r = 0; r < 2; ++r) {
        double s = 0.0;
        for (int64_t t = 0; t <= j; ++t) s += Cm[(size_t)(r + 2 * t)] * L0[(size_t)(j + t * n)];
        W[(size_t)(n + r + j * m)] = s;
      }
    }
    CHECK(chol_lower(W.data(), m, n, m) == 0);
    for (int64_t j = 0; j < n; ++j)
      for (int r = 0; r < 2; ++r) CHECK(W[(size_t)(n + r + j * m)] == Cm[(size_t)(r + 2 * j)]);
  }
  for (int diag = 0; diag < 2; ++diag) {  // a saddle-point system: residual of the solution, diagonal and dense R
    const int64_t nobs = 83, K = 5;
    std::vector<double> E((size_t)nobs * K), HX((size_t)nobs), b((size_t)nobs + 1), x((size_t)nobs + 1),
        R(diag ? (size_t)nobs : (size_t)nobs * nobs, 0.0);
    for (auto& v : E) v = unit();
    for (auto& v : HX) v = unit();
    for (auto& v : b) v = unit();
    for (int64_t i = 0; i < nobs; ++i) R[(size_t)(diag ? i : i + i * nobs)] = 0.25 + 0.01 * (double)i;
    if (!diag)
      for (int64_t i = 1; i < nobs; ++i) R[(size_t)(i + (i - 1) * nobs)] = R[(size_t)(i - 1 + i * nobs)] = 0.05;
    CHECK(solve(E.data(), nobs, K, HX.data(), R.data(), diag != 0, b.data(), x.data()) == 0);
    double worst = 0.0;
    for (int64_t i = 0; i <= nobs; ++i) {
      double s = 0.0;
      if (i < nobs) {
        for (int64_t j = 0; j < nobs; ++j) {
          double a = diag ? (i == j ? R[(size_t)i] : 0.0) : R[(size_t)(i + j * nobs)];
          for (int64_t t = 0; t < K; ++t) a += E[(size_t)(i + t * nobs)] * E[(size_t)(j + t * nobs)];
          s += a * x[(size_t)j];
        }
        s += HX[(size_t)i] * x[(size_t)nobs];
      } else {
        for (int64_t j = 0; j < nobs; ++j) s += HX[(size_t)j] * x[(size_t)j];
      }
      worst = std::fmax(worst, std::fabs(s - b[(size_t)i]));
    }
    CHECK(worst < 1e-11);
    // HX = 0: singular
    std::vector<double> zero((size_t)nobs, 0.0);
    CHECK(solve(E.data(), nobs, K, zero.data(), R.data(), diag != 0, b.data(), x.data()) == -2);
    // R = -I: not positive definite, and the column is reported
    std::vector<double> neg((size_t)nobs, -1.0);
    CHECK(solve(E.data(), nobs, K, HX.data(), neg.data(), true, b.data(), x.data()) > 0);
  }
  std::printf("saddle host ok\n");
  return 0;
}
