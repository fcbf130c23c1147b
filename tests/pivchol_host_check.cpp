// The scalar rules (pchol_state.hpp) and the host path (pivoted_chol_host.hpp) of the diagonal-pivoted Cholesky factorization
// as a program of its own, for the address and undefined-behaviour sanitizers: every array is a heap block of exactly the
// size the interface promises, on the smallest and the odd shapes (n = 1, K = 1, K = n, a leading dimension larger than n,
// a rank-deficient matrix, a zero matrix, a NaN), checked against a long double restatement of the identities.
// tests/test_pivchol_cpu.py builds and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "pivoted_chol_host.hpp"

namespace pc = gsi::pchol;

static uint64_t g_state = 88172645463325252ull;
static double rnd() {                                  // xorshift: uniform in (-1, 1)
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

static int g_bad = 0;
static void expect(bool ok, const char* what, int64_t a, int64_t b, int64_t c) {
  if (!ok) { std::printf("FAILED %s (%lld, %lld, %lld)\n", what, (long long)a, (long long)b, (long long)c); ++g_bad; }
}

// A = B B' + shift I, B n x r
static std::vector<double> gram(int64_t n, int64_t r, double shift) {
  std::vector<double> B((size_t)(n * r)), A((size_t)(n * n));
  for (auto& v : B) v = rnd();
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) {
      double s = (i == j) ? shift : 0.0;
      for (int64_t k = 0; k < r; ++k) s += B[(size_t)(i + k * n)] * B[(size_t)(j + k * n)];
      A[(size_t)(i + j * n)] = s;
    }
  return A;
}

struct Result { int64_t rank, reason, fetched; std::vector<double> L, d, st; };

static Result run(const std::vector<double>& A, int64_t n, int64_t K, double tol, int64_t ldl) {
  Result r;
  r.d.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) r.d[(size_t)i] = A[(size_t)(i + i * n)];
  r.L.assign((size_t)(ldl * (K - 1) + n), std::numeric_limits<double>::quiet_NaN());     // exactly what n x K with ld ldl spans
  r.fetched = pc::host_factor(n, K, tol, r.d.data(), [&](int64_t p, double* out) {
    expect(p >= 0 && p < n, "pivot in range", n, K, p);
    for (int64_t i = 0; i < n; ++i) out[i] = A[(size_t)(i + p * n)];
  }, r.L.data(), ldl, r.st);
  r.rank = (int64_t)r.st[pc::S_STEP];
  r.reason = (int64_t)r.st[pc::S_REASON];
  return r;
}

// A - L L' vanishes on the pivot columns, its diagonal is d, columns from the rank on are zeros, the pivots are distinct
static void check_identities(const std::vector<double>& A, int64_t n, int64_t K, int64_t ldl, const Result& r) {
  expect(r.st.size() == pc::state_doubles(K), "state size", n, K, (int64_t)r.st.size());
  expect(r.fetched == r.rank, "one column per step", n, K, r.fetched);
  double amax = 0.0;
  for (double v : A) amax = std::fmax(amax, std::fabs(v));
  const double tol = 64.0 * (double)(K + 2) * std::numeric_limits<double>::epsilon() * (amax > 0.0 ? amax : 1.0);
  std::vector<char> seen((size_t)n, 0);
  for (int64_t j = 0; j < r.rank; ++j) {
    const int64_t p = (int64_t)r.st[(size_t)(pc::S_COUNT + j)];
    expect(p >= 0 && p < n && !seen[(size_t)p], "distinct pivots", n, K, j);
    if (p < 0 || p >= n) return;
    seen[(size_t)p] = 1;
    // (zero exactly when its step ends; later steps subtract the squares of entries that are zero up to rounding)
    expect(std::fabs(r.d[(size_t)p]) <= tol && r.d[(size_t)p] <= 0.0, "d_p is zero", n, K, j);
    for (int64_t i = 0; i < n; ++i) {
      long double s = 0;
      for (int64_t c = 0; c < r.rank; ++c) s += (long double)r.L[(size_t)(i + c * ldl)] * r.L[(size_t)(p + c * ldl)];
      expect(std::fabs((double)(A[(size_t)(i + p * n)] - s)) <= tol, "pivot column", n, K, j);
    }
  }
  for (int64_t i = 0; i < n; ++i) {
    long double s = 0;
    for (int64_t c = 0; c < r.rank; ++c) s += (long double)r.L[(size_t)(i + c * ldl)] * r.L[(size_t)(i + c * ldl)];
    expect(std::fabs((double)(A[(size_t)(i + i * n)] - s - r.d[(size_t)i])) <= tol, "diagonal", n, K, i);
    for (int64_t c = r.rank; c < K; ++c) expect(r.L[(size_t)(i + c * ldl)] == 0.0, "zero columns", n, K, c);
  }
}

static void check_rules() {
  // the lowest index wins among equals, in whatever order the partial results are joined
  pc::Red a = pc::red_identity(), b = pc::red_identity(), ab, ba;
  pc::red_row(a, 2.0, 7, false); pc::red_row(a, 1.0, 8, false);
  pc::red_row(b, 2.0, 3, false); pc::red_row(b, -1.0, 4, false);
  ab = a; pc::red_join(ab, b);
  ba = b; pc::red_join(ba, a);
  expect(ab.dmax == 2.0 && ab.idx == 3.0 && ba.idx == 3.0, "lowest index", 0, 0, 0);
  expect(ab.possum == 5.0 && ba.possum == 5.0 && ab.bad == 0.0, "positive sum", 0, 0, 0);
  pc::Red c = pc::red_identity();
  pc::red_row(c, std::numeric_limits<double>::quiet_NaN(), 0, false);
  pc::red_row(c, 1.0, 1, false);
  expect(c.bad == 1.0 && c.dmax == 1.0 && c.idx == 1.0, "a NaN is flagged and never the maximum", 0, 0, 0);
  pc::Red e = pc::red_identity();
  pc::red_row(e, std::numeric_limits<double>::infinity(), 0, false);
  expect(e.bad == 1.0, "an infinity is flagged", 0, 0, 0);
  // the order of the tests: non-finite, exhausted, trace, rank
  std::vector<double> s(pc::state_doubles(2));
  pc::begin(s.data(), 2, 0.5);
  pc::decide(s.data(), pc::Red{4.0, 1.0, 8.0, 0.0}, true);
  expect(s[pc::S_REASON] == 0.0 && s[pc::S_PIVOT] == 1.0 && s[pc::S_ROOT] == 2.0 && s[pc::S_TRACE0] == 8.0, "first decision", 0, 0, 0);
  pc::decide(s.data(), pc::Red{1.0, 0.0, 4.0, 0.0}, false);                    // 4 <= 0.5 * 8
  expect(s[pc::S_REASON] == 2.0 && s[pc::S_STEP] == 1.0, "trace rule", 0, 0, 0);
  pc::decide(s.data(), pc::Red{1.0, 0.0, 4.0, 1.0}, false);                    // stopped: nothing changes
  expect(s[pc::S_REASON] == 2.0 && s[pc::S_STEP] == 1.0, "a stopped state stays", 0, 0, 0);
  pc::begin(s.data(), 2, 0.5);
  pc::decide(s.data(), pc::Red{0.0, 0.0, 0.0, 1.0}, true);
  expect(s[pc::S_REASON] == 4.0, "non-finite before exhausted", 0, 0, 0);
  pc::begin(s.data(), 2, 0.5);
  pc::decide(s.data(), pc::Red{0.0, 0.0, 0.0, 0.0}, true);
  expect(s[pc::S_REASON] == 3.0, "exhausted before trace", 0, 0, 0);
  pc::begin(s.data(), 1, 0.0);
  pc::decide(s.data(), pc::Red{4.0, 0.0, 8.0, 0.0}, true);
  pc::decide(s.data(), pc::Red{1.0, 1.0, 1.0, 0.0}, false);
  expect(s[pc::S_REASON] == 1.0 && s[pc::S_STEP] == 1.0 && s[pc::S_COUNT] == 0.0, "rank rule", 0, 0, 0);
}

int main() {
  check_rules();
  const int64_t shapes[][3] = {{1, 1, 1}, {2, 1, 2}, {2, 2, 2}, {5, 5, 5}, {9, 4, 12}, {33, 17, 33}, {64, 9, 70}};   // n, K, ldl
  for (const auto& sh : shapes) {
    const int64_t n = sh[0], K = sh[1], ldl = sh[2];
    const std::vector<double> A = gram(n, n, 0.25);
    const Result r = run(A, n, K, 0.0, ldl);
    // (K = n: every d is zero or below after n steps, and "exhausted" is tested before "K reached")
    expect(r.rank == K && r.reason == (K == n ? 3 : 1), "full rank: K reached", n, K, r.reason);
    check_identities(A, n, K, ldl, r);
  }
  {                                                              // rank 3 of 20: the trace rule, then zeros
    const std::vector<double> A = gram(20, 3, 0.0);
    const Result r = run(A, 20, 8, 1e-10, 20);
    expect(r.rank == 3 && r.reason == 2, "rank 3 by the trace", 20, 8, r.rank);
    check_identities(A, 20, 8, 20, r);
  }
  {                                                              // a zero matrix
    const std::vector<double> A((size_t)(7 * 7), 0.0);
    const Result r = run(A, 7, 3, 0.0, 7);
    expect(r.rank == 0 && r.reason == 3 && r.fetched == 0, "zero matrix", 7, 3, r.reason);
    check_identities(A, 7, 3, 7, r);
  }
  {                                                              // a constant diagonal: the lowest index wins step 0
    std::vector<double> A = gram(6, 6, 0.0);
    for (int64_t i = 0; i < 6; ++i) A[(size_t)(i + i * 6)] = 9.0;
    const Result r = run(A, 6, 2, 0.0, 6);
    expect(r.st[pc::S_COUNT] == 0.0, "lowest index at a tie", 6, 2, (int64_t)r.st[pc::S_COUNT]);
  }
  {                                                              // a NaN on the diagonal: stops before any column is fetched
    std::vector<double> A = gram(6, 6, 0.25);
    A[(size_t)(2 + 2 * 6)] = std::numeric_limits<double>::quiet_NaN();
    const Result r = run(A, 6, 3, 0.0, 6);
    expect(r.rank == 0 && r.reason == 4 && r.fetched == 0, "NaN on the diagonal", 6, 3, r.reason);
  }
  {                                                              // an infinity in a column: stops behind that step
    std::vector<double> A = gram(6, 6, 0.25);
    const Result clean = run(A, 6, 3, 0.0, 6);
    const int64_t p0 = (int64_t)clean.st[pc::S_COUNT], q = (p0 + 1) % 6;
    A[(size_t)(q + p0 * 6)] = A[(size_t)(p0 + q * 6)] = std::numeric_limits<double>::infinity();
    const Result r = run(A, 6, 3, 0.0, 6);
    expect(r.rank == 1 && r.reason == 4, "infinity in a column", 6, 3, r.reason);
  }
  if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
  std::printf("pivchol host ok\n");
  return 0;
}
