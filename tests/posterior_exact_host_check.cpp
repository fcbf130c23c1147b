// posterior_exact_host_check.cpp -- csrc/posterior_exact_host.hpp (the row sums, the trapezoid assembly, the small Cholesky
// and the finish) against brute force, as a stand-alone program for -fsanitize=address,undefined
// (tests/test_posterior_exact_cpu.py builds and runs it).  Every array is allocated at its exact size, so a read or write
// past a panel, the trapezoid or a leading dimension is caught by the sanitizer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "posterior_exact_host.hpp"
#include "saddle_host.hpp"

using namespace gsi;

static uint64_t g_state = 88172645463325252ull;
static double rnd() {                      // xorshift: values in (-1, 1)
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static void check_rowdot(int64_t n, int64_t b, int64_t pad, bool same) {
  const int64_t lda = n + pad, ldb = n + 2 * pad;
  std::vector<double> A((size_t)(lda * (b - 1) + n)), B((size_t)(ldb * (b - 1) + n)), acc((size_t)n), want((size_t)n);
  for (auto& v : A) v = (double)(int)(8.0 * rnd());          // small integers: every sum is exact in any order
  for (auto& v : B) v = (double)(int)(8.0 * rnd());
  for (int64_t i = 0; i < n; ++i) acc[(size_t)i] = want[(size_t)i] = (double)(i % 5) - 2.0;
  const double* Bp = same ? A.data() : B.data();
  const int64_t ldbb = same ? lda : ldb;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t c = 0; c < b; ++c) want[(size_t)i] += A[(size_t)(i + c * lda)] * Bp[(size_t)(i + c * ldbb)];
  postx_host::rowdot_acc(n, b, A.data(), lda, Bp, ldbb, acc.data());
  for (int64_t i = 0; i < n; ++i)
    CHECK(acc[(size_t)i] == want[(size_t)i], "rowdot n=%lld b=%lld same=%d row %lld", (long long)n, (long long)b, (int)same, (long long)i);
}

static void check_trapezoid(int64_t nobs, int64_t p, bool with_diag) {
  const int64_t ld = 2 * nobs + p;
  std::vector<double> T((size_t)(ld * nobs)), M((size_t)(nobs * nobs)), Phi((size_t)(nobs * (p > 0 ? p : 1))), d((size_t)nobs);
  // M = R R' + I: positive definite
  std::vector<double> R((size_t)(nobs * nobs));
  for (auto& v : R) v = rnd();
  for (int64_t i = 0; i < nobs; ++i)
    for (int64_t j = 0; j < nobs; ++j) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int64_t k = 0; k < nobs; ++k) s += R[(size_t)(i + k * nobs)] * R[(size_t)(j + k * nobs)];
      M[(size_t)(i + j * nobs)] = s;
    }
  for (auto& v : Phi) v = rnd();
  for (auto& v : d) v = 0.5 + 0.25 * rnd();
  for (auto& v : T) v = std::nan("");                        // whatever the assembly does not write stays visible
  for (int64_t j = 0; j < nobs; ++j)
    for (int64_t i = 0; i < nobs; ++i) T[(size_t)(i + j * ld)] = M[(size_t)(i + j * nobs)];
  postx_host::assemble(T.data(), ld, nobs, p, with_diag ? d.data() : nullptr, Phi.data(), nobs);
  for (int64_t j = 0; j < nobs; ++j) {
    for (int64_t i = 0; i < nobs; ++i)
      CHECK(T[(size_t)(i + j * ld)] == M[(size_t)(i + j * nobs)] + ((with_diag && i == j) ? d[(size_t)j] : 0.0), "assemble: top block");
    for (int64_t k = 0; k < p; ++k) CHECK(T[(size_t)(nobs + k + j * ld)] == Phi[(size_t)(j + k * nobs)], "assemble: Phi'");
    for (int64_t i = 0; i < nobs; ++i) CHECK(T[(size_t)(nobs + p + i + j * ld)] == ((i == j) ? 1.0 : 0.0), "assemble: identity");
  }
  // the factorization leaves [L; (L^-1 Phi)'; L^-T]: L (L^-T)' = I and L W_d = Phi
  const int64_t col = saddle_host::chol_lower(T.data(), ld, nobs, ld);
  CHECK(col == 0, "chol_lower failed at %lld", (long long)col);
  std::vector<double> Wd((size_t)(nobs * (p > 0 ? p : 1)));
  postx_host::carried_rows(T.data() + nobs, ld, nobs, p, Wd.data());
  for (int64_t i = 0; i < nobs; ++i) {
    for (int64_t j = 0; j < nobs; ++j) {
      double s = 0.0;                                        // (L Linv)(i, j), Linv(k, j) = Linvt(j, k) = T[nobs + p + j, k]
      for (int64_t k = 0; k <= i; ++k) s += T[(size_t)(i + k * ld)] * T[(size_t)(nobs + p + j + k * ld)];
      CHECK(std::fabs(s - ((i == j) ? 1.0 : 0.0)) < 1e-10, "L L^-1 != I at (%lld, %lld): %g", (long long)i, (long long)j, s);
    }
    for (int64_t k = 0; k < p; ++k) {
      double s = 0.0;
      for (int64_t t = 0; t <= i; ++t) s += T[(size_t)(i + t * ld)] * Wd[(size_t)(t + k * nobs)];
      CHECK(std::fabs(s - Phi[(size_t)(i + k * nobs)]) < 1e-10, "L W_d != Phi");
    }
  }
}

static void check_finish(int64_t n, int64_t p) {
  const int64_t ldx = n + 3, ldu = n + 1, pp = p > 0 ? p : 1;
  std::vector<double> X((size_t)(ldx * (pp - 1) + n)), U((size_t)(ldu * (pp - 1) + n)), acc((size_t)n), var((size_t)n), S((size_t)(pp * pp)),
      Ls;
  for (auto& v : X) v = rnd();
  for (auto& v : U) v = rnd();
  for (auto& v : acc) v = std::fabs(rnd());
  for (int64_t i = 0; i < p; ++i)
    for (int64_t j = 0; j < p; ++j) S[(size_t)(i + j * p)] = (i == j ? (double)p + 1.0 : 0.0) + 0.5 / (1.0 + (double)(i + j));
  Ls = S;
  CHECK(postx_host::chol_small(Ls.data(), p) == 0, "chol_small failed on a positive definite S");
  postx_host::finish(n, p, 1.5, acc.data(), U.data(), ldu, X.data(), ldx, Ls.data(), var.data());
  // brute force: q = r' S^-1 r by Gaussian elimination without the factor
  for (int64_t i = 0; i < n; ++i) {
    std::vector<double> Aug((size_t)(pp * (pp + 1)), 0.0), r((size_t)pp, 0.0);
    for (int64_t k = 0; k < p; ++k) r[(size_t)k] = X[(size_t)(i + k * ldx)] - U[(size_t)(i + k * ldu)];
    for (int64_t a = 0; a < p; ++a) {
      for (int64_t c = 0; c < p; ++c) Aug[(size_t)(a * (p + 1) + c)] = S[(size_t)(a + c * p)];
      Aug[(size_t)(a * (p + 1) + p)] = r[(size_t)a];
    }
    for (int64_t a = 0; a < p; ++a)
      for (int64_t a2 = a + 1; a2 < p; ++a2) {
        const double f = Aug[(size_t)(a2 * (p + 1) + a)] / Aug[(size_t)(a * (p + 1) + a)];
        for (int64_t c = a; c <= p; ++c) Aug[(size_t)(a2 * (p + 1) + c)] -= f * Aug[(size_t)(a * (p + 1) + c)];
      }
    std::vector<double> y((size_t)pp, 0.0);
    for (int64_t a = p - 1; a >= 0; --a) {
      double s = Aug[(size_t)(a * (p + 1) + p)];
      for (int64_t c = a + 1; c < p; ++c) s -= Aug[(size_t)(a * (p + 1) + c)] * y[(size_t)c];
      y[(size_t)a] = s / Aug[(size_t)(a * (p + 1) + a)];
    }
    double q = 0.0;
    for (int64_t k = 0; k < p; ++k) q += r[(size_t)k] * y[(size_t)k];
    CHECK(std::fabs(var[(size_t)i] - (1.5 - acc[(size_t)i] + q)) < 1e-12, "finish n=%lld p=%lld row %lld", (long long)n, (long long)p, (long long)i);
  }
}

int main() {
  for (int64_t n : {1, 2, 63, 64, 65, 257})
    for (int64_t b : {1, 7, 8, 9, 17})
      for (int same = 0; same < 2; ++same) check_rowdot(n, b, (n % 3 == 0) ? 0 : 3, same != 0);
  for (int64_t nobs : {1, 2, 5, 33})
    for (int64_t p : {0, 1, 3}) {
      check_trapezoid(nobs, p, false);
      check_trapezoid(nobs, p, true);
    }
  {
    std::vector<double> E(2 * 7 + 5, -1.0);                  // nobs = 5 rows of ld 7, b = 3 columns: the last column ends the array
    postx_host::unit_panel(E.data(), 7, 5, 3, 2);
    for (int64_t c = 0; c < 3; ++c)
      for (int64_t r = 0; r < 5; ++r) CHECK(E[(size_t)(r + c * 7)] == ((r == 2 + c) ? 1.0 : 0.0), "unit_panel");
    CHECK(E[5] == -1.0 && E[6] == -1.0, "unit_panel wrote into the padding of ld");
  }
  for (int64_t p : {0, 1, 3, 4}) check_finish(37, p);
  {
    double S[4] = {1.0, 1.0, 1.0, 1.0};                      // two identical drift columns: singular at column 2
    CHECK(postx_host::chol_small(S, 2) == 2, "chol_small accepted a singular S");
  }
  if (fails) { std::printf("posterior exact host FAILED: %d\n", fails); return 1; }
  std::printf("posterior exact host ok\n");
  return 0;
}
