// bilinear_host_check.cpp -- csrc/bilinear_terms_host.hpp (the bilinear forms of the likelihood gradient, DESIGN.md section
// 4.6n) against brute force, as a stand-alone program for -fsanitize=address,undefined (tests/test_bilinear_cpu.py builds and
// runs it).  Every array is allocated at its exact size -- R and dd are not allocated at all where they must not be read --
// so a read or write past a panel or an output is caught by the sanitizer.  Operands are small integers: every sum is exact
// in any order, and the brute-force sums must be met exactly.  A second check states the ORDER on values where it matters.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bilinear_terms_host.hpp"

using namespace gsi;

static uint64_t g_state = 88172645463325252ull;
static double rnd() {                      // xorshift: values in (-1, 1)
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static void check_exact(int64_t n, int64_t b, int64_t g, bool with_dd) {
  const size_t cnt = (size_t)(n * b);
  std::vector<double> L(cnt), Y(cnt), R(with_dd ? cnt : 0), dd(with_dd ? (size_t)n : 0);
  for (auto& v : L) v = (double)(int)(8.0 * rnd());
  for (auto& v : Y) v = (double)(int)(8.0 * rnd());
  for (auto& v : R) v = (double)(int)(4.0 * rnd());
  for (auto& v : dd) v = (double)(int)(4.0 * rnd());
  std::vector<double> gram((size_t)(g * g)), t((size_t)(b - g));
  bilinear_host::terms(n, b, g, L.data(), Y.data(), with_dd ? R.data() : nullptr, with_dd ? dd.data() : nullptr,
                       g > 0 ? gram.data() : nullptr, b > g ? t.data() : nullptr);
  auto v_at = [&](int64_t i, int64_t c) {
    return Y[(size_t)(i + c * n)] + (with_dd ? dd[(size_t)i] * R[(size_t)(i + c * n)] : 0.0);
  };
  for (int64_t a = 0; a < g; ++a)
    for (int64_t c = 0; c < g; ++c) {
      double s = 0.0;
      for (int64_t i = 0; i < n; ++i) s += L[(size_t)(i + a * n)] * v_at(i, c);
      CHECK(gram[(size_t)(a + g * c)] == s, "gram n=%lld b=%lld g=%lld dd=%d (%lld, %lld)", (long long)n, (long long)b,
            (long long)g, (int)with_dd, (long long)a, (long long)c);
    }
  for (int64_t j = g; j < b; ++j) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += L[(size_t)(i + j * n)] * v_at(i, j);
    CHECK(t[(size_t)(j - g)] == s, "t n=%lld b=%lld g=%lld dd=%d column %lld", (long long)n, (long long)b, (long long)g,
          (int)with_dd, (long long)j);
  }
}

// rows 0 .. CHUNK - 1 hold 1, 2^-53, 2^-53, ...: added one at a time to the chunk's sum every 2^-53 is lost (the sum stays 1);
// the next chunk holds 2^-53 alone CHUNK times and sums to CHUNK 2^-53 exactly, which is then added to 1 exactly.
static void check_order() {
  const int64_t n = 2 * bilinear_host::CHUNK;
  std::vector<double> L((size_t)n, 1.0), Y((size_t)n, 0x1p-53);
  Y[0] = 1.0;
  double gram = 0.0, t = 0.0;
  bilinear_host::terms(n, 1, 1, L.data(), Y.data(), nullptr, nullptr, &gram, nullptr);
  bilinear_host::terms(n, 1, 0, L.data(), Y.data(), nullptr, nullptr, nullptr, &t);
  const double want = 1.0 + (double)bilinear_host::CHUNK * 0x1p-53;
  CHECK(gram == want, "order: gram %.17g, want %.17g", gram, want);
  CHECK(t == want, "order: t %.17g, want %.17g", t, want);
  // d = dd R is rounded before it is added to Y: (1 - e)(1 + e) rounds to 1
  const double e = 0x1p-30, one = 1.0, Rv = 1.0 + e, dv = 1.0 - e;
  bilinear_host::terms(1, 1, 1, &one, &one, &Rv, &dv, &gram, nullptr);
  CHECK(gram == 2.0, "order: dd R is rounded on its own (%.17g)", gram);
}

int main() {
  const int64_t C = bilinear_host::CHUNK;
  const int64_t rows[] = {1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5};
  const int64_t shapes[][2] = {{1, 0}, {1, 1}, {5, 0}, {4, 4}, {16, 16}, {49, 16}, {7, 3}};
  for (int64_t n : rows)
    for (auto& s : shapes)
      for (int dd = 0; dd < 2; ++dd) check_exact(n, s[0], s[1], dd != 0);
  check_order();
  if (fails == 0) std::printf("bilinear host ok\n");
  return fails == 0 ? 0 : 1;
}
