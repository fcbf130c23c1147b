// bilinear_terms_host.hpp -- the host side of the bilinear forms of the likelihood gradient: the
// reduction of bilinear_terms.hip as plain C++ on host arrays, with the same products and the same order of additions, so the
// two agree bit for bit.  It runs when the backend declines (Backend::bilinear_terms says "not mine": the CPU reference
// library) or GSI_BILINEAR_HOST=1; tests/bilinear_host_check.cpp exercises it alone.  Nothing here depends on a backend.
#pragma once
#include <cstddef>
#include <cstdint>

// stated product by product: no fused multiply-add may merge a product with the add behind it
#if defined(__clang__)
#define GSI_BILINEAR_NO_CONTRACT
#define GSI_BILINEAR_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define GSI_BILINEAR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#define GSI_BILINEAR_NO_CONTRACT_BODY
#else
#define GSI_BILINEAR_NO_CONTRACT
#define GSI_BILINEAR_NO_CONTRACT_BODY
#endif

namespace gsi { namespace bilinear_host {

constexpr int64_t CHUNK = 2048;           // hipk::BILINEAR_CHUNK
constexpr int64_t MAX_G = 16;

// L, Y, R: column-major n x b with leading dimension n; dd: n values or null (then R is not read); V = Y + dd .* R.
// gram (g x g, column-major) [a + g c] = sum_i L[i, a] V[i, c]; t (b - g) [j - g] = sum_i L[i, j] V[i, j].  Per chunk of CHUNK
// rows every output starts from 0.0 and adds its products in ascending row order; the chunks' sums are then added in
// ascending chunk order, again from 0.0.  Needs n, b >= 1 and 0 <= g <= min(b, MAX_G).
// one output: sum_i L[i, a] V[i, c] in the order above (no lambda: the no-contraction attribute must cover every product)
GSI_BILINEAR_NO_CONTRACT inline double one(int64_t n, int64_t a, int64_t c, const double* L, const double* Y, const double* R,
                                           const double* dd) {
  GSI_BILINEAR_NO_CONTRACT_BODY
  const double* la = L + (size_t)a * (size_t)n;
  const double* yc = Y + (size_t)c * (size_t)n;
  const double* rc = (dd != nullptr) ? R + (size_t)c * (size_t)n : nullptr;
  double total = 0.0;
  for (int64_t r0 = 0; r0 < n; r0 += CHUNK) {
    const int64_t rend = (n - r0 < CHUNK) ? n : r0 + CHUNK;
    double s = 0.0;
    for (int64_t i = r0; i < rend; ++i) {
      double v = yc[i];
      if (dd != nullptr) {
        const double d = dd[i] * rc[i];
        v = v + d;
      }
      const double p = la[i] * v;
      s = s + p;
    }
    total = total + s;
  }
  return total;
}
inline void terms(int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R, const double* dd,
                  double* gram, double* t) {
  for (int64_t c = 0; c < g; ++c)
    for (int64_t a = 0; a < g; ++a) gram[a + g * c] = one(n, a, c, L, Y, R, dd);
  for (int64_t j = g; j < b; ++j) t[j - g] = one(n, j, j, L, Y, R, dd);
}

}}  // namespace gsi::bilinear_host
