// pivoted_chol_host.hpp -- the host-driven ("composed") form of the diagonal-pivoted Cholesky factorization: pchol_state.hpp's
// rules around an update loop in the contract's order, every column fetched by the caller (solvers.cpp: the operator
// product with a unit vector).  What the CPU reference library runs, the in-process A/B leg of the device kernels
// (GSI_PCHOL_COMPOSED=1) and their first reference.  Plain host code with no backend in it, so that
// tests/pivchol_host_check.cpp can run it under the sanitizers.  Included by solvers.cpp only.
#pragma once
#include <cstdint>
#include <vector>
#include "pchol_state.hpp"

namespace gsi { namespace pchol {

#if defined(__clang__)
#define GSI_PCHOL_NOCONTRACT
#elif defined(__GNUC__)
#define GSI_PCHOL_NOCONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define GSI_PCHOL_NOCONTRACT
#endif

// the reduction of d (n values) in ascending row order
inline Red host_reduce(int64_t n, const double* d) {
  Red r = red_identity();
  for (int64_t i = 0; i < n; ++i) red_row(r, d[i], i, false);
  return r;
}

// Step j with pivot p and root = sqrt(d_p): col (n) = A(:, p); L (n x >= j + 1, ld ldl) gains column j, d (n) is updated.
// Returns the reduction of the new d.  Every product and sum is rounded on its own, c ascending within a row.
GSI_PCHOL_NOCONTRACT inline Red host_step(int64_t n, int64_t j, int64_t p, double root, const double* col, double* L,
                                          int64_t ldl, double* d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  Red r = red_identity();
  for (int64_t i = 0; i < n; ++i) {
    double s = 0.0;
    for (int64_t c = 0; c < j; ++c) {
      const double t = L[i + c * ldl] * L[p + c * ldl];
      s = s + t;
    }
    const double l = (col[i] - s) / root;
    L[i + j * ldl] = l;
    const double t = l * l;
    double di = d[i] - t;
    if (i == p) di = 0.0;
    d[i] = di;
    red_row(r, di, i, !is_fin(l));
  }
  return r;
}

// The whole factorization.  d (n): the diagonal of A on entry, the diagonal of A - L L' on return; column(p, out): out (n)
// <- A(:, p); L: n x K (ld ldl), columns from the rank on are written as zeros; st: state_doubles(K) doubles, left as the
// device path's state block would be.  Returns the number of columns fetched.
template <class Column>
int64_t host_factor(int64_t n, int64_t K, double tol, double* d, Column&& column, double* L, int64_t ldl,
                    std::vector<double>& st) {
  st.assign(state_doubles(K), 0.0);
  double* s = st.data();
  begin(s, K, tol);
  for (int64_t c = 0; c < K; ++c)
    for (int64_t i = 0; i < n; ++i) L[i + c * ldl] = 0.0;
  decide(s, host_reduce(n, d), true);
  std::vector<double> col((size_t)n);
  int64_t fetched = 0;
  while (s[S_REASON] == 0.0) {
    const int64_t j = (int64_t)s[S_STEP], p = (int64_t)s[S_PIVOT];
    column(p, col.data());
    ++fetched;
    const Red r = host_step(n, j, p, s[S_ROOT], col.data(), L, ldl, d);
    decide(s, r, false);
  }
  return fetched;
}

}}  // namespace gsi::pchol
