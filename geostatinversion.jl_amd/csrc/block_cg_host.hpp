// block_cg_host.hpp -- the host-driven ("composed") form of the multi-column conjugate-gradient solver: cg_state.hpp's
// recurrences with the backend's existing primitives (diag_mul_add, dot, axpy, scal), column by column, every scalar
// crossing to the host.  What the CPU reference library runs, the in-process A/B leg of the fused kernels
// (GSI_CG_COMPOSED=1) and their first reference.  Included by pipeline.cpp only.
#pragma once
#include <cstdint>
#include <vector>
#include "backend.hpp"
#include "cg_state.hpp"

namespace gsi {

// R and P hold B, X is zero (n x b, ld n); mul(P, Q): Q = A P on the whole panel.  st: cgst::state_doubles(b) doubles,
// left as the device path's state block would be.  Returns the operator products performed.  trace (HOST,
// cgst::trace_doubles(b, qmax) doubles, or null): the coefficient trace of cg_state.hpp's trace_col.
template <class Mul>
int64_t block_cg_composed(Backend* be, Mul&& mul, int64_t n, int64_t b, const double* diag, const double* B, double* X,
                          double* R, double* P, double* Q, double tol, int64_t maxiter, std::vector<double>& st,
                          double* trace = nullptr, int64_t qmax = 0) {
  using namespace cgst;
  st.assign(state_doubles(b), 0.0);
  double* s = st.data();
  begin(s, b, tol, maxiter);
  for (int64_t j = 0; j < b; ++j) {
    begin_col(s, j, be->dot(n, B + j * n, B + j * n));
    if (trace) trace_begin_col(s, j, trace, qmax);
  }
  after_iter(s);
  int64_t products = 0;
  while (s[H_ACTIVE] > 0.0) {
    mul(P, Q);
    ++products;
    for (int64_t j = 0; j < b; ++j) {
      double* p = P + j * n;
      double* q = Q + j * n;
      double* r = R + j * n;
      const bool live = colv(s, STOPPED, j) == 0.0 && colv(s, ITERS, j) < s[H_MAXITER] && s[H_BREAKDOWN] == 0.0;
      double pq = 0.0, rr = 0.0;
      if (live) {
        if (diag) be->diag_mul_add(n, diag, p, q);              // q <- (A + D) p
        pq = be->dot(n, p, q);
      }
      after_pq(s, j, pq);
      if (colv(s, APPLY, j) != 0.0) {
        be->axpy(n, colv(s, ALPHA, j), p, X + j * n);
        be->axpy(n, -colv(s, ALPHA, j), q, r);
        rr = be->dot(n, r, r);
      }
      after_rr(s, j, rr);
      if (trace) trace_col(s, j, trace, qmax);
      if (colv(s, UPDP, j) != 0.0) {                            // p = r + beta p
        be->scal(n, colv(s, BETA, j), p);
        be->axpy(n, 1.0, r, p);
      }
    }
    after_iter(s);
  }
  return products;
}

}  // namespace gsi
