// block_pcg_host.hpp -- the host-driven ("composed") form of the preconditioned multi-column conjugate-gradient solver
// (DESIGN.md section 4.6i): cg_state.hpp's pcg_* recurrences with the backend's existing primitives (gemm_tn, gemm_nn,
// diag_mul_add, dot, axpy, scal), every scalar crossing to the host.  What the CPU reference library runs, the in-process
// A/B leg of block_pcg.hip (GSI_CG_COMPOSED=1) and its first reference.  Included by pipeline.cpp only.
#pragma once
#include <cstdint>
#include <vector>
#include "backend.hpp"
#include "cg_state.hpp"

namespace gsi {

// Zout (n x b, ld n) = P^-1 R = e .* R - W (W'R) for P^-1 = diag(e) - W W' (W: n x K, ld n); S: K x b scratch
inline void precond_apply_composed(Backend* be, int64_t n, int64_t K, const double* e, const double* W, const double* R,
                                   int64_t b, double* S, double* Zout) {
  be->gemm_tn(K, b, n, 1.0, W, n, R, n, 0.0, S, K);
  be->gemm_nn(n, b, K, -1.0, W, n, S, K, 0.0, Zout, n);
  for (int64_t j = 0; j < b; ++j) be->diag_mul_add(n, e, R + j * n, Zout + j * n);
}

// R holds B, X is zero (n x b, ld n); mul(P, Q): Q = A P on the whole panel; Zp (n x b) and S (K x b): scratch.
// st: cgst::pcg_state_doubles(b) doubles, left as the device path's state block would be.  Returns the operator products.
// trace (HOST, cgst::trace_doubles(b, qmax) doubles, or null): the coefficient trace of cg_state.hpp's trace_col.
template <class Mul>
int64_t block_pcg_composed(Backend* be, Mul&& mul, int64_t n, int64_t b, int64_t K, const double* diag, const double* e,
                           const double* W, const double* B, double* X, double* R, double* P, double* Q, double* Zp, double* S,
                           double tol, int64_t maxiter, std::vector<double>& st, double* trace = nullptr, int64_t qmax = 0) {
  using namespace cgst;
  st.assign(pcg_state_doubles(b), 0.0);
  double* s = st.data();
  begin(s, b, tol, maxiter);
  precond_apply_composed(be, n, K, e, W, B, b, S, Zp);
  be->copy2d(P, n, Zp, n, n, b);
  for (int64_t j = 0; j < b; ++j) {
    pcg_begin_col(s, j, be->dot(n, B + j * n, B + j * n), be->dot(n, B + j * n, Zp + j * n));
    if (trace) trace_begin_col(s, j, trace, qmax);
  }
  after_iter(s);
  int64_t products = 0;
  while (s[H_ACTIVE] > 0.0) {
    mul(P, Q);
    ++products;
    bool wanted = false;
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
      pcg_after_pq(s, j, pq);
      if (colv(s, APPLY, j) != 0.0) {
        be->axpy(n, colv(s, ALPHA, j), p, X + j * n);
        be->axpy(n, -colv(s, ALPHA, j), q, r);
        rr = be->dot(n, r, r);
      }
      pcg_after_rr(s, j, rr);
      wanted = wanted || colv(s, UPDP, j) != 0.0;
    }
    if (wanted) precond_apply_composed(be, n, K, e, W, R, b, S, Zp);   // (on all b columns, as the device path does)
    for (int64_t j = 0; j < b; ++j) {
      double* p = P + j * n;
      const double* z = Zp + j * n;
      pcg_after_rz(s, j, colv(s, UPDP, j) != 0.0 ? be->dot(n, R + j * n, z) : 0.0);
      if (trace) trace_col(s, j, trace, qmax);
      if (colv(s, UPDP, j) != 0.0) {                            // p = z + beta p
        be->scal(n, colv(s, BETA, j), p);
        be->axpy(n, 1.0, z, p);
      }
    }
    after_iter(s);
  }
  return products;
}

}  // namespace gsi
