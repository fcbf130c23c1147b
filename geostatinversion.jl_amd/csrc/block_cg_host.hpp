// block_cg_host.hpp -- the host-driven ("composed") form of the multi-column conjugate-gradient solver, plain or
// preconditioned (DESIGN.md sections 4.6h, 4.6i): cg_state.hpp's recurrences with the backend's existing primitives
// (diag_mul_add, dot, axpy, scal; gemm_tn, gemm_nn for the preconditioner), column by column, every scalar crossing to the
// host.  What the CPU reference library runs, the in-process A/B leg of the fused kernels (GSI_CG_COMPOSED=1) and their
// first reference.  Included by solvers.cpp only.
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

// R holds B, X is zero (n x b, ld n); mul(P, Q): Q = A P on the whole panel.  Plain (W null): P holds B too, and st is
// cgst::state_doubles(b) doubles.  Preconditioned by P^-1 = diag(e) - W W' (W: n x K): P is written here, Zp (n x b) and
// S (K x b) are scratch, and st is cgst::pcg_state_doubles(b) doubles.  st is left as the device path's state block would
// be.  Returns the operator products performed.  trace (HOST, cgst::trace_doubles(b, qmax) doubles, or null): the
// coefficient trace of cg_state.hpp's trace_col.
template <class Mul>
int64_t block_cg_composed(Backend* be, Mul&& mul, int64_t n, int64_t b, const double* diag, const double* B, double* X,
                          double* R, double* P, double* Q, double tol, int64_t maxiter, std::vector<double>& st,
                          double* trace = nullptr, int64_t qmax = 0, const double* e = nullptr, const double* W = nullptr,
                          int64_t K = 0, double* Zp = nullptr, double* S = nullptr) {
  using namespace cgst;
  const bool pc = W != nullptr;
  st.assign(pc ? pcg_state_doubles(b) : state_doubles(b), 0.0);
  double* s = st.data();
  begin(s, b, tol, maxiter);
  if (pc) {
    precond_apply_composed(be, n, K, e, W, B, b, S, Zp);
    be->copy2d(P, n, Zp, n, n, b);
  }
  for (int64_t j = 0; j < b; ++j) {
    const double bb = be->dot(n, B + j * n, B + j * n);
    if (pc) pcg_begin_col(s, j, bb, be->dot(n, B + j * n, Zp + j * n));
    else begin_col(s, j, bb);
    if (trace) trace_begin_col(s, j, trace, qmax);
  }
  after_iter(s);
  int64_t products = 0;
  while (s[H_ACTIVE] > 0.0) {
    mul(P, Q);
    ++products;
    bool wanted = false;
    for (int64_t j = 0; j < b; ++j) {                           // x += alpha p, r -= alpha (A + D) p
      double* p = P + j * n;
      double* q = Q + j * n;
      double* r = R + j * n;
      const bool live = colv(s, STOPPED, j) == 0.0 && colv(s, ITERS, j) < s[H_MAXITER] && s[H_BREAKDOWN] == 0.0;
      double pq = 0.0, rr = 0.0;
      if (live) {
        if (diag) be->diag_mul_add(n, diag, p, q);              // q <- (A + D) p
        pq = be->dot(n, p, q);
      }
      if (pc) pcg_after_pq(s, j, pq);
      else after_pq(s, j, pq);
      if (colv(s, APPLY, j) != 0.0) {
        be->axpy(n, colv(s, ALPHA, j), p, X + j * n);
        be->axpy(n, -colv(s, ALPHA, j), q, r);
        rr = be->dot(n, r, r);
      }
      if (pc) pcg_after_rr(s, j, rr);
      else after_rr(s, j, rr);
      wanted = wanted || colv(s, UPDP, j) != 0.0;
    }
    if (pc && wanted) precond_apply_composed(be, n, K, e, W, R, b, S, Zp);   // (on all b columns, as the device path does)
    for (int64_t j = 0; j < b; ++j) {                           // p = z + beta p, with z = r where there is no preconditioner
      double* p = P + j * n;
      const double* z = (pc ? Zp : R) + j * n;
      if (pc) pcg_after_rz(s, j, colv(s, UPDP, j) != 0.0 ? be->dot(n, R + j * n, z) : 0.0);
      if (trace) trace_col(s, j, trace, qmax);
      if (colv(s, UPDP, j) != 0.0) {
        be->scal(n, colv(s, BETA, j), p);
        be->axpy(n, 1.0, z, p);
      }
    }
    after_iter(s);
  }
  return products;
}

}  // namespace gsi
