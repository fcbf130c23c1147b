// pchol_state.hpp -- the scalar side of the diagonal-pivoted Cholesky factorization of a covariance read by entries
// (DESIGN.md section 4.6j): which row is the next pivot, and whether to stop.  The rules are written ONCE here and run by
// the device kernels (pivoted_chol.hip: one workgroup after every step) and by the host path (pivoted_chol_host.hpp: the
// CPU reference library, GSI_PCHOL_COMPOSED=1), as cg_state.hpp does for the solvers: the state block lives in backend
// memory, a step needs no scalar on the host, and the host only polls the block every few steps.
//
// The contract.  d_i = A(i, i).  Before step j: trace_j = sum of max(d_i, 0); p = the LOWEST index attaining max d_i; stop,
// tested in this order, with reason 4 (a non-finite value in d, in a column or in the trace), 3 (d_p is not > 0),
// 2 (trace_j <= tol trace_0), 1 (j == K).  Step j: r = sqrt(d_p); L[i, j] = (A(i, p) - sum_{c < j, ascending} L[i, c] L[p, c]) / r;
// d_i -= L[i, j]^2; then d_p = 0 exactly.  Every product, sum, quotient and square root is rounded on its own.
#pragma once
#include <cmath>
#include <cstdint>
#ifndef GSI_HD
#if defined(__HIPCC__)
#define GSI_HD __host__ __device__
#else
#define GSI_HD
#endif
#endif

namespace gsi { namespace pchol {

// the state block: S_COUNT doubles, then the K pivots chosen so far (as doubles: indices are below 2^53)
enum {
  S_K = 0,        // the rank asked for
  S_TOL,          // stop when trace_j <= tol trace_0
  S_TRACE0,       // sum of max(A(i, i), 0)
  S_TRACE,        // trace_j of the last decision
  S_DMAX,         // max d_i of the last decision
  S_PIVOT,        // the row the next step eliminates
  S_ROOT,         // sqrt(d_pivot)
  S_STEP,         // j: columns of L written so far = the rank when S_REASON is set
  S_REASON,       // 0 while running, else why it stopped (below)
  S_COUNT = 16
};
enum { RUNNING = 0, STOP_RANK = 1, STOP_TRACE = 2, STOP_EXHAUSTED = 3, STOP_NONFINITE = 4 };

GSI_HD inline size_t state_doubles(int64_t K) { return (size_t)S_COUNT + (size_t)K; }

// what a pass over d reduces to.  All doubles (a partial is four doubles in backend memory); idx is an integer value.
struct Red {
  double dmax, idx, possum, bad;
};
GSI_HD inline Red red_identity() { return Red{-HUGE_VAL, 9007199254740992.0, 0.0, 0.0}; }
GSI_HD inline bool is_fin(double v) { return v - v == 0.0; }             // false for NaN and the infinities
// the larger d wins, the lower index among equals: the result does not depend on the order of the combinations
GSI_HD inline void red_max(Red& r, double d, double idx) {
  if (d > r.dmax || (d == r.dmax && idx < r.idx)) { r.dmax = d; r.idx = idx; }
}
// one row: its d after the step, and whether the row met a non-finite value (in d or in its entry of the new column)
GSI_HD inline void red_row(Red& r, double d, int64_t i, bool bad) {
  red_max(r, d, (double)i);
  r.possum = r.possum + (d > 0.0 ? d : 0.0);
  if (bad || !is_fin(d)) r.bad = 1.0;
}
// b after a: the caller fixes the order, the positive sum depends on it
GSI_HD inline void red_join(Red& a, const Red& b) {
  red_max(a, b.dmax, b.idx);
  a.possum = a.possum + b.possum;
  if (b.bad != 0.0) a.bad = 1.0;
}

GSI_HD inline void begin(double* s, int64_t K, double tol) {
  for (int i = 0; i < S_COUNT; ++i) s[i] = 0.0;
  s[S_K] = (double)K; s[S_TOL] = tol;
  s[S_PIVOT] = -1.0;
}
// r: the reduction of d over all rows.  first: d is the diagonal of A (before step 0); otherwise a step has just been
// applied and S_STEP counts it.  Sets S_REASON, or the next pivot and its root.
GSI_HD inline void decide(double* s, const Red& r, bool first) {
  if (s[S_REASON] != 0.0) return;
  if (first) s[S_TRACE0] = r.possum;
  else s[S_STEP] = s[S_STEP] + 1.0;
  s[S_TRACE] = r.possum;
  s[S_DMAX] = r.dmax;
  const int64_t j = (int64_t)s[S_STEP];
  if (r.bad != 0.0 || !is_fin(r.possum)) { s[S_REASON] = (double)STOP_NONFINITE; return; }
  if (!(r.dmax > 0.0)) { s[S_REASON] = (double)STOP_EXHAUSTED; return; }
  if (r.possum <= s[S_TOL] * s[S_TRACE0]) { s[S_REASON] = (double)STOP_TRACE; return; }
  if (j >= (int64_t)s[S_K]) { s[S_REASON] = (double)STOP_RANK; return; }
  s[S_PIVOT] = r.idx;
  s[S_ROOT] = std::sqrt(r.dmax);
  s[S_COUNT + j] = r.idx;
}

}}  // namespace gsi::pchol
