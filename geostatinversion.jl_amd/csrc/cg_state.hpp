// cg_state.hpp -- the scalar side of the multi-column conjugate-gradient solver: plain CG per
// column on (A + diag(d)) X = B with x0 = 0, the b columns advanced together and sharing only the operator product
// Q = A P.  The recurrences are written ONCE here and run by the device kernels (block_cg.hip, one thread per column) and
// by the host-driven path of solvers.cpp:block_cg (the CPU reference library, GSI_CG_COMPOSED=1), as lsqr_state.hpp
// does for LSQR: the state block lives in backend memory, an iteration needs no scalar on the host, and the host only
// polls the header every few iterations.
//
// One iteration, per column j:    q = A p;  w = q + d .* p;  after_pq(p'w);   x += alpha p;  r -= alpha w;
//                                 after_rr(r'r);   p = r + beta p             (the last three only where APPLY / UPDP say so)
// then after_iter once for the batch.
#pragma once
#include <cmath>
#include <cstdint>
#if defined(__HIPCC__)
#define GSI_HD __host__ __device__
#else
#define GSI_HD
#endif

namespace gsi { namespace cgst {

// the header: H_COUNT doubles in front of the per-column fields
enum {
  H_TOL = 0,      // a column stops when its recurred |r| <= tol |b|
  H_MAXITER,      // iteration budget: no column is advanced beyond it, whatever the host enqueues
  H_NCOLS,        // b
  H_ACTIVE,       // columns that the next iteration would still advance (0: nothing left to do)
  H_SWEEPS,       // iterations of the batch that advanced at least one column (= operator products that were needed)
  H_BREAKDOWN,    // 0, or the 1-based column of the first breakdown
  H_CONVERGED,    // columns stopped by the residual rule (zero columns included)
  H_COUNT = 8
};
// the per-column fields: field f of column j at s[H_COUNT + f * b + j]
enum {
  RHO = 0,        // r'r
  ALPHA, BETA,
  BNORM,          // |b|
  STOPPED,        // != 0: converged, a zero column, or broken down -- x, r and p of the column are never written again
  ITERS,          // iterations applied to this column
  BREAKDOWN,      // != 0: p'(A + D)p was not positive and finite
  APPLY,          // != 0: this iteration's x and r updates are to be applied (set by after_pq)
  UPDP,           // != 0: this iteration's p update is to be applied (set by after_rr)
  NFIELDS
};

GSI_HD inline size_t state_doubles(int64_t b) { return (size_t)H_COUNT + (size_t)NFIELDS * (size_t)b; }
GSI_HD inline double& col(double* s, int field, int64_t j) {
  return s[H_COUNT + (int64_t)field * (int64_t)s[H_NCOLS] + j];
}
GSI_HD inline double colv(const double* s, int field, int64_t j) {
  return s[H_COUNT + (int64_t)field * (int64_t)s[H_NCOLS] + j];
}

// the header of a fresh solve (the per-column fields are set by begin_col)
GSI_HD inline void begin(double* s, int64_t b, double tol, int64_t maxiter) {
  s[H_TOL] = tol; s[H_MAXITER] = (double)maxiter; s[H_NCOLS] = (double)b;
  s[H_ACTIVE] = 0.0; s[H_SWEEPS] = 0.0; s[H_BREAKDOWN] = 0.0; s[H_CONVERGED] = 0.0;
}
// x = 0, r = p = b_j:  bb = b_j' b_j.  A zero column stops here, at iteration 0, and nothing is ever divided by its norm.
GSI_HD inline void begin_col(double* s, int64_t j, double bb) {
  col(s, RHO, j) = bb;
  col(s, ALPHA, j) = 0.0; col(s, BETA, j) = 0.0;
  col(s, BNORM, j) = std::sqrt(bb);
  col(s, STOPPED, j) = (bb > 0.0) ? 0.0 : 1.0;       // (a NaN in b: stopped too, reported through relres)
  col(s, ITERS, j) = 0.0; col(s, BREAKDOWN, j) = 0.0; col(s, APPLY, j) = 0.0; col(s, UPDP, j) = 0.0;
}
// (after begin_col of every column, after_iter below sets the header's counts: nothing was applied, so no sweep is counted)

// after w = (A + D) p:  pq = p'w
GSI_HD inline void after_pq(double* s, int64_t j, double pq) {
  col(s, APPLY, j) = 0.0; col(s, UPDP, j) = 0.0;
  col(s, ALPHA, j) = 0.0; col(s, BETA, j) = 0.0;
  if (colv(s, STOPPED, j) != 0.0 || colv(s, ITERS, j) >= s[H_MAXITER]) return;
  if (s[H_BREAKDOWN] != 0.0) return;                             // an earlier iteration broke down: the call is over
  if (!(pq > 0.0) || !(pq <= 1.79769313486231570815e308)) {      // <= 0, NaN or Inf: (A + D) is not positive definite on p
    col(s, BREAKDOWN, j) = 1.0;
    col(s, STOPPED, j) = 1.0;
    return;
  }
  col(s, ALPHA, j) = colv(s, RHO, j) / pq;
  col(s, APPLY, j) = 1.0;
}

// after x += alpha p, r -= alpha w:  rr = r'r
GSI_HD inline void after_rr(double* s, int64_t j, double rr) {
  if (colv(s, APPLY, j) == 0.0) return;
  col(s, ITERS, j) += 1.0;
  const double rho = colv(s, RHO, j);                            // > 0: the column was active
  col(s, RHO, j) = rr;
  if (std::sqrt(rr) <= s[H_TOL] * colv(s, BNORM, j)) {           // converged: p stays as it is
    col(s, STOPPED, j) = 1.0;
    return;
  }
  if (!(rr <= 1.79769313486231570815e308)) {                     // the residual left the floating-point range
    col(s, BREAKDOWN, j) = 1.0;
    col(s, STOPPED, j) = 1.0;
    return;
  }
  col(s, BETA, j) = rr / rho;
  col(s, UPDP, j) = 1.0;
}

// Once per iteration, after after_rr of every column: the tally of one column (the device adds the columns' tallies with
// integer LDS atomics, the host in a loop) ...
struct Tally { int active, converged, applied, first_breakdown; };   // first_breakdown: 1-based column, or INT32_MAX
GSI_HD inline Tally tally_col(const double* s, int64_t j) {
  Tally t = {0, 0, 0, 0x7fffffff};
  if (colv(s, APPLY, j) != 0.0) t.applied = 1;
  if (colv(s, BREAKDOWN, j) != 0.0) t.first_breakdown = (int)(j + 1);
  else if (colv(s, STOPPED, j) != 0.0) t.converged = 1;
  else if (colv(s, ITERS, j) < s[H_MAXITER]) t.active = 1;
  return t;
}
// ... and the header from the sums (first_breakdown: the minimum)
GSI_HD inline void after_iter(double* s, const Tally& t) {
  if (t.applied > 0) s[H_SWEEPS] += 1.0;
  if (s[H_BREAKDOWN] == 0.0 && t.first_breakdown != 0x7fffffff) s[H_BREAKDOWN] = (double)t.first_breakdown;
  s[H_ACTIVE] = (s[H_BREAKDOWN] != 0.0) ? 0.0 : (double)t.active;   // a breakdown ends the call
  s[H_CONVERGED] = (double)t.converged;
}
GSI_HD inline void after_iter(double* s) {                          // the host-driven path
  const int64_t b = (int64_t)s[H_NCOLS];
  Tally t = {0, 0, 0, 0x7fffffff};
  for (int64_t j = 0; j < b; ++j) {
    const Tally c = tally_col(s, j);
    t.active += c.active; t.converged += c.converged; t.applied += c.applied;
    if (c.first_breakdown < t.first_breakdown) t.first_breakdown = c.first_breakdown;
  }
  after_iter(s, t);
}

// the recurred |r_j| / |b_j| (0 for a zero column)
GSI_HD inline double relres(const double* s, int64_t j) {
  const double bn = colv(s, BNORM, j);
  return bn > 0.0 ? std::sqrt(colv(s, RHO, j)) / bn : (bn == 0.0 ? 0.0 : bn);
}

// ---- the preconditioned recurrences: P = Z Z' + diag(d + shift), z = P^-1 r.  The same header and
//      per-column fields, with RHO holding r'z (so that after_pq above gives alpha = r'z / p'w unchanged) and three fields
//      more behind NFIELDS.  One iteration, per column j:
//        q = A p;  w = q + d .* p;  pcg_after_pq(p'w);   x += alpha p;  r -= alpha w;   pcg_after_rr(r'r);
//        z = P^-1 r;   pcg_after_rz(r'z);   p = z + beta p
//      then after_iter once for the batch.  The stopping rule is the plain one, on the recurred |r|.
enum {
  RR = NFIELDS,   // r'r (RHO holds r'z)
  BKIND,          // 0, or what broke down: 1 = p'(A + D)p, 2 = r'z was not positive and finite
  PCG_NFIELDS
};
GSI_HD inline size_t pcg_state_doubles(int64_t b) { return (size_t)H_COUNT + (size_t)PCG_NFIELDS * (size_t)b; }

// x = 0, r = b_j, z = p = P^-1 b_j:  bb = b_j'b_j, bz = b_j'z.  A zero column stops here, as in begin_col.
GSI_HD inline void pcg_begin_col(double* s, int64_t j, double bb, double bz) {
  begin_col(s, j, bb);
  col(s, RR, j) = bb;
  col(s, BKIND, j) = 0.0;
  if (colv(s, STOPPED, j) != 0.0) return;
  col(s, RHO, j) = bz;
  if (!(bz > 0.0) || !(bz <= 1.79769313486231570815e308)) {      // P^-1 is not positive definite on b (a NaN in Z's factor)
    col(s, BREAKDOWN, j) = 1.0;
    col(s, BKIND, j) = 2.0;
    col(s, STOPPED, j) = 1.0;
  }
}
GSI_HD inline void pcg_after_pq(double* s, int64_t j, double pq) {
  after_pq(s, j, pq);
  if (colv(s, BREAKDOWN, j) != 0.0 && colv(s, BKIND, j) == 0.0) col(s, BKIND, j) = 1.0;
}
// after x += alpha p, r -= alpha w:  rr = r'r.  UPDP here means "z and r'z are wanted"; pcg_after_rz has the last word.
GSI_HD inline void pcg_after_rr(double* s, int64_t j, double rr) {
  if (colv(s, APPLY, j) == 0.0) return;
  col(s, ITERS, j) += 1.0;
  col(s, RR, j) = rr;
  if (std::sqrt(rr) <= s[H_TOL] * colv(s, BNORM, j)) {           // converged: p stays as it is
    col(s, STOPPED, j) = 1.0;
    return;
  }
  if (!(rr <= 1.79769313486231570815e308)) {                     // the residual left the floating-point range
    col(s, BREAKDOWN, j) = 1.0;
    col(s, BKIND, j) = 1.0;
    col(s, STOPPED, j) = 1.0;
    return;
  }
  col(s, UPDP, j) = 1.0;
}
// after z = P^-1 r:  rz = r'z
GSI_HD inline void pcg_after_rz(double* s, int64_t j, double rz) {
  if (colv(s, UPDP, j) == 0.0) return;
  if (!(rz > 0.0) || !(rz <= 1.79769313486231570815e308)) {
    col(s, BREAKDOWN, j) = 1.0;
    col(s, BKIND, j) = 2.0;
    col(s, STOPPED, j) = 1.0;
    col(s, UPDP, j) = 0.0;
    return;
  }
  col(s, BETA, j) = rz / colv(s, RHO, j);                        // RHO > 0: the column was active
  col(s, RHO, j) = rz;
}
GSI_HD inline double pcg_relres(const double* s, int64_t j) {
  const double bn = colv(s, BNORM, j);
  return bn > 0.0 ? std::sqrt(colv(s, RR, j)) / bn : (bn == 0.0 ? 0.0 : bn);
}

// ---- the coefficient trace: alpha_k and beta_k of every column, kept for slq_state.hpp's
//      quadrature.  They are the Lanczos tridiagonal of P^-1/2 (A + D) P^-1/2 started at P^-1/2 b_j (P = I for plain CG).
//      tr = [alpha (qmax x b) | beta (qmax x b) | rho0 (b)], step k of column j at k * b + j: column-interleaved, so that
//      one thread per column reads and writes neighbouring words.  The trace only reads the state: a traced solve returns
//      the bits of an untraced one.
GSI_HD inline size_t trace_doubles(int64_t b, int64_t qmax) { return (size_t)(2 * qmax + 1) * (size_t)b; }
GSI_HD inline double* trace_alpha(double* tr, int64_t b, int64_t qmax) { (void)b; (void)qmax; return tr; }
GSI_HD inline double* trace_beta(double* tr, int64_t b, int64_t qmax) { return tr + qmax * b; }
GSI_HD inline double* trace_rho0(double* tr, int64_t b, int64_t qmax) { return tr + 2 * qmax * b; }
// once per column, after begin_col (rho0 = b'b) or pcg_begin_col (rho0 = r0'z0); 0 for a zero column
GSI_HD inline void trace_begin_col(const double* s, int64_t j, double* tr, int64_t qmax) {
  const int64_t b = (int64_t)s[H_NCOLS];
  trace_rho0(tr, b, qmax)[j] = colv(s, RHO, j);
}
// once per column and iteration, after after_rr (CG) or pcg_after_rz (PCG): ITERS has been advanced where APPLY is set
GSI_HD inline void trace_col(const double* s, int64_t j, double* tr, int64_t qmax) {
  if (colv(s, APPLY, j) == 0.0) return;
  const int64_t b = (int64_t)s[H_NCOLS];
  const int64_t k = (int64_t)colv(s, ITERS, j) - 1;
  if (k < 0 || k >= qmax) return;
  trace_alpha(tr, b, qmax)[k * b + j] = colv(s, ALPHA, j);
  if (colv(s, UPDP, j) != 0.0) trace_beta(tr, b, qmax)[k * b + j] = colv(s, BETA, j);
}

}}  // namespace gsi::cgst
