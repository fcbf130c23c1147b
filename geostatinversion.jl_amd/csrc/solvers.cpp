// solvers.cpp -- the one-rank iterative solvers and factorizations of solvers.hpp.  All arithmetic happens in the Backend
// (or, where it declines, in the *_host.hpp forms of the same recurrences); this file sequences operator products around
// state that lives in backend memory and polls it.
#include "solvers.hpp"
#include "lsqr_state.hpp"
#include "block_cg_host.hpp"
#include "pivoted_chol_host.hpp"
#include "slq_state.hpp"
#include "pointcov.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include "../../include/gsi_hip.h"

namespace gsi {

// ---- IterativeSolvers.lsqr (third-party, Project.toml:21; not under the reference tree): Paige & Saunders' LSQR
//      with that package's defaults, restated from the published algorithm exactly as oracle/oracle.py:lsqr does
//      (same order of operations, same stopping rules).  Vectors AND the scalar recurrences live in backend memory
//      (lsqr_state.hpp): an iteration is the two operator products plus two fused launch groups, nothing waits for the
//      host; the host polls {stopped, iterations} every LSQR_POLL iterations (iterations enqueued past the stopping point
//      are no-ops on the device, so x and the iteration count are exactly those of the one-scalar-at-a-time loop).
int64_t lsqr(Context& c, const LsqrOperator& A, const double* b, double* x, int64_t maxiter) {
  using namespace lsqrst;
  Backend* be = c.be.get();
  const int64_t m = A.nrows, n = A.ncols;
  const double tol = std::sqrt(2.220446049250313e-16);
  const double conlim = 1e8;
  if (maxiter < 0) maxiter = std::max(m, n);
  Buf u(be, (size_t)m), v(be, (size_t)n), w(be, (size_t)n), t(be, (size_t)std::max(m, n));
  be->fill_zero(x, (size_t)n);
  be->copy2d(u.p, m, b, m, m, 1);
  const double beta = be->nrm2(m, u.p);                // the two start-up norms are read by the host: once per solve
  if (beta == 0.0) return 0;
  be->scal(m, 1.0 / beta, u.p);
  A.mul_t(u.p, v.p);
  const double alpha = be->nrm2(n, v.p);
  if (alpha == 0.0) return 0;
  be->scal(n, 1.0 / alpha, v.p);
  be->copy2d(w.p, n, v.p, n, n, 1);
  double st[COUNT] = {0.0};
  st[ALPHA] = alpha; st[BETA] = beta; st[RHOBAR] = alpha; st[PHIBAR] = beta; st[BNORM] = beta;
  st[CS2] = -1.0; st[SN2] = 0.0; st[MAXITER] = (double)maxiter;
  st[ATOL] = tol; st[BTOL] = tol; st[CTOL] = 1.0 / conlim;
  Buf work(be, be->lsqr_work_doubles());
  be->upload2d(work.p, COUNT, st, COUNT, COUNT, 1);
  be->lsqr_begin(n, w.p, work.p);
  static const int64_t poll = getenv("GSI_LSQR_POLL") ? std::max(1, atoi(getenv("GSI_LSQR_POLL"))) : 8;
  int64_t enq = 0;
  while (enq < maxiter) {
    const int64_t burst = std::min<int64_t>(poll, maxiter - enq);
    for (int64_t k = 0; k < burst; ++k) {
      A.mul(v.p, t.p);                                 // u = A v - alpha u; beta = |u|; u /= beta
      be->lsqr_step_u(m, t.p, u.p, work.p);
      A.mul_t(u.p, t.p);                               // v = A' u - beta v; alpha = |v|; v /= alpha; x, w updates
      be->lsqr_step_v(n, t.p, v.p, w.p, x, work.p);
    }
    enq += burst;
    be->download2d(st, COUNT, work.p, COUNT, COUNT, 1);
    if (st[STOPPED] != 0.0) break;
  }
  return (int64_t)st[ITERS];
}

int64_t lowrank_solve(const Operator& A, const double* b, double* x) {
  Context& c = *A.ctx;
  Backend* be = c.be.get();
  if (A.kind != OP_LOWRANK) throw Error(GSI_ERR_ARG, "lowrank_solve: the operator is not a LowRankCovMatrix");
  LsqrOperator L;
  L.nrows = L.ncols = A.n;
  Buf yloc(be, (size_t)std::max<int64_t>(A.mloc, 1));
  L.mul = [&](const double* xin, double* y) {          // adjoint(A) === A (lowrank.jl:38-40)
    op_mul(A, xin, A.n, 1, yloc.p, A.mloc);
    gather_rows(c, A, yloc.p, A.mloc, 1, y);
  };
  L.mul_t = L.mul;
  return lsqr(c, L, b, x, A.N);                        // maxiter = length(A.samples)   lowrank.jl:142
}

// ---- conjugate gradients on (A + diag(d)) X = B, the b columns together (solvers.hpp).  The
//      operator product goes through op_mul on the whole panel in both paths; everything else of an iteration is either
//      Backend::block_cg_step (state in backend memory, nothing waits for the host; iterations enqueued past the point
//      where every column has stopped are no-ops on the device, so X, relres and iters do not depend on the poll interval)
//      or block_cg_host.hpp.  GSI_CG_POLL: 4 by default.  A poll is one small copy and a drain of the stream: measured at
//      0.04 ms each (10^6 points, 64 columns, 9.7 ms per iteration: polling every iteration adds 0.3 % to the call, every
//      4th 0.04 %; profiles/op_solve.json, "poll_sweep"), while an interval of k can run k - 1 operator products after the last
//      column has stopped.  4 keeps both below a percent of any solve long enough to matter.
//      With a preconditioner (pc) the same driver runs Backend::block_pcg_* and the preconditioned
//      form of block_cg_host.hpp: two buffers more (z = P^-1 r and the K x b coefficients), a larger state block.
void block_cg_check(const Operator& A, const LowRankPrecond* pc, int64_t b, double tol, int64_t maxiter) {
  Context& c = *A.ctx;
  if (c.comm) throw Error(GSI_ERR_ARG, "block_cg: ctx has a communicator; the solver runs on one rank");
  if (A.m != A.n) throw Error(GSI_ERR_ARG, "block_cg: op is " + std::to_string(A.m) + " x " + std::to_string(A.n) + ", not square");
  if (A.pending_upload != nullptr) throw Error(GSI_ERR_ARG, "block_cg: op has an upload pending");
  if (b < 1) throw Error(GSI_ERR_ARG, "block_cg: B needs at least one column");
  if (!(tol > 0.0 && tol < 1.0)) throw Error(GSI_ERR_ARG, "block_cg: tol must lie in (0, 1)");
  if (maxiter < 1) throw Error(GSI_ERR_ARG, "block_cg: maxiter must be at least 1");
  if (!pc) return;
  if (pc->ctx != A.ctx) throw Error(GSI_ERR_ARG, "block_pcg: pc belongs to another context");
  if (pc->n != A.n) throw Error(GSI_ERR_ARG, "block_pcg: pc was built for " + std::to_string(pc->n) + " rows, op has " +
                                                 std::to_string(A.n));
}
// the composed paths keep the trace on the host: it goes to the caller's buffer at the end; the columns beyond qmax
static void trace_finish(Backend* be, CgTrace* trace, const std::vector<double>& host_trace, const double* st, int64_t b) {
  if (!host_trace.empty()) be->upload2d(trace->tr.p, (int64_t)host_trace.size(), host_trace.data(), (int64_t)host_trace.size(),
                                        (int64_t)host_trace.size(), 1);
  trace->truncated = 0;
  for (int64_t j = 0; j < b; ++j)
    if ((int64_t)cgst::colv(st, cgst::ITERS, j) > trace->qmax) ++trace->truncated;
}

BlockCgInfo block_cg(const Operator& A, const double* diag, const LowRankPrecond* pc, const double* B, double* X, int64_t b,
                     double tol, int64_t maxiter, double* relres, int64_t* iters, CgTrace* trace) {
  using namespace cgst;
  block_cg_check(A, pc, b, tol, maxiter);
  Backend* be = A.ctx->be.get();
  const int64_t n = A.n, K = pc ? pc->K : 0;
  const char* ec = getenv("GSI_CG_COMPOSED");
  const size_t wd = (ec && atoi(ec) != 0) ? 0 : (pc ? be->block_pcg_work_doubles(b) : be->block_cg_work_doubles(b));
  BlockCgInfo info;
  info.path = wd ? 1 : 3;
  info.K = K;
  Buf R(be, (size_t)n * b), P(be, (size_t)n * b), Q(be, (size_t)n * b), Y, S;
  if (pc) { Y = Buf(be, (size_t)n * b); S = Buf(be, (size_t)K * b); }
  be->copy2d(R.p, n, B, n, n, b);
  if (!pc) be->copy2d(P.p, n, B, n, n, b);                      // (the preconditioned begin writes P = P^-1 B)
  be->fill_zero(X, (size_t)n * b);
  std::vector<double> st(pc ? pcg_state_doubles(b) : state_doubles(b), 0.0), host_trace;
  if (trace) be->fill_zero(trace->tr.p, trace_doubles(b, trace->qmax));
  if (wd) {
    int64_t poll = 4;
    if (const char* e = getenv("GSI_CG_POLL")) poll = std::max<int64_t>(1, atoll(e));
    Buf work(be, wd);
    be->fill_zero(work.p, wd);
    {
      ScopedPhase ph(be, PH_OTHER);
      if (pc) be->block_pcg_begin(n, b, K, B, pc->e.p, pc->W.p, S.p, Y.p, P.p, tol, maxiter, work.p);
      else be->block_cg_begin(n, b, B, tol, maxiter, work.p);
      if (trace) be->cg_trace_begin(work.p, trace->tr.p, trace->qmax);
    }
    double hdr[H_COUNT];
    be->download2d(hdr, H_COUNT, work.p, H_COUNT, H_COUNT, 1);
    int64_t enq = 0;
    while (hdr[H_ACTIVE] > 0.0 && enq < maxiter) {
      const int64_t burst = std::min<int64_t>(poll, maxiter - enq);
      for (int64_t k = 0; k < burst; ++k) {
        op_mul(A, P.p, n, b, Q.p, n);
        ScopedPhase ph(be, PH_OTHER);
        if (pc) be->block_pcg_step(n, b, K, Q.p, diag, pc->e.p, pc->W.p, X, R.p, P.p, S.p, Y.p, work.p);
        else be->block_cg_step(n, b, Q.p, diag, X, R.p, P.p, work.p);
        if (trace) be->cg_trace_step(work.p, trace->tr.p, trace->qmax);
      }
      enq += burst;
      be->download2d(hdr, H_COUNT, work.p, H_COUNT, H_COUNT, 1);
    }
    info.products = enq;
    be->download2d(st.data(), (int64_t)st.size(), work.p, (int64_t)st.size(), (int64_t)st.size(), 1);
  } else {
    if (trace) host_trace.assign(trace_doubles(b, trace->qmax), 0.0);
    info.products = block_cg_composed(be, [&](const double* p, double* q) { op_mul(A, p, n, b, q, n); }, n, b, diag, B, X, R.p,
                                      P.p, Q.p, tol, maxiter, st, trace ? host_trace.data() : nullptr, trace ? trace->qmax : 0,
                                      pc ? pc->e.p : nullptr, pc ? pc->W.p : nullptr, K, Y.p, S.p);
  }
  if (trace) trace_finish(be, trace, host_trace, st.data(), b);
  info.converged = (int64_t)st[H_CONVERGED];
  info.breakdown_column = (int64_t)st[H_BREAKDOWN];
  // (the plain state block has no BKIND field: its only breakdown is p'(A + D)p)
  if (info.breakdown_column != 0) info.breakdown_kind = pc ? (int64_t)colv(st.data(), BKIND, info.breakdown_column - 1) : 1;
  for (int64_t j = 0; j < b; ++j) {
    if (relres) relres[j] = pc ? pcg_relres(st.data(), j) : cgst::relres(st.data(), j);
    if (iters) iters[j] = (int64_t)colv(st.data(), ITERS, j);
  }
  return info;
}

// ---- the preconditioner P = Z Z' + diag(d + shift) and the preconditioned solve (solvers.hpp).
//      The setup is composed from what exists -- scale_rows, gemm_tn, chol_upper, trsm_right_upper -- around the backend's
//      precond_rows / add_identity; a backend that declines those (the CPU reference backend) gets the row scalings and the
//      identity from the host.
void precond_lowrank_check(Context& c, int64_t n, int64_t zcols, int64_t K, const double* diag, double shift, double* dmin,
                           double* dmax) {
  if (c.comm) throw Error(GSI_ERR_ARG, "precond_lowrank: ctx has a communicator; the preconditioner lives on one rank");
  if (n < 1) throw Error(GSI_ERR_ARG, "precond_lowrank: Z has no rows");
  if (K < 1) throw Error(GSI_ERR_ARG, "precond_lowrank: K must be at least 1");
  if (K > zcols) throw Error(GSI_ERR_ARG, "precond_lowrank: K exceeds the columns of Z, " + std::to_string(zcols));
  if (K > n) throw Error(GSI_ERR_ARG, "precond_lowrank: K exceeds the rows of Z, " + std::to_string(n));
  if (K > 2048) throw Error(GSI_ERR_ARG, "precond_lowrank: K exceeds 2048, the limit of the small Cholesky");
  if (!(shift >= 0.0 && shift <= 1.79769313486231570815e308))
    throw Error(GSI_ERR_ARG, "precond_lowrank: shift is negative or not finite");
  double lo = 1.79769313486231570815e308, hi = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double v = (diag ? diag[i] : 0.0) + shift;
    if (!(v > 0.0 && v <= 1.79769313486231570815e308))
      throw Error(GSI_ERR_ARG, diag ? "precond_lowrank: diag[" + std::to_string(i) + "] + shift is not positive and finite"
                                    : std::string("precond_lowrank: without diag, shift must be positive (diag + shift is not positive)"));
    lo = std::min(lo, v);
    hi = std::max(hi, v);
  }
  if (dmin) *dmin = lo;
  if (dmax) *dmax = hi;
}

void precond_lowrank_build(LowRankPrecond& pc, Context& c, const double* Z, int64_t n, int64_t K, const double* diag,
                           double shift) {
  precond_lowrank_check(c, n, K, K, diag, shift, &pc.dmin, &pc.dmax);
  Backend* be = c.be.get();
  pc.ctx = &c; pc.n = n; pc.K = K;
  std::vector<double> eh((size_t)n), sh((size_t)n);
  for (int64_t i = 0; i < n; ++i) eh[(size_t)i] = (diag ? diag[i] : 0.0) + shift;
  pc.e = Buf(be, (size_t)n);
  Buf sqe(be, (size_t)n), C(be, (size_t)K * K);
  be->upload2d(pc.e.p, n, eh.data(), n, n, 1);
  if (!be->precond_rows(n, pc.e.p, sqe.p)) {
    for (int64_t i = 0; i < n; ++i) { eh[(size_t)i] = 1.0 / eh[(size_t)i]; sh[(size_t)i] = std::sqrt(eh[(size_t)i]); }
    be->upload2d(pc.e.p, n, eh.data(), n, n, 1);
    be->upload2d(sqe.p, n, sh.data(), n, n, 1);
  }
  std::vector<double> zh;                                       // Z on the host, where the backend does not scale rows
  {
    Buf T(be, (size_t)n * K);                                   // T = diag(sqrt(e)) Z;  C = I + T'T
    if (!be->scale_rows(n, K, sqe.p, Z, n, T.p, n)) {
      be->download2d(sh.data(), n, sqe.p, n, n, 1);
      be->download2d(eh.data(), n, pc.e.p, n, n, 1);
      zh.resize((size_t)n * K);
      be->download2d(zh.data(), n, Z, n, n, K);
      std::vector<double> th((size_t)n * K);
      for (int64_t k = 0; k < K; ++k)
        for (int64_t i = 0; i < n; ++i) th[(size_t)(i + k * n)] = sh[(size_t)i] * zh[(size_t)(i + k * n)];
      be->upload2d(T.p, n, th.data(), n, n, K);
    }
    be->gemm_tn(K, K, n, 1.0, T.p, n, T.p, n, 0.0, C.p, K);
  }
  if (!be->add_identity(C.p, K)) {
    std::vector<double> ch((size_t)K * K);
    be->download2d(ch.data(), K, C.p, K, K, K);
    for (int64_t k = 0; k < K; ++k) ch[(size_t)(k + k * K)] += 1.0;
    be->upload2d(C.p, K, ch.data(), K, K, K);
  }
  be->chol_upper(C.p, K);
  // R and log det P = sum log(d + shift) + 2 sum log R_kk stay on the host (K^2 numbers, read by precond_sample)
  pc.R.assign((size_t)K * K, 0.0);
  be->download2d(pc.R.data(), K, C.p, K, K, K);
  {
    long double acc = 0.0L;
    for (int64_t i = 0; i < n; ++i) acc += std::log((long double)((diag ? diag[i] : 0.0) + shift));
    for (int64_t k = 0; k < K; ++k) {
      acc += 2.0L * std::log((long double)pc.R[(size_t)(k + k * K)]);
      for (int64_t i = k + 1; i < K; ++i) pc.R[(size_t)(i + k * K)] = 0.0;
    }
    pc.logdet = (double)acc;
  }
  pc.W = Buf(be, (size_t)n * K);                                // W = diag(e) Z R^-1
  if (zh.empty()) {
    be->scale_rows(n, K, pc.e.p, Z, n, pc.W.p, n);
  } else {
    for (int64_t k = 0; k < K; ++k)
      for (int64_t i = 0; i < n; ++i) zh[(size_t)(i + k * n)] *= eh[(size_t)i];
    be->upload2d(pc.W.p, n, zh.data(), n, n, K);
  }
  be->trsm_right_upper(pc.W.p, n, K, n, C.p);
  check_async_errors(c);                                        // the Cholesky's flag: GSI_ERR_NOT_POSDEF
}

void precond_apply(const LowRankPrecond& pc, const double* R, int64_t b, double* Zout) {
  Backend* be = pc.ctx->be.get();
  Buf S(be, (size_t)pc.K * b);
  precond_apply_composed(be, pc.n, pc.K, pc.e.p, pc.W.p, R, b, S.p, Zout);
}

void precond_sample(const LowRankPrecond& pc, const double* G1, const double* G2, int64_t b, double* Zout) {
  Backend* be = pc.ctx->be.get();
  const int64_t n = pc.n, K = pc.K;
  Buf Rd(be, (size_t)K * K), T(be, (size_t)K * b), Y(be, (size_t)n * b);
  be->upload2d(Rd.p, K, pc.R.data(), K, K, K);
  be->gemm_nn(K, b, K, 1.0, Rd.p, K, G1, K, 0.0, T.p, K);        // T = R G1
  be->gemm_nn(n, b, K, 1.0, pc.W.p, n, T.p, K, 0.0, Y.p, n);     // Y = W T = diag(e) Z G1
  if (!be->precond_sample_rows(n, b, pc.e.p, Y.p, G2, Zout)) {
    std::vector<double> eh((size_t)n), yh((size_t)n * b), gh((size_t)n * b);
    be->download2d(eh.data(), n, pc.e.p, n, n, 1);
    be->download2d(yh.data(), n, Y.p, n, n, b);
    be->download2d(gh.data(), n, G2, n, n, b);
    for (int64_t j = 0; j < b; ++j)
      for (int64_t i = 0; i < n; ++i)
        yh[(size_t)(i + j * n)] = yh[(size_t)(i + j * n)] / eh[(size_t)i] + gh[(size_t)(i + j * n)] / std::sqrt(eh[(size_t)i]);
    be->upload2d(Zout, n, yh.data(), n, n, b);
  }
}

// ---- the Gauss quadrature of a coefficient trace (solvers.hpp; slq_state.hpp) ----
void slq_quadrature_check(int64_t qmax, int64_t b) {
  if (qmax < 1) throw Error(GSI_ERR_ARG, "slq: qmax must be at least 1");
  if (qmax > slq::QMAX_LIMIT) throw Error(GSI_ERR_ARG, "slq: qmax exceeds " + std::to_string(slq::QMAX_LIMIT));
  if (b < 1) throw Error(GSI_ERR_ARG, "slq: b must be at least 1");
}
void slq_quadrature(Context& c, const double* alpha, const double* beta, const int64_t* steps, const double* rho0, int64_t qmax,
                    int64_t b, double* out) {
  slq_quadrature_check(qmax, b);
  Backend* be = c.be.get();
  std::vector<double> sh((size_t)b);
  for (int64_t j = 0; j < b; ++j) sh[(size_t)j] = (double)std::min<int64_t>(std::max<int64_t>(steps[j], 0), qmax);
  {
    Buf sd(be, (size_t)b), od(be, (size_t)b), work(be, slq::work_doubles(b, qmax));
    be->upload2d(sd.p, b, sh.data(), b, b, 1);
    ScopedPhase ph(be, PH_OTHER);
    if (be->slq_quadrature(alpha, beta, sd.p, rho0, qmax, b, work.p, od.p)) {
      be->download2d(out, b, od.p, b, b, 1);
      return;
    }
  }
  std::vector<double> ah((size_t)qmax * b), bh((size_t)qmax * b), rh((size_t)b), work(slq::work_doubles(b, qmax));
  be->download2d(ah.data(), qmax * b, alpha, qmax * b, qmax * b, 1);
  be->download2d(bh.data(), qmax * b, beta, qmax * b, qmax * b, 1);
  be->download2d(rh.data(), b, rho0, b, b, 1);
  for (int64_t j = 0; j < b; ++j)
    out[j] = slq::quadrature_log(ah.data() + j, bh.data() + j, (int64_t)sh[(size_t)j], rh[(size_t)j], b, work.data() + j,
                                 work.data() + qmax * b + j, work.data() + 2 * qmax * b + j);
}

// ---- diagonal-pivoted Cholesky of a covariance read by entries (solvers.hpp) ----
static int pchol_form(const Operator& A) {
  switch (A.kind) {
    case OP_DENSE: return 1;
    case OP_GRIDCOV_IMPLICIT: return 2;
    case OP_POINTCOV: return 3;
    default: return 0;
  }
}
void pivoted_cholesky_check(const Operator& A, int64_t K, double tol, int64_t Lrows, int64_t Lcols) {
  Context& c = *A.ctx;
  if (c.comm) throw Error(GSI_ERR_ARG, "pivoted_cholesky: ctx has a communicator; the factorization runs on one rank");
  if (pchol_form(A) == 0)
    throw Error(GSI_ERR_ARG, "pivoted_cholesky: op must be a dense, an implicit grid-covariance or an implicit point-covariance "
                             "operator (the kinds whose entries can be read); use randsvd for the others");
  if (A.m != A.n) throw Error(GSI_ERR_ARG, "pivoted_cholesky: op is " + std::to_string(A.m) + " x " + std::to_string(A.n) + ", not square");
  if (A.kind == OP_DENSE && (A.row0 != 0 || A.mloc != A.m))
    throw Error(GSI_ERR_ARG, "pivoted_cholesky: op does not hold all its rows on this rank");
  if (A.pending_upload != nullptr) throw Error(GSI_ERR_ARG, "pivoted_cholesky: op has an upload pending");
  if (K < 1) throw Error(GSI_ERR_ARG, "pivoted_cholesky: K must be at least 1");
  if (K > A.n) throw Error(GSI_ERR_ARG, "pivoted_cholesky: K exceeds the size of op, " + std::to_string(A.n));
  if (K > 2048) throw Error(GSI_ERR_ARG, "pivoted_cholesky: K exceeds 2048");
  if (Lrows != A.n) throw Error(GSI_ERR_ARG, "pivoted_cholesky: L must have size(op, 1) = " + std::to_string(A.n) + " rows");
  if (K > Lcols) throw Error(GSI_ERR_ARG, "pivoted_cholesky: K exceeds the columns of L, " + std::to_string(Lcols));
  if (!(tol >= 0.0 && tol < 1.0)) throw Error(GSI_ERR_ARG, "pivoted_cholesky: tol must lie in [0, 1)");
}

PcholInfo pivoted_cholesky(const Operator& A, int64_t K, double tol, double* L, int64_t* piv) {
  using namespace pchol;
  Backend* be = A.ctx->be.get();
  const int64_t n = A.n;
  Backend::PcholSource src;
  src.form = pchol_form(A);
  src.data = A.data.p; src.ld = A.ld; src.gx = A.gx; src.gy = A.gy;
  src.pc_d = A.pc_d; src.pc_kind = A.pc_kind; src.pc_ell = A.pc_ell; src.pc_sigma2 = A.pc_sigma2; src.pc_nugget = A.pc_nugget;
  const char* ec = getenv("GSI_PCHOL_COMPOSED");
  const size_t wd = (ec && atoi(ec) != 0) ? 0 : be->pchol_work_doubles(src, n, K);
  PcholInfo info;
  info.path = wd ? 1 : 3;
  info.form = src.form;
  std::vector<double> st(state_doubles(K), 0.0);
  if (wd) {
    int64_t poll = 8;
    if (const char* e = getenv("GSI_PCHOL_POLL")) poll = std::max<int64_t>(1, atoll(e));
    Buf work(be, wd), d(be, (size_t)n);
    be->fill_zero(L, (size_t)n * K);
    ScopedPhase ph(be, PH_OTHER);
    be->pchol_begin(src, n, K, tol, L, n, d.p, work.p);
    double hdr[S_COUNT];
    be->download2d(hdr, S_COUNT, work.p, S_COUNT, S_COUNT, 1);
    info.polls = 1;
    int64_t enq = 0;
    while (hdr[S_REASON] == 0.0 && enq < K) {
      const int64_t burst = std::min<int64_t>(poll, K - enq);
      for (int64_t k = 0; k < burst; ++k) be->pchol_step(src, n, K, L, n, d.p, work.p);
      enq += burst;
      be->download2d(hdr, S_COUNT, work.p, S_COUNT, S_COUNT, 1);
      ++info.polls;
    }
    be->download2d(st.data(), (int64_t)st.size(), work.p, (int64_t)st.size(), (int64_t)st.size(), 1);
  } else {
    // the diagonal by entries, as the kernels read it; the columns by the operator product with a unit vector
    std::vector<double> dh((size_t)n), Lh((size_t)n * K);
    if (src.form == 1) be->download2d(dh.data(), 1, A.data.p, A.ld + 1, 1, n);
    else if (src.form == 2) { double t0 = 0.0; be->download2d(&t0, 1, A.data.p, 1, 1, 1); std::fill(dh.begin(), dh.end(), t0); }
    else {
      const pointcov::Params pp = {A.pc_d, A.pc_kind, 1.0 / A.pc_ell, A.pc_sigma2, A.pc_nugget};
      std::fill(dh.begin(), dh.end(), pointcov::kernel(pp, 0.0, true));
    }
    Buf e(be, (size_t)n), y(be, (size_t)n);
    be->fill_zero(e.p, (size_t)n);
    const double one = 1.0, zero = 0.0;
    host_factor(n, K, tol, dh.data(), [&](int64_t p, double* out) {
      be->upload2d(e.p + p, 1, &one, 1, 1, 1);
      op_mul(A, e.p, n, 1, y.p, n);
      be->upload2d(e.p + p, 1, &zero, 1, 1, 1);
      be->download2d(out, n, y.p, n, n, 1);
    }, Lh.data(), n, st);
    be->upload2d(L, n, Lh.data(), n, n, K);
  }
  info.rank = (int64_t)st[S_STEP];
  info.reason = (int64_t)st[S_REASON];
  info.trace0 = st[S_TRACE0]; info.trace = st[S_TRACE]; info.dmax = st[S_DMAX];
  if (piv)
    for (int64_t j = 0; j < K; ++j) piv[j] = (j < info.rank) ? (int64_t)st[(size_t)S_COUNT + (size_t)j] : -1;
  return info;
}

void principal_factor(Context& c, const double* L, int64_t n, int64_t K, double* Z, double* S) {
  Backend* be = c.be.get();
  Buf W(be, (size_t)n * K);
  be->copy2d(W.p, n, L, n, n, K);
  svd_tall(c, W.p, n, K, -1, Z, S);                             // Z = U (plain), S = the singular values
  if (!be->scale_cols(n, K, Z, n, S)) {
    std::vector<double> zh((size_t)n * K), sh((size_t)K);
    be->download2d(zh.data(), n, Z, n, n, K);
    be->download2d(sh.data(), K, S, K, K, 1);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t i = 0; i < n; ++i) zh[(size_t)(i + k * n)] *= sh[(size_t)k];
    be->upload2d(Z, n, zh.data(), n, n, K);
  }
}

}  // namespace gsi
