// solvers.hpp -- the one-rank iterative solvers and factorizations over a gsi::Backend: LSQR, multi-column conjugate
// gradients with an optional low-rank-plus-diagonal preconditioner and coefficient trace, the Gauss quadrature of a
// trace, pivoted Cholesky.  They share nothing with the row-sharded randomized pipeline of pipeline.hpp except the
// operator product.  No kernel code here.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>
#include "pipeline.hpp"

namespace gsi {

// IterativeSolvers.jl 0.9 `lsqr(A, b; maxiter)` (Paige & Saunders 1982) with that package's defaults
// (atol = btol = sqrt(eps), conlim = 1e8) on backend-resident vectors.  Call sites in the reference: lsqr.jl:54,
// lowrank.jl:142.  mul(x, y): y = A x (x: ncols, y: nrows); mul_t(x, y): y = A' x.  Returns the iteration count.
struct LsqrOperator {
  int64_t nrows = 0, ncols = 0;
  std::function<void(const double*, double*)> mul, mul_t;
};
int64_t lsqr(Context& c, const LsqrOperator& A, const double* b, double* x, int64_t maxiter);
// x = A \ b for a LowRankCovMatrix: lsqr with maxiter = number of samples  (lowrank.jl:141-144); b, x replicated (n)
int64_t lowrank_solve(const Operator& A, const double* b, double* x);
// ---- the preconditioner P = Z Z' + diag(d + shift) of block_cg below.  P^-1 = diag(e) - W W' exactly,
//      with e = 1 / (d + shift), R'R = I + Z' diag(e) Z and W = diag(e) Z R^-1: the handle keeps e (n) and W (n x K) in
//      backend memory, and on the host R (K x K, ld K, zeros below the diagonal) and log det P = sum log(d + shift) +
//      2 sum log R_kk.
struct LowRankPrecond {
  Context* ctx = nullptr;
  int64_t n = 0, K = 0;
  double dmin = 0.0, dmax = 0.0;       // min and max of d + shift
  double logdet = 0.0;
  Buf e, W;
  std::vector<double> R;
};
// what precond_lowrank_build refuses (GSI_ERR_ARG naming the argument), before anything is allocated; dmin / dmax filled
void precond_lowrank_check(Context& c, int64_t n, int64_t zcols, int64_t K, const double* diag, double shift, double* dmin,
                           double* dmax);
// Z: n x (>= K) in backend memory, ld n, not modified; diag: n HOST values or null.  A Cholesky that fails (a NaN in Z):
// GSI_ERR_NOT_POSDEF.
void precond_lowrank_build(LowRankPrecond& pc, Context& c, const double* Z, int64_t n, int64_t K, const double* diag,
                           double shift);
// Zout (n x b) = P^-1 R (n x b), both in backend memory, ld n
void precond_apply(const LowRankPrecond& pc, const double* R, int64_t b, double* Zout);
// Zout (n x b) = (W (R G1)) ./ e + G2 ./ sqrt(e) = Z G1 + sqrt(d + shift) .* G2 for G1 (K x b, ld K) and G2 (n x b, ld n),
// all in backend memory: with standard normals in G1 and G2, the columns of Zout are draws of N(0, P).  Zout is neither G1 nor G2.
void precond_sample(const LowRankPrecond& pc, const double* G1, const double* G2, int64_t b, double* Zout);
// (A + diag(d)) X = B by conjugate gradients, all b columns advanced together (cg_state.hpp): plain
// CG per column from x0 = 0, the columns sharing only the operator product Q = A P on the whole n x b panel.  A: square,
// symmetric positive semidefinite, one rank, nothing pending; diag (backend memory, n, may be null): entries >= 0 (checked
// by the caller); B, X: n x b in backend memory (ld n), B untouched.  relres, iters (HOST, b each, may be null): the
// recurred |r_j| / |b_j| at exit and the iterations applied to column j.  A column stops at |r_j| <= tol |b_j|; columns
// still active after maxiter iterations are reported (converged < b), not an error; a breakdown (p'(A + D)p not positive
// and finite) ends the call: breakdown_column is set, the outputs are filled, and the caller raises GSI_ERR_NOT_POSDEF.
// Path 1: the backend's fused panel kernels with the state resident in backend memory, polled every GSI_CG_POLL
// iterations (read per call).  Path 3: block_cg_host.hpp -- when the backend has no such kernels, or GSI_CG_COMPOSED=1
// (read per call).  Workspace: three n x b panels, the state block and the partial sums.
// pc (may be null): the same solve preconditioned by P (cg_state.hpp's pcg_* recurrences, Backend::block_pcg_*, the
// preconditioned form of block_cg_host.hpp); one n x b and one K x b panel more.  breakdown_kind: 0, 1 = p'(A + D)p,
// 2 = r'z was not positive and finite (with pc only).  K: the preconditioner's rank, 0 without one.
struct BlockCgInfo { int64_t products = 0, converged = 0, path = 0, breakdown_column = 0, breakdown_kind = 0, K = 0; };
// The traced form of block_cg: tr, cgst::trace_doubles(b, qmax) doubles in backend
// memory made by the caller, receives alpha_k and beta_k of the first qmax iterations of every column and the columns'
// rho0 (cg_state.hpp's trace_col).  On the fused path it costs one single-block launch per iteration, which only reads the
// solver's state; on the composed path the trace is kept on the host and uploaded at the end.  X, relres and iters are the
// bits of the untraced solve.  truncated: the columns that went beyond qmax iterations.
struct CgTrace {
  int64_t qmax = 0;
  Buf tr;
  int64_t truncated = 0;
};
// what block_cg refuses (GSI_ERR_ARG naming the argument), for callers that allocate before they call it
void block_cg_check(const Operator& A, const LowRankPrecond* pc, int64_t b, double tol, int64_t maxiter);
BlockCgInfo block_cg(const Operator& A, const double* diag, const LowRankPrecond* pc, const double* B, double* X, int64_t b,
                     double tol, int64_t maxiter, double* relres, int64_t* iters, CgTrace* trace = nullptr);
// ---- the Gauss quadrature of a coefficient trace (slq_state.hpp): out[j] (HOST, b) = rho0_j e1'
//      log(T_j) e1 from the first steps[j] (HOST, b; 0 .. qmax) coefficients of column j.  alpha, beta (qmax x b, step k of
//      column j at k * b + j) and rho0 (b) in backend memory.  The backend's kernel (one thread per column), or the same
//      function on the host where the backend has none.
void slq_quadrature_check(int64_t qmax, int64_t b);
void slq_quadrature(Context& c, const double* alpha, const double* beta, const int64_t* steps, const double* rho0, int64_t qmax,
                    int64_t b, double* out);
// ---- diagonal-pivoted Cholesky of a covariance read by entries (pchol_state.hpp): L L' ~ A from K
//      columns of A, without an operator product.  A: OP_DENSE (one rank, all rows resident, nothing pending),
//      OP_GRIDCOV_IMPLICIT or OP_POINTCOV, square.  L: n x >= K in backend memory, ld n; columns rank .. K - 1 are zeros.
//      piv (HOST, K, may be null): the pivots, -1 beyond the rank.  reason: pchol::STOP_*; a non-finite value (reason 4) is
//      reported, the caller raises GSI_ERR_NOT_POSDEF.  Path 1: the backend's kernels with the state resident in backend
//      memory, polled every GSI_PCHOL_POLL steps (8; read per call).  Path 3: pivoted_chol_host.hpp with columns from
//      op_mul on a unit vector -- when the backend has no such kernels, or GSI_PCHOL_COMPOSED=1 (read per call); it holds
//      L on the host.  form: 1 stored, 2 table, 3 points.
struct PcholInfo {
  int64_t rank = 0, reason = 0, path = 0, form = 0, polls = 0;
  double trace0 = 0.0, trace = 0.0, dmax = 0.0;
};
// what pivoted_cholesky refuses (GSI_ERR_ARG naming the argument), before anything is allocated
void pivoted_cholesky_check(const Operator& A, int64_t K, double tol, int64_t Lrows, int64_t Lcols);
PcholInfo pivoted_cholesky(const Operator& A, int64_t K, double tol, double* L, int64_t* piv);
// Z (n x K, ld n) = U diag(s) for the thin SVD L[:, :K] = U diag(s) V' of a resident n x >= K matrix (ld n): Z Z' = L L'
// with orthogonal columns, the form randsvd returns.  S (backend memory, K): the singular values.  L is not modified.
void principal_factor(Context& c, const double* L, int64_t n, int64_t K, double* Z, double* S);

}  // namespace gsi
