// pipeline.hpp -- host-side order of operations of RandMatFact.jl over a gsi::Backend,
// row-sharded over gsi::Comm ranks.  No kernel code here.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <vector>
#include "backend.hpp"

namespace gsi {

// RAII panel in backend memory
struct Buf {
  Backend* be = nullptr;
  double* p = nullptr;
  size_t count = 0;
  Buf() {}
  Buf(Backend* b, size_t n) : be(b), p(b->alloc(n)), count(n) {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : be(o.be), p(o.p), count(o.count) { o.p = nullptr; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { reset(); be = o.be; p = o.p; count = o.count; o.p = nullptr; }
    return *this;
  }
  ~Buf() { reset(); }
  void reset() { if (p) { be->release(p); p = nullptr; } }
};

struct Context {
  std::unique_ptr<Backend> be;
  std::unique_ptr<Comm> comm;  // null when single rank
  std::map<int64_t, bool> lus_mr_ok;   // panel height -> all ranks can run the sharded LU with in-kernel pivot exchange
  int lus_mr_selftest = -1;            // -1 not run yet; else bit f set: form f of the in-kernel exchange (0 one hop, 1 two hops,
                                       // 2 two hops + overflow rows) reproduced the per-step factors on this communicator
  int64_t lus_mr_gen = -1;             // Backend::lus_mr_generation() the entries of lus_mr_ok were agreed under
  // ---- which path ran (gsi_ctx_path_info) ----
  // form of a panel LU under a communicator: 0 none yet, 1 replicated (gathered panel, every rank factors it), 2 row-sharded
  // with one collective per pivot step, 3 / 4 / 5 row-sharded persistent leaves with the in-kernel exchange in one hop / two
  // hops / two hops + overflow rows
  enum LuForm { LU_NONE = 0, LU_REPLICATED = 1, LU_PER_STEP = 2, LU_MR_1HOP = 3, LU_MR_2HOP = 4, LU_MR_OV = 5, LU_FORMS = 6 };
  int64_t lu_form_last = LU_NONE;
  int64_t lu_form_count[LU_FORMS] = {0, 0, 0, 0, 0, 0};
  int64_t ranks_seen = 1;              // sum over the communicator of one per rank, taken when it was created
  int profile_level = 0;               // gsi_ctx_profile: 2 = skew barriers in front of collectives / sharded LUs (PH_COMM_WAIT)
  int64_t lu_timeouts_recovered = 0;   // entry points re-run transparently after a lost co-residency (api.cpp:with_retry)
  int64_t lowrank_tails = 0;           // randsvd steps of a LowRankCovMatrix that ran their tail in sample space (randsvd_lowrank_single)
  int64_t lowrank_power_steps = 0;     // power steps S'L formed in sample space (randsvd_lowrank_single)
  int64_t lowrank_power_declines = 0;  // ... and the ones the backend declined (that call took the direct path from there on)
  int64_t lowrank_split_lus = 0;       // panels of those power steps factored as two column halves
  int64_t lowrank_split_declines = 0;  // ... and the ones whose power step declined them (factored again whole; off for the rest of that call)
  int rank() const { return comm ? comm->rank : 0; }
  int nranks() const { return comm ? comm->nranks : 1; }
};

enum OpKind { OP_DENSE = 0, OP_LOWRANK = 1, OP_GRIDCOV_IMPLICIT = 2, OP_FFT_COV = 3, OP_POINTCOV = 4, OP_FFT_COV_AT = 5,
              OP_FWD_COV = 6 };

struct FwdModel;   // pcga.hpp

// A linear operator m x n; this rank holds rows [row0, row0 + mloc).
struct Operator {
  Context* ctx = nullptr;
  OpKind kind = OP_DENSE;
  int64_t m = 0, n = 0, row0 = 0, mloc = 0;
  Buf data;        // dense: mloc x n (ld mloc).  lowrank: samples shard mloc x N (ld mloc)
  int64_t ld = 0;
  int64_t N = 0;   // lowrank: number of samples
  int64_t gx = 0, gy = 0;   // implicit grid covariance: data = the gx * gy table of the kernel over grid offsets; never stored
  // OP_POINTCOV (scattered points): data = the d x n coordinates; entries generated panel by panel, never stored whole
  int pc_d = 0, pc_kind = 0;
  double pc_ell = 1.0, pc_sigma2 = 1.0, pc_nugget = 0.0;
  // OP_FFT_COV: the backend's circulant-embedding plan.  plan_ref owns it (own_fft_plan) and is shared with every
  // OP_FFT_COV_AT built on this operator: the plan lives until the last of them is destroyed, in whatever order.
  void* plan = nullptr;
  std::shared_ptr<void> plan_ref;
  int fft_ndims = 0;                    // OP_FFT_COV / OP_FFT_COV_AT: the grid as the caller gave it (axes of one point included)
  int64_t fft_N[3] = {1, 1, 1};
  // OP_FFT_COV_AT (m x m, one rank): A = W C W', C the grid operator whose plan is shared above, W the multilinear
  // interpolation at m scattered points.  at = Backend::points_at_create's handle (owned): the points plan and its inverted
  // index, resident for the operator's lifetime; at_info = what that call reported.
  void* at = nullptr;
  int64_t at_info[4] = {0, 0, 0, 0};
  // OP_FWD_COV (nobs x nobs, one rank): A = H C H', C the grid operator whose plan is shared above, H the sparse matrix of a
  // forward model (gsi_fwd, link 0) over the n = prod fft_N cells of that grid.  The model is shared with its gsi_fwd handle:
  // its resident arrays live until the last of the two is destroyed, in whatever order.
  std::shared_ptr<const FwdModel> fwd;
  // OP_DENSE whose rows are still crossing PCIe (gsi_randsvd_dense_host / gsi_rangefinder_dense_host): the handle of
  // Backend::upload2d_begin and its row-block height.  The FIRST product A*X consumes it -- block by block as the rows land,
  // bit-identical to the product of the resident matrix -- and clears it; the entry point's guard ends the upload on every
  // other exit path.  Null everywhere else.
  mutable void* pending_upload = nullptr;
  mutable int64_t pending_block_rows = 0;
  // OP_LOWRANK, one rank: the sample Gram matrix G = S'S (N x N), made by the first randsvd that runs a step in sample space
  // (pipeline.cpp:randsvd_lowrank_single through sample_gram) and freed with the operator.  Nothing writes `data` after creation, so it cannot go stale.
  mutable Buf gram;
  Operator() = default;
  Operator(const Operator&) = delete;
  Operator& operator=(const Operator&) = delete;
  ~Operator();
};

// A.plan = plan, owned by A.plan_ref: destroyed through the context's backend when the last holder lets go
void own_fft_plan(Operator& A, void* plan);

// block-row layout used whenever a caller does not supply one
void default_shard(int64_t m, int nranks, int rank, int64_t* row0, int64_t* mloc);

// Y_loc (mloc x l, ld ldy) = rows [row0,row0+mloc) of A * X, X replicated n x l (ld ldx)
void op_mul(const Operator& A, const double* X, int64_t ldx, int64_t l, double* Yloc, int64_t ldy);
// Z (n x l, ld ldz, replicated) = A' * X where Xloc (mloc x l, ld ldx) are this rank's rows of X
void op_mul_t(const Operator& A, const double* Xloc, int64_t ldx, int64_t l, double* Z, int64_t ldz);
// Y (m x l, ld m, replicated) <- all ranks' row shards
void gather_rows(Context& c, const Operator& A, const double* Yloc, int64_t ldy, int64_t l, double* Yfull);

// lu(Y).L of a ROW-SHARDED m x l panel (this rank: rows [row0, row0 + mloc), block layout of default_shard(m)), in
// place; bit-identical to the single-rank factorization.  One small all-gather per pivot step, one all-reduce per
// leaf / block for the U12 rows of rank 0; nothing of size m x l is communicated.  Needs l <= rows of rank 0.
void lu_panel_sharded(Context& c, double* Yloc, int64_t m, int64_t row0, int64_t mloc, int64_t l);
// the same with G virtual ranks on ONE device (Yloc[g]: shard g, ld = max(mloc_g, 1), block layout of default_shard(m)):
// every primitive runs with real row offsets, the exchanges are device copies -- the one-GPU check of the multi-rank kernels
void lu_panel_sharded_virtual(Context& c, double* const* Yloc, int64_t m, int64_t l, int G);
bool use_sharded_lu(Context& c, const Operator& A, int64_t rows, int64_t l);
// rangefinder(A, l, numiterations)  RandMatFact.jl:50-80.  Omega replicated n x l (ld n).
// Returns this rank's rows of Q (mloc x l, ld mloc).
Buf rangefinder(const Operator& A, const double* Omega, int64_t l, int64_t q);
// randsvd(A, K, p, q)  RandMatFact.jl:83-90.  Z (n x (K+p), ld n) and S (K+p) replicated.
void randsvd(const Operator& A, const double* Omega, int64_t K, int64_t p, int64_t q, double* Z, double* S);
// The same with Omega given and Z returned as this rank's ROWS (block layout of default_shard(n), ld = max(nloc, 1)):
// nothing n x l is gathered for LowRankCovMatrix / FFT operators.  S replicated.
void randsvd_rows(const Operator& A, const double* Omega_loc, int64_t K, int64_t p, int64_t q, double* Zloc, double* S);
// layout changes of an n x l panel over the ranks: ROWS (own rows, all columns, ld ldr) <-> COLS (all rows, own columns, ld n)
void rows_to_cols(Context& c, int64_t n, int64_t l, const double* Rloc, int64_t ldr, double* Cloc);
void cols_to_rows(Context& c, int64_t n, int64_t l, const double* Cloc, double* Rloc, int64_t ldr);
// eig_nystrom(A, Q)  RandMatFact.jl:92-102.  Q replicated n x j; U (m x j), Sigma (j) replicated.
void eig_nystrom(const Operator& A, const double* Q, int64_t j, double* U, double* Sigma);
// thin SVD of a replicated tall W (n x l, destroyed): V (n x l, may alias W) = left singular
// vectors scaled by `scale_K` rule (K < 0: plain V; else V*sqrt(S) for i<K, 0 otherwise)
// Xr (may be null): l x l right factor, the SVD is that of W Xr (a thin Q left one product short: Backend::qr_thinQ_deferred)
void svd_tall(Context& c, double* W, int64_t n, int64_t l, int64_t K_scale, double* V, double* S, const double* Xr = nullptr);
// rangefinder(A; epsilon, r)  RandMatFact.jl:15-48 (dense operator, single rank)
typedef void (*randn_fn)(void* user, double* buf, int64_t count);
int64_t rangefinder_adaptive(const Operator& A, randn_fn rn, void* user, double epsilon, int64_t r,
                             double* Q_host);
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
struct BlockCgInfo { int64_t products = 0, converged = 0, path = 0, breakdown_column = 0; };
// The traced form of block_cg / block_pcg: tr, cgst::trace_doubles(b, qmax) doubles in backend
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
void block_cg_check(const Operator& A, int64_t b, double tol, int64_t maxiter);
BlockCgInfo block_cg(const Operator& A, const double* diag, const double* B, double* X, int64_t b, double tol, int64_t maxiter,
                     double* relres, int64_t* iters, CgTrace* trace = nullptr);
// ---- the same solve preconditioned by P = Z Z' + diag(d + shift).  P^-1 = diag(e) - W W' exactly,
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
// breakdown_kind: 1 = p'(A + D)p, 2 = r'z was not positive and finite.  Paths and GSI_CG_POLL / GSI_CG_COMPOSED as block_cg.
struct BlockPcgInfo { int64_t products = 0, converged = 0, path = 0, breakdown_column = 0, breakdown_kind = 0, K = 0; };
void block_pcg_check(const Operator& A, const LowRankPrecond& pc, int64_t b, double tol, int64_t maxiter);
BlockPcgInfo block_pcg(const Operator& A, const double* diag, const LowRankPrecond& pc, const double* B, double* X, int64_t b,
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
// throws Error if a kernel raised an asynchronous flag
void check_async_errors(Context& c);

}  // namespace gsi
