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
  // interpolation at m scattered points.  at = Backend::points_at_create's handle: the points plan and its inverted index,
  // resident; at_info = what that call reported.  at_ref owns it (own_points_at) and is shared with every operator that
  // gsi_op_fft_at_like builds on this one's points: the plan lives until the last of them is destroyed, in whatever order.
  void* at = nullptr;
  std::shared_ptr<void> at_ref;
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
// A.at = at, owned by A.at_ref in the same way (Backend::points_at_destroy)
void own_points_at(Operator& A, void* at);

// block-row layout used whenever a caller does not supply one
void default_shard(int64_t m, int nranks, int rank, int64_t* row0, int64_t* mloc);

// Y_loc (mloc x l, ld ldy) = rows [row0,row0+mloc) of A * X, X replicated n x l (ld ldx)
void op_mul(const Operator& A, const double* X, int64_t ldx, int64_t l, double* Yloc, int64_t ldy);
// OP_FFT_COV_AT / OP_FWD_COV: the columns per batch op_mul would take for l columns -- even, both n_grid x lb panels within
// 2 GiB, GSI_FFT_AT_BATCH / GSI_FWD_COV_BATCH (read at every call) overriding it
int64_t op_cov_batch(const Operator& A, int64_t l);
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
// throws Error if a kernel raised an asynchronous flag
void check_async_errors(Context& c);

}  // namespace gsi
