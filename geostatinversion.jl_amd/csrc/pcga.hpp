// pcga.hpp -- the PCGA consumers over a gsi::Backend (DESIGN.md sections 4.7 - 4.7d): the saddle-point matrix and its
// Cholesky solve, the posterior variance from the resident basis, the sparse forward model, and the two products of the
// iteration with that basis.  Each consumer asks the backend first; when it answers "not mine", or the consumer's
// GSI_*_HOST switch is set (read at each call), the operands are downloaded and the host restatement runs.  No kernel code here.
#pragma once
#include "pipeline.hpp"
#include "fwd_plan.hpp"
#include "fwd_adjoint_plan.hpp"

namespace gsi {

// What ran, as the C ABI's info_out[2] reports it: column is 0 or the 1-based column at which a Cholesky factorization stopped
// being positive definite; path is PATH_BACKEND for the backend's kernels, PATH_HOST for the host path (the backend declined,
// or the switch was set), 0 when neither was reached.
struct PathInfo {
  int64_t column = 0;
  int64_t path = 0;
};
enum : int64_t { PATH_BACKEND = 1, PATH_HOST = 3 };
// GSI_ERR_NOT_POSDEF naming col (recorded in info.column) when col > 0; else GSI_ERR_SINGULAR with singular_text when
// `singular`; else nothing
void throw_chol_outcome(PathInfo& info, int64_t col, bool singular, const char* singular_text);

// The resident xi-basis: Z in backend memory, n x K, ld n; bits 64: double, 32: float in a double-typed allocation.
struct BasisRef {
  const void* Z;
  int bits;
  int64_t n, K;
};
// out (host, n x (K + 3), ld n) = paramstorun of direct.jl:39-45 / lsqr.jl:37-43; s and X on the host
void basis_params(Context& c, BasisRef Z, const double* s, const double* X, double delta, double* out);
// s_out (host, n) = X beta_bar + sum_i xis[i] dot(eta_i, xi_bar)  (direct.jl:59-65); X, etas (nobs x K, ld nobs), xi_bar on the host
void basis_update(Context& c, BasisRef Z, const double* X, double beta_bar, const double* etas, int64_t nobs,
                  const double* xi_bar, double* s_out);

// PCGALowRankMatrix(etas, HX, R)  (lowrank.jl:32-36, 83-97): [(HQH + R) HX; HX' 0], HQH = sum eta_i eta_i' kept implicit.
struct PcgaLowRank {
  Context* ctx = nullptr;
  int64_t nobs = 0, K = 0;
  Buf E, HX, R;        // E: nobs x K (eta_i as columns); R: nobs x nobs dense, or nobs values when r_diag
  bool r_diag = false;
  void mul(const double* x, double* y) const;   // x, y: nobs + 1
  // x = A \ b (host vectors, nobs + 1) by Cholesky of HQH + R (direct.jl:56-58 for a positive definite HQH + R; DESIGN.md
  // section 4.7c; GSI_SADDLE_HOST).  Throws GSI_ERR_NOT_POSDEF or GSI_ERR_SINGULAR (w'w == 0 or a non-finite beta) with info filled.
  void solve(const double* b, double* x, PathInfo& info) const;
};
// cholesky(Symmetric(A, :L)).L of a host matrix (n x n, lda) into L (n x n, ld n, strictly upper triangle zero).
// A failed factorization fills info, leaves L unspecified and does not throw.
void chol_lower_host_matrix(Context& c, const double* A, int64_t n, int64_t lda, double* L, PathInfo& info);

// ---- the posterior variance from the resident basis (GSI_POST_HOST) ----
// a[i] = |W' z_i|^2, q[i] = |z_i|^2 (q may be null), t[i] = u' z_i (u, t null together) over the rows of the basis.
// W (K x ncols, ld ldw), u and the outputs are host arrays.
void basis_quadform(Context& c, BasisRef Z, const double* W, int64_t ldw, int64_t ncols, bool upper, const double* u,
                    double* a, double* q, double* t, PathInfo& info);
// W (K x K upper triangular), u (K), gamma of the capacitance form, from the matrix's E, HX and R; host outputs (any may be
// null).  Wdev / udev (may be null): on the backend's path W and u are also left there for the row pass (empty on the host
// path).  Throws GSI_ERR_NOT_POSDEF (info.column = the failing column of R) or GSI_ERR_SINGULAR.
void posterior_factor(const PcgaLowRank& A, double* W, double* u, double* gamma, PathInfo& info, Buf* Wdev = nullptr,
                      Buf* udev = nullptr);
// var (n, host) by the two row formulas of section 4.7d; X (n) and prior (n, or null: the low-rank prior |z_i|^2) on the host
void posterior_variance(Context& c, BasisRef Z, const PcgaLowRank& A, const double* X, const double* prior, double* var,
                        PathInfo& info);

// ---- the exact posterior variance of linear inversion and kriging (GSI_POSTX_HOST) ----
// What gsi_op_posterior_variance reports in info_out[0 .. 5].
struct PostxInfo {
  int64_t column = 0;            // 0, or the 1-based column at which H C H' + D stopped being positive definite
  int64_t path = 0;              // PATH_BACKEND / PATH_HOST
  int64_t batches = 0;           // batches of columns of L^-T that went through the prior adjoint and the row pass
  int64_t width = 0;             // columns per batch
  int64_t adjoint_columns = 0;   // columns sent through V -> C H' V in total (nobs + p)
  int64_t trapezoid_bytes = 0;   // (2 nobs + p) nobs doubles
};
// acc (n, backend memory) += the row sums of A .* B for n x b panels in backend memory (Backend::rowdot_acc); when the
// backend declines, or GSI_POSTX_HOST=1, or force_host: download, posterior_exact_host.hpp, upload.  Returns the path.
int64_t rowdot_acc(Context& c, int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc,
                   bool force_host = false);
// var (n_grid, host) = diag(C - C H'(H C H' + D)^-1 H C) + the drift term, for A = H C H' an OP_FWD_COV or OP_FFT_COV_AT
// operator: diag (host, nobs values, or null), X (host, n_grid x p, ld ldx; null with p = 0), batch columns per batch (0:
// op_cov_batch).  The arguments are validated by the caller.  Throws GSI_ERR_NOT_POSDEF (info.column) or GSI_ERR_SINGULAR
// (H X rank deficient) with info filled.
void posterior_variance_exact(const Operator& A, const double* diag, const double* X, int64_t ldx, int64_t p, int64_t batch,
                              double* var, PostxInfo& info);

// ---- the bilinear forms of the likelihood gradient (GSI_BILINEAR_HOST) ----
// With V = Y + dd .* R for n x b panels L, Y, R in backend memory (ld n; dd: n HOST values or null, then R may be null):
// gram (g x g, host) [a + g c] = sum_i L[i, a] V[i, c] and t (b - g, host) [j - g] = sum_i L[i, j] V[i, j], in the order of
// bilinear_terms_host.hpp on either path: Backend::bilinear_terms, or -- when it declines or GSI_BILINEAR_HOST=1 -- that
// header on downloaded panels.  The arguments are validated by the caller.  Returns the path.
int64_t bilinear_terms(Context& c, int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R,
                       const double* dd, double* gram, double* t);
// The whole term of one parameter: R = [X[:, :g], Wz] (n x b, b = g + Wz's columns) formed in backend memory, Y = dop R by
// op_mul with that operator's own batching (dop null: Y = 0), then bilinear_terms with L = X.  X: n x b, Wz: n x (b - g),
// both in backend memory with ld n.  Only ddiag (n host values, or null) crosses the host link.  One rank.
int64_t op_bilinear_terms(Context& c, const Operator* dop, const double* ddiag, const double* X, int64_t n, int64_t b, int64_t g,
                          const double* Wz, double* gram, double* t);

// A sparse forward model (gsi_fwd): h(s)[r] = sum over the nonzeros t of row r of the CSR matrix H of
// vals[t] g(w[j_t] s[j_t]), g = identity (link 0) or exp (link 1).  The CSR arrays live in backend memory (integers in
// double-typed allocations) with the segment table of fwd_plan.hpp beside them, and on the host for the host path.
struct FwdModel {
  Context* ctx = nullptr;
  int64_t nobs = 0, n = 0, nnz = 0, seg_limit = 0;
  int link = 0;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> colidx;
  std::vector<double> vals, w;     // w empty: ones
  FwdPlan plan;
  Buf d_segptr, d_rowseg, d_colidx, d_vals, d_w;
  // what ran (gsi_fwd_info): form of the last product (0 none yet, 1 lane-per-output, 2 wave-per-segment, 3 host path),
  // products that took the host path, products in total
  mutable int64_t last_form = 0, host_products = 0, products = 0;
  // The adjoint H' (DESIGN.md section 4.6l): the inverted index of fwd_adjoint_plan.hpp.  Built by the first adjoint
  // product, not by fwd_create; uploaded (one allocation, d_adj; adev points into it) by the first one that asks the backend.
  mutable FwdAdjointPlan aplan;
  mutable bool aplan_built = false;
  mutable Buf d_adj;
  mutable FwdAdjoint adev;
  mutable int64_t adj_bytes = 0, adj_products = 0, adj_host_products = 0;
};
enum : int64_t { FWD_DEFAULT_SEG_LIMIT = 16384 };   // nonzeros per segment, from the sweep of DESIGN.md section 4.7b; GSI_FWD_SEG overrides
// Validates (GSI_ERR_ARG naming the offending row or entry, before anything is allocated), plans and uploads.
void fwd_create(Context& c, FwdModel& F, int64_t nobs, int64_t n, const int64_t* rowptr, const int64_t* colidx,
                const double* vals, const double* weights, int link);
// out (host, nobs x (K + 3), ld nobs): column c = h(column c of paramstorun) for the basis, s and X on the host.  The
// backend's kernels, or -- when it declines or GSI_FWD_HOST=1 -- basis_params and a host CSR loop.
void fwd_forward_basis(Context& c, const FwdModel& F, BasisRef Z, const double* s, const double* X, double delta, double* out);
// out (host, nobs x ncols, ld ldo): column c = h(P[:, c]) for the host matrix P (n x ncols, ld ldp)
void fwd_apply(Context& c, const FwdModel& F, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo);
// the same with P (n x ncols, ld ldp) and out (nobs x ncols, ld ldo) in backend memory: nothing crosses the host link on the
// backend's path; on the host path (the backend declined, or GSI_FWD_HOST=1) P is downloaded and out uploaded
void fwd_apply_dev(Context& c, const FwdModel& F, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo);
// G (n x b, ld ldg) = H' V (nobs x b, ld ldv), both in backend memory, H = diag-weighted CSR matrix of a model with link 0
// (link 1: GSI_ERR_ARG).  Every entry of G is written; sums in the order of fwd_adjoint_plan.hpp on either path:
// Backend::fwd_adjoint, or -- when it declines or GSI_FWD_HOST=1 -- download, fwd_adjoint_host.hpp, upload.
void fwd_adjoint(Context& c, const FwdModel& F, const double* V, int64_t ldv, int64_t b, double* G, int64_t ldg);

}  // namespace gsi
