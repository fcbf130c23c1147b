// backend.hpp -- the seam between the host-side algorithm (pipeline.cpp: the order of
// operations of RandMatFact.jl, row-sharded) and the code that executes each operation.
// The product library links exactly one implementation, the HIP/gfx950 one
// (hip_backend.hip).  A second implementation over the C oracle exists ONLY in the test
// tree (oracle/cpu_backend.cpp -> oracle/_build/libgsi_cpuref.so) so that the sharded
// pipeline and the C ABI can be exercised on machines without a GPU; the product loader
// never opens it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace gsi {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& msg) : std::runtime_error(msg), code(c) {}
};

enum Phase : int {
  PH_GEMM_N = 0, PH_GEMM_T = 1, PH_LU = 2, PH_QR = 3, PH_SVD = 4, PH_SMALL_GEMM = 5,
  PH_COMM = 6, PH_OTHER = 7, PH_COMM_WAIT = 8, PH_COUNT = 9
};

// One batch of products of a sparse forward model (gsi_fwd), every pointer in backend memory:
//   dst[r + c ldo] = sum over the nonzeros t of row r of vals[t] g(w[j_t] p(j_t, c)),   g = identity (link 0) or exp (link 1)
// for the columns p(:, c) of
//   plain:   the ncols = K columns of Z (fp64, ld ldz) as they are;
//   else:    the K + 3 columns of paramstorun (direct.jl:39-45), never formed: s + delta Z[:, c] (c < K; Z in fp64 or fp32,
//            widened per element), s + delta X, s + delta s, s.
// The rows are cut into segments (fwd_plan.hpp): segment k = nonzeros [segptr[k], segptr[k + 1]), row r = segments
// [rowseg[r], rowseg[r + 1]).  rowseg == null: no row is split, segment r is row r.  Otherwise `partial` (nseg x ncols)
// takes one sum per segment and the rows' sums are added from it in segment order.
struct FwdProduct {
  int64_t nobs = 0, n = 0, nnz = 0, nseg = 0, maxlen = 0;
  const int64_t* segptr = nullptr;
  const int64_t* rowseg = nullptr;
  const int32_t* colidx = nullptr;
  const double* vals = nullptr;
  const double* w = nullptr;          // n weights, or null for ones
  int link = 0;
  const void* Z = nullptr;
  int zbits = 64;                     // 64: Z is double; 32: float
  int64_t ldz = 0, K = 0;
  bool plain = false;
  const double* s = nullptr;
  const double* X = nullptr;
  double delta = 0.0;
  double* out = nullptr;              // nobs x ncols, ld ldo
  int64_t ldo = 0;
  double* partial = nullptr;          // nseg x ncols when rowseg != null
  int64_t ncols() const { return plain ? K : K + 3; }
};

// One adjoint product of that model, G (n x b, ld ldg) = H' V (nobs x b, ld ldv), every pointer in backend memory: the
// inverted index of fwd_adjoint_plan.hpp (arrays as documented there) and the operands.  Every entry of G is written; a
// cell no observation reaches gets +0.0.  partial: nchunk x b doubles for the chunk sums, or null: the backend takes a
// temporary of its own.
struct FwdAdjoint {
  int64_t n = 0, nobs = 0, nnz = 0, chunk = 0, nlong = 0, nchunk = 0;
  const int64_t* colptr = nullptr;
  const int32_t* row = nullptr;
  const double* val = nullptr;
  const int32_t* long_col = nullptr;
  const int64_t* long_chunk0 = nullptr;
  const int64_t* chunk_off = nullptr;
  const int32_t* chunk_len = nullptr;
  const double* V = nullptr;
  int64_t ldv = 0, b = 0;
  double* G = nullptr;
  int64_t ldg = 0;
  double* partial = nullptr;
};

struct FftrfPointsPlan;   // fftrf_points.hpp

// All pointers below are "backend memory" (HBM for the HIP backend), column-major fp64.
class Backend {
 public:
  virtual ~Backend() {}
  virtual const char* name() const = 0;

  // ---- memory ----
  virtual double* alloc(size_t count) = 0;  // throws Error(GSI_ERR_OOM)
  virtual void release(double* p) = 0;
  virtual int64_t bytes_in_use() const = 0;
  virtual void release_cache() {}            // return cached (released) blocks and idle workspaces to the driver
  virtual void upload2d(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols) = 0;
  virtual void download2d(double* host, int64_t ldh, const double* src, int64_t lds, int64_t rows, int64_t cols) = 0;
  virtual void copy2d(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols) = 0;
  virtual void fill_zero(double* p, size_t count) = 0;
  virtual void sync() = 0;
  // The same upload in ROW BLOCKS of upload_block_rows(rows, cols) rows, in the background: upload2d_begin returns at once
  // (a handle, or null when the backend uploaded synchronously), upload2d_wait_block makes the context's stream wait for
  // block b (rows [b * mb, (b + 1) * mb)), upload2d_end returns when the host buffer is no longer read.  What lets the
  // first pass over a dense host matrix run under its own upload (gsi_randsvd_dense_host; getxis(Q::Matrix, ...),
  // GeostatInversion.jl:63-70).  The default implementation is the synchronous upload.
  virtual int64_t upload_block_rows(int64_t rows, int64_t cols) { (void)cols; return rows; }
  virtual void* upload2d_begin(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols,
                               int64_t block_rows) {
    (void)block_rows;
    upload2d(dst, ldd, host, ldh, rows, cols);
    return nullptr;
  }
  // GB/s of one plain copy of `bytes` from / to pinned host memory on this context's device: the ceiling the staged
  // transfers are measured against (gsi_ctx_pinned_copy_rate).  0: not measurable on this backend.
  virtual void pinned_copy_rate(int64_t bytes, double* h2d_gbs, double* d2h_gbs) { (void)bytes; *h2d_gbs = 0.0; *d2h_gbs = 0.0; }
  virtual void upload2d_wait_block(void* handle, int64_t b) { (void)handle; (void)b; }
  virtual void upload2d_end(void* handle) { (void)handle; }

  // ---- products ----
  // C(m x l) = alpha * A(m x k) * B(k x l) + beta * C      beta in {0, 1}
  virtual void gemm_nn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                       const double* B, int64_t ldb, double beta, double* C, int64_t ldc) = 0;
  // rows [r0, r0 + mb) of the product C(m_full x l) = A(m_full x k) * B that gemm_nn would compute -- the same reduction
  // order per element (the K split is the one the FULL shape gets), so the blocks put together are bit-identical to the one
  // launch.  A, C: the full matrices (element (0, 0)); r0 a multiple of 128.
  virtual void gemm_nn_rowblock(int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k, const double* A, int64_t lda,
                                const double* B, int64_t ldb, double* C, int64_t ldc) {
    (void)m_full;
    gemm_nn(mb, l, k, 1.0, A + r0, lda, B, ldb, 0.0, C + r0, ldc);
  }
  // C(m x l) = alpha * A'(m x k) * B(k x l) + beta * C,  A stored k x m
  virtual void gemm_tn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                       const double* B, int64_t ldb, double beta, double* C, int64_t ldc) = 0;

  // The contraction's host launchers run directly on views the caller laid out (gsi_gemm_view, the kernel tests): form 0 =
  // gemm_nn / gemm_tn by `trans`, 1 = C (l x l) = A'A upper-triangle tiles (A k x l), 2 = C = A B with B (k x l) upper
  // triangular, 3 = rows [r0, r0 + m) of the m_full-row NN product (A, C: element (0, 0) of the full matrices).  plan8: the
  // launcher's own decisions -- nt, column chunks, xmode, wide, K splits launched, persistent, grid.x, output tiles.
  virtual void gemm_view(int form, bool trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                         const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int64_t m_full, int64_t r0,
                         int64_t* plan8) {
    (void)form; (void)trans; (void)m; (void)l; (void)k; (void)alpha; (void)A; (void)lda; (void)B; (void)ldb; (void)beta;
    (void)C; (void)ldc; (void)m_full; (void)r0; (void)plan8;
    throw Error(1 /* GSI_ERR_ARG */, "gemm_view: not available on this backend");
  }
  // every byte of p[0, count) <- `byte`
  virtual void fill_bytes(double* p, int byte, size_t count) {
    (void)p; (void)byte; (void)count;
    throw Error(1 /* GSI_ERR_ARG */, "fill_bytes: not available on this backend");
  }

  // C(m x l) = G * B(k x l) for a stationary grid covariance G(i, j) = tab[|x_i - x_j| * ny + |y_i - y_j|],
  // grid point i = (i / ny, i % ny), rows roff.., reduction indices koff..; tab = the nx * ny table of the kernel over
  // grid offsets.  G is generated, never stored (the "implicit" operator).
  virtual void gemm_nn_gridcov(int64_t m, int64_t l, int64_t k, const double* tab, int64_t nx, int64_t ny,
                               int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                               int64_t ldc) = 0;

  // C (m x l) = G * B(k x l) for the covariance of SCATTERED points, G(i, j) = sigma2 kfun(|p_i - p_j| / ell) (+ nugget if
  // i == j), rows roff.., reduction indices koff..; pts = d x npts coordinates (point i = column i) in backend memory;
  // kind / params: pointcov.hpp.  G is generated panel by panel, never stored whole (the "row-streamed" operator).
  virtual void gemm_nn_pointcov(int64_t m, int64_t l, int64_t k, const double* pts, int d, int kind, double ell,
                                double sigma2, double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb,
                                double* C, int64_t ldc) = 0;

  // Matrix-free stationary covariance on an N[0] x N[1] x N[2] grid (column-major point index) by circulant
  // embedding: A = R F^-1 diag(lambda) F R', lambda(k) = |k|^beta, unit diagonal (fft_cov.hip).  Opaque plan.
  // fftrf != 0: FFTRF.jl's own convention -- embedding of exactly 2 N[a] points, integer wavenumbers (FFTRF.jl:83-90)
  virtual void* fftcov_create(const int64_t N[3], double beta, int fftrf) = 0;
  // The same plan type for a covariance FUNCTION on the grid (gsi_op_fft_gridcov[_table] in include/gsi_hip.h):
  // A(i, j) = c(i - j) + nugget [i == j], c = sigma2 k(r) with pointcov.hpp's kinds, per-axis lengths ell[3] and the 2-D
  // rotation theta -- or, if table != null (host pointers), c(t) = table[t0 + N0 (t1 + N1 t2)] for t_a >= 0 and, for a
  // centrally symmetric 2-D kernel, table_mirror[t0 + N0 t1] = c(t0, -t1) (null: even along every axis).  Arguments are
  // validated by the caller.  Applied and destroyed like any other plan.
  virtual void* fftcov_create_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2,
                                   double nugget, const double* table, const double* table_mirror) {
    (void)N; (void)kind; (void)ell; (void)theta; (void)sigma2; (void)nugget; (void)table; (void)table_mirror;
    throw Error(1 /* GSI_ERR_ARG */, "fft covariance from a covariance function or table: not supported by this backend");
  }
  // The plan of d A / d param for the covariance function of fftcov_create_lags (gsi_op_fft_gridcov_deriv):
  // param = pointcov::D_*.  Its spectrum is not positive.  Arguments are validated by the caller.
  virtual void* fftcov_create_lags_deriv(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, int param) {
    (void)N; (void)kind; (void)ell; (void)theta; (void)sigma2; (void)param;
    throw Error(1 /* GSI_ERR_ARG */, "fft covariance derivative: not supported by this backend");
  }
  virtual void fftcov_destroy(void* plan) = 0;
  // Y (n x l, ld ldy) = A X (n x l, ld ldx)
  virtual void fftcov_apply(void* plan, int64_t l, const double* X, int64_t ldx, double* Y, int64_t ldy) = 0;

  // ---- panel factorizations, in place ----
  // Y (m x l, ld) <- L of lu(Y) in pivoted row order; ipiv (device int32[l]) may be null.
  // Sets *singular_flag (backend int, see flags()) to j+1 on an exactly zero pivot.
  virtual void lu_L(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host_or_null) = 0;
  // lu_L, with the LAPACK interchanges (0-based: row j <-> row ipiv[j] at step j) left on the device at *ipiv_dev, valid
  // until the next factorization.  false: not available, nothing ran.
  virtual bool lu_L_keep(double* Y, int64_t m, int64_t l, int64_t ld, int32_t** ipiv_dev) {
    (void)Y; (void)m; (void)l; (void)ld; (void)ipiv_dev;
    return false;
  }
  // ---- the same factorization ROW-SHARDED (SURVEY.md 8e "sharded alternative"): primitives on this rank's rows
  //      [row0, row0 + mloc) of the m x l panel, ld = leading dimension of the local block; the exchange between ranks is
  //      pipeline.cpp:lu_panel_sharded.  Blocks of `lus_block()` columns, leaves of 8; per element the arithmetic of lu_L.
  //      Record (4 + 2 l doubles): [0] max |value| (-1: none), [1] global row, [2] 1 if this rank holds row j,
  //      [4, 4+l) that row, [4+l, 4+2l) row j.
  virtual int lus_block() const = 0;
  virtual void lus_u12_leaf(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12) = 0;
  virtual void lus_pending(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w,
                           const double* U12) = 0;
  virtual void lus_candidate(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j,
                             double* rec) = 0;
  virtual void lus_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t j0, int s,
                         int w, const double* recs, int nranks) = 0;
  virtual void lus_u12_block(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                             double* U12) = 0;
  virtual void lus_rankk(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
                         const double* U12) = 0;
  virtual void lus_finish(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l) = 0;
  virtual void lus_pivots(int32_t* host, int64_t l) = 0;      // the pivot rows of the last sharded factorization
  // ---- the sharded factorization with ONE persistent launch per 8-column leaf and rank: the 8 pivot exchanges of a leaf
  //      run inside the kernels, through records every rank writes into every rank's peer-mapped buffer (no collective per
  //      pivot step).  lus_mr_begin: can this backend do it over this communicator for an m x l panel (sets up and exchanges
  //      the record buffers on first use)?  false: pipeline.cpp falls back to the per-step form above.  U12 (kp x 8) of the
  //      leaf's pending update comes from lus_u12_leaf + all-reduce as before; lus_swap_pack / _apply move the rows the
  //      leaf's pivots exchange in the columns OUTSIDE the leaf (table: 16 x l doubles, all-reduced in between).
  virtual bool lus_mr_begin(class Comm* comm, int64_t m, int64_t l) { (void)comm; (void)m; (void)l; return false; }
  // The exchange has three forms -- 0: one hop, 1: two hops, 2: two hops with lazily evaluated overflow rows -- chosen by the
  // shard height.  lus_mr_mode: the form the last successful lus_mr_begin chose; lus_mr_force (self-test): the form the next
  // ones must take (1, 2) or the natural choice again (0).
  virtual int lus_mr_mode() { return 0; }
  virtual void lus_mr_force(int mode) { (void)mode; }
  // Launch geometry of the form the last successful lus_mr_begin chose, packed into one number (block size, rows per
  // thread, grid, hops, overflow rows): it depends on rank-local facts (CUs, ranks sharing the device), and ranks with
  // different geometries would address different record slots -- pipeline.cpp lets the path run only if all ranks report
  // the same number.  lus_mr_reason: why the last lus_mr_begin said no (for the error text of GSI_LU_MR_REQUIRE).
  virtual int64_t lus_mr_signature() { return 0; }
  virtual const char* lus_mr_reason() { return ""; }
  // Bumped whenever something that lus_mr_begin's answer depends on changes on this rank (a time-out switched the path
  // off, ...): agreements the ranks reached before are void and must be reached again.  Time-outs are made global
  // (lu_flag_export / _import below), so the ranks' counters move together.
  virtual int64_t lus_mr_generation() { return 0; }
  // Before the first kernel that spins for its peers: launch every kernel the persistent-leaf factorization uses once on
  // dummies, so that no code object is loaded (a runtime call that may wait for the device) while peers spin.
  virtual void lus_mr_warmup() {}
  // The LU's asynchronous time-out flag (info = -1) made GLOBAL without a host round trip: export writes 1.0 / 0.0 into a
  // backend double, the caller all-reduces it on the stream, import raises the flag on this rank if any rank had it up.
  virtual void lu_flag_export(double* flag) { (void)flag; }
  virtual void lu_flag_import(const double* flag) { (void)flag; }
  virtual void lus_leaf_mr(double*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int, const double*) {}
  virtual bool lus_mr_swaps_done() { return false; }   // lus_leaf_mr also moved the rows in the other columns (peer pushes)
  virtual void lus_swap_pack(const double*, int64_t, int64_t, int64_t, int64_t, int64_t, int, double*) {}
  virtual void lus_swap_apply(double*, int64_t, int64_t, int64_t, int64_t, int64_t, int, const double*) {}
  // Y (m x l) <- thin Q; R (l x l, ld l) <- upper triangular factor if R != null.
  // replicated: the same panel is factored by every rank and the results must be bit-identical everywhere
  // (stacked R factors of the TSQR, gathered panels): the backend must then not let anything rank-local
  // (e.g. which algorithm tier an earlier rank-local panel needed) steer the choice of algorithm.
  virtual void qr_thinQ(double* Y, int64_t m, int64_t l, int64_t ld, double* R, bool replicated = false) = 0;
  // The thin Q of Y UP TO A RIGHT FACTOR: on success *Q1 (m x l, ld *ldq1, in backend workspace: valid until this
  // backend's next factorization call) and X2 (l x l upper triangular, caller's buffer) with Q = Q1 X2 orthonormal and
  // range(Q) = range(Y); Y is untouched.  What CholeskyQR2 has after its second Gram matrix, one tall product short of
  // Q.  A caller that only ever multiplies Q from the left (B = Q'A in randsvd) folds X2 into the l x l factor behind
  // it and never pays that product.  false: not available for this panel (the caller runs qr_thinQ).
  virtual bool qr_thinQ_deferred(const double* Y, int64_t m, int64_t l, int64_t ld, const double** Q1, int64_t* ldq1,
                                 double* X2) { (void)Y; (void)m; (void)l; (void)ld; (void)Q1; (void)ldq1; (void)X2; return false; }
  // thin SVD of a tall W (n x l, ld) in one go, W untouched: V (n x l, ldv) = left singular vectors (scaled by sqrt(S_i)
  // for i < K_scale, zero beyond, when K_scale >= 0), S (l).  A backend may decline (false): the caller then runs
  // qr_thinQ + svd_small + the l x l product itself.  The HIP backend fuses the last product of CholeskyQR2 with the
  // product by the small factor: Z = T (R2^-1 U sqrt(S)) -- one tall product instead of two.
  // Xr (may be null): an l x l right factor -- the SVD is that of W Xr (the X2 a deferred thin Q left behind).
  virtual bool svd_tall_fused(const double*, int64_t, int64_t, int64_t, int64_t, double*, int64_t, double*, const double* Xr = nullptr) {
    (void)Xr;
    return false;
  }
  // ---- randsvd's sample-space tail for a LowRankCovMatrix A = S S' c (one rank) ----
  // G (N x N, ld N) <- S'S for the samples S (n x N, ld), both triangles, in a fixed summation order.  false: not available.
  virtual bool sample_gram(const double* S, int64_t ld, int64_t n, int64_t N, double* G) {
    (void)S; (void)ld; (void)n; (void)N; (void)G;
    return false;
  }
  // Everything randsvd computes after its last panel LU L, in the coordinates of range(S): given T = S'L (N x l, ld N) and
  // G = S'S, Y = A L = S (c T) is factored by CholeskyQR2 on coefficient matrices (the Gram matrix of S M is M'(G M)), W = A'Q
  // likewise, and svd(B) comes from the l x l factors; Z (n x l, ld ldz) = S C with C = N_s x K coefficients, its last l - K
  // columns zero, and Sv (l) the singular values.  false (declines, Z and Sv untouched): a Cholesky broke down, a second
  // round's Gram matrix was not near the identity, l > N - 1 (centred samples span N - 1 dimensions), or a shape it does not
  // cover; pipeline.cpp:randsvd_lowrank_single then forms Y = S (c T) and runs the ordinary deferred-Q ending.
  // scratch (optional, scratch_doubles doubles): a dead panel of the caller's that the backend may overwrite instead of taking
  // a temporary of its own (the rows of S B0 formed beside the small SVD; contents undefined on return, whatever the verdict).
  virtual bool lowrank_tail(const double* S, int64_t lds, int64_t n, int64_t N, const double* G, const double* T, int64_t l,
                            int64_t K, double c, double* Z, int64_t ldz, double* Sv, double* scratch = nullptr,
                            size_t scratch_doubles = 0) {
    (void)S; (void)lds; (void)n; (void)N; (void)G; (void)T; (void)l; (void)K; (void)c; (void)Z; (void)ldz; (void)Sv;
    (void)scratch; (void)scratch_doubles;
    return false;
  }
  // calls of lowrank_tail that formed part of Z beside the small SVD
  virtual int64_t lowrank_tail_overlaps() { return 0; }
  // refinement rounds of lowrank_tail's two CholeskyQR2s whose triangular factor came from its series
  virtual int64_t lowrank_tail_series_rounds() { return 0; }
  // One round of the sample-space tail on a Gram matrix the caller has on the device (gsi_cq_gram_round, the kernel tests):
  // Gm (l x l) <- R in place, X (l x l) <- R^-1; check: a refinement round (the 0.1 test, and the series form where it
  // applies).  out3: the CholeskyQR flag, 1 if the series form ran, 0 if the Cholesky did; norm_out: |Gm - I|_F as the series
  // kernel measured it (0 where it did not run).
  virtual void cq_gram_round_view(double* Gm, int64_t l, double* X, bool check, int32_t* out2, double* norm_out) {
    (void)Gm; (void)l; (void)X; (void)check; (void)out2; (void)norm_out;
    throw Error(1 /* GSI_ERR_ARG */, "cq_gram_round: not available on this backend");
  }
  // One power step of the range finder in sample space.  The panel Y = c S T (T: N x l, ld N) was
  // factored by lu_L_keep into ipiv and L (n x l, ld ldl): P Y = L U, so L = (P S) C with C = c T U^-1, where
  // U = L11^-1 (P Y)[0:l] comes from the pivot rows, and
  //   T_next = S'L = G C + S[mv]' ((S[perm(mv)] - S[mv]) C)          (mv: the at most 2 l rows the interchanges move)
  // (N x l, ld N) with no n x l product.  false (declines; T_next undefined): (P S) C differs from the L in memory by more
  // than 1e-8 on the l pivot rows or a fixed sample of the others, the factorization flagged a zero pivot, or a shape it
  // does not cover; randsvd_lowrank_single then forms S'L from L, for this panel and the rest of the call.
  virtual bool lowrank_power_step(const double* S, int64_t lds, int64_t n, int64_t N, const double* G, const double* T,
                                  const int32_t* ipiv, const double* L, int64_t ldl, int64_t l, double c, double* T_next) {
    (void)S; (void)lds; (void)n; (void)N; (void)G; (void)T; (void)ipiv; (void)L; (void)ldl; (void)l; (void)c; (void)T_next;
    return false;
  }
  // The same panel factored as two column halves, split at l1: what the right half's update by the
  // left half's L would do to n x (l - l1) numbers is a change of N x (l - l1) coefficients.  The caller runs
  //   P[:, 0:l1] = S (c T1);  lu_L_keep(P, n, l1);                       lowrank_split_schur  ->  Tt
  //   P[:, l1:l] = S Tt;                                                  lowrank_split_rows
  //   lu_L_keep(P + l1 + l1 ldp, n - l1, l - l1);                         lowrank_split_join   ->  ipiv of the whole panel
  // and then lowrank_power_step on the whole panel, whose check covers both halves.
  // lowrank_split_ok: both halves would take the factorization whose pivots and top block the steps below read (false: the
  //   caller factors the panel whole; also the default, so that no other backend is asked for the rest).
  // lowrank_split_schur: ipiv1, the left half's interchanges, are kept; with [U11 | U12] = c L11^-1 S[perm(0:l1)] T from the
  //   pivot rows and C1 U11 = c T1:  Tt (N x (l - l1), ld N) <- c T2 - C1 U12, so that S Tt is the right half's Schur
  //   complement on all rows, in S's row order.
  // lowrank_split_rows: the right half's rows brought into the left half's pivoted order, its rows [0, l1) cleared.
  // lowrank_split_join: the second factorization's interchanges ipiv2 applied to rows >= l1 of the left half; *ipiv <- the l
  //   interchanges of the whole panel (valid until the next lowrank_split_schur).
  // lowrank_split_undo: the power step declined what the halves gave and the caller factors the panel again, whole: a zero
  //   pivot only a half's factorization flagged is forgotten.
  virtual bool lowrank_split_ok(int64_t n, int64_t N, int64_t l, int64_t l1) {
    (void)n; (void)N; (void)l; (void)l1;
    return false;
  }
  virtual void lowrank_split_schur(const double* S, int64_t lds, int64_t n, int64_t N, const double* T, const int32_t* ipiv1,
                                   const double* P, int64_t ldp, int64_t l, int64_t l1, double c, double* Tt) {
    (void)S; (void)lds; (void)n; (void)N; (void)T; (void)ipiv1; (void)P; (void)ldp; (void)l; (void)l1; (void)c; (void)Tt;
    throw Error(1 /* GSI_ERR_ARG */, "lowrank_split_schur: not available on this backend");
  }
  virtual void lowrank_split_rows(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1) {
    (void)P; (void)ldp; (void)n; (void)l; (void)l1;
    throw Error(1 /* GSI_ERR_ARG */, "lowrank_split_rows: not available on this backend");
  }
  virtual void lowrank_split_join(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1, const int32_t* ipiv2,
                                  int32_t** ipiv) {
    (void)P; (void)ldp; (void)n; (void)l; (void)l1; (void)ipiv2; (void)ipiv;
    throw Error(1 /* GSI_ERR_ARG */, "lowrank_split_join: not available on this backend");
  }
  virtual void lowrank_split_undo() {}
  // G (l x l, ld l), columns orthogonalised in place by one-sided Jacobi; on return
  // U (l x l) = left singular vectors sorted by descending S, S (l) singular values.
  virtual void svd_small(double* G, int64_t l, double* U, double* S) = 0;
  // upper Cholesky factor of the symmetric j x j B (upper triangle read), in place
  virtual void chol_upper(double* B, int64_t j) = 0;
  // F (m x j) <- F * inv(C), C upper triangular j x j
  virtual void trsm_right_upper(double* F, int64_t m, int64_t j, int64_t ldf, const double* C) = 0;

  // ---- small fused helpers ----
  // U (l x l) <- U * diag(sqrt(S_i) for i < K, 0 otherwise)
  virtual void scale_cols_sqrt(double* U, int64_t l, const double* S, int64_t K) = 0;
  // rows of S (n x N, ld): subtract the mean over the N columns (lowrank.jl:17-27)
  virtual void center_rows(double* S, int64_t n, int64_t N, int64_t ld) = 0;
  virtual void randn(double* p, size_t count, uint64_t seed) = 0;
  // synthetic covariance rows [row0,row0+mloc) of an (nx*ny)^2 grid covariance
  virtual void fill_gridcov(double* A, int64_t lda, int64_t nx, int64_t ny, double ell, int kind,
                            int64_t row0, int64_t mloc) = 0;
  // synthetic sample fields (benchmark / test input): S(i, j) = g(row0 + i, j) (j+1)^-decay, g iid N(0,1) addressed
  // by the global index (identical for every rank layout)
  virtual void fill_lowrank_samples(double* S, int64_t ld, int64_t nloc, int64_t N, int64_t row0, uint64_t seed,
                                    double decay) = 0;
  // FFTRF.powerlaw_structuredgrid(N, k0, dk, beta) (FFTRF.jl:83-100) for fields field0 .. field0 + nf - 1, sampled on the
  // device (fftrf_sample.hip): rows [row0, row0 + nloc) of field c go to dst[(r - row0) + c ldd].  phi (HOST, or null): column
  // c = vec() of mulbyphi's randn(size(S)) for field c, leading dimension ldphi; null: field f draws randn(..., seed + f).
  // Arguments are validated by the caller.
  virtual void fftrf_fields(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N,
                            double k0, double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed,
                            int64_t field0) {
    (void)dst; (void)ldd; (void)row0; (void)nloc; (void)nf; (void)ndims; (void)N; (void)k0; (void)dk; (void)beta; (void)phi;
    (void)ldphi; (void)seed; (void)field0;
    throw Error(1 /* GSI_ERR_ARG */, "FFTRF fields sampled on the device: not available on this backend");
  }
  // FFTRF.interpolate (FFTRF.jl:107-129) on the device (fftrf_interp.hip): the nf structured fields grid[:, c] (vec() order,
  // leading dimension ldg) at the plan's points, dst[p + c ldd] for p < plan.m_local.  The plan comes from fftrf_points.hpp.
  virtual void fftrf_interpolate(double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg,
                                 const FftrfPointsPlan& plan) {
    (void)dst; (void)ldd; (void)nf; (void)grid; (void)ldg; (void)plan;
    throw Error(1 /* GSI_ERR_ARG */, "FFTRF interpolation on the device: not available on this backend");
  }
  // A points plan RESIDENT in backend memory, for operators that apply the interpolation matrix W (m_local x n) of the plan
  // and its adjoint many times (OP_FFT_COV_AT): base and frac of fftrf_points.hpp and the inverted index of
  // interp_adjoint_plan.hpp are uploaded once.  Opaque handle; info[4] (may be null) = resident bytes, long nodes, chunks of
  // the long nodes, contributions of the longest node list.
  virtual void* points_at_create(const FftrfPointsPlan& plan, int64_t info[4]) {
    (void)plan; (void)info;
    throw Error(1 /* GSI_ERR_ARG */, "interpolation plans resident on the device: not available on this backend");
  }
  virtual void points_at_destroy(void* at) { (void)at; }
  // dst (m_local x nf, ld ldd) = W grid (n x nf, ld ldg): fftrf_interpolate without the upload
  virtual void points_at_gather(void* at, double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg) {
    (void)at; (void)dst; (void)ldd; (void)nf; (void)grid; (void)ldg;
    throw Error(1 /* GSI_ERR_ARG */, "interpolation plans resident on the device: not available on this backend");
  }
  // grid (n x nf, ld ldg) = W' src (m_local x nf, ld lds), interp_adjoint.hip: every entry of grid is written (a node no
  // point reaches gets 0.0); no atomics, bit-identical from call to call and whatever nf is
  virtual void points_at_spread(void* at, double* grid, int64_t ldg, int64_t nf, const double* src, int64_t lds) {
    (void)at; (void)grid; (void)ldg; (void)nf; (void)src; (void)lds;
    throw Error(1 /* GSI_ERR_ARG */, "interpolation plans resident on the device: not available on this backend");
  }
  // FFTRF.powerlaw_unstructuredgrid (FFTRF.jl:102-105): fftrf_fields whose every field is interpolated at the plan's points
  // while it is still in the batch workspace; the n x nf structured matrix is never formed.
  virtual void fftrf_fields_at(double* dst, int64_t ldd, int64_t nf, int ndims, const int64_t* N, double k0, double dk,
                               double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0,
                               const FftrfPointsPlan& plan) {
    (void)dst; (void)ldd; (void)nf; (void)ndims; (void)N; (void)k0; (void)dk; (void)beta; (void)phi; (void)ldphi; (void)seed;
    (void)field0; (void)plan;
    throw Error(1 /* GSI_ERR_ARG */, "FFTRF fields at scattered points on the device: not available on this backend");
  }
  // Gaussian fields with a grid covariance FUNCTION by circulant embedding (gsi_gridcov_sampler_* in include/gsi_hip.h,
  // gridcov_sample.hip): the plan of the grid N (ndims axes, the others 1) on the torus M -- the spectrum lambda of the torus
  // covariance sigma2 k(r) (+ nugget) and its clamped square root.  info[4] = neg_mass, lambda_min, lambda_max, clamped
  // count, filled whenever the spectrum was computed; neg_mass > neg_tol throws GSI_ERR_NOT_POSDEF and leaves nothing
  // allocated.  Arguments are validated by the caller.  Opaque plan.
  virtual void* gridcov_sampler_create(int ndims, const int64_t N[3], const int64_t M[3], int kind, const double ell[3],
                                       double theta, double sigma2, double nugget, double neg_tol, double info[4]) {
    (void)ndims; (void)N; (void)M; (void)kind; (void)ell; (void)theta; (void)sigma2; (void)nugget; (void)neg_tol; (void)info;
    throw Error(1 /* GSI_ERR_ARG */, "grid covariance fields sampled on the device: not supported by this backend");
  }
  virtual void gridcov_sampler_destroy(void* plan) { (void)plan; }
  // lambda (Mtot values, torus order, unclamped, nugget included) -> HOST array
  virtual void gridcov_sampler_spectrum(void* plan, double* lam_host) {
    (void)plan; (void)lam_host;
    throw Error(1 /* GSI_ERR_ARG */, "grid covariance fields sampled on the device: not supported by this backend");
  }
  // Fields field0 .. field0 + nf - 1 of the plan (field0 even; fields 2 j and 2 j + 1 are Re and Im of one transform): rows
  // [row0, row0 + nloc) of field c go to dst[(r - row0) + c ldd].  eps (HOST, or null): column c = the noise array of role
  // c (Mtot values, even c: real part, odd c: imaginary part), 2 ceil(nf / 2) columns, leading dimension ldeps; null: role
  // f draws randn(..., seed + f).
  virtual void gridcov_sampler_fields(void* plan, double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf,
                                      const double* eps, int64_t ldeps, uint64_t seed, int64_t field0) {
    (void)plan; (void)dst; (void)ldd; (void)row0; (void)nloc; (void)nf; (void)eps; (void)ldeps; (void)seed; (void)field0;
    throw Error(1 /* GSI_ERR_ARG */, "grid covariance fields sampled on the device: not supported by this backend");
  }
  // column norms of Y (m x c) -> host array
  virtual void colnorms(const double* Y, int64_t m, int64_t c, int64_t ld, double* host_out) = 0;
  virtual void axpy(int64_t n, double a, const double* x, double* y) = 0;
  virtual double dot(int64_t n, const double* x, const double* y) = 0;
  virtual double nrm2(int64_t n, const double* x) = 0;
  virtual void scal_copy(int64_t n, double a, const double* x, double* y) = 0;  // y = a*x
  // out (n x (K+3)) = [s + delta*Z[:,i] (i<K), s + delta*X, s + delta*s, s]   direct.jl:39-45
  virtual void pcga_params(const double* Z, int64_t n, int64_t K, const double* s, const double* X, double delta,
                           double* out) = 0;

  // BLAS-2 (adaptive range finder, saddle-point products): y (m) = alpha A x + beta y; y (k) = alpha A' x (A m x k);
  // Y[:, c] -= dot(q, Y[:, c]) q for c < ncols <= 64  (RandMatFact.jl:42-45) -- no scalar leaves the backend
  virtual void gemv_n(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double beta,
                      double* y) = 0;
  virtual void gemv_t(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double* y) = 0;
  virtual void project_out(int64_t m, int64_t ncols, const double* q, double* Y, int64_t ld) = 0;
  virtual void scal(int64_t n, double a, double* x) = 0;                          // x *= a
  virtual void diag_mul_add(int64_t n, const double* d, const double* x, double* y) = 0;   // y += d .* x

  // ---- IterativeSolvers.lsqr with the scalar recurrences resident in backend memory (lsqr_state.hpp): `work` holds
  //      lsqr_work_doubles() doubles = [state | partial sums]; solvers.cpp:lsqr sequences the two operator products
  //      around these and polls the state every few iterations ----
  virtual size_t lsqr_work_doubles() = 0;
  virtual void lsqr_begin(int64_t n, const double* w, double* work) = 0;                       // |w|^2 of the initial w
  virtual void lsqr_step_u(int64_t m, const double* t, double* u, double* work) = 0;           // u = t - alpha u; beta; u /= beta
  virtual void lsqr_step_v(int64_t n, const double* t, double* v, double* w, double* x, double* work) = 0;
  //                                     v = t - beta v; alpha; the recurrences and stopping rules; v /= alpha; x += t1 w; w = v + t2 w

  // ---- conjugate gradients on (A + diag(d)) X = B, all b columns together, with the per-column recurrences resident in
  //      backend memory (cg_state.hpp): `work` holds block_cg_work_doubles(b) doubles = [state |
  //      partial sums]; solvers.cpp:block_cg sequences the operator product Q = A P around these and polls the state's
  //      header every few iterations.  Panels n x b, ld n; d (n, may be null) >= 0.
  //      block_cg_work_doubles: 0 = "not mine" (the default), and solvers.cpp runs the same recurrences column by column
  //      with op_mul, diag_mul_add, dot, axpy and scal.
  virtual size_t block_cg_work_doubles(int64_t b) { (void)b; return 0; }
  // R and P hold B, X is zero: the columns' norms and the state of a fresh solve
  virtual void block_cg_begin(int64_t n, int64_t b, const double* B, double tol, int64_t maxiter, double* work) {
    (void)n; (void)b; (void)B; (void)tol; (void)maxiter; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "block_cg: not available on this backend");
  }
  // after Q = A P: alpha; x += alpha p, r -= alpha (q + d .* p); beta and the stopping rule; p = r + beta p
  virtual void block_cg_step(int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R, double* P,
                             double* work) {
    (void)n; (void)b; (void)Q; (void)d; (void)X; (void)R; (void)P; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "block_cg: not available on this backend");
  }

  // ---- the same solver preconditioned by P = Z Z' + diag(d + shift): P^-1 = diag(e) - W W' with
  //      e (n) and W (n x K, ld n) in backend memory.  `work` holds block_pcg_work_doubles(b) doubles = [state | three sets
  //      of partial sums]; S (K x b, ld K) and Y (n x b, ld n) are the caller's.  0 = "not mine" (the default):
  //      solvers.cpp runs the preconditioned form of block_cg_host.hpp.
  virtual size_t block_pcg_work_doubles(int64_t b) { (void)b; return 0; }
  // R holds B, X is zero: P <- z0 = P^-1 B, the columns' b'b and b'z0, the state of a fresh solve
  virtual void block_pcg_begin(int64_t n, int64_t b, int64_t K, const double* B, const double* e, const double* W, double* S,
                               double* Y, double* P, double tol, int64_t maxiter, double* work) {
    (void)n; (void)b; (void)K; (void)B; (void)e; (void)W; (void)S; (void)Y; (void)P; (void)tol; (void)maxiter; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "block_pcg: not available on this backend");
  }
  // after Q = A P: alpha; x += alpha p, r -= alpha (q + d .* p); the stopping rule; z = e .* r - W (W'r); beta; p = z + beta p
  virtual void block_pcg_step(int64_t n, int64_t b, int64_t K, const double* Q, const double* d, const double* e,
                              const double* W, double* X, double* R, double* P, double* S, double* Y, double* work) {
    (void)n; (void)b; (void)K; (void)Q; (void)d; (void)e; (void)W; (void)X; (void)R; (void)P; (void)S; (void)Y; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "block_pcg: not available on this backend");
  }
  // the preconditioner's setup: e (n, holding d + shift) <- 1 / e and sqe (n) <- sqrt of that; C (K x K, ld K) += I.
  // 1, or 0: "not mine" (the caller does both on the host).
  virtual int precond_rows(int64_t n, double* e, double* sqe) { (void)n; (void)e; (void)sqe; return 0; }
  virtual int add_identity(double* C, int64_t K) { (void)C; (void)K; return 0; }

  // ---- the coefficient trace of the two solvers above and its Gauss quadrature (cg_state.hpp's trace_col, slq_state.hpp;
  //      DESIGN.md section 4.6k).  work: the solver's `work` (its state block in front); tr: cgst::trace_doubles(b, qmax)
  //      doubles in backend memory.  Called behind block_cg_begin / block_pcg_begin and behind every block_cg_step /
  //      block_pcg_step of a traced solve.  A backend with the fused solvers has these; the default is never reached.
  virtual void cg_trace_begin(const double* work, double* tr, int64_t qmax) {
    (void)work; (void)tr; (void)qmax;
    throw Error(1 /* GSI_ERR_ARG */, "cg_trace: not available on this backend");
  }
  virtual void cg_trace_step(const double* work, double* tr, int64_t qmax) {
    (void)work; (void)tr; (void)qmax;
    throw Error(1 /* GSI_ERR_ARG */, "cg_trace: not available on this backend");
  }
  // out[j] = rho0[j] * e1' log(T_j) e1 from steps[j] (a whole number in a double) coefficients of column j; alpha, beta
  // (qmax x b, step k of column j at k * b + j), steps, rho0, out (b) and work (3 * qmax * b) in backend memory.
  // 1, or 0: "not mine" (the caller runs slq_state.hpp on the host).
  virtual int slq_quadrature(const double* alpha, const double* beta, const double* steps, const double* rho0, int64_t qmax,
                             int64_t b, double* work, double* out) {
    (void)alpha; (void)beta; (void)steps; (void)rho0; (void)qmax; (void)b; (void)work; (void)out;
    return 0;
  }
  // Zout = Y ./ e + G2 ./ sqrt(e) on n x b panels (ld n).  1, or 0: "not mine" (the caller forms it on the host).
  virtual int precond_sample_rows(int64_t n, int64_t b, const double* e, const double* Y, const double* G2, double* Zout) {
    (void)n; (void)b; (void)e; (void)Y; (void)G2; (void)Zout;
    return 0;
  }

  // ---- diagonal-pivoted Cholesky of a covariance read by entries (pchol_state.hpp).  Where
  //      A(i, p) comes from: form 1 -- data = the stored n x n matrix (ld); 2 -- data = the gx * gy table over grid offsets;
  //      3 -- data = the d x n coordinates of a scattered-point covariance with the parameters below.
  struct PcholSource {
    int form = 0;
    const double* data = nullptr;
    int64_t ld = 0, gx = 0, gy = 0;
    int pc_d = 0, pc_kind = 0;
    double pc_ell = 1.0, pc_sigma2 = 1.0, pc_nugget = 0.0;
  };
  // `work` holds pchol_work_doubles doubles and starts with the state block (pchol::state_doubles(K)); d: n doubles;
  // L: n x >= K, ld ldl, its first K columns cleared by the caller.  0 = "not mine" (the default): solvers.cpp runs
  // pivoted_chol_host.hpp.
  virtual size_t pchol_work_doubles(const PcholSource& a, int64_t n, int64_t K) { (void)a; (void)n; (void)K; return 0; }
  // d <- diag(A), the state of a fresh factorization, the first decision
  virtual void pchol_begin(const PcholSource& a, int64_t n, int64_t K, double tol, const double* L, int64_t ldl, double* d,
                           double* work) {
    (void)a; (void)n; (void)K; (void)tol; (void)L; (void)ldl; (void)d; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "pivoted_cholesky: not available on this backend");
  }
  // one step and the decision behind it, enqueued; a no-op once the state block says stop
  virtual void pchol_step(const PcholSource& a, int64_t n, int64_t K, double* L, int64_t ldl, double* d, double* work) {
    (void)a; (void)n; (void)K; (void)L; (void)ldl; (void)d; (void)work;
    throw Error(1 /* GSI_ERR_ARG */, "pivoted_cholesky: not available on this backend");
  }
  // U (n x K, ld ldu): column k *= S[k], S in backend memory.  1, or 0: "not mine" (the caller scales on the host).
  virtual int scale_cols(int64_t n, int64_t K, double* U, int64_t ldu, const double* S) {
    (void)n; (void)K; (void)U; (void)ldu; (void)S; return 0;
  }

  // ---- fp32-STORED xi-basis (BASELINE configs[4], "fp32 mixed precision"): the n x K basis is the one big HBM stream
  //      of the PCGA iteration's own algebra; stored in fp32 it is half the bytes, every sum stays in fp64 ----
  virtual void f64_to_f32(const double* src, void* dst32, size_t count) = 0;
  // as pcga_params with Z given in fp32 (n x K, ld n); out is fp64
  virtual void pcga_params_f32(const void* Z32, int64_t n, int64_t K, const double* s, const double* X, double delta,
                               double* out) = 0;
  // y (n) = beta * X + Z32 (n x K, fp32) * w (K): fp64 accumulation   (direct.jl:59-65 with the basis in fp32)
  virtual void basis_gemv_f32(const void* Z32, int64_t n, int64_t K, const double* w, double beta, const double* X,
                              double* y) = 0;

  // ---- sparse forward model on the device (FwdProduct above) ----
  // Returns the form that computed a.out -- 1: one lane per output, 2: one wave per segment -- or 0: "not mine", nothing
  // ran, and pcga.cpp forms the batch with pcga_params and multiplies on the host.
  virtual int fwd_products(const FwdProduct& a) { (void)a; return 0; }
  // The adjoint product (FwdAdjoint above; fwd_adjoint.hip).  Returns 1 when it computed a.G, or 0: "not mine", nothing
  // ran, and pcga.cpp downloads V and sums on the host in the plan's order (fwd_adjoint_host.hpp).
  virtual int fwd_adjoint(const FwdAdjoint& a) { (void)a; return 0; }

  // ---- pcgadirect's saddle-point system by Cholesky ----
  // The m x n trapezoid A (m >= n, ld; lower triangle of the top n x n read) <- [L; (L^-1 B')'] in place, B = rows n .. m-1.
  // Returns 0, the 1-based column at which the matrix stopped being positive definite (A is then partly factored), or
  // -1: "not mine", nothing ran, and pcga.cpp factors on the host (saddle_host.hpp).
  virtual int64_t chol_lower(double* A, int64_t m, int64_t n, int64_t ld) { (void)A; (void)m; (void)n; (void)ld; return -1; }
  // x (nobs + 1) = [(E E' + R) HX; HX' 0] \ b with E nobs x K (ld nobs), R dense (ld nobs) or its diagonal: formation,
  // chol_lower with HX' and b1' carried as rows nobs, nobs + 1, beta = (w'v - b2) / (w'w), xi = L^-T (v - beta w).
  // Returns as chol_lower does; *singular <- w'w is zero or beta is not finite (x is then not meaningful).
  virtual int64_t saddle_solve(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag,
                               const double* b, double* x, bool* singular) {
    (void)E; (void)nobs; (void)K; (void)HX; (void)R; (void)r_diag; (void)b; (void)x; (void)singular;
    return -1;
  }

  // ---- the posterior variance from the resident basis ----
  // One pass over the rows z_i of the basis Z (n x K, ld ldz; zbits 64: double, 32: float widened per element), every sum in
  // fp64:  a[i] = |W' z_i|^2 for W (K x ncols, ld ldw; upper: W[k, j] with k > j is zero and never read),
  // q[i] = |z_i|^2 (q may be null), t[i] = u' z_i (u and t null together).  Z W is never formed.
  // Returns 1, or 0: "not mine", nothing ran, and pcga.cpp runs posterior_host.hpp on a downloaded basis.
  virtual int basis_quadform(const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw,
                             int64_t ncols, bool upper, const double* u, double* a, double* q, double* t) {
    (void)Z; (void)zbits; (void)n; (void)ldz; (void)K; (void)W; (void)ldw; (void)ncols; (void)upper; (void)u; (void)a; (void)q;
    (void)t;
    return 0;
  }
  // dst (m x c, ld ldd) = diag(d) src (m x c, ld lds): the rows of E and HX scaled by 1 / sqrt(R_jj).  1, or 0: "not mine".
  virtual int scale_rows(int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst, int64_t ldd) {
    (void)m; (void)c; (void)d; (void)src; (void)lds; (void)dst; (void)ldd;
    return 0;
  }

  // ---- the exact posterior variance of linear inversion and kriging ----
  // The row pass: acc[i] += sum over c < b of A[i, c] B[i, c] for column-major n x b panels (ld lda, ldb), every product
  // rounded on its own and added to the row's sum, which starts from acc[i], in ascending c.  B == A: the sum of squares.
  // 1, or 0: "not mine", nothing ran, and the caller runs posterior_exact_host.hpp on downloaded panels.
  virtual int rowdot_acc(int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc) {
    (void)n; (void)b; (void)A; (void)lda; (void)B; (void)ldb; (void)acc;
    return 0;
  }
  // E (nobs x b, ld) <- zeros with a one at (c0 + c, c).  1, or 0: "not mine".
  virtual int unit_panel(double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) {
    (void)E; (void)ld; (void)nobs; (void)b; (void)c0;
    return 0;
  }
  // The assembly of the (2 nobs + p) x nobs trapezoid T (ld) whose top block holds H C H': diag (nobs values, or null) is
  // added to the diagonal, rows [nobs, nobs + p) <- Phi' (Phi: nobs x p, ld ldphi), rows [nobs + p, 2 nobs + p) <- I.
  // 1, or 0: "not mine".
  virtual int trapezoid_rows(double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi,
                             int64_t ldphi) {
    (void)T; (void)ld; (void)nobs; (void)p; (void)diag; (void)Phi; (void)ldphi;
    return 0;
  }
  // After chol_lower: Wd (nobs x p, ld nobs) <- the transpose of rows [nobs, nobs + p) of T, W_d = L^-1 Phi.
  // 1, or 0: "not mine".
  virtual int carried_rows(const double* T, int64_t ld, int64_t nobs, int64_t p, double* Wd) {
    (void)T; (void)ld; (void)nobs; (void)p; (void)Wd;
    return 0;
  }

  // ---- the bilinear forms of the likelihood gradient ----
  // L, Y, R: n x b panels in backend memory (ld n); dd: n values in backend memory, or null (then R is not read); with
  // V = Y + dd .* R: gram (g x g, HOST) [a + g c] = sum_i L[i, a] V[i, c], t (b - g, HOST) [j - g] = sum_i L[i, j] V[i, j], in
  // the order of bilinear_terms_host.hpp.  1, or 0: "not mine", nothing ran, and the caller runs that header on downloaded panels.
  virtual int bilinear_terms(int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R, const double* dd,
                             double* gram, double* t) {
    (void)n; (void)b; (void)g; (void)L; (void)Y; (void)R; (void)dd; (void)gram; (void)t;
    return 0;
  }

  // error flags raised asynchronously by kernels (zero pivot, non-posdef); checked and
  // cleared by the pipeline at the end of each entry point. Returns GSI_* code or 0.
  virtual int take_error(std::string* msg) = 0;
  // true (once) if the last error was a lost resource rather than a property of the input, and the backend has switched
  // to a path that does not need it: the caller may run the same entry point again on its intact inputs
  virtual bool retryable_failure() { return false; }
  virtual void forgive_lost_coresidency() {}     // undo what a time-out inside a self-test switched off

  // ---- profiling ----
  virtual void profile(bool on) = 0;
  virtual void phase_begin(Phase p) = 0;
  virtual void phase_end(Phase p) = 0;
  // phase_end for an interval that belongs to an entry the phase has already counted (the second product and the second
  // factorization of a panel that is factored in two halves): its time is added, the phase's count stays.  bench.py divides a
  // phase's time by its count, so one panel must stay one entry.
  virtual void phase_end_more(Phase p) { phase_end(p); }
  virtual void phase_reset() = 0;
  virtual void phase_times(double* ms, int64_t* counts) = 0;
  // [0] CholeskyQR2 factorizations, [1] Householder factorizations (incl. fallbacks), [2] Jacobi sweeps of
  // the last small SVD, [3] shifted CholeskyQR3 factorizations
  virtual void counters(int64_t* out4) { out4[0] = out4[1] = out4[2] = out4[3] = 0; }
  // [0] LU pivot-exchange time-outs seen by this backend since creation (take_error mapped info = -1)
  virtual int64_t lu_timeouts() { return 0; }
  // small SVDs that used up their sweep budget with rotatable column pairs left (the result is still the best available)
  virtual int64_t svd_cap_hits() { return 0; }
  // how many ranks of the context's communicator run on this backend's device (Comm::ranks_on_my_device, told once the
  // communicator exists): kernels that need all their workgroups resident at once must not assume the whole chip
  virtual void set_ranks_sharing_device(int n) { (void)n; }
};

class Comm {
 public:
  int rank = 0, nranks = 1;
  int64_t ncollectives = 0;       // collectives entered since creation (gsi_ctx_path_info reports the count per timed region)
  virtual ~Comm() {}
  // The four collectives.  Callers use these; implementations override the do_* hooks below.
  void allreduce_sum(double* buf, size_t count) { ++ncollectives; do_allreduce_sum(buf, count); }
  // every rank contributes `count` doubles; recv holds nranks*count, rank-major
  void allgather(const double* send, double* recv, size_t count) { ++ncollectives; do_allgather(send, recv, count); }
  // send holds nranks blocks of `count` doubles (block g is destined for rank g); recv (count) = sum over ranks
  // of their block `rank`
  void reduce_scatter_sum(const double* send, double* recv, size_t count) { ++ncollectives; do_reduce_scatter_sum(send, recv, count); }
  // send holds nranks blocks of `count` doubles, block g for rank g; recv block s = what rank s sent to this rank
  void alltoall(const double* send, double* recv, size_t count) { ++ncollectives; do_alltoall(send, recv, count); }
  // every rank hands in a device buffer; all[g] = rank g's buffer as THIS rank can address it (same process: the pointer
  // itself; other processes: an IPC mapping).  false: not supported by this communicator.  Collective.
  virtual bool share_pointers(void* mine, size_t bytes, void** all) { (void)mine; (void)bytes; (void)all; return false; }
  // ranks of this communicator that run on the SAME device as this one (itself included).  1 with RCCL (it refuses two ranks
  // on one device); the RCCL-free communicators allow any placement, and kernels that need all their workgroups resident
  // at once (the persistent LU leaves) must share the chip between that many launches.
  virtual int ranks_on_my_device() { return 1; }
  // Ranks that are THREADS of one process share one HIP runtime: a call that waits for the device (hipFree does, and a
  // hipMalloc that has to map new memory was seen to) waits for the other ranks' kernels too.  Before a rank launches a
  // kernel that spins for its peers, all ranks meet here with their allocations done.  No-op for ranks in processes.
  virtual void host_barrier() {}

 protected:
  virtual void do_allreduce_sum(double* buf, size_t count) = 0;
  virtual void do_allgather(const double* send, double* recv, size_t count) = 0;
  virtual void do_reduce_scatter_sum(const double* send, double* recv, size_t count) = 0;
  virtual void do_alltoall(const double* send, double* recv, size_t count) = 0;
};

// Provided by whichever backend is linked into the library.
Backend* make_backend(int device_id);
Comm* make_comm(Backend* be, int nranks, int rank, const void* unique_id);
void comm_unique_id(void* id_out);
const char* backend_name();

struct ScopedPhase {
  Backend* be; Phase p;
  ScopedPhase(Backend* b, Phase ph) : be(b), p(ph) { be->phase_begin(p); }
  ~ScopedPhase() { be->phase_end(p); }
};
struct ScopedPhaseMore {       // more time for the entry a ScopedPhase of the same phase counted (Backend::phase_end_more)
  Backend* be; Phase p;
  ScopedPhaseMore(Backend* b, Phase ph) : be(b), p(ph) { be->phase_begin(p); }
  ~ScopedPhaseMore() { be->phase_end_more(p); }
};

}  // namespace gsi
