// hip_backend_impl.hpp -- the declaration of HipBackend, the gfx950 implementation of gsi::Backend, for the hip_backend*.hip files
// alone (the communicators see hip_backend.hpp).  What each operation computes is documented at Backend (backend.hpp); the
// bodies are split by subsystem:
//   hip_backend.hip           construction, the block cache and the workspaces, the host boundary, streams, errors, profiling
//   hip_backend_products.hip  contractions, generated operators, the FFT covariance plans, FFTRF fields
//   hip_backend_sampler.hip   fields with a grid covariance function by circulant embedding: plan and batches
//   hip_backend_panels.hip    panel LU (one rank and row-sharded), the QR tiers, the fused tall SVD, the small factorizations
//   hip_backend_lowrank.hip   the LowRankCovMatrix chains in sample space
//   hip_backend_pcga.hip      BLAS-1/2, LSQR, block CG and the PCGA consumers
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>
#include "hip_backend.hpp"
#include "hip_common.hpp"
#include "host_staging.hpp"
#include "fftrf_points.hpp"

namespace gsi {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool pooled = false;      // a panel-sized workspace taken from (and returned to) the block cache instead of hipMalloc / hipFree
};

// The layout of several buffers inside one allocation: take(count) is the offset of the next buffer, and the one after it
// starts count rounded up to 8 further on (64 bytes, in doubles).  The unit is the caller's: doubles, or bytes where a
// workspace holds integers.  packed(count): the next buffer follows directly (arrays that one copy reads together; the last
// buffer of an allocation whose size shows in bytes_in_use()).  total: what to allocate.
struct Carve {
  size_t total = 0;
  static constexpr size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }
  size_t take(size_t count) { const size_t o = total; total += up8(count); return o; }
  size_t packed(size_t count) { const size_t o = total; total += count; return o; }
};

class __attribute__((visibility("hidden"))) HipBackend final : public HipDevice {
  // A pooled temporary that goes back to the block cache on every exit path (a throwing HIP_CHECK between alloc
  // and release leaked pooled blocks).  release() is ordered on the stream: WHERE a Scratch ends is part of what a function does.
  // try_alloc: null instead of an exception, where memory is no reason to fail.
  struct Scratch {
    HipBackend* be; double* p;
    explicit Scratch(HipBackend* b, size_t doubles = 0) : be(b), p(doubles ? b->alloc(doubles) : nullptr) {}
    ~Scratch() { if (p) be->release(p); }
    double* try_alloc(size_t doubles) { try { return p = be->alloc(doubles); } catch (const Error&) { return p = nullptr; } }
    void adopt(double* q) { p = q; }
    double* give_up() { double* q = p; p = nullptr; return q; }
    Scratch(const Scratch&) = delete; Scratch& operator=(const Scratch&) = delete;
  };
  struct TrimGuard { HipBackend* be; DevBuf* b; ~TrimGuard() { be->trim(*b); } };
  // Joins the side stream into st_ on every way out of the scope that forked it.  join(): the ordinary way (st_ waits for what
  // the side stream was given; the host does not).  Left to the destructor -- an exception is in flight -- the host waits too.
  struct SideJoin {
    HipBackend* be; bool open = false;
    explicit SideJoin(HipBackend* b) : be(b) {}
    void fork() {
      hipStream_t s2 = be->side_stream();
      HIP_CHECK(hipEventRecord(be->ev_fork_, be->st_));
      HIP_CHECK(hipStreamWaitEvent(s2, be->ev_fork_, 0));
      open = true;
    }
    void join() {
      if (!open) return;
      open = false;
      HIP_CHECK(hipEventRecord(be->ev_join_, be->st2_));
      HIP_CHECK(hipStreamWaitEvent(be->st_, be->ev_join_, 0));
    }
    ~SideJoin() {
      if (!open) return;
      if (hipEventRecord(be->ev_join_, be->st2_) == hipSuccess) (void)hipStreamWaitEvent(be->st_, be->ev_join_, 0);
      (void)hipStreamSynchronize(be->st2_);
    }
    SideJoin(const SideJoin&) = delete;
    SideJoin& operator=(const SideJoin&) = delete;
  };
  enum FlagSlot {                // the slots of flags_; the first FLAG_ERROR_WORDS are what take_error reads and clears
    FLAG_LU_INFO = 0,            // lu: 0, the column of an exactly zero pivot, or < 0 when the pivot exchange timed out
    FLAG_CHOL_INFO = 1,          // chol_upper: 0 or the column at which the matrix stopped being positive definite
    FLAG_WAIT_PHASE = 2, FLAG_WAIT_SLOT = 3, FLAG_WAIT_EPOCH = 4, FLAG_WAIT_WHO = 5,   // what a timed-out LU workgroup waited for
    FLAG_ERROR_WORDS = 8, FLAG_SVD_ROTATIONS = 8,     // (behind the error words:) the Jacobi SVD's rotation counter
    FLAG_CHOLQR = 9,             // the verdict of a CholeskyQR attempt: non-zero = this tier does not apply (read_flag)
    FLAG_CHOL_LOWER = 10,        // chol_lower / saddle_solve: 0 or the 1-based column of the first bad pivot (read_flag)
    FLAG_CQ_SERIES = 12,         // four words of cq_gram_round's series form: rounds taken, taken this time, |Gram - I|_F (a double)
    FLAG_COUNT = 16
  };
  struct GemmWs { double* p; size_t doubles; };      // the contractions' split-K workspace and how many doubles it holds
  struct Rec { Phase phase; hipEvent_t a, b; bool counted; };
  struct FftCov;                 // hip_backend_products.hip
  struct PointsAt;               // hip_backend_products.hip
  struct GridCovSampler;         // hip_backend_sampler.hip
  struct LusWs;                  // hip_backend_panels.hip
  struct SplitWs;                // hip_backend_lowrank.hip
  enum FftFactor { FFT_F_COS = 0, FFT_F_COS_WEIGHTED = 1, FFT_F_SIN_WEIGHTED = 2 };

 public:
  // ---- hip_backend.hip ----
  explicit HipBackend(int device);
  ~HipBackend() override;
  const char* name() const override { return "hip-gfx950"; }
  double* alloc(size_t count) override;
  void release(double* p) override;
  void release_cache() override;
  int64_t bytes_in_use() const override;
  void upload2d(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols) override;
  void download2d(double* host, int64_t ldh, const double* src, int64_t lds, int64_t rows, int64_t cols) override;
  int64_t upload_block_rows(int64_t rows, int64_t cols) override;
  void* upload2d_begin(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols,
                       int64_t block_rows) override;
  void upload2d_wait_block(void* handle, int64_t b) override;
  void upload2d_end(void* handle) override;
  void pinned_copy_rate(int64_t bytes, double* h2d_gbs, double* d2h_gbs) override;
  void copy2d(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols) override;
  void fill_zero(double* p, size_t count) override;
  void fill_bytes(double* p, int byte, size_t count) override;
  void sync() override;
  void forgive_lost_coresidency() override;
  bool retryable_failure() override;
  int take_error(std::string* msg) override;
  void profile(bool on) override { prof_ = on; }
  void phase_begin(Phase p) override;
  void phase_end(Phase) override { phase_end_counted(true); }
  void phase_end_more(Phase) override { phase_end_counted(false); }
  void phase_reset() override;
  void phase_times(double* ms, int64_t* counts) override;
  void counters(int64_t* out4) override;
  int64_t lu_timeouts() override { return n_lu_timeouts_; }
  int64_t svd_cap_hits() override { return n_svd_cap_hits_; }
  int64_t lowrank_tail_overlaps() override { return n_tail_overlaps_; }
  int64_t lowrank_tail_series_rounds() override { return n_tail_series_rounds_; }
  void set_ranks_sharing_device(int n) override { ranks_sharing_device_ = n; }

  // ---- hip_backend_products.hip ----
  void gemm_nn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
               int64_t ldb, double beta, double* C, int64_t ldc) override;
  void gemm_nn_rowblock(int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k, const double* A, int64_t lda,
                        const double* B, int64_t ldb, double* C, int64_t ldc) override;
  void gemm_tn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
               int64_t ldb, double beta, double* C, int64_t ldc) override;
  void gemm_view(int form, bool trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                 const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int64_t m_full, int64_t r0,
                 int64_t* plan8) override;
  void gemm_nn_gridcov(int64_t m, int64_t l, int64_t k, const double* tab, int64_t nx, int64_t ny, int64_t roff,
                       int64_t koff, const double* B, int64_t ldb, double* C, int64_t ldc) override;
  void gemm_nn_pointcov(int64_t m, int64_t l, int64_t k, const double* pts, int d, int kind, double ell, double sigma2,
                        double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                        int64_t ldc) override;
  void* fftcov_create(const int64_t N[3], double beta, int fftrf) override;
  void* fftcov_create_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, double nugget,
                           const double* table, const double* table_mirror) override;
  void* fftcov_create_lags_deriv(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, int param) override;
  void fftcov_destroy(void* plan) override;
  void fftcov_apply(void* plan, int64_t l, const double* X, int64_t ldx, double* Y, int64_t ldy) override;
  void center_rows(double* S, int64_t n, int64_t N, int64_t ld) override;
  void randn(double* p, size_t count, uint64_t seed) override;
  void fill_gridcov(double* A, int64_t lda, int64_t nx, int64_t ny, double ell, int kind, int64_t row0,
                    int64_t mloc) override;
  void fill_lowrank_samples(double* S, int64_t ld, int64_t nloc, int64_t N, int64_t row0, uint64_t seed,
                            double decay) override;
  void fftrf_fields(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                    double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0) override;
  void fftrf_fields_at(double* dst, int64_t ldd, int64_t nf, int ndims, const int64_t* N, double k0, double dk, double beta,
                       const double* phi, int64_t ldphi, uint64_t seed, int64_t field0, const FftrfPointsPlan& plan) override;
  void fftrf_interpolate(double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg,
                         const FftrfPointsPlan& plan) override;
  void* points_at_create(const FftrfPointsPlan& plan, int64_t info[4]) override;
  void points_at_destroy(void* at) override;
  void points_at_gather(void* at, double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg) override;
  void points_at_spread(void* at, double* grid, int64_t ldg, int64_t nf, const double* src, int64_t lds) override;

  // ---- hip_backend_sampler.hip ----
  void* gridcov_sampler_create(int ndims, const int64_t N[3], const int64_t M[3], int kind, const double ell[3], double theta,
                               double sigma2, double nugget, double neg_tol, double info[4]) override;
  void gridcov_sampler_destroy(void* plan) override;
  void gridcov_sampler_spectrum(void* plan, double* lam_host) override;
  void gridcov_sampler_fields(void* plan, double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, const double* eps,
                              int64_t ldeps, uint64_t seed, int64_t field0) override;

  // ---- hip_backend_panels.hip ----
  void lu_L(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host) override;
  bool lu_L_keep(double* Y, int64_t m, int64_t l, int64_t ld, int32_t** ipiv_dev) override;
  int lus_block() const override { return hipk::LU2_NB; }
  void lus_u12_leaf(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12) override;
  void lus_pending(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w,
                   const double* U12) override;
  void lus_candidate(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j, double* rec) override;
  void lus_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t j0, int s, int w,
                 const double* recs, int nranks) override;
  void lus_u12_block(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                     double* U12) override;
  void lus_rankk(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
                 const double* U12) override;
  void lus_finish(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l) override;
  bool lus_mr_begin(Comm* comm, int64_t m, int64_t l) override;
  int64_t lus_mr_signature() override;
  const char* lus_mr_reason() override { return mr_reason_.c_str(); }
  int64_t lus_mr_generation() override { return mr_gen_; }
  void lus_mr_warmup() override;
  void lu_flag_export(double* flag) override;
  void lu_flag_import(const double* flag) override;
  void lus_leaf_mr(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t jb, int64_t j0, int w,
                   const double* U12) override;
  bool lus_mr_swaps_done() override { return mr_peer_swaps_; }
  int lus_mr_mode() override { return mr_work_.ov ? 2 : (mr_work_.hier ? 1 : 0); }
  void lus_mr_force(int mode) override { mr_force_ = mode; }
  void lus_swap_pack(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                     double* table) override;
  void lus_swap_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                      const double* table) override;
  void lus_pivots(int32_t* host, int64_t l) override;
  void qr_thinQ(double* Y, int64_t m, int64_t l, int64_t ld, double* R, bool replicated) override;
  bool qr_thinQ_deferred(const double* Y, int64_t m, int64_t l, int64_t ld, const double** Q1, int64_t* ldq1, double* X2) override;
  bool svd_tall_fused(const double* W, int64_t m, int64_t l, int64_t ld, int64_t K_scale, double* V, int64_t ldv,
                      double* S, const double* Xr) override;
  void svd_small(double* G, int64_t l, double* U, double* S) override;
  void chol_upper(double* B, int64_t j) override;
  void trsm_right_upper(double* F, int64_t m, int64_t j, int64_t ldf, const double* C) override;
  void scale_cols_sqrt(double* U, int64_t l, const double* S, int64_t K) override;

  // ---- hip_backend_lowrank.hip ----
  bool sample_gram(const double* S, int64_t ld, int64_t n, int64_t N, double* G) override;
  bool lowrank_tail(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T, int64_t l,
                    int64_t K, double c, double* Z, int64_t ldz, double* Sv, double* scratch, size_t scratch_doubles) override;
  void cq_gram_round_view(double* Gm, int64_t l, double* X, bool check, int32_t* out2, double* norm_out) override;
  bool lowrank_power_step(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T,
                          const int32_t* ipiv, const double* L, int64_t ldl, int64_t l, double c, double* Tn) override;
  bool lowrank_split_ok(int64_t n, int64_t N, int64_t l, int64_t l1) override;
  void lowrank_split_schur(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* T, const int32_t* ipiv1,
                           const double* P, int64_t ldp, int64_t l, int64_t l1, double c, double* Tt) override;
  void lowrank_split_rows(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1) override;
  void lowrank_split_join(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1, const int32_t* ipiv2,
                          int32_t** ipiv) override;
  void lowrank_split_undo() override;

  // ---- hip_backend_pcga.hip ----
  void colnorms(const double* Y, int64_t m, int64_t c, int64_t ld, double* host_out) override;
  void axpy(int64_t n, double a, const double* x, double* y) override;
  double dot(int64_t n, const double* x, const double* y) override;
  double nrm2(int64_t n, const double* x) override;
  void scal_copy(int64_t n, double a, const double* x, double* y) override;
  void scal(int64_t n, double a, double* x) override;
  void diag_mul_add(int64_t n, const double* d, const double* x, double* y) override;
  void gemv_n(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double beta,
              double* y) override;
  void gemv_t(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double* y) override;
  void project_out(int64_t m, int64_t ncols, const double* q, double* Y, int64_t ld) override;
  size_t lsqr_work_doubles() override { return hipk::lsqr_work_doubles(); }
  void lsqr_begin(int64_t n, const double* w, double* work) override;
  void lsqr_step_u(int64_t m, const double* t, double* u, double* work) override;
  void lsqr_step_v(int64_t n, const double* t, double* v, double* w, double* x, double* work) override;
  size_t block_cg_work_doubles(int64_t b) override { return hipk::block_cg_work_doubles(b); }
  size_t block_pcg_work_doubles(int64_t b) override { return hipk::block_pcg_work_doubles(b); }
  void block_pcg_begin(int64_t n, int64_t b, int64_t K, const double* B, const double* e, const double* W, double* S, double* Y,
                       double* P, double tol, int64_t maxiter, double* work) override;
  void block_pcg_step(int64_t n, int64_t b, int64_t K, const double* Q, const double* d, const double* e, const double* W,
                      double* X, double* R, double* P, double* S, double* Y, double* work) override;
  int precond_rows(int64_t n, double* e, double* sqe) override;
  int add_identity(double* C, int64_t K) override;
  void cg_trace_begin(const double* work, double* tr, int64_t qmax) override;
  void cg_trace_step(const double* work, double* tr, int64_t qmax) override;
  int slq_quadrature(const double* alpha, const double* beta, const double* steps, const double* rho0, int64_t qmax, int64_t b,
                     double* work, double* out) override;
  int precond_sample_rows(int64_t n, int64_t b, const double* e, const double* Y, const double* G2, double* Zout) override;
  size_t pchol_work_doubles(const PcholSource& a, int64_t n, int64_t K) override { return hipk::pchol_work_doubles(a.form, n, K); }
  void pchol_begin(const PcholSource& a, int64_t n, int64_t K, double tol, const double* L, int64_t ldl, double* d,
                   double* work) override;
  void pchol_step(const PcholSource& a, int64_t n, int64_t K, double* L, int64_t ldl, double* d, double* work) override;
  int scale_cols(int64_t n, int64_t K, double* U, int64_t ldu, const double* S) override;
  void block_cg_begin(int64_t n, int64_t b, const double* B, double tol, int64_t maxiter, double* work) override;
  void block_cg_step(int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R, double* P,
                     double* work) override;
  void f64_to_f32(const double* src, void* dst32, size_t count) override;
  void pcga_params(const double* Z, int64_t n, int64_t K, const double* s, const double* X, double delta,
                   double* out) override;
  void pcga_params_f32(const void* Z32, int64_t n, int64_t K, const double* s, const double* X, double delta,
                       double* out) override;
  void basis_gemv_f32(const void* Z32, int64_t n, int64_t K, const double* w, double beta, const double* X,
                      double* y) override;
  int fwd_products(const FwdProduct& a) override;
  int fwd_adjoint(const FwdAdjoint& a) override;
  int64_t chol_lower(double* A, int64_t m, int64_t n, int64_t ld) override;
  int64_t saddle_solve(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag, const double* b,
                       double* x, bool* singular) override;
  int basis_quadform(const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw, int64_t ncols,
                     bool upper, const double* u, double* a, double* q, double* t) override;
  int scale_rows(int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst, int64_t ldd) override;
  int rowdot_acc(int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc) override;
  int unit_panel(double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) override;
  int trapezoid_rows(double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi,
                     int64_t ldphi) override;
  int carried_rows(const double* T, int64_t ld, int64_t nobs, int64_t p, double* Wd) override;
  int bilinear_terms(int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R, const double* dd,
                     double* gram, double* t) override;

 private:
  // ---- hip_backend.hip ----
  void trim_pool(int64_t keep_bytes);
  void free_ws(DevBuf& b);
  void collect_garbage();                      // caller: this context's stream is idle
  void trim(DevBuf& b);
  void grow(DevBuf& b, size_t bytes);
  GemmWs gemm_ws(size_t doubles);
  HostStager* stager();
  static size_t stage_min_bytes();
  bool staged(bool h2d, double* dev, int64_t ldd, double* host, int64_t ldh, int64_t rows, int64_t cols);
  void drain_side() { if (st2_) (void)hipStreamSynchronize(st2_); }
  hipStream_t side_stream();
  int32_t read_flag(int slot);                 // one 4-byte read-back: the stream is idle afterwards
  void check_launch(const char* what);
  void phase_end_counted(bool counted);
  hipEvent_t get_event();

  // ---- hip_backend_products.hip ----
  // The contraction launchers of hipk::, each checked first against the workspace it was given (gemm_ws): a product whose
  // split-K slabs would not fit throws GSI_ERR_INTERNAL, naming `who` and the shape, instead of writing past ws_gemm_.
  void fits_ws(const char* who, const char* form, size_t need, const GemmWs& ws, int64_t m, int64_t l, int64_t k);
  void gemm(const char* who, const GemmWs& ws, bool trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A,
            int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, hipk::GemmPlan* plan = nullptr);
  void gemm_rowblock(const char* who, const GemmWs& ws, int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k,
                     const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                     hipk::GemmPlan* plan = nullptr);
  void gemm_syrk_upper(const char* who, const GemmWs& ws, int64_t l, int64_t k, const double* A, int64_t lda, double* C,
                       int64_t ldc, hipk::GemmPlan* plan = nullptr);
  void gemm_trmm_upper(const char* who, const GemmWs& ws, int64_t m, int64_t l, int64_t k, const double* A, int64_t lda,
                       const double* B, int64_t ldb, double* C, int64_t ldc, hipk::GemmPlan* plan = nullptr);
  std::unique_ptr<FftCov> fftcov_new_plan(const int64_t N[3], int fftrf, bool* reembed, int* dims);
  // fftcov_create_lags and fftcov_create_lags_deriv (dparam = pointcov::D_*, or -1: the covariance itself)
  void* fftcov_plan_of_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, double nugget,
                            const double* table, const double* table_mirror, int dparam);
  void fft_rotate_apply(Scratch& buf, int64_t cur[3], int64_t& tot, int d, int64_t rows_out, int64_t period, FftFactor f);
  void fftcov_lags_to_spectrum(Scratch& bufh, int64_t cur[3], int64_t& tot, const FftCov* p, int d, bool sine);
  static size_t points_plan_doubles(const FftrfPointsPlan& plan);
  void upload_points_plan(const FftrfPointsPlan& plan, double* d);
  void interp_batch(const FftrfPointsPlan& plan, const double* dplan, const double* V, int64_t v_fs, int nb, double* dst,
                    int64_t ldd);
  void fftrf_batches(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                     double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0,
                     const FftrfPointsPlan* at);

  // ---- hip_backend_panels.hip ----
  void lu_L_impl(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host, int32_t** ipiv_dev_out);
  bool lu2_resident_ok() const;
  bool lu2_takes(int64_t m, hipk::Lu2Work* w);  // lu_L_impl's first choice: the leaves held in registers (geometry in *w)
  bool lu2_fits(int bs, int rpt, int grid);
  LusWs lus_ws(int64_t, int64_t l);
  bool cholqr_gate(int64_t m, int64_t l);
  static size_t cholqr_ws_doubles(int64_t m, int64_t l);
  bool cholqr2_try(const double* Y, int64_t m, int64_t l, int64_t ld, double* T, int64_t ldt, double* small, double* ws, int& skip);

  // ---- hip_backend_lowrank.hip ----
  SplitWs split_ws(int64_t l1);

  // ---- the device, its streams and what kernels report through ----
  int ncus_ = 0;
  std::string arch_;
  // the side stream of lowrank_tail's overlap (created at its first use, lower priority than st_) and the two events that
  // order it against st_: work is put on it only between a fork and a join inside one call, so whatever drains st_ after
  // that call has drained it too; the places that drain or tear down st_ drain it all the same (drain_side)
  hipStream_t st2_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  int32_t* flags_ = nullptr;
  double* scal_ = nullptr;
  int ranks_sharing_device_ = 1;

  // ---- the block cache and the cached workspaces ----
  DevBuf ws_gemm_, ws_lu_, ws_split_, ws_qr_, ws_svd_, ws_blas2_, ws_lus_, ws_svdf_, ws_qr_hh_;
  DevBuf* const ws_all_[9] = {&ws_gemm_, &ws_lu_, &ws_split_, &ws_qr_, &ws_svd_, &ws_blas2_, &ws_lus_, &ws_svdf_, &ws_qr_hh_};
  std::mutex mu_;
  std::vector<DevBuf> sizes_;
  std::vector<DevBuf> pool_;
  std::vector<void*> garbage_;                 // outgrown workspaces, freed when this context's call has finished (free_ws)
  size_t garbage_bytes_ = 0;
  int64_t in_use_ = 0, pooled_ = 0;

  // ---- the pinned staging ring ----
  std::unique_ptr<HostStager> stager_;        // the pinned staging ring of the host boundary (created at the first large transfer)
  bool stager_failed_ = false;
  hipEvent_t ev_stage_ = nullptr;

  // ---- profiling and counters ----
  bool prof_ = false;
  Rec cur_{};
  std::vector<Rec> records_;
  std::vector<hipEvent_t> ev_pool_;
  double acc_ms_[PH_COUNT] = {0};
  int64_t acc_n_[PH_COUNT] = {0};
  int last_svd_sweeps_ = 0;
  int64_t n_svd_cap_hits_ = 0;
  int64_t n_cholqr_ = 0, n_householder_ = 0, n_scholqr3_ = 0;
  int64_t n_tail_overlaps_ = 0;
  int64_t n_tail_series_rounds_ = 0;

  // ---- the QR tiers ----
  std::map<std::pair<int64_t, bool>, int> skip_tier1_by_height_;

  // ---- panel LU on one rank ----
  std::map<int, int> lu2_resident_;   // (bs, rpt) -> resident workgroups per CU of that leaf instantiation
  bool lu2_lost_ = false, lu2_retry_ = false;
  int lu2_ov_resident_ = -1;

  // ---- panel LU sharded over ranks ----
  int mr_force_ = 0;
  // multi-rank persistent leaves: this rank's record buffer, the peers' (as this rank addresses them), the running epoch
  unsigned long long* mr_recs_ = nullptr;
  unsigned long long* mr_peer_[hipk::LU2_MAX_RANKS] = {nullptr};
  Comm* mr_comm_ = nullptr;
  uint32_t mr_epoch_ = 0;
  bool mr_disabled_ = false, mr_peer_swaps_ = true;
  bool mr_share_tried_ = false, mr_in_flight_ = false;
  int64_t mr_gen_ = 0, n_lu_timeouts_ = 0;
  std::string mr_reason_, mr_why_disabled_;
  std::set<int64_t> mr_warm_;
  hipk::Lu2MrWork mr_work_{};
  int64_t lus_part_col_ = -1, lus_part_mloc_ = 0;     // sharded LU: column whose arg-max partials the last apply kernel left
  const double* lus_part_Y_ = nullptr;

  // ---- the LowRankCovMatrix chains ----
  void* pin_power_ = nullptr; // pinned: the verdict of a power step (lowrank_power_step)
};

}  // namespace gsi
