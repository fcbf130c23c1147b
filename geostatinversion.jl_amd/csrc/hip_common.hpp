// hip_common.hpp -- declarations shared by the gfx950 kernel files and hip_backend.hip
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "pointcov.hpp"

namespace gsi { struct FwdProduct; struct FwdAdjoint; }   // backend.hpp

namespace gsi { namespace hipk {

// The > 64 KB dynamic-LDS opt-in (hipFuncSetAttribute) is a property of a kernel ON ONE DEVICE.  A process may
// hold one context per GPU (one thread per GPU, include/gsi_hip.h), so "done once" is tracked per device: one
// bit per device ordinal, one mask per kernel instantiation.  Racing first calls both set the attribute (idempotent).
inline bool first_use_on_this_device(std::atomic<uint64_t>& mask) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;   // unknown: set the attribute again
  const uint64_t bit = (uint64_t)1 << dev;
  return (mask.fetch_or(bit, std::memory_order_acq_rel) & bit) == 0;
}

// ---- gemm_f64.hip ----
// What the launcher decided for one product, filled where it computes each value when a host launcher is given a plan
// (gsi_gemm_view hands it to the kernel tests, which assert on what ran): column tiles per chunk, column chunks, XMODE of the
// instantiation, 16-byte operator loads, K splits launched, persistent mode, grid.x, output tiles.
struct GemmPlan { int64_t nt, nchunks, xmode, wide, nsplit, persistent, grid_x, active; };
size_t gemm_workspace_doubles(int64_t M, int64_t L, int64_t K);
void gemm_f64(hipStream_t st, bool transA, int64_t M, int64_t L, int64_t K, double alpha, const double* A,
              int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, double* ws,
              GemmPlan* plan = nullptr);
// C = A * B on at most max_grid (a multiple of 8) workgroups and with one K split (no workspace): the persistent mode on
// min(CUs, max_grid) workgroups, or a plain grid that already fits.  false: not applicable, nothing launched; query_only: the
// verdict and the plan without the launch.
bool gemm_f64_nn_capped(hipStream_t st, int64_t M, int64_t L, int64_t K, const double* A, int64_t lda, const double* B,
                        int64_t ldb, double* C, int64_t ldc, int max_grid, bool query_only = false, GemmPlan* plan = nullptr);
// rows [r0, r0 + mb) of the NN product of an M_full-row launch, with that launch's K split (bit-identical blocks)
size_t gemm_rowblock_workspace_doubles(int64_t M_full, int64_t mb, int64_t L, int64_t K);
void gemm_f64_nn_rowblock(hipStream_t st, int64_t M_full, int64_t r0, int64_t mb, int64_t L, int64_t K, const double* A,
                          int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, double* ws,
                          GemmPlan* plan = nullptr);
// C (l x l) = A'A, upper-triangle tiles only; C = A * B with B upper triangular (CholeskyQR: half the flops each)
size_t gemm_syrk_workspace_doubles(int64_t l, int64_t m);
// syrk_f64.hip: G = A'A (both triangles) for l <= 320 by the register-resident kernel; false = shape not covered
size_t syrk_upper_workspace_doubles(int64_t l, int64_t m);
bool syrk_full_from_upper(hipStream_t st, int64_t l, int64_t m, const double* Y, int64_t ld, double* G, int64_t ldg, double* ws);
// C (m x l) = A X, X (l x l) upper triangular, l <= 320, C not aliasing A; false = shape not covered
bool trmm_upper_tall(hipStream_t st, int64_t m, int64_t l, const double* A, int64_t lda, const double* X, int64_t ldx, double* C,
                     int64_t ldc);
void gemm_f64_syrk_upper(hipStream_t st, int64_t l, int64_t m, const double* A, int64_t lda, double* C, int64_t ldc,
                         double* ws, GemmPlan* plan = nullptr);
void gemm_f64_trmm_upper(hipStream_t st, int64_t M, int64_t L, int64_t K, const double* A, int64_t lda, const double* B,
                         int64_t ldb, double* C, int64_t ldc, double* ws, GemmPlan* plan = nullptr);
// C = G * B, G(i,k) = tab[|x_i-x_k| * ny + |y_i-y_k|] generated in registers (tab: nx * ny kernel table)
void gemm_f64_gridcov(hipStream_t st, int64_t M, int64_t L, int64_t K, const double* tab, int64_t nx, int64_t ny,
                      int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C, int64_t ldc, double* ws);

// ---- the scattered-point covariance (gemm_f64.hip GEN 2, pointcov_gemm.hip) ----
// the scattered-point covariance generated inside the contraction's tile loader (gemm_f64.hip, GEN 2); pts4: 32-byte records
void gemm_f64_pointcov(hipStream_t st, int64_t M, int64_t L, int64_t K, const double* pts4, int64_t npts, int d, int kind,
                       double sigma2, double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                       int64_t ldc, double* ws, double* xpack);
double pointcov_point_scale(int kind, double inv_ell);
// pointcov_gemm.hip: the same product with 96-row x 320-column tiles (every entry generated once for sketches of up to 320
// columns); false = not applicable (L <= 160, GSI_POINTCOV_WIDE=0, X beyond 32-bit tile offsets)
bool gemm_f64_pointcov_wide(hipStream_t st, int64_t M, int64_t L, int64_t K, const double* pts4, int64_t npts, int d, int kind,
                            double sigma2, double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                            int64_t ldc, double* ws, double* xpack);
size_t gemm_pointcov_workspace_doubles(int64_t M, int64_t L, int64_t K);   // covers both tilings
size_t gemm_pointcov_pack_doubles(int64_t M, int64_t L, int64_t K);        // the wide kernel's packed copy of X (0: not its product)
int gemm_choose_split(int64_t nwg, int64_t K);
// C = sum over the nsplit slabs (M x L each, leading dimension M), fixed order
void gemm_splitk_reduce(hipStream_t st, int64_t M, int64_t L, int nsplit, const double* slabs, double* C, int64_t ldc);
void pointcov_pad_points(hipStream_t st, const double* pts, int d, int64_t n, double scale, double* out4);
// ---- fft_cov.hip ----
int64_t fft_embed_size(int64_t N);   // next power of two >= 2 N (1 for a singleton axis)
size_t fft_plan_doubles(const int64_t M[3]);   // spectrum + scratch + twiddle table
// lam (fft_plan_doubles) <- |k|^beta / sum, scratch part64 = lam + Mtot, twiddles behind it
void fft_spectrum(hipStream_t st, double* lam, double* part64, const int64_t M[3], double beta, int fftrf);
// FFTRF's 2 N embedding on grids that are not powers of two (fft_cov.hip): pieces of the re-embedded spectrum
void fft_cos_matrix(hipStream_t st, double* out, int64_t rows, int64_t cols, int64_t period, bool weighted);
void fft_lines_layout(hipStream_t st, const double* nat, double* out, const int64_t M[3]);
void fft_spectrum_natural(hipStream_t st, double* lam, const int64_t M[3], double beta, int fftrf);
void fft_finish_plan(hipStream_t st, double* lam, double* part64, const int64_t M[3]);
void fft_plan_twiddles(hipStream_t st, double* lam, const int64_t M[3]);   // the twiddle table of a plan, nothing else
// ---- fft_gridcov_plan.hip: plans whose lags come from a covariance function or the caller's table ----
// cp (and cm = the lags (t0, -t1) of a rotated 2-D kernel, or null) <- sigma2 k(r) over the box N, pointcov::kernel's kinds
void fft_lag_table(hipStream_t st, double* cp, double* cm, const int64_t N[3], int kind, const double inv_ell[3], double cs,
                   double sn, double sigma2);
// the same lags of d (sigma2 k(r)) / d param (pointcov::D_*); cm is written whenever it is not null
void fft_lag_table_deriv(hipStream_t st, double* cp, double* cm, const int64_t N[3], int kind, int param, const double inv_ell[3],
                         double cs, double sn, double sigma2);
void fft_even_odd_split(hipStream_t st, double* cp, double* cm, int64_t total);   // -> ((c+ + c-) / 2, (c+ - c-) / 2)
void fft_sin_matrix(hipStream_t st, double* out, int64_t rows, int64_t cols, int64_t period);   // w_r sin(2 pi r c / period)
void fft_subtract(hipStream_t st, double* a, const double* b, int64_t total);     // a -= b
// lam (line-by-line layout) <- (lam + nugget) / Mtot, twiddles behind it: no normalisation to a unit diagonal
void fft_finish_plan_lags(hipStream_t st, double* lam, const int64_t M[3], double nugget);
void fft_cov_apply(hipStream_t st, const int64_t N[3], const int64_t M[3], const double* lam, double2* W, int nb_max,
                   int64_t l, const double* X, int64_t ldx, double* Y, int64_t ldy);

// ---- fftrf_sample.hip: FFTRF.powerlaw_structuredgrid fields on the device ----
// The grid as the sampler sees it: A = (N[1], N[0], N[2]) the half lengths along the ARRAY axes (the reference's axis swap),
// L = 2 A the doubled grid, per axis Bluestein (2 A not a power of two) with convolution length P (P = L on a direct axis).
struct FftrfGeom { int d; int64_t A[3], L[3], P[3]; int blue[3]; int64_t Mtot, n; };
void fftrf_geometry(int ndims, const int64_t* N, FftrfGeom* g);
size_t fftrf_plan_doubles(const FftrfGeom& g);     // twiddles + per Bluestein axis the chirp and its spectrum
size_t fftrf_field_doubles(const FftrfGeom& g);    // workspace of one field of a batch: phi | W | raw field | partial sums
void fftrf_plan(hipStream_t st, const FftrfGeom& g, double* plan);
// nb fields whose phi sits at ws + b fs (fs even, >= fftrf_field_doubles): dst[(r - row0) + b ldd] for r in [row0, row0 + nloc)
void fftrf_sample(hipStream_t st, const FftrfGeom& g, const double* plan, double* ws, int64_t fs, int nb, double k0, double dk,
                  double beta, double* dst, int64_t ldd, int64_t row0, int64_t nloc);
int fftrf_tile_lines(int Ma, bool contiguous, int64_t nl0);   // lines per tile of a pass (gridcov_sample.hip takes the same)
void fftrf_twiddles(hipStream_t st, double* twg);             // exp(-2 pi i k / FFT_TW_LEN), k < FFT_TW_LEN / 2
// ---- gridcov_sample.hip: Gaussian fields with a grid covariance function by circulant embedding ----
// N (box) and M (torus, powers of two) squeezed to 3 axes (1 beyond d); torus order t0 + M0 (t1 + M1 t2)
struct GcsGeom { int d; int64_t N[3], M[3]; int64_t Mtot, n; };
constexpr int GCS_PARTS = 64;                       // partial results per reduction: fixed, so the plan's numbers are too
size_t gcs_pair_doubles(const GcsGeom& g);          // workspace of one pair of fields: eps1 | eps2 | W (N0 x M1 x M2 complex)
// amp <- the torus covariance sigma2 k(r), the even part taken where a lag is M_a / 2 (nugget not included)
void gcs_lag_table(hipStream_t st, const GcsGeom& g, int kind, const double inv_ell[3], double cs, double sn, double sigma2,
                   double* amp);
// lam <- Re of the transform of the table in amp, by the sampler's own passes (W: Mtot complex)
void gcs_plan_transform(hipStream_t st, const GcsGeom& g, const double* twg, const double* amp, double* W, double* lam);
// lam += nugget; amp <- sqrt(max(lam, 0) / Mtot); part (4 GCS_PARTS) <- partial sums of |lam| over lam < 0, minima, maxima
// and counts of lam < 0, each over a fixed chunk in a fixed order
void gcs_plan_finish(hipStream_t st, const GcsGeom& g, double nugget, double* lam, double* amp, double* part);
// nb pairs whose noise sits at ws + b fs (eps1 | eps2, Mtot each; fs even, >= gcs_pair_doubles): fields 2 b and 2 b + 1 (the
// latter only if 2 b + 1 < ncols) into dst[(r - row0) + c ldd] for r in [row0, row0 + nloc)
void gcs_sample(hipStream_t st, const GcsGeom& g, const double* twg, const double* amp, double* ws, int64_t fs, int nb,
                double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t ncols);
// ---- fftrf_interp.hip: FFTRF.interpolate (FFTRF.jl:107-129), nb structured fields at m scattered points ----
// base (m), frac (d x m, axis-major): the plan of fftrf_points.hpp on the device; field b at V + b v_fs, vec() order, strides
// 1, s1, s2 along its axes; dst[p + b ldd] = the nested two-term sums, each product and sum rounded on its own
void fftrf_interp(hipStream_t st, int d, const int32_t* base, const double* frac, int64_t m, int64_t s1, int64_t s2,
                  const double* V, int64_t v_fs, int nb, double* dst, int64_t ldd);
// ---- interp_adjoint.hip: the adjoint of that gather, G = W' X, through the inverted index of interp_adjoint_plan.hpp ----
// The index and the points plan's frac on the device (arrays as documented there).  G (n x nf, ld ldg): every entry is
// written, a node nobody reaches gets 0.0; X is m x nf (ld ldx); partial: nchunk x nf doubles (unused when nchunk == 0).
struct IadjDev {
  int d;
  int64_t n, m, chunk, nlong, nchunk;
  const int64_t* nodeptr;
  const int32_t* point;
  const uint8_t* corner;
  const double* frac;
  const int32_t* long_node;
  const int64_t* long_chunk0;
  const int64_t* chunk_off;
  const int32_t* chunk_len;
};
void interp_adjoint(hipStream_t st, const IadjDev& p, const double* X, int64_t ldx, int64_t nf, double* G, int64_t ldg,
                    double* partial);

// ---- panel_lu_leaf.hip: register-resident leaves (panels of <= 4096 rows per CU, a little more with overflow rows); the
//      updates between the blocks are panel_lu_blocks.hip's ----
constexpr int LU2_LEAF = 8;           // leaf width: columns a thread keeps in registers
constexpr int LU2_NB = 64;            // widest block (left-looking leaves inside; lu_schedule.hpp: LU_SCHED_MAX_W)
constexpr int LU2_RES_COPIES = 8;     // copies of the per-step result record (one per group of pollers)
constexpr int LU2_REC_GRANULES = 64;  // one published record per workgroup and pivot step: 64 8-byte granules (512 B)
struct Lu2Work {
  unsigned long long* recs;   // [2][grid][LU2_REC_GRANULES] candidate records, then [2][LU2_RES_COPIES][LU2_REC_GRANULES] results
  double* u12;      // [l * l]: the U rows of every block, U(p, c) at p + c * l
  int32_t* ipiv;    // [l]
  int32_t* info;    // [1] first exactly-zero pivot (1-based); -1: the exchange between workgroups timed out
  int bs, rpt, grid;
  std::vector<int> widths;     // the block schedule (lu_schedule.hpp): 16 .. 64 columns each, a last block of what is left
  int poll_limit = 0;          // polls before a workgroup gives up on a record (0: the default, ~ seconds)
  uint32_t mute_epoch = 0;     // tests only: the last workgroup publishes nothing at this pivot step (1-based)
  bool cooperative = false;    // launch the leaves with hipLaunchCooperativeKernel (co-residency guaranteed by the runtime)
  bool ov = false;             // the panel is taller than grid x 4096 rows: <512, 8> leaves with lazily evaluated overflow rows
};
int lu2_resident_per_cu_ov();
// workgroups of the (bs, rpt) leaf kernel that fit one CU (occupancy query); 0 if the query fails
int lu2_resident_per_cu(int bs, int rpt);
// the same leaf kernel across RANKS (one launch per rank, records written into every rank's peer-mapped buffer); the
// interchanges across ranks that follow a leaf (lus_swap_*) are panel_lu_sharded.hip's
constexpr int LU2_MAX_RANKS = 16;
constexpr int LU2_MR_MAXL = 8192;        // widest panel of the multi-rank persistent-leaf path (row boxes)
struct Lu2MrWork {
  unsigned long long* peer[LU2_MAX_RANKS];   // every rank's record buffer: [2][nranks * grid][LU2_REC_GRANULES]
  int32_t* ipiv;                             // [l] this rank's copy of the pivot rows (identical on every rank)
  int32_t* info;
  int rank, nranks, bs, rpt, grid;
  int hier = 0;                              // two-hop exchange (ranks reduce among their own workgroups first)
  int ov = 0;                                // the shard is taller than grid x 4096 rows: overflow rows evaluated lazily
  int poll_limit = 0;
};
bool lu2_mr_config(int64_t pad, int nranks, int ncus, int* bs, int* rpt, int* grid, int* hier, int* ov, int force = 0);
int lu2_mr_resident_per_cu(int bs, int rpt);
int lu2_mr_resident_per_cu_ov();
size_t lu2_mr_record_granules(int nranks, int grid);
void lu2_leaf_mr(hipStream_t st, const Lu2MrWork& w, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l,
                 int64_t jb, int64_t j0, int wd, const double* us, uint32_t epoch_base);
void lus_swap_peer(hipStream_t st, const Lu2MrWork& w, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l,
                   int64_t j0, int wd, uint32_t epoch_base);
void lus_swap_pack(hipStream_t st, const double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j0, int w,
                   const int32_t* ipiv, double* table);
void lus_swap_apply(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j0, int w,
                    const int32_t* ipiv, const double* table);
// launch geometry for an m-row panel on a chip with `ncus` CUs; false: the panel does not fit the register file
bool lu2_config(int64_t m, int ncus, int* bs, int* rpt, int* grid);
// the workspace of lu2_L for w.grid workgroups, and w.recs / w.u12 / w.ipiv laid into it
size_t lu2_work_bytes(int64_t l, int grid);
void lu2_carve(Lu2Work& w, int64_t l, void* work);
void lu2_L(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, const Lu2Work& w);

// ---- panel_lu_streamed.hip: panels taller than the register file: streamed leaves, lazily evaluated (no spin-waits);
//      `work` = lu3_work_bytes(l) bytes ----
size_t lu3_work_bytes(int64_t l);
void lu3_L(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, void* work, int32_t* info, int32_t** ipiv_out);

// ---- panel_lu_sharded.hip: row-sharded form (the exchange between ranks is pipeline.cpp's): primitives on this rank's rows
//      [row0, row0 + mloc); lus_u12_block and lus_rankk, the right-looking block update, are panel_lu_blocks.hip's ----
int lus_grid(int64_t mloc);
void lus_candidate(hipStream_t st, const double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j, double* rec,
                   double* pval, int64_t* pidx, bool partials_ready);
void lus_apply(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l, int64_t j0, int s, int w,
               const double* recs, int nranks, int32_t* ipiv, int32_t* info, double* next_pval, int64_t* next_pidx);
void lus_u12_leaf(hipStream_t st, const double* Y, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12);
void lus_pending(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t jb, int64_t j0, int w,
                 const double* U12);
void lus_u12_block(hipStream_t st, const double* Y, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                   double* U12);
void lus_rankk(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
               const double* U12);
void lus_finish(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l);
// the factorization's time-out flag (info < 0) as a double (1.0 / 0.0) for an all-reduce on the stream, and back: raise
// info = -1 here if any rank had it up
void lu_flag_export(hipStream_t st, const int32_t* info, double* flag);
void lu_flag_import(hipStream_t st, int32_t* info, const double* flag);

// ---- lsqr_dev.hip: IterativeSolvers.lsqr's vector updates with device-resident scalars ----
size_t lsqr_work_doubles();
void lsqr_begin(hipStream_t st, int64_t n, const double* w, double* work);
void lsqr_step_u(hipStream_t st, int64_t m, const double* t, double* u, double* work);
void lsqr_step_v(hipStream_t st, int64_t n, const double* t, double* v, double* w, double* x, double* work);

// ---- block_cg.hip: the multi-column conjugate-gradient solver's panel passes with device-resident scalars (cg_state.hpp) ----
constexpr int BLOCK_CG_PARTS = 128;    // row parts of the fixed grid = partial sums per column and reduction
size_t block_cg_work_doubles(int64_t b);
void block_cg_begin(hipStream_t st, int64_t n, int64_t b, const double* B, double tol, int64_t maxiter, double* work);
void block_cg_step(hipStream_t st, int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R, double* P,
                   double* work);
// passes 1 and 2 of block_cg_step alone (s: the state block, part: b x BLOCK_CG_PARTS sums), for block_pcg.hip; vec: the
// 16-byte form, allowed where block_cg_vec says so of every panel the pass touches
bool block_cg_vec(int64_t n, const void* a, const void* b2, const void* c, const void* d, const void* e);
void block_cg_pass_pq(hipStream_t st, bool vec, int64_t n, int64_t b, const double* P, const double* Q, const double* d,
                      const double* s, double* part);
void block_cg_pass_xr(hipStream_t st, bool vec, int64_t n, int64_t b, const double* P, const double* Q, const double* d,
                      double* X, double* R, const double* s, double* part);

// ---- block_pcg.hip: the same solver preconditioned by a low-rank-plus-diagonal P ----
size_t block_pcg_work_doubles(int64_t b);
// Y = W (W'B) has been formed by the caller: P <- z0 = e .* B - Y, the sums b'b and b'z0, the state of a fresh solve
void block_pcg_begin(hipStream_t st, int64_t n, int64_t b, const double* B, const double* e, const double* Y, double* P,
                     double tol, int64_t maxiter, double* work);
// passes 1 and 2 and their scalar kernels; then, once the caller has formed Y = W (W'R): passes 3a and 3b and theirs
void block_pcg_step_xr(hipStream_t st, int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R,
                       const double* P, double* work);
void block_pcg_step_p(hipStream_t st, int64_t n, int64_t b, const double* e, const double* R, const double* Y, double* P,
                      double* work);
void pcg_precond_rows(hipStream_t st, int64_t n, double* e, double* sqe);
void pcg_add_identity(hipStream_t st, double* C, int64_t K);

// ---- block_slq.hip: the coefficient trace of the two solvers above and its Gauss quadrature (cg_state.hpp's trace_col,
//      slq_state.hpp).  state: the solver's state block (the front of its `work`); tr:
//      cgst::trace_doubles(b, qmax) doubles; alpha, beta, work: column-interleaved, work 3 * qmax * b doubles ----
void slq_trace_begin(hipStream_t st, const double* state, double* tr, int64_t qmax);
void slq_trace_step(hipStream_t st, const double* state, double* tr, int64_t qmax);
void slq_quadrature(hipStream_t st, const double* alpha, const double* beta, const double* steps, const double* rho0,
                    int64_t qmax, int64_t b, double* work, double* out);
// Zout = Y ./ e + G2 ./ sqrt(e), n x b panels (ld n)
void slq_sample_rows(hipStream_t st, int64_t n, int64_t b, const double* e, const double* Y, const double* G2, double* Zout);

// ---- pivoted_chol.hip: diagonal-pivoted Cholesky of a covariance read by entries (pchol_state.hpp) ----
// where A(i, p) comes from.  form 1: a = the stored matrix (ld); 2: a = the nx * ny table over grid offsets; 3: a = the points
// as the 32-byte records of pointcov_pad_points, entries by the generator of pointcov_gen.hpp
struct PcholCol {
  int form;
  const double* a;
  int64_t ld;
  int32_t ny;
  int dim, kind;
  double sigma2, nugget;
};
size_t pchol_work_doubles(int form, int64_t n, int64_t K);
double* pchol_points(double* work, int64_t n, int64_t K);     // form 3: where the 4 n doubles of the records lie in `work`
void pchol_begin(hipStream_t st, const PcholCol& a, int64_t n, int64_t K, double tol, const double* L, int64_t ldl, double* d,
                 double* work);
void pchol_step(hipStream_t st, const PcholCol& a, int64_t n, int64_t K, double* L, int64_t ldl, double* d, double* work);
void scale_cols(hipStream_t st, int64_t n, int64_t K, double* U, int64_t ldu, const double* S);

// ---- panel_qr.hip ----
constexpr int QR_NB = 16;
struct QrWork {
  double* coef;     // [2 + NB]: scale, tau, tw[NB]
  double* part;     // [maxblocks * NB] partial sums
  double* tau;      // [l]
  double* T;        // [l * NB]   T factors, panel k at T + k*NB*NB
  double* G;        // [NB*NB]    V'V
  double* Vbuf;     // [m * NB]
  double* Wt;       // [l * NB]
  double* W2;       // [NB * l]
  double* Qo;       // [m * l]
  int64_t maxblocks;
};
int64_t qr_max_blocks(int64_t m);
void qr_thinQ(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, double* R, const QrWork& w,
              double* gemm_ws);
// the Householder tier's range guard: amax_ws[0] <- max |Y| (amax_ws: 1 + QR_AMAX_PARTS doubles), the exponent e of the
// exact prescale 2^-e that max calls for (0: none), and A *= s
constexpr int QR_AMAX_PARTS = 256;
void qr_absmax(hipStream_t st, const double* Y, int64_t m, int64_t l, int64_t ld, double* amax_ws);
int qr_prescale_exponent(double amax);
void qr_scale(hipStream_t st, double* A, int64_t rows, int64_t cols, int64_t ld, double s);

// ---- cholqr.hip ----
size_t cholqr_small_doubles(int64_t l);
void cholqr2_factor(hipStream_t st, const double* Y, int64_t m, int64_t l, int64_t ld, double* T, int64_t ldt,
                    double* small_ws, int32_t* flag, double* gemm_ws);
void cholqr2_apply(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, const double* T, int64_t ldt,
                   double* R, double* small_ws, double* gemm_ws);
void cholqr2_R(hipStream_t st, int64_t l, double* small_ws, double* R);         // R = R2 R1 after cholqr2_factor
const double* cholqr2_X2(const double* small_ws, int64_t l);                    // R2^-1 (l x l) after cholqr2_factor
void mirror_upper(hipStream_t st, double* G, int64_t l);                          // strictly lower <- upper
// R = chol(Gm) in place and X = R^-1 for a Gram matrix formed by the caller (upper triangle read, then mirrored); check: the
// second round's |Gm - I| test.  series (four device words, 8-byte aligned: rounds taken, taken this time, |Gm - I|_F as a
// double) and tmp (l x l), with check: R and X by their second-order series where |Gm - I|_F <= 6e-6.  false: l > 384 (nothing
// queued)
bool cq_gram_round(hipStream_t st, double* Gm, int64_t l, double* X, bool check, int32_t* flag, int32_t* series = nullptr,
                   double* tmp = nullptr);
void tri_product(hipStream_t st, const double* R2, const double* R1, int64_t l, double* R);   // R = R2 R1 (upper triangular)
// X = R^-1 of an upper triangular R by the inverse half of the fused Cholesky kernel (false: l > 384, nothing queued)
bool tri_inverse(hipStream_t st, const double* R, int64_t l, double* X);
// randsvd's power steps in sample space (with lowrank_power.hip): R (nr x N, ld ldr) <- rows S[src[k]] - S[sub[k]] (S[src[k]]
// where sub[k] < 0); part[0 .. nparts) <- partial maxima of |E[k, j] - L[rows[k], j]| over k < nchk, j < l (NaN: +inf)
void lr_gather_rows(hipStream_t st, const double* S, int64_t lds, int64_t N, const int64_t* src, const int64_t* sub,
                    int64_t nr, double* R, int64_t ldr);
void lr_check_rows(hipStream_t st, const double* E, int64_t lde, const double* L, int64_t ldl, const int64_t* rows,
                   int64_t nchk, int64_t l, double* part, int nparts);
void scholqr3_factor(hipStream_t st, const double* Y, int64_t m, int64_t l, int64_t ld, double* T, int64_t ldt,
                     double* S, int64_t lds, double* small_ws, int32_t* flag, double* gemm_ws);
void scholqr3_apply(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, const double* S, int64_t lds,
                    double* R, double* small_ws, double* gemm_ws);

// ---- lowrank_power.hip ----
// The LU's interchanges piv[0:l) composed on the device into the index lists of lr_gather_rows / lr_check_rows (blocks of 2 l,
// nchk and 2 l rows at 0, o_chk and o_sm; unused rows S[0] - S[0]); verdict[0:4) <- *info, invalid pivot seen, moved rows, 0
void lr_compose(hipStream_t st, const int32_t* piv, const int32_t* info, int64_t n, int64_t l, int64_t nchk, int64_t o_chk,
                int64_t o_sm, int64_t ldr, int64_t* src, int64_t* sub, int64_t* chk, int32_t* verdict);
// Ut (l x l) <- (c L11^-1 Mp)' on and below the diagonal, L11 the unit lower triangle on top of L;  C (N x l) <- c T U^-1
void lr_solve_u(hipStream_t st, const double* L, int64_t ldl, const double* Mp, int64_t l, double c, double* Ut);
void lr_solve_c(hipStream_t st, const double* Ut, int64_t l, const double* T, int64_t N, double c, double* C);
// A panel factored in two column halves.  [U11 | U12] = c L11^-1 Mp from the left half's pivot rows,
// Mp (l1 x l, ld l1): Ut11 (l1 x l1) <- U11' on and below its diagonal, U12 (l1 x (l - l1), ld l1) as it stands
void lr_solve_u12(hipStream_t st, const double* L, int64_t ldl, const double* Mp, int64_t l1, int64_t l, double c, double* Ut11,
                  double* U12);
// X[sub[k]] <- X[src[k]] on nc columns of X (ld ldx) for the k < verdict[2] (<= maxmv) moved rows of lr_compose's first block,
// all read into tmp (maxmv x nc, ld ldt) before any is written; then rows [0, nzero) <- 0
void lr_move_rows(hipStream_t st, double* X, int64_t ldx, int64_t nc, const int64_t* src, const int64_t* sub,
                  const int32_t* verdict, int64_t maxmv, double* tmp, int64_t ldt, int64_t nzero);
void lr_pivots(hipStream_t st, const int32_t* piv, int64_t cnt, int64_t add, int32_t* dst);   // dst[j] <- piv[j] + add
void lr_forget_zero_pivot(hipStream_t st, int32_t* info);                                      // *info > 0: <- 0
// ---- jacobi_svd.hip ----
struct SvdWork {
  int32_t* rotcount;  // [1]
  double* norms;      // [l]
  int32_t* pairs;     // [SVD_SCHED_INTS] block-pair activity flags, then the sparse sweep's schedule (null: plain sweeps only)
};
constexpr int SVD_SCHED_INTS = 4096;
// returns number of sweeps used
int svd_small(hipStream_t st, double* G, int64_t l, double* U, double* S, const SvdWork& w);

// ---- misc.hip ----
void center_rows(hipStream_t st, double* S, int64_t n, int64_t N, int64_t ld);
void scale_cols_sqrt(hipStream_t st, double* U, int64_t l, const double* S, int64_t K);
void randn_fill(hipStream_t st, double* p, size_t count, uint64_t seed);
void fill_gridcov(hipStream_t st, double* A, int64_t lda, int64_t nx, int64_t ny, double ell, int kind,
                  int64_t row0, int64_t mloc);
void fill_lowrank_samples(hipStream_t st, double* S, int64_t ld, int64_t nloc, int64_t N, int64_t row0, uint64_t seed,
                          double decay);
void colnorms_sq(hipStream_t st, const double* Y, int64_t m, int64_t c, int64_t ld, double* out_dev);
void chol_upper(hipStream_t st, double* B, int64_t j, int32_t* info);
void trsm_right_upper(hipStream_t st, double* F, int64_t m, int64_t j, int64_t ldf, const double* C);
void axpy(hipStream_t st, int64_t n, double a, const double* x, double* y);
void scal_copy(hipStream_t st, int64_t n, double a, const double* x, double* y);
void dot_dev(hipStream_t st, int64_t n, const double* x, const double* y, double* out_dev);   // out_dev: >= 8 + 256 doubles
void scal(hipStream_t st, int64_t n, double a, double* x);
void gemv_n(hipStream_t st, int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double beta,
            double* y);
size_t gemv_t_workspace_doubles(int64_t k);
void gemv_t(hipStream_t st, int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double* y,
            double* part);
void project_out(hipStream_t st, int64_t m, int64_t ncols, const double* q, double* Y, int64_t ld, double* part);
void diag_mul_add(hipStream_t st, int64_t n, const double* d, const double* x, double* y);
void f64_to_f32(hipStream_t st, const double* src, float* dst, size_t count);
void pcga_params_f32(hipStream_t st, const float* Z, int64_t n, int64_t K, const double* s, const double* X, double delta,
                     double* out);
void basis_gemv_f32(hipStream_t st, const float* Z, int64_t n, int64_t K, const double* w, double beta, const double* X,
                    double* y);
void extract_upper(hipStream_t st, const double* Y, int64_t ld, int64_t l, double* R);
void pcga_params(hipStream_t st, const double* Z, int64_t n, int64_t K, const double* s, const double* X,
                 double delta, double* out);

// ---- pcga_forward.hip: the sparse forward model (backend.hpp: FwdProduct) ----
// one lane per (segment, column) output, for short rows; one wave per segment and group of 16 columns, for long ones
void fwd_lane(hipStream_t st, const FwdProduct& a);
void fwd_wave(hipStream_t st, const FwdProduct& a);
// out[r, c] = the partial sums of row r's segments, added in segment order (only when rows were split)
void fwd_reduce(hipStream_t st, const FwdProduct& a);
// ---- fwd_adjoint.hip: G = H' V through the inverted index of fwd_adjoint_plan.hpp (backend.hpp: FwdAdjoint) ----
// throws std::runtime_error for a shape one launch cannot take (the caller batches the columns: FADJ_MAX_COLS)
constexpr int64_t FADJ_MAX_COLS = 4096;
void fwd_adjoint(hipStream_t st, const FwdAdjoint& a);

// ---- chol_saddle.hip: blocked Cholesky and the saddle-point solve of pcgadirect ----
// C (mc x nc lower trapezoid, mc >= nc) = beta C + alpha P P' (+ R): rmode 0 none, 1 dense lower (ld ldr), 2 diagonal entries.
// P: mc x k.  flag: the factorization's pivot flag -- nothing is done once it is non-zero.
void cs_syrk_lower(hipStream_t st, double* C, int64_t ldc, int64_t mc, int64_t nc, const double* P, int64_t ldp, int64_t k,
                   double alpha, double beta, const double* R, int64_t ldr, int rmode, const int32_t* flag);
// the m x n trapezoid A (m >= n, lower triangle of the top n x n read) <- [L; (L^-1 B')'] in place, blocks of 64 columns;
// *flag (zero on entry) <- the 1-based column of the first pivot that is not a positive finite number
void cs_chol_lower(hipStream_t st, double* A, int64_t m, int64_t n, int64_t ld, int32_t* flag);
void cs_set_rows(hipStream_t st, double* W, int64_t ld, int64_t nobs, const double* HX, const double* b);
void cs_schur(hipStream_t st, const double* W, int64_t ld, int64_t nobs, const double* b, double* x, double* out3);
size_t cs_backsolve_workspace_doubles();
void cs_backsolve(hipStream_t st, const double* A, int64_t n, int64_t ld, double* x, double* part);

// ---- posterior_var.hip: the row pass of the posterior variance (Backend::basis_quadform) ----
// a[i] = |W' z_i|^2, q[i] = |z_i|^2 (q may be null), t[i] = u' z_i (u, t null together) for the rows of Z (n x K, ld ldz,
// double or float by zbits) and W (K x ncols, ld ldw, device; upper: entries below the diagonal are not read)
void pv_quadform(hipStream_t st, const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw,
                 int64_t ncols, bool upper, const double* u, double* a, double* q, double* t);
void pv_scale_rows(hipStream_t st, int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst,
                   int64_t ldd);

// ---- posterior_exact.hip: the exact posterior variance of linear inversion and kriging ----
// acc[i] += sum_c A[i, c] B[i, c] over column-major n x b panels, products rounded one by one and added in ascending c;
// A == B with lda == ldb takes the instantiation that loads each entry once
void px_rowdot_acc(hipStream_t st, int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc);
void px_unit_panel(hipStream_t st, double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0);
void px_trapezoid_rows(hipStream_t st, double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi,
                       int64_t ldphi);
void px_carried_rows(hipStream_t st, const double* T, int64_t ld, int64_t nobs, int64_t p, double* Wd);

// ---- bilinear_terms.hip: the bilinear forms of the likelihood gradient ----
// With V = Y + dd .* R (dd, R null: V = Y) over column-major n x b panels of leading dimension n:
// gram[a + g c] = sum_i L[i, a] V[i, c] (a, c < g) and t[j - g] = sum_i L[i, j] V[i, j] (g <= j < b), summed per chunk of
// BILINEAR_CHUNK rows into `partial` (bilinear_partial_doubles(n, b, g) doubles) and then over the chunks in ascending order.
constexpr int64_t BILINEAR_CHUNK = 2048;
size_t bilinear_partial_doubles(int64_t n, int64_t b, int64_t g);
void bilinear_terms(hipStream_t st, int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R,
                    const double* dd, double* partial, double* out);

}}  // namespace gsi::hipk
