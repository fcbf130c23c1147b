// hip_backend_products.hip -- HipBackend's products: the contraction launchers (each checked against the workspace it was given),
// the operators generated inside the contraction's loader, the matrix-free FFT covariance plans, and the generators (samples,
// FFTRF fields).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "hip_backend_impl.hpp"
#include "interp_adjoint_plan.hpp"

namespace gsi {

// ---- the checked launchers ----
// The split-K workspace of a product is sized where the method that launches it sizes ws_gemm_ (a gmax list, or the product's
// own *_workspace_doubles): `need` is what the launcher itself is about to use.  Host arithmetic only, and never true for a
// shape the sizing covers.
void HipBackend::fits_ws(const char* who, const char* form, size_t need, const GemmWs& ws, int64_t m, int64_t l, int64_t k) {
  if (need <= ws.doubles) return;
  throw Error(GSI_ERR_INTERNAL, std::string(who) + ": the " + form + " product " + std::to_string(m) + " x " + std::to_string(l) +
                                    " (K = " + std::to_string(k) + ") needs a workspace of " + std::to_string(need) +
                                    " doubles and was given " + std::to_string(ws.doubles));
}
void HipBackend::gemm(const char* who, const GemmWs& ws, bool trans, int64_t m, int64_t l, int64_t k, double alpha,
                      const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc,
                      hipk::GemmPlan* plan) {
  fits_ws(who, trans ? "A'B" : "AB", hipk::gemm_workspace_doubles(m, l, k), ws, m, l, k);
  hipk::gemm_f64(st_, trans, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc, ws.p, plan);
}
void HipBackend::gemm_rowblock(const char* who, const GemmWs& ws, int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k,
                               const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                               hipk::GemmPlan* plan) {
  fits_ws(who, "row-block", hipk::gemm_rowblock_workspace_doubles(m_full, mb, l, k), ws, mb, l, k);
  hipk::gemm_f64_nn_rowblock(st_, m_full, r0, mb, l, k, A, lda, B, ldb, C, ldc, ws.p, plan);
}
void HipBackend::gemm_syrk_upper(const char* who, const GemmWs& ws, int64_t l, int64_t k, const double* A, int64_t lda,
                                 double* C, int64_t ldc, hipk::GemmPlan* plan) {
  fits_ws(who, "A'A", hipk::gemm_syrk_workspace_doubles(l, k), ws, l, l, k);
  hipk::gemm_f64_syrk_upper(st_, l, k, A, lda, C, ldc, ws.p, plan);
}
void HipBackend::gemm_trmm_upper(const char* who, const GemmWs& ws, int64_t m, int64_t l, int64_t k, const double* A,
                                 int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, hipk::GemmPlan* plan) {
  fits_ws(who, "A triu(B)", hipk::gemm_workspace_doubles(m, l, k), ws, m, l, k);
  hipk::gemm_f64_trmm_upper(st_, m, l, k, A, lda, B, ldb, C, ldc, ws.p, plan);
}

// ---- products ----
void HipBackend::gemm_nn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
                         int64_t ldb, double beta, double* C, int64_t ldc) {
  bind();
  const GemmWs ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
  gemm("gemm_nn", ws, false, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc);
  check_launch("gemm_nn");
}
void HipBackend::gemm_nn_rowblock(int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k, const double* A, int64_t lda,
                                  const double* B, int64_t ldb, double* C, int64_t ldc) {
  bind();
  const GemmWs ws = gemm_ws(hipk::gemm_rowblock_workspace_doubles(m_full, mb, l, k));
  gemm_rowblock("gemm_nn_rowblock", ws, m_full, r0, mb, l, k, A, lda, B, ldb, C, ldc);
  check_launch("gemm_nn_rowblock");
}
void HipBackend::gemm_tn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
                         int64_t ldb, double beta, double* C, int64_t ldc) {
  bind();
  const GemmWs ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
  gemm("gemm_tn", ws, true, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc);
  check_launch("gemm_tn");
}
void HipBackend::gemm_view(int form, bool trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                           const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int64_t m_full, int64_t r0,
                           int64_t* plan8) {
  bind();
  hipk::GemmPlan p = {0, 0, 0, 0, 0, 0, 0, 0};
  if (form == 0) {
    const GemmWs ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
    gemm("gemm_view", ws, trans, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc, &p);
  } else if (form == 1) {
    const GemmWs ws = gemm_ws(hipk::gemm_syrk_workspace_doubles(l, k));
    gemm_syrk_upper("gemm_view", ws, l, k, A, lda, C, ldc, &p);
  } else if (form == 2) {
    const GemmWs ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
    gemm_trmm_upper("gemm_view", ws, m, l, k, A, lda, B, ldb, C, ldc, &p);
  } else {
    const GemmWs ws = gemm_ws(hipk::gemm_rowblock_workspace_doubles(m_full, m, l, k));
    gemm_rowblock("gemm_view", ws, m_full, r0, m, l, k, A, lda, B, ldb, C, ldc, &p);
  }
  check_launch("gemm_view");
  const int64_t out[8] = {p.nt, p.nchunks, p.xmode, p.wide, p.nsplit, p.persistent, p.grid_x, p.active};
  for (int i = 0; i < 8; ++i) plan8[i] = out[i];
}
void HipBackend::gemm_nn_gridcov(int64_t m, int64_t l, int64_t k, const double* tab, int64_t nx, int64_t ny, int64_t roff,
                                 int64_t koff, const double* B, int64_t ldb, double* C, int64_t ldc) {
  bind();
  double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k)).p;
  hipk::gemm_f64_gridcov(st_, m, l, k, tab, nx, ny, roff, koff, B, ldb, C, ldc, ws);
  check_launch("gemm_nn_gridcov");
}

// Scattered-point covariance, row-streamed: the entries are generated inside the contraction's tile loader (gemm_f64.hip
// GEN 2: 128 x 160 tiles; pointcov_gemm.hip: 96 x 320) -- nothing of A ever exists in HBM.  (Round 3's form, row panels of A
// generated into HBM on a second stream, is kept as tools/rejected_kernels/pointcov_round3_panels.hip.txt: 39 TFLOP/s
// against 59.)
void HipBackend::gemm_nn_pointcov(int64_t m, int64_t l, int64_t k, const double* pts, int d, int kind, double ell, double sigma2,
                                  double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                                  int64_t ldc) {
  bind();
  if (m <= 0 || l <= 0 || k <= 0) return;
  const int64_t npts = std::max(roff + m, koff + k);
  Scratch p4(this, (size_t)4 * npts);                  // the points as 32-byte records (x, y, z, 0): one scalar load each
  hipk::pointcov_pad_points(st_, pts, d, npts, hipk::pointcov_point_scale(kind, 1.0 / ell), p4.p);
  double* ws = gemm_ws(hipk::gemm_pointcov_workspace_doubles(m, l, k)).p;
  // the wide kernel streams a tile-ordered copy of the sketch panel (k x l doubles); memory is never a reason to fail: without
  // the copy the product runs on the 128 x 160 kernel, which reads X where it lies
  Scratch xpack(this);
  const size_t xdoubles = hipk::gemm_pointcov_pack_doubles(m, l, k);          // 0: not the wide kernel's product
  if (xdoubles > 0) xpack.try_alloc(xdoubles);
  hipk::gemm_f64_pointcov(st_, m, l, k, p4.p, npts, d, kind, sigma2, nugget, roff, koff, B, ldb, C, ldc, ws, xpack.p);
  check_launch("gemm_nn_pointcov (in-loader generator)");
}

// ---- matrix-free FFT covariance ----
struct HipBackend::FftCov {               // (W goes back before lam, on every way out)
  int64_t N[3], M[3]; Scratch lam, W; int nb_max;
  explicit FftCov(HipBackend* be) : lam(be), W(be) {}
};
// the grid squeezed of its singleton axes, its embedding, the limits, and the plan's two arrays (spectrum, work array);
// *reembed: FFTRF's exact 2 N embedding is not a power of two on some axis
std::unique_ptr<HipBackend::FftCov> HipBackend::fftcov_new_plan(const int64_t N[3], int fftrf, bool* reembed, int* dims) {
  std::unique_ptr<FftCov> p(new FftCov(this));
  int64_t Mtot = 1;
  int d = 0;
  for (int a = 0; a < 3; ++a) { p->N[a] = 1; p->M[a] = 1; }
  *reembed = false;
  for (int a = 0; a < 3; ++a) {        // squeeze singleton axes: vec() of a 1 x 50 field is a 50-point line
    if (N[a] < 1) throw Error(GSI_ERR_ARG, "fft covariance: grid dimensions must be >= 1");
    if (N[a] == 1) continue;
    p->N[d] = N[a]; p->M[d] = hipk::fft_embed_size(N[a]);
    if (fftrf && p->M[d] != 2 * N[a]) *reembed = true;
    if (p->M[d] > 8192) throw Error(GSI_ERR_ARG, "fft covariance: at most 4096 grid points per axis (a line must fit LDS)");
    Mtot *= p->M[d];
    ++d;
  }
  // element offsets inside one column pair's array are 32-bit in the pass kernels (fft_cov.hip): refuse such grids HERE, before
  // the spectrum and the work array (tens of GB) are allocated, not at the first product
  if (Mtot >= ((int64_t)1 << 31))
    throw Error(GSI_ERR_ARG, "fft covariance: the embedding grid must have fewer than 2^31 points (e.g. 1024 x 512 x 512 embeds to 2^31)");
  // work array: as many column pairs at once as fit ~2 GB, at most 64.  (GSI_FFT_W_MB: the experiment of VERDICT r4 item 7 --
  // few enough pairs per batch that the array between the passes stays in the 256 MB Infinity Cache: DESIGN.md 4.6,
  // profiles/r05_fft_pair_major.log)
  // 2-D grids whose pair array is <= 128 MB run 256 MB batches: +4 % at 1000^2 (6.57 -> 6.31 ms per 256 columns), the only
  // place the experiment moved anything; 128 MB and less lose to the shorter launches.
  static const int64_t w_env = getenv("GSI_FFT_W_MB") ? std::max<int64_t>(1, atoll(getenv("GSI_FFT_W_MB"))) : 0;
  const int64_t w_mb = w_env > 0 ? w_env : ((d == 2 && 16 * Mtot <= ((int64_t)128 << 20)) ? 256 : 2048);
  int64_t nb = (w_mb << 20) / (16 * Mtot);
  p->nb_max = (int)std::max<int64_t>(1, std::min<int64_t>(nb, 64));
  p->lam.adopt(alloc(hipk::fft_plan_doubles(p->M)));
  p->W.adopt(alloc((size_t)2 * Mtot * p->nb_max));
  *dims = d;
  return p;
}
// One per-axis factor of the re-embedding, applied to the FASTEST axis of the array in bufh (dimensions cur, tot elements,
// d real axes) as cur' = cur^T B (the contraction kernel's A'B form: the array as a k x rest matrix), which also rotates
// that axis to the back: d applications restore the natural order.
void HipBackend::fft_rotate_apply(Scratch& buf, int64_t cur[3], int64_t& tot, int d, int64_t rows_out, int64_t period, FftFactor f) {
  // cur = (k, rest) column-major; B = k x rows_out; result (rest x rows_out) = the array with axis 0 replaced and last
  const int64_t k = cur[0], rest = (tot / k);
  Scratch B(this, (size_t)k * rows_out);
  // B[kk + t k] : weighted (the D and S factors) is indexed [t = row of the INPUT, k' = output]; unweighted [k, t]
  if (f == FFT_F_COS) hipk::fft_cos_matrix(st_, B.p, k, rows_out, period, false);              // C_a^T: B[k, t]
  else if (f == FFT_F_COS_WEIGHTED) hipk::fft_cos_matrix(st_, B.p, k, rows_out, period, true);  // D_a^T: B[t, k'] = w_t cos(.)
  else hipk::fft_sin_matrix(st_, B.p, k, rows_out, period);                                   // S_a^T: B[t, k'] = w_t sin(.)
  Scratch out(this, (size_t)rest * rows_out);
  const GemmWs ws = gemm_ws(hipk::gemm_workspace_doubles(rest, rows_out, k));
  gemm("fft_rotate_apply", ws, true, rest, rows_out, k, 1.0, buf.p, k, B.p, k, 0.0, out.p, rest);
  check_launch("fft re-embedding product");
  release(buf.give_up());
  buf.adopt(out.give_up());
  tot = rest * rows_out;
  // rotate the dimension list: (k, c1, c2) -> (c1, c2, rows_out) over the d real axes
  int64_t nd[3] = {1, 1, 1};
  for (int a = 0; a + 1 < d; ++a) nd[a] = cur[a + 1];
  nd[d - 1] = rows_out;
  for (int a = 0; a < 3; ++a) cur[a] = nd[a];
}
// The second half of the re-embedding, shared by the power-law and the covariance-function plans: the lags of a kernel over
// the box (bufh: N[0] x N[1] x N[2], natural order) -> (x_a D_a) c on the power-of-two embedding M, natural order; with
// sine = true (x_a S_a) c, the odd-odd part of a centrally symmetric 2-D kernel.
void HipBackend::fftcov_lags_to_spectrum(Scratch& bufh, int64_t cur[3], int64_t& tot, const FftCov* p, int d, bool sine) {
  for (int a = 0; a < d; ++a) fft_rotate_apply(bufh, cur, tot, d, p->M[a], p->M[a], sine ? FFT_F_SIN_WEIGHTED : FFT_F_COS_WEIGHTED);
}
void* HipBackend::fftcov_create(const int64_t N[3], double beta, int fftrf) {
  bind();
  bool reembed = false;
  int d = 0;
  std::unique_ptr<FftCov> p = fftcov_new_plan(N, fftrf, &reembed, &d);
  const int64_t Mtot = p->M[0] * p->M[1] * p->M[2];
  if (!reembed) {
    hipk::fft_spectrum(st_, p->lam.p, p->lam.p + Mtot, p->M, beta, fftrf);
    check_launch("fft_spectrum");
    return p.release();
  }
  // FFTRF's convention on an arbitrary grid (FFTRF.jl:83-90 embeds on exactly 2 N points for ANY N): the same matrix
  // through the power-of-two passes with a re-embedded spectrum (fft_cov.hip, "FFTRF's convention on a grid ...").
  //   c  = (x_a C_a) lambda_{2N}    C_a[t, k]  = cos(2 pi t k / 2 N_a),            t < N_a, k < 2 N_a     (lags 0 .. N_a - 1)
  //   l' = (x_a D_a) c              D_a[k', t] = w_t cos(2 pi t k' / M'_a), w_0 = 1, w_t = 2              (c' even, 0 beyond)
  int64_t cur[3] = {1, 1, 1};
  for (int a = 0; a < d; ++a) cur[a] = 2 * p->N[a];
  int64_t tot = cur[0] * cur[1] * cur[2];
  Scratch bufh(this, (size_t)tot);
  hipk::fft_spectrum_natural(st_, bufh.p, cur, beta, 1);
  for (int a = 0; a < d; ++a) fft_rotate_apply(bufh, cur, tot, d, p->N[a], 2 * p->N[a], FFT_F_COS);   // lags 0 .. N_a - 1 of c
  fftcov_lags_to_spectrum(bufh, cur, tot, p.get(), d, false);              // the spectrum of the re-embedded kernel
  hipk::fft_lines_layout(st_, bufh.p, p->lam.p, p->M);
  hipk::fft_finish_plan(st_, p->lam.p, p->lam.p + Mtot, p->M);
  check_launch("fft re-embedded spectrum");
  return p.release();
}
// The same operator type for a covariance FUNCTION of the grid lags (gsi_op_fft_gridcov[_table]):
//   lambda' = (x_a D_a) c                              kernels even along every axis
//   lambda' = (D_0 x D_1) c_ee - (S_0 x S_1) c_oo      centrally symmetric 2-D kernels (cos(a + b) = cos a cos b - sin a sin b;
//                                                      c_ee, c_oo = half the sum / difference of the lags (t0, t1), (t0, -t1))
// stored as (lambda' + nugget) / Mtot: no unit diagonal, and nugget * I on the box exactly.
void* HipBackend::fftcov_create_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, double nugget,
                                     const double* table, const double* table_mirror) {
  return fftcov_plan_of_lags(N, kind, ell, theta, sigma2, nugget, table, table_mirror, -1);
}
// The derivative of that covariance with respect to one parameter (gsi_op_fft_gridcov_deriv): the same plan
// from the derivative's lags (fft_lag_table_deriv).  d / d nugget = I: zero lags and a unit shift of the spectrum.  The
// derivative with respect to theta is odd along each axis even at theta = 0, so it always takes the second quadrant.
void* HipBackend::fftcov_create_lags_deriv(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, int param) {
  return fftcov_plan_of_lags(N, kind, ell, theta, sigma2, param == pointcov::D_NUGGET ? 1.0 : 0.0, nullptr, nullptr, param);
}
void* HipBackend::fftcov_plan_of_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, double nugget,
                                      const double* table, const double* table_mirror, int dparam) {
  bind();
  bool reembed = false;
  int d = 0;
  std::unique_ptr<FftCov> p = fftcov_new_plan(N, 0, &reembed, &d);
  int64_t cur[3] = {p->N[0], p->N[1], p->N[2]};      // singleton axes do not move an element of the lag table
  int64_t tot = cur[0] * cur[1] * cur[2];
  // a second quadrant only where it differs from the first: both axes of a 2-D grid longer than one point
  const bool mirrored = (table ? table_mirror != nullptr : (theta != 0.0 || dparam == pointcov::D_THETA)) && d == 2 && N[2] == 1;
  Scratch cp(this, (size_t)tot), cm(this, mirrored ? (size_t)tot : 0);
  if (table) {
    upload2d(cp.p, tot, table, tot, tot, 1);
    if (mirrored) upload2d(cm.p, tot, table_mirror, tot, tot, 1);
  } else {
    const double inv_ell[3] = {1.0 / ell[0], 1.0 / ell[1], 1.0 / ell[2]};
    if (dparam < 0) hipk::fft_lag_table(st_, cp.p, cm.p, N, kind, inv_ell, std::cos(theta), std::sin(theta), sigma2);
    else hipk::fft_lag_table_deriv(st_, cp.p, cm.p, N, kind, dparam, inv_ell, std::cos(theta), std::sin(theta), sigma2);
    check_launch("fft_lag_table");
  }
  if (mirrored) {
    hipk::fft_even_odd_split(st_, cp.p, cm.p, tot);
    int64_t cur_s[3] = {cur[0], cur[1], cur[2]};
    int64_t tot_s = tot;
    fftcov_lags_to_spectrum(cm, cur_s, tot_s, p.get(), d, true);
  }
  fftcov_lags_to_spectrum(cp, cur, tot, p.get(), d, false);
  if (mirrored) hipk::fft_subtract(st_, cp.p, cm.p, tot);
  hipk::fft_lines_layout(st_, cp.p, p->lam.p, p->M);
  hipk::fft_finish_plan_lags(st_, p->lam.p, p->M, nugget);
  check_launch("fft covariance-function spectrum");
  return p.release();
}
void HipBackend::fftcov_destroy(void* plan) {
  delete static_cast<FftCov*>(plan);
}
void HipBackend::fftcov_apply(void* plan, int64_t l, const double* X, int64_t ldx, double* Y, int64_t ldy) {
  bind();
  FftCov* p = static_cast<FftCov*>(plan);
  hipk::fft_cov_apply(st_, p->N, p->M, p->lam.p, reinterpret_cast<double2*>(p->W.p), p->nb_max, l, X, ldx, Y, ldy);
  check_launch("fft_cov_apply");
}

// ---- generators ----
void HipBackend::center_rows(double* S, int64_t n, int64_t N, int64_t ld) {
  bind();
  hipk::center_rows(st_, S, n, N, ld);
}
void HipBackend::randn(double* p, size_t count, uint64_t seed) {
  bind();
  hipk::randn_fill(st_, p, count, seed);
}
void HipBackend::fill_gridcov(double* A, int64_t lda, int64_t nx, int64_t ny, double ell, int kind, int64_t row0,
                              int64_t mloc) {
  bind();
  hipk::fill_gridcov(st_, A, lda, nx, ny, ell, kind, row0, mloc);
  check_launch("fill_gridcov");
}
void HipBackend::fill_lowrank_samples(double* S, int64_t ld, int64_t nloc, int64_t N, int64_t row0, uint64_t seed,
                                      double decay) {
  bind();
  hipk::fill_lowrank_samples(st_, S, ld, nloc, N, row0, seed, decay);
  check_launch("fill_lowrank_samples");
}
// Batches of fields: phi and the intermediate array of a batch stay within 2 GiB of workspace (GSI_FFTRF_BATCH=<b>, read
// at every call, overrides the batch size).  Nothing a field computes depends on the batch it rides in.
void HipBackend::fftrf_fields(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                              double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0) {
  fftrf_batches(dst, ldd, row0, nloc, nf, ndims, N, k0, dk, beta, phi, ldphi, seed, field0, nullptr);
}
// The same batches, each field interpolated at the plan's points (fftrf_interp.hip) instead of copied out: the
// normalising write goes to the field's own workspace (over its phi, dead after the first pass) and the gather reads it
// there.  dst is plan.m_local x nf.
void HipBackend::fftrf_fields_at(double* dst, int64_t ldd, int64_t nf, int ndims, const int64_t* N, double k0, double dk, double beta,
                                 const double* phi, int64_t ldphi, uint64_t seed, int64_t field0, const FftrfPointsPlan& plan) {
  fftrf_batches(dst, ldd, 0, 0, nf, ndims, N, k0, dk, beta, phi, ldphi, seed, field0, &plan);
}
void HipBackend::fftrf_interpolate(double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg,
                                   const FftrfPointsPlan& plan) {
  bind();
  if (nf <= 0 || plan.m_local <= 0) return;
  Scratch dplan(this, points_plan_doubles(plan));
  upload_points_plan(plan, dplan.p);
  for (int64_t f0 = 0; f0 < nf; f0 += 4096) {
    const int b = (int)((nf - f0 < 4096) ? (nf - f0) : 4096);
    interp_batch(plan, dplan.p, grid + f0 * ldg, ldg, b, dst + f0 * ldd, ldd);
  }
}
// the plan on the device: frac (ndims x m_local doubles), then base (m_local int32)
size_t HipBackend::points_plan_doubles(const FftrfPointsPlan& plan) {
  return (size_t)plan.m_local * plan.ndims + (size_t)(plan.m_local + 1) / 2;
}
void HipBackend::upload_points_plan(const FftrfPointsPlan& plan, double* d) {
  const int64_t m = plan.m_local, nfr = m * plan.ndims;
  upload2d(d, nfr, plan.frac.data(), nfr, nfr, 1);
  std::vector<double> packed((size_t)(m + 1) / 2, 0.0);
  std::memcpy(packed.data(), plan.base.data(), sizeof(int32_t) * (size_t)m);
  upload2d(d + nfr, (int64_t)packed.size(), packed.data(), (int64_t)packed.size(), (int64_t)packed.size(), 1);
}
void HipBackend::interp_batch(const FftrfPointsPlan& plan, const double* dplan, const double* V, int64_t v_fs, int nb, double* dst,
                              int64_t ldd) {
  const int64_t m = plan.m_local;
  hipk::fftrf_interp(st_, plan.ndims, reinterpret_cast<const int32_t*>(dplan + m * plan.ndims), dplan, m, plan.N[0],
                     plan.N[0] * plan.N[1], V, v_fs, nb, dst, ldd);
  check_launch("fftrf_interp");
}
// ---- a points plan resident in HBM: the forward plan and its inverted index (interp_adjoint_plan.hpp), one allocation ----
struct HipBackend::PointsAt {
  Scratch mem;
  int ndims = 0;
  int64_t N[3] = {1, 1, 1}, m = 0, n = 0;
  const double* frac = nullptr;
  const int32_t* base = nullptr;
  hipk::IadjDev dev{};
  explicit PointsAt(HipBackend* be) : mem(be) {}
};
void* HipBackend::points_at_create(const FftrfPointsPlan& plan, int64_t info[4]) {
  bind();
  const InterpAdjointPlan ip = interp_adjoint_plan(plan);
  const int64_t m = plan.m_local, nc = (int64_t)1 << plan.ndims;
  auto words = [](size_t bytes) { return (bytes + 7) / 8; };
  Carve cv;
  const size_t o_frac = cv.take((size_t)m * plan.ndims), o_base = cv.take(words(4 * (size_t)m)),
               o_ptr = cv.take((size_t)ip.n + 1), o_point = cv.take(words(4 * (size_t)(nc * m))),
               o_corner = cv.take(words((size_t)(nc * m))), o_lnode = cv.take(words(4 * (size_t)ip.nlong())),
               o_lchunk = cv.take((size_t)ip.nlong() + 1), o_coff = cv.take((size_t)ip.nchunk()),
               o_clen = cv.packed(words(4 * (size_t)ip.nchunk()));
  std::unique_ptr<PointsAt> at(new PointsAt(this));
  double* d = at->mem.p = alloc(cv.total);
  std::vector<double> packed;
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes == 0) return;
    packed.assign(words(bytes), 0.0);
    std::memcpy(packed.data(), src, bytes);
    upload2d(d + off, (int64_t)packed.size(), packed.data(), (int64_t)packed.size(), (int64_t)packed.size(), 1);
  };
  put(o_frac, plan.frac.data(), 8 * (size_t)m * plan.ndims);
  put(o_base, plan.base.data(), 4 * (size_t)m);
  put(o_ptr, ip.nodeptr.data(), 8 * ((size_t)ip.n + 1));
  put(o_point, ip.point.data(), 4 * (size_t)(nc * m));
  put(o_corner, ip.corner.data(), (size_t)(nc * m));
  put(o_lnode, ip.long_node.data(), 4 * (size_t)ip.nlong());
  put(o_lchunk, ip.long_chunk0.data(), 8 * ((size_t)ip.nlong() + 1));
  put(o_coff, ip.chunk_off.data(), 8 * (size_t)ip.nchunk());
  put(o_clen, ip.chunk_len.data(), 4 * (size_t)ip.nchunk());
  at->ndims = plan.ndims;
  for (int a = 0; a < 3; ++a) at->N[a] = plan.N[a];
  at->m = m; at->n = ip.n;
  at->frac = d + o_frac;
  at->base = reinterpret_cast<const int32_t*>(d + o_base);
  hipk::IadjDev& v = at->dev;
  v.d = plan.ndims; v.n = ip.n; v.m = m; v.chunk = ip.chunk; v.nlong = ip.nlong(); v.nchunk = ip.nchunk();
  v.nodeptr = reinterpret_cast<const int64_t*>(d + o_ptr);
  v.point = reinterpret_cast<const int32_t*>(d + o_point);
  v.corner = reinterpret_cast<const uint8_t*>(d + o_corner);
  v.frac = at->frac;
  v.long_node = reinterpret_cast<const int32_t*>(d + o_lnode);
  v.long_chunk0 = reinterpret_cast<const int64_t*>(d + o_lchunk);
  v.chunk_off = reinterpret_cast<const int64_t*>(d + o_coff);
  v.chunk_len = reinterpret_cast<const int32_t*>(d + o_clen);
  if (info) { info[0] = (int64_t)(8 * cv.total); info[1] = ip.nlong(); info[2] = ip.nchunk(); info[3] = ip.maxlen; }
  return at.release();
}
void HipBackend::points_at_destroy(void* at) {
  delete static_cast<PointsAt*>(at);
}
void HipBackend::points_at_gather(void* at_, double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg) {
  bind();
  const PointsAt* at = static_cast<const PointsAt*>(at_);
  if (nf <= 0 || at->m <= 0) return;
  for (int64_t f0 = 0; f0 < nf; f0 += 4096) {
    const int b = (int)((nf - f0 < 4096) ? (nf - f0) : 4096);
    hipk::fftrf_interp(st_, at->ndims, at->base, at->frac, at->m, at->N[0], at->N[0] * at->N[1], grid + f0 * ldg, ldg, b,
                       dst + f0 * ldd, ldd);
  }
  check_launch("fftrf_interp");
}
// The column groups of interp_adjoint.hip ride in blockIdx.y: 4096 columns per launch stay far below its limit.  The chunk
// sums of the long nodes live in a pooled temporary of nchunk x (columns of the launch).
void HipBackend::points_at_spread(void* at_, double* grid, int64_t ldg, int64_t nf, const double* src, int64_t lds) {
  bind();
  const PointsAt* at = static_cast<const PointsAt*>(at_);
  if (nf <= 0) return;
  const int64_t step = nf < 4096 ? nf : 4096;
  Scratch partial(this, (size_t)at->dev.nchunk * (size_t)step);
  for (int64_t f0 = 0; f0 < nf; f0 += step) {
    const int64_t b = (nf - f0 < step) ? (nf - f0) : step;
    hipk::interp_adjoint(st_, at->dev, src + f0 * lds, lds, b, grid + f0 * ldg, ldg, partial.p);
  }
  check_launch("interp_adjoint");
}
void HipBackend::fftrf_batches(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                               double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0,
                               const FftrfPointsPlan* at) {
  bind();
  if (nf <= 0 || (at && at->m_local <= 0)) return;
  hipk::FftrfGeom g;
  hipk::fftrf_geometry(ndims, N, &g);
  int64_t fs = (int64_t)hipk::fftrf_field_doubles(g);
  fs += fs & 1;                                     // the complex array of every field 16-byte aligned
  int64_t nb = (((int64_t)2 << 30) / (int64_t)sizeof(double)) / fs;
  if (const char* e = getenv("GSI_FFTRF_BATCH")) { if (atoll(e) >= 1) nb = atoll(e); }
  if (nb > 4096) nb = 4096;
  if (nb > nf) nb = nf;
  if (nb < 1) nb = 1;
  Scratch plan(this, hipk::fftrf_plan_doubles(g)), ws(this, (size_t)(fs * nb));
  Scratch dplan(this, at ? points_plan_doubles(*at) : 0);
  if (at) upload_points_plan(*at, dplan.p);
  hipk::fftrf_plan(st_, g, plan.p);
  for (int64_t f0 = 0; f0 < nf; f0 += nb) {
    const int b = (int)((nf - f0 < nb) ? (nf - f0) : nb);
    if (phi) {
      if (f0 > 0) HIP_CHECK(hipStreamSynchronize(st_));      // the previous batch still reads the workspace
      upload2d(ws.p, fs, phi + f0 * ldphi, ldphi, g.Mtot, b);
    } else {
      for (int i = 0; i < b; ++i) hipk::randn_fill(st_, ws.p + (int64_t)i * fs, (size_t)g.Mtot, seed + (uint64_t)(field0 + f0 + i));
    }
    if (!at) {
      hipk::fftrf_sample(st_, g, plan.p, ws.p, fs, b, k0, dk, beta, dst + f0 * ldd, ldd, row0, nloc);
      check_launch("fftrf_sample");
    } else {
      hipk::fftrf_sample(st_, g, plan.p, ws.p, fs, b, k0, dk, beta, ws.p, fs, 0, g.n);   // field i: ws + i fs, n values
      check_launch("fftrf_sample");
      interp_batch(*at, dplan.p, ws.p, fs, b, dst + f0 * ldd, ldd);
    }
  }
}

}  // namespace gsi
