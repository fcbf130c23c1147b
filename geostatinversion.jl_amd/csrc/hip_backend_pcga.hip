// hip_backend_pcga.hip -- HipBackend's solver side: column norms, the BLAS-1/2 helpers, the LSQR steps, and what the PCGA
// consumers (pcga.cpp) run on the device: the parameter products, the sparse forward model, the saddle-point solve, the
// posterior variance's row pass.
#include <cmath>
#include <cstdlib>
#include "hip_backend_impl.hpp"

namespace gsi {

void HipBackend::colnorms(const double* Y, int64_t m, int64_t c, int64_t ld, double* host_out) {
  bind();
  if (c > 64) throw Error(GSI_ERR_ARG, "colnorms: at most 64 columns at a time");
  hipk::colnorms_sq(st_, Y, m, c, ld, scal_);
  HIP_CHECK(hipMemcpyAsync(host_out, scal_, sizeof(double) * c, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  for (int64_t i = 0; i < c; ++i) host_out[i] = std::sqrt(host_out[i]);
}
void HipBackend::axpy(int64_t n, double a, const double* x, double* y) { bind(); hipk::axpy(st_, n, a, x, y); }
double HipBackend::dot(int64_t n, const double* x, const double* y) {
  bind();
  hipk::dot_dev(st_, n, x, y, scal_);
  double v = 0.0;
  HIP_CHECK(hipMemcpyAsync(&v, scal_, sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  return v;
}
double HipBackend::nrm2(int64_t n, const double* x) { return std::sqrt(dot(n, x, x)); }
void HipBackend::scal_copy(int64_t n, double a, const double* x, double* y) {
  bind();
  hipk::scal_copy(st_, n, a, x, y);
}
void HipBackend::pcga_params(const double* Z, int64_t n, int64_t K, const double* s, const double* X, double delta,
                             double* out) {
  bind();
  hipk::pcga_params(st_, Z, n, K, s, X, delta, out);
  check_launch("pcga_params");
}
void HipBackend::gemv_n(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double beta,
                        double* y) {
  bind();
  hipk::gemv_n(st_, m, k, alpha, A, lda, x, beta, y);
  check_launch("gemv_n");
}
void HipBackend::gemv_t(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double* y) {
  bind();
  grow(ws_blas2_, sizeof(double) * hipk::gemv_t_workspace_doubles(k));
  hipk::gemv_t(st_, m, k, alpha, A, lda, x, y, (double*)ws_blas2_.p);
  check_launch("gemv_t");
}
void HipBackend::project_out(int64_t m, int64_t ncols, const double* q, double* Y, int64_t ld) {
  bind();
  if (ncols > 64) throw Error(GSI_ERR_ARG, "project_out: at most 64 columns at a time");
  grow(ws_blas2_, sizeof(double) * hipk::gemv_t_workspace_doubles(ncols));
  hipk::project_out(st_, m, ncols, q, Y, ld, (double*)ws_blas2_.p);
  check_launch("project_out");
}
void HipBackend::scal(int64_t n, double a, double* x) { bind(); hipk::scal(st_, n, a, x); }
void HipBackend::diag_mul_add(int64_t n, const double* d, const double* x, double* y) {
  bind();
  hipk::diag_mul_add(st_, n, d, x, y);
}
void HipBackend::lsqr_begin(int64_t n, const double* w, double* work) {
  bind();
  hipk::lsqr_begin(st_, n, w, work);
  check_launch("lsqr_begin");
}
void HipBackend::lsqr_step_u(int64_t m, const double* t, double* u, double* work) {
  bind();
  hipk::lsqr_step_u(st_, m, t, u, work);
  check_launch("lsqr_step_u");
}
void HipBackend::lsqr_step_v(int64_t n, const double* t, double* v, double* w, double* x, double* work) {
  bind();
  hipk::lsqr_step_v(st_, n, t, v, w, x, work);
  check_launch("lsqr_step_v");
}
void HipBackend::block_cg_begin(int64_t n, int64_t b, const double* B, double tol, int64_t maxiter, double* work) {
  bind();
  hipk::block_cg_begin(st_, n, b, B, tol, maxiter, work);
  check_launch("block_cg_begin");
}
void HipBackend::block_cg_step(int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R, double* P,
                               double* work) {
  bind();
  hipk::block_cg_step(st_, n, b, Q, d, X, R, P, work);
  check_launch("block_cg_step");
}
// The preconditioned solver (block_pcg.hip): z = e .* r - W (W'r) is the two contraction launchers
// on all b columns between the panel passes.
void HipBackend::block_pcg_begin(int64_t n, int64_t b, int64_t K, const double* B, const double* e, const double* W, double* S,
                                 double* Y, double* P, double tol, int64_t maxiter, double* work) {
  bind();
  gemm_tn(K, b, n, 1.0, W, n, B, n, 0.0, S, K);
  gemm_nn(n, b, K, 1.0, W, n, S, K, 0.0, Y, n);
  hipk::block_pcg_begin(st_, n, b, B, e, Y, P, tol, maxiter, work);
  check_launch("block_pcg_begin");
}
void HipBackend::block_pcg_step(int64_t n, int64_t b, int64_t K, const double* Q, const double* d, const double* e,
                                const double* W, double* X, double* R, double* P, double* S, double* Y, double* work) {
  bind();
  hipk::block_pcg_step_xr(st_, n, b, Q, d, X, R, P, work);
  check_launch("block_pcg_step: passes 1 and 2");
  gemm_tn(K, b, n, 1.0, W, n, R, n, 0.0, S, K);
  gemm_nn(n, b, K, 1.0, W, n, S, K, 0.0, Y, n);
  hipk::block_pcg_step_p(st_, n, b, e, R, Y, P, work);
  check_launch("block_pcg_step: pass 3");
}
int HipBackend::precond_rows(int64_t n, double* e, double* sqe) {
  bind();
  hipk::pcg_precond_rows(st_, n, e, sqe);
  check_launch("precond_rows");
  return 1;
}
int HipBackend::add_identity(double* C, int64_t K) {
  bind();
  hipk::pcg_add_identity(st_, C, K);
  check_launch("add_identity");
  return 1;
}
// The coefficient trace and its quadrature (block_slq.hip)
void HipBackend::cg_trace_begin(const double* work, double* tr, int64_t qmax) {
  bind();
  hipk::slq_trace_begin(st_, work, tr, qmax);
  check_launch("cg_trace_begin");
}
void HipBackend::cg_trace_step(const double* work, double* tr, int64_t qmax) {
  bind();
  hipk::slq_trace_step(st_, work, tr, qmax);
  check_launch("cg_trace_step");
}
int HipBackend::slq_quadrature(const double* alpha, const double* beta, const double* steps, const double* rho0, int64_t qmax,
                               int64_t b, double* work, double* out) {
  bind();
  hipk::slq_quadrature(st_, alpha, beta, steps, rho0, qmax, b, work, out);
  check_launch("slq_quadrature");
  return 1;
}
int HipBackend::precond_sample_rows(int64_t n, int64_t b, const double* e, const double* Y, const double* G2, double* Zout) {
  bind();
  hipk::slq_sample_rows(st_, n, b, e, Y, G2, Zout);
  check_launch("precond_sample_rows");
  return 1;
}
// Diagonal-pivoted Cholesky (pivoted_chol.hip).  The scattered-point form keeps the points as the
// generator's pre-scaled 32-byte records inside `work`, made once by pchol_begin.
static hipk::PcholCol pchol_col(const Backend::PcholSource& a, double* work, int64_t n, int64_t K) {
  hipk::PcholCol c;
  c.form = a.form; c.a = a.data; c.ld = a.ld; c.ny = (int32_t)a.gy;
  c.dim = a.pc_d; c.kind = a.pc_kind; c.sigma2 = a.pc_sigma2; c.nugget = a.pc_nugget;
  if (a.form == 3) c.a = hipk::pchol_points(work, n, K);
  return c;
}
void HipBackend::pchol_begin(const PcholSource& a, int64_t n, int64_t K, double tol, const double* L, int64_t ldl, double* d,
                             double* work) {
  bind();
  if (a.form == 3)
    hipk::pointcov_pad_points(st_, a.data, a.pc_d, n, hipk::pointcov_point_scale(a.pc_kind, 1.0 / a.pc_ell),
                              hipk::pchol_points(work, n, K));
  hipk::pchol_begin(st_, pchol_col(a, work, n, K), n, K, tol, L, ldl, d, work);
  check_launch("pchol_begin");
}
void HipBackend::pchol_step(const PcholSource& a, int64_t n, int64_t K, double* L, int64_t ldl, double* d, double* work) {
  bind();
  hipk::pchol_step(st_, pchol_col(a, work, n, K), n, K, L, ldl, d, work);
  check_launch("pchol_step");
}
int HipBackend::scale_cols(int64_t n, int64_t K, double* U, int64_t ldu, const double* S) {
  bind();
  hipk::scale_cols(st_, n, K, U, ldu, S);
  check_launch("scale_cols");
  return 1;
}
void HipBackend::f64_to_f32(const double* src, void* dst32, size_t count) {
  bind();
  hipk::f64_to_f32(st_, src, (float*)dst32, count);
  check_launch("f64_to_f32");
}
void HipBackend::pcga_params_f32(const void* Z32, int64_t n, int64_t K, const double* s, const double* X, double delta,
                                 double* out) {
  bind();
  hipk::pcga_params_f32(st_, (const float*)Z32, n, K, s, X, delta, out);
  check_launch("pcga_params_f32");
}
void HipBackend::basis_gemv_f32(const void* Z32, int64_t n, int64_t K, const double* w, double beta, const double* X,
                                double* y) {
  bind();
  if (K > 8000) throw Error(GSI_ERR_ARG, "basis_gemv_f32: K too large for the LDS-resident weights");
  hipk::basis_gemv_f32(st_, (const float*)Z32, n, K, w, beta, X, y);
  check_launch("basis_gemv_f32");
}
// The sparse forward model (pcga_forward.hip).  The form follows the mean segment length: FWD_WAVE_MIN nonzeros and more
// go one wave per segment, shorter ones one lane per output (the crossover of the sweep in profiles/pcga_forward.json:
// 4096 rays of 16 cells run 0.65 ms in the wave form against 0.83 ms, rays of 4 cells 0.66 against 0.62;
// DESIGN.md section 4.7b).  GSI_FWD_FORM=lane|wave, read at every call, overrides.
static constexpr int64_t FWD_WAVE_MIN = 16;
int HipBackend::fwd_products(const FwdProduct& a) {
  bind();
  int form = (a.nseg > 0 && a.nnz / a.nseg >= FWD_WAVE_MIN) ? 2 : 1;
  if (const char* e = getenv("GSI_FWD_FORM")) {
    const std::string f(e);
    if (f == "lane") form = 1;
    else if (f == "wave") form = 2;
    else if (!f.empty()) throw Error(GSI_ERR_ARG, "GSI_FWD_FORM must be lane or wave, not '" + f + "'");
  }
  if (form == 1) hipk::fwd_lane(st_, a);
  else hipk::fwd_wave(st_, a);
  check_launch(form == 1 ? "fwd_lane" : "fwd_wave");
  if (a.rowseg) {
    hipk::fwd_reduce(st_, a);
    check_launch("fwd_reduce");
  }
  return form;
}

// The adjoint of the forward model (fwd_adjoint.hip): FADJ_MAX_COLS columns per launch; the chunk sums of the long columns
// live in a pooled temporary of nchunk x (columns of the launch) unless the caller brought one.
int HipBackend::fwd_adjoint(const FwdAdjoint& a) {
  bind();
  if (a.b <= 0 || a.n <= 0) return 1;
  const int64_t step = a.b < hipk::FADJ_MAX_COLS ? a.b : hipk::FADJ_MAX_COLS;
  Scratch partial(this, a.partial ? 0 : (size_t)a.nchunk * (size_t)step);
  for (int64_t f0 = 0; f0 < a.b; f0 += step) {
    FwdAdjoint s = a;
    s.b = (a.b - f0 < step) ? (a.b - f0) : step;
    s.V = a.V + f0 * a.ldv;
    s.G = a.G + f0 * a.ldg;
    s.partial = a.partial ? a.partial + f0 * a.nchunk : partial.p;
    hipk::fwd_adjoint(st_, s);
  }
  check_launch("fwd_adjoint");
  return 1;
}

// The blocked Cholesky and the saddle-point solve (chol_saddle.hip).  The pivot flag has a slot
// of its own behind the error words: the caller gets the column as a return value, not through take_error.
int64_t HipBackend::chol_lower(double* A, int64_t m, int64_t n, int64_t ld) {
  bind();
  if (n < 1 || m < n || ld < m || n >= ((int64_t)1 << 31)) throw Error(GSI_ERR_ARG, "chol_lower: need 1 <= n <= m <= ld, n < 2^31");
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOL_LOWER, 0, sizeof(int32_t), st_));
  hipk::cs_chol_lower(st_, A, m, n, ld, flags_ + FLAG_CHOL_LOWER);
  check_launch("chol_lower");
  return read_flag(FLAG_CHOL_LOWER);
}
int64_t HipBackend::saddle_solve(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag, const double* b,
                                 double* x, bool* singular) {
  bind();
  const int64_t ld = nobs + 2;
  Scratch W(this, (size_t)ld * nobs);
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOL_LOWER, 0, sizeof(int32_t), st_));
  phase_begin(PH_SMALL_GEMM);                              // (profiling: the formation counts as a small product ...
  hipk::cs_syrk_lower(st_, W.p, ld, nobs, nobs, E, nobs, K, 1.0, 0.0, R, nobs, r_diag ? 2 : 1, flags_ + FLAG_CHOL_LOWER);
  hipk::cs_set_rows(st_, W.p, ld, nobs, HX, b);
  phase_end(PH_SMALL_GEMM);
  phase_begin(PH_OTHER);                                   // ... the factorization as "other": tools/pcga_direct_bench.py)
  hipk::cs_chol_lower(st_, W.p, nobs + 2, nobs, ld, flags_ + FLAG_CHOL_LOWER);
  phase_end(PH_OTHER);
  check_launch("saddle_solve: factorization");
  const int64_t col = read_flag(FLAG_CHOL_LOWER);
  *singular = false;
  if (col != 0) return col;
  hipk::cs_schur(st_, W.p, ld, nobs, b, x, scal_);
  grow(ws_blas2_, sizeof(double) * hipk::cs_backsolve_workspace_doubles());
  hipk::cs_backsolve(st_, W.p, nobs, ld, x, (double*)ws_blas2_.p);
  check_launch("saddle_solve: substitution");
  double out3[3] = {0.0, 0.0, 0.0};
  HIP_CHECK(hipMemcpyAsync(out3, scal_, sizeof(out3), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  *singular = (out3[2] == 0.0);
  return 0;
}

// The row pass of the posterior variance (posterior_var.hip).
int HipBackend::basis_quadform(const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw, int64_t ncols,
                               bool upper, const double* u, double* a, double* q, double* t) {
  bind();
  if (n < 1 || K < 1 || ncols < 1 || ldz < n || ldw < K || (zbits != 64 && zbits != 32) || (u == nullptr) != (t == nullptr))
    throw Error(GSI_ERR_ARG, "basis_quadform: need n, K, ncols >= 1, ldz >= n, ldw >= K, 32 or 64 bits, u and t together");
  hipk::pv_quadform(st_, Z, zbits, n, ldz, K, W, ldw, ncols, upper, u, a, q, t);
  check_launch("basis_quadform");
  return 1;
}
int HipBackend::scale_rows(int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst, int64_t ldd) {
  bind();
  hipk::pv_scale_rows(st_, m, c, d, src, lds, dst, ldd);
  check_launch("scale_rows");
  return 1;
}

// The row pass and the trapezoid's carried rows of the exact posterior variance (posterior_exact.hip).
int HipBackend::rowdot_acc(int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc) {
  bind();
  if (n < 1 || b < 1 || lda < n || ldb < n || A == nullptr || B == nullptr || acc == nullptr)
    throw Error(GSI_ERR_ARG, "rowdot_acc: need n, b >= 1, lda, ldb >= n and no NULL operand");
  hipk::px_rowdot_acc(st_, n, b, A, lda, B, ldb, acc);
  check_launch("rowdot_acc");
  return 1;
}
int HipBackend::unit_panel(double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) {
  bind();
  if (nobs < 1 || b < 1 || ld < nobs || c0 < 0) throw Error(GSI_ERR_ARG, "unit_panel: need nobs, b >= 1, ld >= nobs, c0 >= 0");
  hipk::px_unit_panel(st_, E, ld, nobs, b, c0);
  check_launch("unit_panel");
  return 1;
}
int HipBackend::trapezoid_rows(double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi,
                               int64_t ldphi) {
  bind();
  if (nobs < 1 || p < 0 || ld < 2 * nobs + p || (p > 0 && (Phi == nullptr || ldphi < nobs)))
    throw Error(GSI_ERR_ARG, "trapezoid_rows: need nobs >= 1, p >= 0, ld >= 2 nobs + p, Phi (ld >= nobs) when p > 0");
  hipk::px_trapezoid_rows(st_, T, ld, nobs, p, diag, Phi, ldphi);
  check_launch("trapezoid_rows");
  return 1;
}
int HipBackend::carried_rows(const double* T, int64_t ld, int64_t nobs, int64_t p, double* Wd) {
  bind();
  if (nobs < 1 || p < 0 || ld < 2 * nobs + p || (p > 0 && Wd == nullptr))
    throw Error(GSI_ERR_ARG, "carried_rows: need nobs >= 1, p >= 0, ld >= 2 nobs + p, Wd when p > 0");
  hipk::px_carried_rows(st_, T, ld, nobs, p, Wd);
  check_launch("carried_rows");
  return 1;
}

// The bilinear forms of the likelihood gradient (bilinear_terms.hip): per-chunk partial sums and their
// ordered sum on the device, g g + b - g doubles back to the host.
int HipBackend::bilinear_terms(int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R, const double* dd,
                               double* gram, double* t) {
  bind();
  if (n < 1 || b < 1 || g < 0 || g > b || g > 16 || b - g > (int64_t)32 * 65534 || L == nullptr || Y == nullptr ||
      (dd != nullptr && R == nullptr) || (g > 0 && gram == nullptr) || (b > g && t == nullptr))
    throw Error(GSI_ERR_ARG, "bilinear_terms: need n, b >= 1, 0 <= g <= min(b, 16), L, Y, R with dd, and the outputs");
  const int64_t nout = g * g + (b - g);
  Scratch partial(this, hipk::bilinear_partial_doubles(n, b, g)), out(this, (size_t)nout);
  hipk::bilinear_terms(st_, n, b, g, L, Y, R, dd, partial.p, out.p);
  check_launch("bilinear_terms");
  std::vector<double> h((size_t)nout);
  download2d(h.data(), nout, out.p, nout, nout, 1);
  for (int64_t e = 0; e < g * g; ++e) gram[e] = h[(size_t)e];
  for (int64_t e = 0; e < b - g; ++e) t[e] = h[(size_t)(g * g + e)];
  return 1;
}

}  // namespace gsi
