// pcga.cpp -- the PCGA consumers (pcga.hpp; DESIGN.md sections 4.7 - 4.7d).  Every consumer has the same shape: a backend
// attempt that returns false when the backend declined (nothing thrown, nothing written), and a host path that downloads
// the operands and runs the restatement of saddle_host.hpp / posterior_host.hpp / the CSR loop below.
#include "pcga.hpp"
#include "saddle_host.hpp"
#include "posterior_host.hpp"
#include "posterior_exact_host.hpp"
#include "bilinear_terms_host.hpp"
#include "fwd_adjoint_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/gsi_hip.h"

namespace gsi {

namespace {
// GSI_SADDLE_HOST / GSI_POST_HOST / GSI_FWD_HOST: set, not empty and not "0".  Read at every call.
bool env_forces_host(const char* name) {
  const char* e = getenv(name);
  return e != nullptr && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0');
}

const char* const kSaddleSingular =
    "SingularException: the saddle-point matrix [(HQH + R) HX; HX' 0] is singular (HX' (HQH + R)^-1 HX is zero or not finite)";
const char* const kPostSingular =
    "SingularException: the posterior needs HX' (HQH + R)^-1 HX positive and finite (HX is zero, or the operands are not finite)";

// The operands of the matrix on the host, as gsi_pcgamat_create stored them
struct HostOperands {
  std::vector<double> E, HX, R;
};
HostOperands download_operands(const PcgaLowRank& A) {
  Backend* be = A.ctx->be.get();
  const int64_t nobs = A.nobs;
  HostOperands h;
  h.E.resize((size_t)nobs * A.K);
  h.HX.resize((size_t)nobs);
  h.R.resize(A.r_diag ? (size_t)nobs : (size_t)nobs * nobs);
  be->download2d(h.E.data(), nobs, A.E.p, nobs, nobs, A.K);
  be->download2d(h.HX.data(), nobs, A.HX.p, nobs, nobs, 1);
  be->download2d(h.R.data(), nobs, A.R.p, nobs, nobs, A.r_diag ? 1 : nobs);
  return h;
}
}  // namespace

void throw_chol_outcome(PathInfo& info, int64_t col, bool singular, const char* singular_text) {
  if (col > 0) {
    info.column = col;
    throw Error(GSI_ERR_NOT_POSDEF, "PosDefException: matrix is not positive definite; Cholesky failed at " + std::to_string(col));
  }
  if (singular) throw Error(GSI_ERR_SINGULAR, singular_text);
}

// ---- the two products of the iteration with the resident basis ---------------------------------------------------------
void basis_params(Context& c, BasisRef Z, const double* s, const double* X, double delta, double* out) {
  Backend* be = c.be.get();
  const int64_t n = Z.n, K = Z.K;
  Buf O(be, (size_t)n * (K + 3)), sv(be, (size_t)n), Xv(be, (size_t)n);
  be->upload2d(sv.p, n, s, n, n, 1);
  be->upload2d(Xv.p, n, X, n, n, 1);
  if (Z.bits == 32) be->pcga_params_f32(Z.Z, n, K, sv.p, Xv.p, delta, O.p);
  else be->pcga_params((const double*)Z.Z, n, K, sv.p, Xv.p, delta, O.p);       // direct.jl:39-45 / lsqr.jl:37-43
  be->download2d(out, n, O.p, n, n, K + 3);
}

void basis_update(Context& c, BasisRef Z, const double* X, double beta_bar, const double* etas, int64_t nobs,
                  const double* xi_bar, double* s_out) {
  Backend* be = c.be.get();
  const int64_t n = Z.n, K = Z.K;
  Buf E(be, (size_t)nobs * K), xb(be, (size_t)nobs), w(be, (size_t)K), sd(be, (size_t)n), Xd(be, (size_t)n);
  be->upload2d(E.p, nobs, etas, nobs, nobs, K);
  be->upload2d(xb.p, nobs, xi_bar, nobs, nobs, 1);
  be->upload2d(Xd.p, n, X, n, n, 1);
  be->gemm_tn(K, 1, nobs, 1.0, E.p, nobs, xb.p, nobs, 0.0, w.p, K);     // w_i = dot(eta_i, xi_bar)
  if (Z.bits == 32) {
    be->basis_gemv_f32(Z.Z, n, K, w.p, beta_bar, Xd.p, sd.p);           // s = X beta_bar + sum_i xis[i] w_i
  } else {
    be->scal_copy(n, beta_bar, Xd.p, sd.p);                             // s = X * beta_bar      direct.jl:61
    be->gemm_nn(n, 1, K, 1.0, (const double*)Z.Z, n, w.p, K, 1.0, sd.p, n);   // s += sum_i xis[i]*w_i  direct.jl:62-65
  }
  be->download2d(s_out, n, sd.p, n, n, 1);
}

// v[1:end-1] = R xs + sum_i eta_i dot(eta_i, xs) + HX x[end];  v[end] = dot(HX, xs)      lowrank.jl:83-97
void PcgaLowRank::mul(const double* x, double* y) const {
  Backend* be = ctx->be.get();
  Buf t(be, (size_t)K);
  be->gemv_t(nobs, K, 1.0, E.p, nobs, x, t.p);                                    // t_i = dot(eta_i, xs)
  be->gemv_n(nobs, K, 1.0, E.p, nobs, t.p, 0.0, y);                               // sum_i eta_i t_i
  if (r_diag) be->diag_mul_add(nobs, R.p, x, y);                                  // + R xs
  else be->gemv_n(nobs, nobs, 1.0, R.p, nobs, x, 1.0, y);
  be->gemv_n(nobs, 1, 1.0, HX.p, nobs, x + nobs, 1.0, y);                         // + HX x[end]
  be->gemv_t(nobs, 1, 1.0, HX.p, nobs, x, y + nobs);                              // dot(HX, xs)
}

// ---- the saddle-point system by Cholesky ------------------------------------------------------
void PcgaLowRank::solve(const double* b, double* x, PathInfo& info) const {
  Backend* be = ctx->be.get();
  const int64_t n1 = nobs + 1;
  info = PathInfo();
  if (!env_forces_host("GSI_SADDLE_HOST")) {
    Buf bd(be, (size_t)n1), xd(be, (size_t)n1);
    be->upload2d(bd.p, n1, b, n1, n1, 1);
    bool singular = false;
    const int64_t col = be->saddle_solve(E.p, nobs, K, HX.p, R.p, r_diag, bd.p, xd.p, &singular);
    if (col != -1) {
      info.path = PATH_BACKEND;
      throw_chol_outcome(info, col, singular, kSaddleSingular);
      be->download2d(x, n1, xd.p, n1, n1, 1);
      return;
    }
  }
  info.path = PATH_HOST;                                // the same algebra on the downloaded operands (saddle_host.hpp)
  const HostOperands h = download_operands(*this);
  const int64_t col = saddle_host::solve(h.E.data(), nobs, K, h.HX.data(), h.R.data(), r_diag, b, x);
  throw_chol_outcome(info, col, col != 0, kSaddleSingular);
}

void chol_lower_host_matrix(Context& c, const double* A, int64_t n, int64_t lda, double* L, PathInfo& info) {
  Backend* be = c.be.get();
  info = PathInfo();
  int64_t col = -1;
  if (!env_forces_host("GSI_SADDLE_HOST")) {
    Buf W(be, (size_t)n * n);
    be->upload2d(W.p, n, A, lda, n, n);
    col = be->chol_lower(W.p, n, n, n);
    if (col != -1) {
      info.path = PATH_BACKEND;
      be->download2d(L, n, W.p, n, n, n);
    }
  }
  if (col == -1) {
    info.path = PATH_HOST;
    for (int64_t j = 0; j < n; ++j)
      for (int64_t i = 0; i < n; ++i) L[i + j * n] = A[i + j * lda];
    col = saddle_host::chol_lower(L, n, n, n);
  }
  info.column = col;
  for (int64_t j = 1; j < n; ++j)
    for (int64_t i = 0; i < j; ++i) L[i + j * n] = 0.0;
}

// ---- the posterior variance from the resident basis -------------------------------------------
namespace {
// The backend's row pass with W (K x ncols, ld K) and u (or null) already in its memory; a, q (or null), t (with u) on the host.
bool quadform_on_backend(Context& c, BasisRef Z, const double* Wd, int64_t ncols, bool upper, const double* ud, double* a,
                         double* q, double* t) {
  Backend* be = c.be.get();
  const int64_t n = Z.n;
  Buf out(be, (size_t)n * 3);
  double* ad = out.p;
  double* qd = q ? out.p + n : nullptr;
  double* td = ud ? out.p + 2 * n : nullptr;
  int ran = 0;
  {
    ScopedPhase ph(be, PH_OTHER);                      // (profiling: the row pass alone; tools/pcga_posterior_bench.py)
    ran = be->basis_quadform(Z.Z, Z.bits, n, n, Z.K, Wd, Z.K, ncols, upper, ud, ad, qd, td);
  }
  if (ran == 0) return false;
  be->download2d(a, n, ad, n, n, 1);
  if (q) be->download2d(q, n, qd, n, n, 1);
  if (ud) be->download2d(t, n, td, n, n, 1);
  return true;
}

// The row pass on the host, over the values the basis stores: fp64 as they are, fp32 as the floats of the double-typed allocation.
void quadform_on_host(Context& c, BasisRef Z, const double* W, int64_t ldw, int64_t ncols, bool upper, const double* u,
                      double* a, double* q, double* t) {
  const size_t count = (size_t)Z.n * (size_t)Z.K;
  const size_t doubles = Z.bits == 32 ? (count + 1) / 2 : count;
  std::vector<double> store(doubles);
  c.be->download2d(store.data(), (int64_t)doubles, (const double*)Z.Z, (int64_t)doubles, (int64_t)doubles, 1);
  if (Z.bits == 32)
    posterior_host::quadform((const float*)(const void*)store.data(), Z.n, Z.n, Z.K, W, ldw, ncols, upper, u, a, q, t);
  else
    posterior_host::quadform(store.data(), Z.n, Z.n, Z.K, W, ldw, ncols, upper, u, a, q, t);
}
}  // namespace

void basis_quadform(Context& c, BasisRef Z, const double* W, int64_t ldw, int64_t ncols, bool upper, const double* u,
                    double* a, double* q, double* t, PathInfo& info) {
  Backend* be = c.be.get();
  const int64_t K = Z.K;
  info = PathInfo();
  if (!env_forces_host("GSI_POST_HOST")) {
    Buf Wd(be, (size_t)K * (size_t)ncols), ud(be, (size_t)K);
    if (upper) {                                       // only the promised part travels: what lies below may be anything
      std::vector<double> Wu((size_t)K * (size_t)ncols, 0.0);
      for (int64_t j = 0; j < ncols; ++j)
        for (int64_t k = 0; k < K && k <= j; ++k) Wu[(size_t)(k + j * K)] = W[k + j * ldw];
      be->upload2d(Wd.p, K, Wu.data(), K, K, ncols);
    } else {
      be->upload2d(Wd.p, K, W, ldw, K, ncols);
    }
    if (u) be->upload2d(ud.p, K, u, K, K, 1);
    if (quadform_on_backend(c, Z, Wd.p, ncols, upper, u ? ud.p : nullptr, a, q, t)) {
      info.path = PATH_BACKEND;
      return;
    }
  }
  info.path = PATH_HOST;
  quadform_on_host(c, Z, W, ldw, ncols, upper, u, a, q, t);
}

namespace {
// B (nobs x K) = L_R^-1 E and wt = L_R^-1 HX in backend memory for a diagonal R: its entries are checked and inverted on the
// host, the rows scaled by the backend.  Throws for an entry that is not positive and finite, before the backend is asked.
bool whiten_diag_on_backend(const PcgaLowRank& A, Buf& B, Buf& wt, PathInfo& info) {
  Backend* be = A.ctx->be.get();
  const int64_t nobs = A.nobs, K = A.K;
  std::vector<double> d((size_t)nobs);
  be->download2d(d.data(), nobs, A.R.p, nobs, nobs, 1);
  for (int64_t i = 0; i < nobs; ++i) {
    if (!(d[(size_t)i] > 0.0) || !std::isfinite(d[(size_t)i])) throw_chol_outcome(info, i + 1, false, nullptr);
    d[(size_t)i] = 1.0 / std::sqrt(d[(size_t)i]);
  }
  Buf dd(be, (size_t)nobs);
  be->upload2d(dd.p, nobs, d.data(), nobs, nobs, 1);
  return be->scale_rows(nobs, K, dd.p, A.E.p, nobs, B.p, nobs) != 0 &&
         be->scale_rows(nobs, 1, dd.p, A.HX.p, nobs, wt.p, nobs) != 0;
}

// The same for a dense R: one chol_lower of [R; E'; w'] (nobs + K + 1 rows).  The carried rows are transposed on the host,
// they are (K + 1) x nobs numbers.
bool whiten_dense_on_backend(const PcgaLowRank& A, Buf& B, Buf& wt, PathInfo& info) {
  Backend* be = A.ctx->be.get();
  const int64_t nobs = A.nobs, K = A.K, kc = K + 1, ld = nobs + kc;
  std::vector<double> Eh((size_t)nobs * (size_t)kc), C((size_t)kc * (size_t)nobs);
  be->download2d(Eh.data(), nobs, A.E.p, nobs, nobs, K);
  be->download2d(Eh.data() + (size_t)nobs * (size_t)K, nobs, A.HX.p, nobs, nobs, 1);
  for (int64_t j = 0; j < nobs; ++j)
    for (int64_t cix = 0; cix < kc; ++cix) C[(size_t)(cix + j * kc)] = Eh[(size_t)(j + cix * nobs)];
  Buf T(be, (size_t)ld * (size_t)nobs);
  be->copy2d(T.p, ld, A.R.p, nobs, nobs, nobs);
  be->upload2d(T.p + nobs, ld, C.data(), kc, kc, nobs);
  const int64_t col = be->chol_lower(T.p, ld, nobs, ld);
  if (col == -1) return false;
  throw_chol_outcome(info, col, false, nullptr);
  be->download2d(C.data(), kc, T.p + nobs, ld, kc, nobs);
  for (int64_t j = 0; j < nobs; ++j)
    for (int64_t cix = 0; cix < kc; ++cix) Eh[(size_t)(j + cix * nobs)] = C[(size_t)(cix + j * kc)];
  be->upload2d(B.p, nobs, Eh.data(), nobs, nobs, K);
  be->upload2d(wt.p, nobs, Eh.data() + (size_t)nobs * (size_t)K, nobs, nobs, 1);
  return true;
}

// The backend's factor: B and wt as above, the TN product for N = I + B'B, chol_lower on [N; I] for W = L_N^-T.  Its throws
// report info.path as the caller set it.
bool factor_on_backend(const PcgaLowRank& A, double* W, double* u, double* gamma, PathInfo& info, Buf* Wdev, Buf* udev) {
  Backend* be = A.ctx->be.get();
  const int64_t nobs = A.nobs, K = A.K, ld2 = 2 * K;
  Buf B(be, (size_t)nobs * (size_t)K), wt(be, (size_t)nobs);
  if (!(A.r_diag ? whiten_diag_on_backend(A, B, wt, info) : whiten_dense_on_backend(A, B, wt, info))) return false;
  std::vector<double> T2h((size_t)ld2 * (size_t)K, 0.0);
  for (int64_t j = 0; j < K; ++j) T2h[(size_t)(j + j * ld2)] = T2h[(size_t)(K + j + j * ld2)] = 1.0;
  Buf T2(be, (size_t)ld2 * (size_t)K);
  be->upload2d(T2.p, ld2, T2h.data(), ld2, ld2, K);
  be->gemm_tn(K, K, nobs, 1.0, B.p, nobs, B.p, nobs, 1.0, T2.p, ld2);            // N = I + B'B
  const int64_t col = be->chol_lower(T2.p, ld2, K, ld2);
  if (col == -1) return false;
  throw_chol_outcome(info, 0, col != 0, kPostSingular);                          // N >= I: only non-finite operands
  Buf Wd(be, (size_t)K * (size_t)K), r(be, (size_t)K), y(be, (size_t)K), ud(be, (size_t)K);
  be->copy2d(Wd.p, K, T2.p + K, ld2, K, K);                                      // W = L_N^-T
  be->gemv_t(nobs, K, 1.0, B.p, nobs, wt.p, r.p);                                // r = B'wt
  be->gemv_t(K, K, 1.0, Wd.p, K, r.p, y.p);                                      // u = W (W'r)
  be->gemv_n(K, K, 1.0, Wd.p, K, y.p, 0.0, ud.p);
  const double ww = be->dot(nobs, wt.p, wt.p);
  const double g = ww - be->dot(K, r.p, ud.p);
  throw_chol_outcome(info, 0, !(ww > 0.0) || !std::isfinite(g) || !(g > 0.0), kPostSingular);
  if (gamma) *gamma = g;
  if (W) {
    be->download2d(W, K, Wd.p, K, K, K);
    for (int64_t j = 0; j < K; ++j)
      for (int64_t i = j + 1; i < K; ++i) W[i + j * K] = 0.0;
  }
  if (u) be->download2d(u, K, ud.p, K, K, 1);
  if (Wdev) *Wdev = std::move(Wd);
  if (udev) *udev = std::move(ud);
  return true;
}
}  // namespace

void posterior_factor(const PcgaLowRank& A, double* W, double* u, double* gamma, PathInfo& info, Buf* Wdev, Buf* udev) {
  const int64_t nobs = A.nobs, K = A.K;
  info = PathInfo();
  if (!env_forces_host("GSI_POST_HOST")) {
    info.path = PATH_BACKEND;
    if (factor_on_backend(A, W, u, gamma, info, Wdev, udev)) return;
  }
  info.path = PATH_HOST;                               // the same algebra on the downloaded operands (posterior_host.hpp)
  const HostOperands h = download_operands(A);
  std::vector<double> Wh((size_t)K * (size_t)K), uh((size_t)K);
  double g = 0.0;
  const int64_t col = posterior_host::factor(h.E.data(), nobs, K, h.HX.data(), h.R.data(), A.r_diag, Wh.data(), uh.data(), &g);
  throw_chol_outcome(info, col, col != 0, kPostSingular);
  if (W) std::copy(Wh.begin(), Wh.end(), W);
  if (u) std::copy(uh.begin(), uh.end(), u);
  if (gamma) *gamma = g;
}

void posterior_variance(Context& c, BasisRef Z, const PcgaLowRank& A, const double* X, const double* prior, double* var,
                        PathInfo& info) {
  const int64_t n = Z.n, K = Z.K;
  std::vector<double> Wh((size_t)K * (size_t)K), uh((size_t)K), a((size_t)n), q((size_t)n), t((size_t)n);
  double gamma = 0.0;
  Buf Wd, ud;
  posterior_factor(A, Wh.data(), uh.data(), &gamma, info, &Wd, &ud);
  PathInfo row;
  // W and u still in backend memory never leave it for the pass; otherwise the pass starts from the host copies
  if (Wd.p != nullptr && quadform_on_backend(c, Z, Wd.p, K, true, ud.p, a.data(), q.data(), t.data())) row.path = PATH_BACKEND;
  else basis_quadform(c, Z, Wh.data(), K, K, true, uh.data(), a.data(), q.data(), t.data(), row);
  info.path = row.path;
  posterior_host::finish(n, a.data(), q.data(), t.data(), X, prior, gamma, var);
}

// ---- the sparse forward model (gsi_fwd) ------------------------------------------------------
namespace {
template <class T>
void upload_as_doubles(Backend* be, Buf& dst, const T* src, size_t count) {
  // integers travel as the bytes of a double-typed allocation: every transfer is a byte copy
  const size_t nd = (count * sizeof(T) + sizeof(double) - 1) / sizeof(double);
  std::vector<double> stage(std::max<size_t>(nd, 1), 0.0);
  if (count) std::memcpy(stage.data(), src, count * sizeof(T));
  dst = Buf(be, stage.size());
  be->upload2d(dst.p, (int64_t)stage.size(), stage.data(), (int64_t)stage.size(), (int64_t)stage.size(), 1);
}

// The backend's product: the caller has set the operand (Z, zbits, ldz, K, plain, and s, X, delta unless plain); this fills
// in the model and the outputs, runs, and brings the nobs x a.ncols() results to out (host, ld ldo).
void fwd_model_args(const FwdModel& F, FwdProduct& a) {
  a.nobs = F.nobs; a.n = F.n; a.nnz = F.nnz; a.nseg = F.plan.nseg(); a.maxlen = F.plan.maxlen;
  a.segptr = reinterpret_cast<const int64_t*>(F.d_segptr.p);
  a.rowseg = F.plan.nsplit ? reinterpret_cast<const int64_t*>(F.d_rowseg.p) : nullptr;
  a.colidx = reinterpret_cast<const int32_t*>(F.d_colidx.p);
  a.vals = F.d_vals.p;
  a.w = F.w.empty() ? nullptr : F.d_w.p;
  a.link = F.link;
}
bool fwd_on_backend(Backend* be, const FwdModel& F, FwdProduct& a, double* out, int64_t ldo) {
  const int64_t nobs = F.nobs, nc = a.ncols();
  Buf O(be, (size_t)nobs * nc), part;
  if (F.plan.nsplit) part = Buf(be, (size_t)F.plan.nseg() * nc);
  fwd_model_args(F, a);
  a.out = O.p; a.ldo = nobs; a.partial = part.p;
  const int form = be->fwd_products(a);
  if (form == 0) return false;
  be->download2d(out, ldo, O.p, nobs, nobs, nc);
  F.last_form = form;
  return true;
}

// out[:, c] = h(P[:, c]) on the host, nonzeros of a row in storage order
void fwd_on_host(const FwdModel& F, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo) {
  const bool has_w = !F.w.empty();
  for (int64_t c = 0; c < ncols; ++c) {
    const double* p = P + c * ldp;
    for (int64_t r = 0; r < F.nobs; ++r) {
      double acc = 0.0;
      for (int64_t t = F.rowptr[(size_t)r]; t < F.rowptr[(size_t)r + 1]; ++t) {
        const int64_t j = F.colidx[(size_t)t];
        double a = (has_w ? F.w[(size_t)j] : 1.0) * p[j];
        if (F.link) a = std::exp(a);
        acc += F.vals[(size_t)t] * a;
      }
      out[r + c * ldo] = acc;
    }
  }
  F.host_products += 1;
  F.last_form = 3;
}
}  // namespace

void fwd_create(Context& c, FwdModel& F, int64_t nobs, int64_t n, const int64_t* rowptr, const int64_t* colidx,
                const double* vals, const double* weights, int link) {
  auto bad = [](const std::string& m) { throw Error(GSI_ERR_ARG, "gsi_fwd_linear_create: " + m); };
  if (nobs < 1 || n < 1) bad("nobs = " + std::to_string(nobs) + ", n = " + std::to_string(n) + ": both must be at least 1");
  if (n >= ((int64_t)1 << 31)) bad("n = " + std::to_string(n) + " does not fit the 32-bit column indices (n < 2^31)");
  if (link != 0 && link != 1) bad("link = " + std::to_string(link) + " (0: identity, 1: exp)");
  if (!rowptr) bad("rowptr is NULL");
  if (rowptr[0] != 0) bad("rowptr[0] = " + std::to_string(rowptr[0]) + ", not 0 (offsets are 0-based)");
  for (int64_t r = 0; r < nobs; ++r)
    if (rowptr[r + 1] < rowptr[r])
      bad("rowptr decreases at row " + std::to_string(r) + ": " + std::to_string(rowptr[r]) + " -> " +
          std::to_string(rowptr[r + 1]));
  const int64_t nnz = rowptr[nobs];
  if (nnz > 0 && (!colidx || !vals)) bad("colidx / vals is NULL");
  for (int64_t r = 0; r < nobs; ++r)
    for (int64_t t = rowptr[r]; t < rowptr[r + 1]; ++t)
      if (colidx[t] < 0 || colidx[t] >= n)
        bad("entry " + std::to_string(t) + " (row " + std::to_string(r) + ") has column index " + std::to_string(colidx[t]) +
            " outside [0, " + std::to_string(n) + ")");
  int64_t limit = FWD_DEFAULT_SEG_LIMIT;
  if (const char* e = getenv("GSI_FWD_SEG")) {
    if (e[0] != '\0') {
      limit = atoll(e);
      if (limit < 1) bad(std::string("GSI_FWD_SEG = '") + e + "': a segment holds at least one nonzero");
    }
  }
  F.ctx = &c; F.nobs = nobs; F.n = n; F.nnz = nnz; F.link = link; F.seg_limit = limit;
  F.rowptr.assign(rowptr, rowptr + nobs + 1);
  F.colidx.resize((size_t)nnz);
  for (int64_t t = 0; t < nnz; ++t) F.colidx[(size_t)t] = (int32_t)colidx[t];
  F.vals.assign(vals, vals + nnz);
  if (weights) F.w.assign(weights, weights + n);
  F.plan = fwd_plan(rowptr, nobs, limit);
  Backend* be = c.be.get();
  upload_as_doubles(be, F.d_segptr, F.plan.segptr.data(), F.plan.segptr.size());
  if (F.plan.nsplit) upload_as_doubles(be, F.d_rowseg, F.plan.rowseg.data(), F.plan.rowseg.size());
  upload_as_doubles(be, F.d_colidx, F.colidx.data(), F.colidx.size());
  F.d_vals = Buf(be, std::max<size_t>((size_t)nnz, 1));
  if (nnz) be->upload2d(F.d_vals.p, nnz, F.vals.data(), nnz, nnz, 1);
  if (weights) {
    F.d_w = Buf(be, (size_t)n);
    be->upload2d(F.d_w.p, n, F.w.data(), n, n, 1);
  }
}

void fwd_forward_basis(Context& c, const FwdModel& F, BasisRef Z, const double* s, const double* X, double delta, double* out) {
  Backend* be = c.be.get();
  const int64_t n = F.n, nobs = F.nobs, nc = Z.K + 3;
  F.products += 1;
  if (!env_forces_host("GSI_FWD_HOST")) {
    Buf sv(be, (size_t)n), Xv(be, (size_t)n);
    be->upload2d(sv.p, n, s, n, n, 1);
    be->upload2d(Xv.p, n, X, n, n, 1);
    FwdProduct a;
    a.Z = Z.Z; a.zbits = Z.bits; a.ldz = n; a.K = Z.K; a.plain = false;
    a.s = sv.p; a.X = Xv.p; a.delta = delta;
    if (fwd_on_backend(be, F, a, out, nobs)) return;
  }
  // the host path: the batch as direct.jl:39-45 forms it, on the host, and the model applied column by column
  std::vector<double> P((size_t)n * nc);
  basis_params(c, Z, s, X, delta, P.data());
  fwd_on_host(F, P.data(), n, nc, out, nobs);
}

void fwd_apply(Context& c, const FwdModel& F, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo) {
  Backend* be = c.be.get();
  const int64_t n = F.n;
  F.products += 1;
  if (!env_forces_host("GSI_FWD_HOST")) {
    Buf Pd(be, (size_t)n * ncols);
    be->upload2d(Pd.p, n, P, ldp, n, ncols);
    FwdProduct a;
    a.Z = Pd.p; a.zbits = 64; a.ldz = n; a.K = ncols; a.plain = true;
    if (fwd_on_backend(be, F, a, out, ldo)) return;
  }
  fwd_on_host(F, P, ldp, ncols, out, ldo);
}

void fwd_apply_dev(Context& c, const FwdModel& F, const double* P, int64_t ldp, int64_t ncols, double* out, int64_t ldo) {
  Backend* be = c.be.get();
  const int64_t n = F.n, nobs = F.nobs;
  F.products += 1;
  if (!env_forces_host("GSI_FWD_HOST")) {
    Buf part;
    if (F.plan.nsplit) part = Buf(be, (size_t)F.plan.nseg() * ncols);
    FwdProduct a;
    a.Z = P; a.zbits = 64; a.ldz = ldp; a.K = ncols; a.plain = true;
    fwd_model_args(F, a);
    a.out = out; a.ldo = ldo; a.partial = part.p;
    const int form = be->fwd_products(a);
    if (form != 0) { F.last_form = form; return; }
  }
  std::vector<double> Ph((size_t)n * ncols), Oh((size_t)nobs * ncols);
  be->download2d(Ph.data(), n, P, ldp, n, ncols);
  fwd_on_host(F, Ph.data(), n, ncols, Oh.data(), nobs);
  be->upload2d(out, ldo, Oh.data(), nobs, nobs, ncols);
}

// ---- the adjoint of the forward model -----------------------------------------------------------
namespace {
// the index resident in backend memory: one allocation, integers as the bytes of doubles
void fwd_adjoint_upload(Backend* be, const FwdModel& F) {
  const FwdAdjointPlan& ap = F.aplan;
  auto words = [](size_t bytes) { return (bytes + 7) / 8; };
  size_t total = 0;
  auto take = [&](size_t w) { const size_t o = total; total += w; return o; };
  const size_t nnz = (size_t)ap.nnz, nl = (size_t)ap.nlong(), nc = (size_t)ap.nchunk();
  const size_t o_ptr = take((size_t)ap.n + 1), o_val = take(nnz), o_row = take(words(4 * nnz)), o_lchunk = take(nl + 1),
               o_coff = take(nc), o_lcol = take(words(4 * nl)), o_clen = take(words(4 * nc));
  F.d_adj = Buf(be, total);
  double* d = F.d_adj.p;
  std::vector<double> packed;
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes == 0) return;
    packed.assign(words(bytes), 0.0);
    std::memcpy(packed.data(), src, bytes);
    be->upload2d(d + off, (int64_t)packed.size(), packed.data(), (int64_t)packed.size(), (int64_t)packed.size(), 1);
  };
  put(o_ptr, ap.colptr.data(), 8 * ((size_t)ap.n + 1));
  put(o_val, ap.val.data(), 8 * nnz);
  put(o_row, ap.row.data(), 4 * nnz);
  put(o_lchunk, ap.long_chunk0.data(), 8 * (nl + 1));
  put(o_coff, ap.chunk_off.data(), 8 * nc);
  put(o_lcol, ap.long_col.data(), 4 * nl);
  put(o_clen, ap.chunk_len.data(), 4 * nc);
  FwdAdjoint& a = F.adev;
  a.n = ap.n; a.nobs = ap.nobs; a.nnz = ap.nnz; a.chunk = ap.chunk; a.nlong = ap.nlong(); a.nchunk = ap.nchunk();
  a.colptr = reinterpret_cast<const int64_t*>(d + o_ptr);
  a.val = d + o_val;
  a.row = reinterpret_cast<const int32_t*>(d + o_row);
  a.long_chunk0 = reinterpret_cast<const int64_t*>(d + o_lchunk);
  a.chunk_off = reinterpret_cast<const int64_t*>(d + o_coff);
  a.long_col = reinterpret_cast<const int32_t*>(d + o_lcol);
  a.chunk_len = reinterpret_cast<const int32_t*>(d + o_clen);
  F.adj_bytes = (int64_t)(8 * total);
}
}  // namespace

void fwd_adjoint(Context& c, const FwdModel& F, const double* V, int64_t ldv, int64_t b, double* G, int64_t ldg) {
  if (F.link != 0)
    throw Error(GSI_ERR_ARG, "gsi_fwd_adjoint: the model has link = " + std::to_string(F.link) +
                                 " (exp): only a linear model (link = 0) has an adjoint");
  if (b <= 0) return;
  Backend* be = c.be.get();
  if (!F.aplan_built) {
    F.aplan = fwd_adjoint_plan(F.nobs, F.n, F.rowptr.data(), F.colidx.data(), F.vals.data(), F.w.empty() ? nullptr : F.w.data());
    F.aplan_built = true;
  }
  F.adj_products += 1;
  if (!env_forces_host("GSI_FWD_HOST")) {
    if (F.d_adj.p == nullptr) fwd_adjoint_upload(be, F);
    FwdAdjoint a = F.adev;
    a.V = V; a.ldv = ldv; a.b = b; a.G = G; a.ldg = ldg; a.partial = nullptr;
    if (be->fwd_adjoint(a) != 0) return;
  }
  std::vector<double> Vh((size_t)F.nobs * b), Gh((size_t)F.n * b);
  be->download2d(Vh.data(), F.nobs, V, ldv, F.nobs, b);
  fwd_adjoint_host::apply(F.aplan, Vh.data(), F.nobs, b, Gh.data(), F.n);
  be->upload2d(G, ldg, Gh.data(), F.n, F.n, b);
  F.adj_host_products += 1;
}

// ---- the exact posterior variance of linear inversion and kriging -------------------------------
int64_t rowdot_acc(Context& c, int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc,
                   bool force_host) {
  Backend* be = c.be.get();
  if (n < 1 || b < 1) return PATH_BACKEND;
  if (!force_host && !env_forces_host("GSI_POSTX_HOST") && be->rowdot_acc(n, b, A, lda, B, ldb, acc) != 0) return PATH_BACKEND;
  const bool same = (A == B && lda == ldb);
  std::vector<double> Ah((size_t)n * (size_t)b), Bh(same ? (size_t)0 : (size_t)n * (size_t)b), ah((size_t)n);
  be->download2d(Ah.data(), n, A, lda, n, b);
  if (!same) be->download2d(Bh.data(), n, B, ldb, n, b);
  be->download2d(ah.data(), n, acc, n, n, 1);
  postx_host::rowdot_acc(n, b, Ah.data(), n, same ? Ah.data() : Bh.data(), n, ah.data());
  be->upload2d(acc, n, ah.data(), n, n, 1);
  return PATH_HOST;
}

// ---- the bilinear forms of the likelihood gradient ------------------------------------------------
int64_t bilinear_terms(Context& c, int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R,
                       const double* dd, double* gram, double* t) {
  Backend* be = c.be.get();
  if (!env_forces_host("GSI_BILINEAR_HOST")) {
    Buf ddev;
    if (dd != nullptr) {
      ddev = Buf(be, (size_t)n);
      be->upload2d(ddev.p, n, dd, n, n, 1);
    }
    if (be->bilinear_terms(n, b, g, L, Y, R, ddev.p, gram, t) != 0) return PATH_BACKEND;
  }
  const size_t cnt = (size_t)n * (size_t)b;
  std::vector<double> Lh(cnt), Yh(cnt), Rh(dd != nullptr ? cnt : (size_t)0);
  be->download2d(Lh.data(), n, L, n, n, b);
  be->download2d(Yh.data(), n, Y, n, n, b);
  if (dd != nullptr) be->download2d(Rh.data(), n, R, n, n, b);
  bilinear_host::terms(n, b, g, Lh.data(), Yh.data(), dd != nullptr ? Rh.data() : nullptr, dd, gram, t);
  return PATH_HOST;
}

int64_t op_bilinear_terms(Context& c, const Operator* dop, const double* ddiag, const double* X, int64_t n, int64_t b, int64_t g,
                          const double* Wz, double* gram, double* t) {
  Backend* be = c.be.get();
  Buf R(be, (size_t)n * (size_t)b), Y(be, (size_t)n * (size_t)b);
  if (g > 0) be->copy2d(R.p, n, X, n, n, g);
  if (b > g) be->copy2d(R.p + (size_t)n * (size_t)g, n, Wz, n, n, b - g);
  if (dop != nullptr) {
    op_mul(*dop, R.p, n, b, Y.p, n);
  } else {
    be->scal_copy(n * b, 0.0, R.p, Y.p);
  }
  return bilinear_terms(c, n, b, g, X, Y.p, R.p, ddiag, gram, t);
}

void posterior_variance_exact(const Operator& A, const double* diag, const double* X, int64_t ldx, int64_t p, int64_t batch,
                              double* var, PostxInfo& info) {
  Context& c = *A.ctx;
  Backend* be = c.be.get();
  const int64_t nobs = A.n, n = A.fft_N[0] * A.fft_N[1] * A.fft_N[2], ld = 2 * nobs + p;
  info = PostxInfo();
  info.trapezoid_bytes = (int64_t)sizeof(double) * ld * nobs;
  const int64_t bw = std::max<int64_t>(1, std::min(batch > 0 ? batch : op_cov_batch(A, nobs), nobs));
  info.width = bw;
  bool host = env_forces_host("GSI_POSTX_HOST");

  // V (nobs x b, ld ldv) -> Hh (n x b) = C H' V through G (n x b): the model's adjoint or the interpolation's spread, then
  // the grid product; profiled as the operator's own products are (gemm_t, gemm_n)
  auto prior_adjoint = [&](const double* V, int64_t ldv, int64_t b, double* G, double* Hh) {
    {
      ScopedPhase ph(be, PH_GEMM_T);
      if (A.kind == OP_FWD_COV) fwd_adjoint(c, *A.fwd, V, ldv, b, G, n);
      else be->points_at_spread(A.at, G, n, b, V, ldv);
    }
    ScopedPhase ph(be, PH_GEMM_N);
    be->fftcov_apply(A.plan, b, G, n, Hh, n);
  };

  Buf T(be, (size_t)ld * (size_t)nobs);
  {                                                    // the top block: columns [c0, c0 + b) of H C H' from unit columns
    Buf E(be, (size_t)nobs * (size_t)bw);
    std::vector<double> Eh;
    for (int64_t c0 = 0; c0 < nobs; c0 += bw) {
      const int64_t b = std::min(bw, nobs - c0);
      if (!host && be->unit_panel(E.p, nobs, nobs, b, c0) == 0) host = true;
      if (host) {
        Eh.resize((size_t)nobs * (size_t)b);
        postx_host::unit_panel(Eh.data(), nobs, nobs, b, c0);
        be->upload2d(E.p, nobs, Eh.data(), nobs, nobs, b);
      }
      op_mul(A, E.p, nobs, b, T.p + (size_t)c0 * (size_t)ld, ld);
    }
  }
  Buf Phi(be, (size_t)nobs * (size_t)std::max<int64_t>(p, 1)), dd;
  if (p > 0) {                                         // Phi = H X
    Buf Xd(be, (size_t)n * (size_t)p);
    be->upload2d(Xd.p, n, X, ldx, n, p);
    if (A.kind == OP_FWD_COV) fwd_apply_dev(c, *A.fwd, Xd.p, n, p, Phi.p, nobs);
    else be->points_at_gather(A.at, Phi.p, nobs, p, Xd.p, n);
  }
  if (diag) {
    dd = Buf(be, (size_t)nobs);
    be->upload2d(dd.p, nobs, diag, nobs, nobs, 1);
  }

  // [M; Phi'; I] <- [L; W_d'; L^-T] by one factorization of the trapezoid
  int64_t col = -1;
  bool assembled = false;
  if (!host) {
    if (be->trapezoid_rows(T.p, ld, nobs, p, dd.p, Phi.p, nobs) == 0) host = true;
    else assembled = true;
  }
  if (!host) {
    ScopedPhase ph(be, PH_LU);
    col = be->chol_lower(T.p, ld, nobs, ld);
  }
  if (col == -1) {                                     // the same on the downloaded trapezoid (saddle_host.hpp)
    host = true;
    std::vector<double> Th((size_t)ld * (size_t)nobs);
    be->download2d(Th.data(), ld, T.p, ld, ld, nobs);
    if (!assembled) {
      std::vector<double> Ph((size_t)nobs * (size_t)std::max<int64_t>(p, 1));
      if (p > 0) be->download2d(Ph.data(), nobs, Phi.p, nobs, nobs, p);
      postx_host::assemble(Th.data(), ld, nobs, p, diag, Ph.data(), nobs);
    }
    col = saddle_host::chol_lower(Th.data(), ld, nobs, ld);
    if (col == 0) be->upload2d(T.p, ld, Th.data(), ld, ld, nobs);
  }
  info.path = host ? PATH_HOST : PATH_BACKEND;
  if (col > 0) {
    info.column = col;
    throw Error(GSI_ERR_NOT_POSDEF, "PosDefException: H C H' + D is not positive definite; Cholesky failed at " + std::to_string(col));
  }
  const double* Linvt = T.p + nobs + p;                // L^-T, nobs x nobs upper triangular, ld

  // the p x p algebra: S = W_d'W_d = Ls Ls' on the host, V = L^-T W_d by the contraction
  std::vector<double> Ls((size_t)std::max<int64_t>(p * p, 1));
  Buf V;
  if (p > 0) {
    Buf Wd(be, (size_t)nobs * (size_t)p), S(be, (size_t)p * (size_t)p);
    if (host || be->carried_rows(T.p, ld, nobs, p, Wd.p) == 0) {
      host = true;
      std::vector<double> rows((size_t)p * (size_t)nobs), Wh((size_t)nobs * (size_t)p);
      be->download2d(rows.data(), p, T.p + nobs, ld, p, nobs);
      postx_host::carried_rows(rows.data(), p, nobs, p, Wh.data());
      be->upload2d(Wd.p, nobs, Wh.data(), nobs, nobs, p);
    }
    {
      ScopedPhase ph(be, PH_SMALL_GEMM);
      be->gemm_tn(p, p, nobs, 1.0, Wd.p, nobs, Wd.p, nobs, 0.0, S.p, p);
    }
    be->download2d(Ls.data(), p, S.p, p, p, p);
    const int64_t scol = postx_host::chol_small(Ls.data(), p);
    if (scol != 0)
      throw Error(GSI_ERR_SINGULAR, "SingularException: the drift columns H X are linearly dependent (X' H' (H C H' + D)^-1 H X is "
                                    "singular at column " + std::to_string(scol) + ")");
    V = Buf(be, (size_t)nobs * (size_t)p);
    ScopedPhase ph(be, PH_SMALL_GEMM);
    be->gemm_nn(nobs, p, nobs, 1.0, Linvt, ld, Wd.p, nobs, 0.0, V.p, nobs);
  }

  // the n-sized work: T_J = C H' (L^-T)[:, J] batch by batch and its running row sums of squares; U = C H' V
  Buf G(be, (size_t)n * (size_t)bw), Hh(be, (size_t)n * (size_t)bw), acc(be, (size_t)n);
  be->fill_zero(acc.p, (size_t)n);
  for (int64_t c0 = 0; c0 < nobs; c0 += bw) {
    const int64_t b = std::min(bw, nobs - c0);
    prior_adjoint(Linvt + (size_t)c0 * (size_t)ld, ld, b, G.p, Hh.p);
    ScopedPhase ph(be, PH_OTHER);
    if (rowdot_acc(c, n, b, Hh.p, n, Hh.p, n, acc.p, host) == PATH_HOST) host = true;     // a pass the backend declined
    info.batches += 1;
  }
  std::vector<double> Uh((size_t)n * (size_t)std::max<int64_t>(p, 1));
  for (int64_t c0 = 0; c0 < p; c0 += bw) {
    const int64_t b = std::min(bw, p - c0);
    prior_adjoint(V.p + (size_t)c0 * (size_t)nobs, nobs, b, G.p, Hh.p);
    be->download2d(Uh.data() + (size_t)c0 * (size_t)n, n, Hh.p, n, n, b);
  }
  info.adjoint_columns = nobs + p;
  info.path = host ? PATH_HOST : PATH_BACKEND;         // the host path if any of the backend's steps was declined
  // C_00 = (C e_0)_0: constant over the cells for every FFT grid operator, whatever its convention
  double c00 = 1.0;
  be->fill_zero(G.p, (size_t)n);
  be->upload2d(G.p, n, &c00, 1, 1, 1);
  be->fftcov_apply(A.plan, 1, G.p, n, Hh.p, n);
  be->download2d(&c00, 1, Hh.p, n, 1, 1);
  std::vector<double> ah((size_t)n);
  be->download2d(ah.data(), n, acc.p, n, n, 1);
  postx_host::finish(n, p, c00, ah.data(), Uh.data(), n, X, ldx, Ls.data(), var);
}

}  // namespace gsi
