// hip_backend_sampler.hip -- HipBackend's sampler of Gaussian fields with a grid covariance function (gridcov_sample.hip,
// DESIGN.md 4.6f): the plan (spectrum, admissibility, square root) and the batches of pairs of fields.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "hip_backend_impl.hpp"
#include "fft_line.hpp"

namespace gsi {

struct HipBackend::GridCovSampler {       // one allocation: twiddles | lambda | amp
  hipk::GcsGeom g;
  Scratch buf;
  double *twg = nullptr, *lam = nullptr, *amp = nullptr;
  explicit GridCovSampler(HipBackend* be) : buf(be) {}
};

void* HipBackend::gridcov_sampler_create(int ndims, const int64_t N[3], const int64_t M[3], int kind, const double ell[3],
                                         double theta, double sigma2, double nugget, double neg_tol, double info[4]) {
  bind();
  const int64_t pooled0 = pooled_;
  std::unique_ptr<GridCovSampler> p(new GridCovSampler(this));
  hipk::GcsGeom& g = p->g;
  g.d = ndims; g.Mtot = 1; g.n = 1;
  for (int a = 0; a < 3; ++a) {
    g.N[a] = a < ndims ? N[a] : 1;
    g.M[a] = a < ndims ? M[a] : 1;
    g.Mtot *= g.M[a];
    g.n *= g.N[a];
  }
  Carve c;
  const size_t o_tw = c.take(hipk::FFT_TW_LEN), o_lam = c.take((size_t)g.Mtot), o_amp = c.packed((size_t)g.Mtot);
  p->buf.adopt(alloc(c.total));
  p->twg = p->buf.p + o_tw; p->lam = p->buf.p + o_lam; p->amp = p->buf.p + o_amp;
  double h[4 * hipk::GCS_PARTS];
  {
    Carve cw;
    const size_t o_w = cw.take((size_t)2 * g.Mtot), o_part = cw.packed((size_t)4 * hipk::GCS_PARTS);
    Scratch work(this, cw.total);                                   // the plan transform's complex array | the partial results
    const double inv_ell[3] = {1.0 / ell[0], 1.0 / ell[1], 1.0 / ell[2]};
    hipk::fftrf_twiddles(st_, p->twg);
    hipk::gcs_lag_table(st_, g, kind, inv_ell, std::cos(theta), std::sin(theta), sigma2, p->amp);
    hipk::gcs_plan_transform(st_, g, p->twg, p->amp, work.p + o_w, p->lam);
    hipk::gcs_plan_finish(st_, g, nugget, p->lam, p->amp, work.p + o_part);
    check_launch("gridcov sampler plan");
    download2d(h, 4 * hipk::GCS_PARTS, work.p + o_part, 4 * hipk::GCS_PARTS, 4 * hipk::GCS_PARTS, 1);
  }
  double neg = 0.0, mn = INFINITY, mx = -INFINITY, cnt = 0.0;
  for (int b = 0; b < hipk::GCS_PARTS; ++b) {                         // left to right: a fixed order
    neg += h[b];
    mn = std::min(mn, h[hipk::GCS_PARTS + b]);
    mx = std::max(mx, h[2 * hipk::GCS_PARTS + b]);
    cnt += h[3 * hipk::GCS_PARTS + b];
  }
  const double neg_mass = neg / ((double)g.Mtot * (sigma2 + nugget));
  info[0] = neg_mass; info[1] = mn; info[2] = mx; info[3] = cnt;
  if (!(neg_mass <= neg_tol)) {
    char msg[512];
    snprintf(msg, sizeof msg,
             "grid covariance sampler: the covariance is not non-negative definite on the embedding %lld x %lld x %lld: neg_mass = "
             "%.6g > neg_tol = %.6g, lambda_min / lambda_max = %.6g (%lld of %lld lambda < 0): use a larger embedding or a larger "
             "neg_tol",
             (long long)g.M[0], (long long)g.M[1], (long long)g.M[2], neg_mass, neg_tol, mn / mx, (long long)cnt, (long long)g.Mtot);
    p.reset();                        // a refusal leaves bytes_in_use() as it was: the blocks it cached (the last ones) are freed
    trim_pool(pooled0);
    throw Error(GSI_ERR_NOT_POSDEF, msg);
  }
  return p.release();
}
void HipBackend::gridcov_sampler_destroy(void* plan) {
  delete static_cast<GridCovSampler*>(plan);
}
void HipBackend::gridcov_sampler_spectrum(void* plan, double* lam_host) {
  const GridCovSampler* p = static_cast<GridCovSampler*>(plan);
  download2d(lam_host, p->g.Mtot, p->lam, p->g.Mtot, p->g.Mtot, 1);
}
// Batches of pairs: the noise and the intermediate array of a batch stay within 2 GiB of workspace (GSI_GRIDCOV_BATCH=<pairs>,
// read at every call, overrides the batch size).  Nothing a pair computes depends on the batch it rides in.
void HipBackend::gridcov_sampler_fields(void* plan, double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf,
                                        const double* eps, int64_t ldeps, uint64_t seed, int64_t field0) {
  bind();
  if (nf <= 0) return;
  const GridCovSampler* p = static_cast<GridCovSampler*>(plan);
  const hipk::GcsGeom& g = p->g;
  const int64_t fs = (int64_t)hipk::gcs_pair_doubles(g);             // even: every term is
  const int64_t npairs = (nf + 1) / 2;
  int64_t nb = (((int64_t)2 << 30) / (int64_t)sizeof(double)) / fs;
  if (const char* e = getenv("GSI_GRIDCOV_BATCH")) { if (atoll(e) >= 1) nb = atoll(e); }
  if (nb > 4096) nb = 4096;
  if (nb > npairs) nb = npairs;
  if (nb < 1) nb = 1;
  Scratch ws(this, (size_t)(fs * nb));
  for (int64_t j0 = 0; j0 < npairs; j0 += nb) {
    const int b = (int)((npairs - j0 < nb) ? (npairs - j0) : nb);
    if (eps) {
      if (j0 > 0) HIP_CHECK(hipStreamSynchronize(st_));             // the previous batch still reads the workspace
      for (int i = 0; i < b; ++i) upload2d(ws.p + (int64_t)i * fs, g.Mtot, eps + 2 * (j0 + i) * ldeps, ldeps, g.Mtot, 2);
    } else {
      for (int i = 0; i < 2 * b; ++i)
        hipk::randn_fill(st_, ws.p + (int64_t)(i / 2) * fs + (int64_t)(i & 1) * g.Mtot, (size_t)g.Mtot,
                         seed + (uint64_t)(field0 + 2 * j0 + i));
    }
    hipk::gcs_sample(st_, g, p->twg, p->amp, ws.p, fs, b, dst + 2 * j0 * ldd, ldd, row0, nloc, nf - 2 * j0);
    check_launch("gridcov_sample");
  }
}

}  // namespace gsi
