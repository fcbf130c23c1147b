// gridcov_sample.hip -- Gaussian fields with a grid covariance FUNCTION, sampled on the device by circulant embedding
// (Dietrich-Newsam / Wood-Chan; gsi_gridcov_sampler_*), a batch of PAIRS of fields at a time.
//
// The box N sits on a torus M (powers of two, M_a >= 2 N_a), torus order t0 + M0 (t1 + M1 t2).  The plan holds the spectrum
// lambda of the torus covariance and amp = sqrt(max(lambda, 0) / Mtot).  One pair:  w = unnormalised inverse DFT of
// amp (eps1 + i eps2), field 2 j = Re w and field 2 j + 1 = Im w on the box -- two independent fields per complex transform.
// The transform is separable and the crop follows each axis's pass at once:
//   FIRST   lines along axis 0 (contiguous), all M1 M2 of them: forms amp (eps1 + i eps2) while loading, stores the first N0
//           outputs into W (N0 x M1 x M2 complex);
//   MIDDLE  (3-D) lines along axis 1 (stride N0), tiles of neighbouring lines, in place, first N1 outputs;
//   LAST    lines along the last axis: Re into column 2 j and Im into column 2 j + 1 of the destination, rows
//           [row0, row0 + nloc) only, with the destination's leading dimension.  No intermediate real field, no normalising pass.
// Every line is a power of two: one inverse Stockham transform of fft_line.hpp, no Bluestein.  One workgroup per (pair, tile);
// nothing here depends on how many pairs share a launch.  The plan's spectrum is made by the same passes (no noise, no crop).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include "hip_common.hpp"
#include "fft_line.hpp"

namespace gsi { namespace hipk {

enum { GCS_FIRST = 0, GCS_MIDDLE = 1, GCS_LAST = 2 };

struct GcsPass {
  int Ma, log2Ma;             // points of a line
  int A;                      // outputs that survive the crop
  int T, lstride;             // lines per tile; elements between the lines of a tile in LDS
  int contig;                 // fill / drain order: position fastest (else line fastest)
  uint32_t nl0, nl1;          // lines (t0, t1), t0 < nl0, t1 < nl1; a tile = T neighbouring t0 at one t1
  uint32_t ls0, ls1, ks;      // input element k of line (t0, t1):  t0 ls0 + t1 ls1 + k ks
  uint32_t os0, os1, oks;     // output element k of that line:     t0 os0 + t1 os1 + k oks
};

// KIND FIRST: amp, eps -> W;  MIDDLE: W -> W in place;  LAST: W -> dst (Re, Im: two columns).  Per-pair strides e_fs, w_fs.
// eps == null (the plan's own transform): the input is amp + 0 i.
template <int KIND, int LR, bool SHORT>
__global__ __launch_bounds__(512) void gcs_line_kernel(GcsPass ps, const double* __restrict__ amp, const double* __restrict__ eps,
                                                      double2* W, double* __restrict__ dst, const double2* __restrict__ twg,
                                                      int64_t mtot, int64_t e_fs, int64_t w_fs, int tiles, int64_t ldd,
                                                      int64_t row0, int64_t nloc, int64_t ncols) {
  constexpr int P = SHORT ? (1 << LR) : 16;
  extern __shared__ double2 gsm[];
  const int Ma = ps.Ma, Lg = ps.log2Ma, T = ps.T;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int n16 = SHORT ? 0 : (Lg >> 2);
  const int ltpl = SHORT ? 0 : Lg - 4;
  FftLine f;
  f.L = Lg;
  f.tpl = 1 << ltpl;
  f.tabA = gsm;
  f.tabB = gsm + 64;
  const int ntabB = Ma >= 128 ? (Ma >> 7) : 1;
  double2* buf = gsm + 64 + ntabB;
  const int jl = tid >> ltpl;                      // line of the tile
  f.jt = tid & (f.tpl - 1);
  f.x = buf + (jl < T ? jl : 0) * ps.lstride;
  {
    const int tstep = FFT_TW_LEN / Ma;
    const int half = Ma / 2;                       // Ma >= 2
    if (tid < 64) st2(&gsm[tid], ld2(&twg[(tid < half ? tid : 0) * tstep]));
    for (int b = tid; b < ntabB; b += nth) st2(&gsm[64 + b], ld2(&twg[(b * 64 < half ? b * 64 : 0) * tstep]));
  }
  f.wpl = (f.tpl >= 64) ? (f.tpl >> 6) : 1;
  const int pair = (int)blockIdx.x / tiles;
  const int tile = (int)blockIdx.x - pair * tiles;
  const uint32_t tpo = (ps.nl0 + (uint32_t)T - 1) / (uint32_t)T;
  const uint32_t t1 = (uint32_t)tile / tpo;
  const uint32_t t00 = ((uint32_t)tile - t1 * tpo) * (uint32_t)T;
  const uint32_t nlines = (ps.nl0 - t00 < (uint32_t)T) ? (ps.nl0 - t00) : (uint32_t)T;
  f.act = ((uint32_t)jl < nlines);
  double2* Wp = W + (int64_t)pair * w_fs;
  // ---- the tile's lines into LDS
  {
    const uint32_t nin = (uint32_t)Ma, total = nlines * nin;
    const double* e1 = eps ? eps + (int64_t)pair * e_fs : nullptr;
    for (uint32_t e = (uint32_t)tid; e < total; e += (uint32_t)nth) {
      uint32_t l, k;
      if (ps.contig) { l = e / nin; k = e - l * nin; } else { k = e / nlines; l = e - k * nlines; }
      double2 v;
      if (KIND == GCS_FIRST) {
        const uint32_t i = (t00 + l) * ps.ls0 + k;
        const double a = amp[i];
        v = e1 ? make_double2(a * e1[i], a * e1[mtot + i]) : make_double2(a, 0.0);
      } else {
        v = ld2(&Wp[(t00 + l) * ps.ls0 + t1 * ps.ls1 + k * ps.ks]);
      }
      st2(&buf[l * (uint32_t)ps.lstride + (uint32_t)swz((int)k)], v);
    }
  }
  lds_barrier();
  // ---- the transform
  double2 v[P];
  auto nothing = []() {};
  fft_line<1, LR, SHORT, false, false, true>(v, f, n16, false, 0, nothing);
  // ---- the first A outputs of every line
  {
    const uint32_t nout = (uint32_t)ps.A, total = nlines * nout;
    for (uint32_t e = (uint32_t)tid; e < total; e += (uint32_t)nth) {
      uint32_t l, k;
      if (ps.contig) { l = e / nout; k = e - l * nout; } else { k = e / nlines; l = e - k * nlines; }
      const double2 y = ld2(&buf[l * (uint32_t)ps.lstride + (uint32_t)swz((int)k)]);
      const uint32_t o = (t00 + l) * ps.os0 + t1 * ps.os1 + k * ps.oks;
      if (KIND == GCS_LAST) {
        const int64_t r = (int64_t)o - row0;
        if (r >= 0 && r < nloc) {
          double* d = dst + (int64_t)(2 * pair) * ldd + r;
          d[0] = y.x;
          if ((int64_t)(2 * pair + 1) < ncols) d[ldd] = y.y;
        }
      } else {
        st2(&Wp[o], y);
      }
    }
  }
}

// ---- the plan: the torus covariance, and what is made of its transform -----------------------------------------------
static inline int gcs_grid_for(int64_t total, int cap) {
  int64_t g = (total + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// amp[t0 + M0 (t1 + M1 t2)] = sigma2 k(r(s)), s_a = t_a if t_a <= M_a / 2, else t_a - M_a; u, r and k as fft_lag_table_kernel.
// The mirror point -t mod M has the lag -s (the same value: k is centrally symmetric) except on an axis with t_a = M_a / 2,
// where it is + M_a / 2 again: there the two are averaged -- the even part, which is what the real part of the transform sees.
__global__ __launch_bounds__(256) void gcs_lag_table_kernel(double* __restrict__ amp, int64_t M0, int64_t M1, int64_t M2, int kind,
                                                            double ie0, double ie1, double ie2, double cs, double sn,
                                                            double sigma2) {
  const int64_t total = M0 * M1 * M2;
  pointcov::Params prm;
  prm.d = 3; prm.kind = kind; prm.inv_ell = 1.0; prm.sigma2 = sigma2; prm.nugget = 0.0;
  auto cov = [&](double a0, double a1, double a2) {
    const double u = (cs * a0 + sn * a1) * ie0, v = (-sn * a0 + cs * a1) * ie1, w = a2 * ie2;
    return pointcov::kernel(prm, u * u + v * v + w * w, false);
  };
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t t0 = e % M0, r = e / M0, t1 = r % M1, t2 = r / M1;
    const bool h0 = (2 * t0 == M0), h1 = (2 * t1 == M1), h2 = (2 * t2 == M2);
    const double s0 = (double)(2 * t0 <= M0 ? t0 : t0 - M0), s1 = (double)(2 * t1 <= M1 ? t1 : t1 - M1),
                 s2 = (double)(2 * t2 <= M2 ? t2 : t2 - M2);
    double c = cov(s0, s1, s2);
    if (h0 || h1 || h2) c = 0.5 * (c + cov(h0 ? s0 : -s0, h1 ? s1 : -s1, h2 ? s2 : -s2));
    amp[e] = c;
  }
}
void gcs_lag_table(hipStream_t st, const GcsGeom& g, int kind, const double inv_ell[3], double cs, double sn, double sigma2,
                   double* amp) {
  hipLaunchKernelGGL(gcs_lag_table_kernel, dim3(gcs_grid_for(g.Mtot, 4096)), dim3(256), 0, st, amp, g.M[0], g.M[1], g.M[2], kind,
                     inv_ell[0], inv_ell[1], inv_ell[2], cs, sn, sigma2);
}

// Chunk b of GCS_PARTS: lam += nugget, amp = sqrt(max(lam, 0) / Mtot), and the chunk's part of the four reductions (256 strided
// accumulators and a tree: a fixed order).  part[q GCS_PARTS + b], q = 0 sum of |lam| over lam < 0, 1 min, 2 max, 3 count.
__global__ __launch_bounds__(256) void gcs_finish_kernel(double* __restrict__ lam, double* __restrict__ amp, int64_t Mtot,
                                                         double nugget, double inv_mtot, double* __restrict__ part) {
  __shared__ double s[4][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t chunk = (Mtot + GCS_PARTS - 1) / GCS_PARTS;
  const int64_t i0 = (int64_t)b * chunk, i1 = (i0 + chunk < Mtot) ? i0 + chunk : Mtot;
  double neg = 0.0, mn = INFINITY, mx = -INFINITY, cnt = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += 256) {
    const double l = lam[i] + nugget;
    lam[i] = l;
    amp[i] = sqrt((l > 0.0 ? l : 0.0) * inv_mtot);
    if (l < 0.0) { neg -= l; cnt += 1.0; }
    mn = fmin(mn, l);
    mx = fmax(mx, l);
  }
  s[0][tid] = neg; s[1][tid] = mn; s[2][tid] = mx; s[3][tid] = cnt;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      s[0][tid] += s[0][tid + st];
      s[1][tid] = fmin(s[1][tid], s[1][tid + st]);
      s[2][tid] = fmax(s[2][tid], s[2][tid + st]);
      s[3][tid] += s[3][tid + st];
    }
    __syncthreads();
  }
  if (tid < 4) part[tid * GCS_PARTS + b] = s[tid][0];
}
void gcs_plan_finish(hipStream_t st, const GcsGeom& g, double nugget, double* lam, double* amp, double* part) {
  hipLaunchKernelGGL(gcs_finish_kernel, dim3(GCS_PARTS), dim3(256), 0, st, lam, amp, g.Mtot, nugget, 1.0 / (double)g.Mtot, part);
}

// ---- the passes --------------------------------------------------------------------------------------------------------
static int gcs_ilog2(int64_t v) { int r = 0; while (((int64_t)1 << r) < v) ++r; return r; }

size_t gcs_pair_doubles(const GcsGeom& g) { return (size_t)(2 * g.Mtot + 2 * g.N[0] * g.M[1] * g.M[2]); }

struct GcsLaunch {
  hipStream_t st;
  int threads, nb, tiles;
  size_t shmem;
  const double *amp, *eps; double2* W; double* dst;
  const double2* twg;
  int64_t mtot, e_fs, w_fs, ldd, row0, nloc, ncols;
};

template <int KIND, int LR, bool SHORT>
static void gcs_launch_k(const GcsLaunch& q, const GcsPass& ps) {
  static std::atomic<uint64_t> mask{0};
  if (first_use_on_this_device(mask))
    (void)hipFuncSetAttribute((const void*)gcs_line_kernel<KIND, LR, SHORT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024 - 64);
  hipLaunchKernelGGL((gcs_line_kernel<KIND, LR, SHORT>), dim3((unsigned)((int64_t)q.tiles * q.nb)), dim3(q.threads), q.shmem, q.st,
                     ps, q.amp, q.eps, q.W, q.dst, q.twg, q.mtot, q.e_fs, q.w_fs, q.tiles, q.ldd, q.row0, q.nloc, q.ncols);
}
// the kernel is specialised on the last radix (log2 Ma mod 4) and on lines shorter than 16 points (2, 4 or 8: one thread each)
template <int KIND>
static void gcs_launch_kind(const GcsLaunch& q, const GcsPass& ps) {
  const int lr = ps.log2Ma & 3;
  if (ps.Ma < 16) {
    if (lr == 1) gcs_launch_k<KIND, 1, true>(q, ps);
    else if (lr == 2) gcs_launch_k<KIND, 2, true>(q, ps);
    else gcs_launch_k<KIND, 3, true>(q, ps);
  } else {
    if (lr == 0) gcs_launch_k<KIND, 0, false>(q, ps);
    else if (lr == 1) gcs_launch_k<KIND, 1, false>(q, ps);
    else if (lr == 2) gcs_launch_k<KIND, 2, false>(q, ps);
    else gcs_launch_k<KIND, 3, false>(q, ps);
  }
}

// one axis of nb pairs: N = what survives each axis's crop (the box; the torus itself for the plan's transform)
static void gcs_pass(hipStream_t st, int d, const int64_t* N, const int64_t* M, int axis, int nb, const double2* twg, const double* amp,
                     const double* eps, double2* W, int64_t fs, double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t ncols) {
  GcsPass ps;
  ps.Ma = (int)M[axis]; ps.A = (int)N[axis];
  ps.log2Ma = gcs_ilog2(ps.Ma);
  if (ps.Ma < 2 || ps.Ma > FFT_TW_LEN || (1 << ps.log2Ma) != ps.Ma || ps.A > ps.Ma)
    throw std::runtime_error("gridcov_sample: a line must be a power of two of 2 to 8192 points");
  const bool last = (axis == d - 1);
  ps.contig = (axis == 0);
  ps.ls1 = 0; ps.os1 = 0; ps.nl1 = 1;
  if (axis == 0) {                    // amp, eps (M0, M1, M2) -> W (N0, M1, M2)
    ps.nl0 = (uint32_t)(M[1] * M[2]); ps.ls0 = (uint32_t)M[0]; ps.ks = 1; ps.os0 = (uint32_t)N[0]; ps.oks = 1;
  } else if (axis == 1) {             // lines (i0, t2): element k at i0 + N0 k + N0 M1 t2
    ps.nl0 = (uint32_t)N[0]; ps.nl1 = (uint32_t)M[2]; ps.ls0 = 1; ps.ls1 = (uint32_t)(N[0] * M[1]); ps.ks = (uint32_t)N[0];
    ps.os0 = ps.ls0; ps.os1 = ps.ls1; ps.oks = ps.ks;
    if (last) { ps.os1 = 0; }                                                          // point i0 + N0 k  (M2 = 1)
  } else {                            // lines (i0, i1): element k at i0 + N0 i1 + N0 M1 k
    ps.nl0 = (uint32_t)N[0]; ps.nl1 = (uint32_t)N[1]; ps.ls0 = 1; ps.ls1 = (uint32_t)N[0]; ps.ks = (uint32_t)(N[0] * M[1]);
    ps.os0 = 1; ps.os1 = (uint32_t)N[0]; ps.oks = (uint32_t)(N[0] * N[1]);             // point i0 + N0 (i1 + N1 k)
  }
  const int T = fftrf_tile_lines(ps.Ma, ps.contig != 0, ps.nl0);
  ps.T = T;
  ps.lstride = ps.Ma + ((!ps.contig && T >= 2) ? ((16 / T > 1) ? 16 / T : 1) : 0);
  const int tpl = ps.Ma >= 16 ? ps.Ma / 16 : 1;
  GcsLaunch q;
  q.st = st; q.nb = nb;
  q.threads = (T * tpl + 63) / 64 * 64;
  if (q.threads > 512) throw std::runtime_error("gridcov_sample: tile exceeds 16 points per thread");
  const int ntabB = ps.Ma >= 128 ? ps.Ma / 128 : 1;
  q.shmem = ((size_t)64 + ntabB + (size_t)T * ps.lstride) * sizeof(double2);
  if (q.shmem > (size_t)160 * 1024 - 64) throw std::runtime_error("gridcov_sample: tile exceeds the LDS of a workgroup");
  const int64_t tiles = (int64_t)((ps.nl0 + T - 1) / T) * ps.nl1;
  if (tiles * nb >= ((int64_t)1 << 31)) throw std::runtime_error("gridcov_sample: too many work items");
  q.tiles = (int)tiles;
  q.amp = amp; q.eps = eps; q.W = W; q.dst = dst; q.twg = twg;
  q.mtot = M[0] * M[1] * M[2];
  q.e_fs = fs; q.w_fs = fs / 2;                      // fs doubles per pair in every section: W counts in complex elements
  q.ldd = ldd; q.row0 = row0; q.nloc = nloc; q.ncols = ncols;
  if (axis == 0) gcs_launch_kind<GCS_FIRST>(q, ps);
  else if (!last) gcs_launch_kind<GCS_MIDDLE>(q, ps);
  else gcs_launch_kind<GCS_LAST>(q, ps);
}

void gcs_plan_transform(hipStream_t st, const GcsGeom& g, const double* twg, const double* amp, double* W, double* lam) {
  for (int a = 0; a < g.d; ++a)
    gcs_pass(st, g.d, g.M, g.M, a, 1, reinterpret_cast<const double2*>(twg), amp, nullptr, reinterpret_cast<double2*>(W), 0, lam,
             g.Mtot, 0, g.Mtot, 1);
}

void gcs_sample(hipStream_t st, const GcsGeom& g, const double* twg, const double* amp, double* ws, int64_t fs, int nb, double* dst,
                int64_t ldd, int64_t row0, int64_t nloc, int64_t ncols) {
  if (nloc <= 0) return;
  for (int a = 0; a < g.d; ++a)
    gcs_pass(st, g.d, g.N, g.M, a, nb, reinterpret_cast<const double2*>(twg), amp, ws, reinterpret_cast<double2*>(ws + 2 * g.Mtot),
             fs, dst, ldd, row0, nloc, ncols);
}

}}  // namespace gsi::hipk
