// fftrf_sample.hip -- FFTRF.powerlaw_structuredgrid (FFTRF.jl:83-100) sampled on the device, a batch of fields at a time.
//
// One field:  K = sqrtS .* exp(2 pi i phi) on the EXACTLY doubled grid, stored (2 N_2, 2 N_1[, 2 N_3]) -- the reference's
// axis swap: the first, fastest axis runs over coordinate 2 --, field = Re ifftn(K) cropped to the first N_a points per
// axis, axes 1 and 2 swapped back, then dk (f - mean) / std + k0 with the corrected std over the field's n points.
//
// The transform is separable and the crop can follow each axis's pass at once, so with A = (N_2, N_1, N_3) the half
// lengths along the ARRAY axes and L = 2 A:
//   pass 1  lines along array axis 0 (contiguous), all L_1 L_2 of them: builds sqrtS e^{2 pi i phi} while loading phi,
//           unnormalised inverse DFT, stores the first A_0 outputs into W (A_0 x L_1 x L_2 complex);
//   pass 2  lines along axis 1 (stride A_0), tiles of neighbouring lines, in place, first A_1 outputs;
//   pass 3  (3-D) lines along axis 2 (stride A_0 L_1), in place, first A_2 outputs;
//   the LAST pass writes only Re / Mtot, in the point order of finalk (j + N_1 (i + N_2 h) for array element (i, j, h));
//   two fixed-order reductions give each field's mean and corrected std; the normalising write fills the caller's rows.
// A line of L points is one inverse Stockham transform when L is a power of two, and Bluestein's chirp-z otherwise:
//   c_j = exp(i pi (j^2 mod 2L) / L),   y_j = c_j sum_k (x_k c_k) conj(c)_{j - k},   j < A,
// a circular convolution of length P = next power of two >= L + A - 1: load x chirp, zero padding, forward transform of
// length P, times the chirp's spectrum, inverse transform of length P, first A outputs x chirp / P -- forward, multiply,
// inverse while the line sits in LDS and registers, the shape of fft_cov.hip's fused pass.  One workgroup per
// (field, tile); nothing here depends on how many fields share a launch.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include "hip_common.hpp"
#include "fft_line.hpp"

namespace gsi { namespace hipk {

enum { FRF_FIRST = 0, FRF_MIDDLE = 1, FRF_LAST = 2 };
constexpr int FRF_PARTS = 64;        // partial sums per field and reduction: fixed, so a field's bits are too

struct FrfPass {
  int Ma, log2Ma;             // transform length: P (Bluestein) or L (direct)
  int L, A;                   // points of a line on the doubled grid; outputs that survive the crop
  int T, lstride;             // lines per tile; elements between the lines of a tile in LDS
  int contig, drain_kfast;    // fill / drain order: position fastest (else line fastest)
  uint32_t nl0, nl1;          // lines (t0, t1), t0 < nl0, t1 < nl1; a tile = T neighbouring t0 at one t1
  uint32_t ls0, ls1, ks;      // input element k of line (t0, t1):  t0 ls0 + t1 ls1 + k ks
  uint32_t os0, os1, oks;     // output element k of that line:     t0 os0 + t1 os1 + k oks
  uint32_t L1, L2;            // FIRST: line t0 = j + L1 h;  wavenumbers min(j, L1 - j), min(h, L2 - h)
  double invP;                // Bluestein: 1 / P
};

// KIND FIRST: phi -> W;  MIDDLE: W -> W in place;  LAST: W -> R (real part, scaled).  Per-field strides phi_fs, w_fs, r_fs.
template <int KIND, bool BLUE, int LR, bool SHORT>
__global__ __launch_bounds__(512) void fftrf_line_kernel(FrfPass ps, const double* __restrict__ phi, double2* W,
                                                        double* __restrict__ R, const double2* __restrict__ twg,
                                                        const double2* __restrict__ chirp, const double2* __restrict__ bspec,
                                                        int64_t phi_fs, int64_t w_fs, int64_t r_fs, int tiles, double beta4,
                                                        double scale) {
  constexpr int P = SHORT ? (1 << LR) : 16;
  extern __shared__ double2 fsm[];
  const int Ma = ps.Ma, Lg = ps.log2Ma, T = ps.T;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int n16 = SHORT ? 0 : (Lg >> 2);
  const int ltpl = SHORT ? 0 : Lg - 4;
  FftLine f;
  f.L = Lg;
  f.tpl = 1 << ltpl;
  f.tabA = fsm;
  f.tabB = fsm + 64;
  const int ntabB = Ma >= 128 ? (Ma >> 7) : 1;
  double2* buf = fsm + 64 + ntabB;
  const int jl = tid >> ltpl;                      // line of the tile
  f.jt = tid & (f.tpl - 1);
  f.x = buf + (jl < T ? jl : 0) * ps.lstride;
  {
    const int tstep = FFT_TW_LEN / Ma;
    const int half = Ma >= 2 ? Ma / 2 : 1;
    if (tid < 64) st2(&fsm[tid], ld2(&twg[(tid < half ? tid : 0) * tstep]));
    for (int b = tid; b < ntabB; b += nth) st2(&fsm[64 + b], ld2(&twg[(b * 64 < half ? b * 64 : 0) * tstep]));
  }
  f.wpl = (f.tpl >= 64) ? (f.tpl >> 6) : 1;
  const int fld = (int)blockIdx.x / tiles;
  const int tile = (int)blockIdx.x - fld * tiles;
  const uint32_t tpo = (ps.nl0 + (uint32_t)T - 1) / (uint32_t)T;
  const uint32_t t1 = (uint32_t)tile / tpo;
  const uint32_t t00 = ((uint32_t)tile - t1 * tpo) * (uint32_t)T;
  const uint32_t nlines = (ps.nl0 - t00 < (uint32_t)T) ? (ps.nl0 - t00) : (uint32_t)T;
  f.act = ((uint32_t)jl < nlines);
  const double* phif = phi + (int64_t)fld * phi_fs;
  double2* Wf = W + (int64_t)fld * w_fs;
  // ---- the tile's lines into LDS (positions >= L are the zero padding of the first gather, never written)
  {
    const uint32_t nin = (uint32_t)ps.L, total = nlines * nin;
    for (uint32_t e = (uint32_t)tid; e < total; e += (uint32_t)nth) {
      uint32_t l, k;
      if (ps.contig) { l = e / nin; k = e - l * nin; } else { k = e / nlines; l = e - k * nlines; }
      double2 v;
      if (KIND == FRF_FIRST) {
        const uint32_t line = t00 + l;
        const double ph = phif[line * ps.ls0 + k];
        const uint32_t h = line / ps.L1, j = line - h * ps.L1;
        const double w0 = (double)(k <= nin - k ? k : nin - k);          // integer wavenumbers 0..N, -(N-1)..-1  (FFTRF.jl:86-89)
        const double w1 = (double)(j <= ps.L1 - j ? j : ps.L1 - j);
        const double w2 = (double)(h <= ps.L2 - h ? h : ps.L2 - h);
        const double S = w0 * w0 + w1 * w1 + w2 * w2;
        const double a = (S > 0.0) ? pow(S, beta4) : ((beta4 == 0.0) ? 1.0 : 0.0);   // S ^ (beta / 4), inf -> 0  (:62-66)
        double sn, cs;
        sincospi(2.0 * ph, &sn, &cs);                                    // cospi(2 phi), sinpi(2 phi): exact reduction  (:78)
        v = make_double2(a * cs, a * sn);
      } else {
        v = ld2(&Wf[(t00 + l) * ps.ls0 + t1 * ps.ls1 + k * ps.ks]);
      }
      if (BLUE) v = cmul(v, ld2(&chirp[k]));
      st2(&buf[l * (uint32_t)ps.lstride + (uint32_t)swz((int)k)], v);
    }
  }
  lds_barrier();
  // ---- the transform
  double2 v[P];
  auto nothing = []() {};
  if (BLUE) {
    fft_line<-1, LR, SHORT, false, true, true>(v, f, n16, true, ps.L, nothing);
#pragma unroll
    for (int s = 0; s < P; ++s) v[s] = cmul(v[s], ld2(&bspec[f.jt + s * f.tpl]));
    fft_line<1, LR, SHORT, true, false, true>(v, f, n16, false, 0, nothing);
  } else {
    fft_line<1, LR, SHORT, false, false, true>(v, f, n16, false, 0, nothing);
  }
  // ---- the first A outputs of every line
  {
    const uint32_t nout = (uint32_t)ps.A, total = nlines * nout;
    double* Rf = R + (int64_t)fld * r_fs;
    for (uint32_t e = (uint32_t)tid; e < total; e += (uint32_t)nth) {
      uint32_t l, k;
      if (ps.drain_kfast) { l = e / nout; k = e - l * nout; } else { k = e / nlines; l = e - k * nlines; }
      double2 y = ld2(&buf[l * (uint32_t)ps.lstride + (uint32_t)swz((int)k)]);
      if (BLUE) {
        y = cmul(y, ld2(&chirp[k]));
        y.x *= ps.invP;
        y.y *= ps.invP;
      }
      const uint32_t o = (t00 + l) * ps.os0 + t1 * ps.os1 + k * ps.oks;
      if (KIND == FRF_LAST) Rf[o] = y.x * scale; else st2(&Wf[o], y);
    }
  }
}

// Per-axis plan data of a Bluestein axis: chirp[j] = c_j, j < L, and bspec = F_P b, b_m = conj(c_|m|) at m mod P for
// -(L - 1) <= m <= A - 1, built with the line transform itself (one workgroup).
template <int LR, bool SHORT>
__global__ __launch_bounds__(512) void fftrf_chirp_kernel(int P_, int log2P, int L, int A, const double2* __restrict__ twg,
                                                         double2* __restrict__ chirp, double2* __restrict__ bspec) {
  constexpr int P = SHORT ? (1 << LR) : 16;
  extern __shared__ double2 fsm[];
  const int Ma = P_;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int n16 = SHORT ? 0 : (log2P >> 2);
  const int ltpl = SHORT ? 0 : log2P - 4;
  FftLine f;
  f.L = log2P;
  f.tpl = 1 << ltpl;
  f.tabA = fsm;
  f.tabB = fsm + 64;
  const int ntabB = Ma >= 128 ? (Ma >> 7) : 1;
  double2* buf = fsm + 64 + ntabB;
  const int jl = tid >> ltpl;
  f.jt = tid & (f.tpl - 1);
  f.x = buf;
  f.act = (jl == 0);
  {
    const int tstep = FFT_TW_LEN / Ma;
    const int half = Ma >= 2 ? Ma / 2 : 1;
    if (tid < 64) st2(&fsm[tid], ld2(&twg[(tid < half ? tid : 0) * tstep]));
    for (int b = tid; b < ntabB; b += nth) st2(&fsm[64 + b], ld2(&twg[(b * 64 < half ? b * 64 : 0) * tstep]));
  }
  f.wpl = (f.tpl >= 64) ? (f.tpl >> 6) : 1;
  auto chirp_of = [&](int j) -> double2 {
    const int64_t r = ((int64_t)j * (int64_t)j) % (int64_t)(2 * L);      // the INTEGER j^2 mod 2L, then the division
    double sn, cs;
    sincospi((double)r / (double)L, &sn, &cs);
    return make_double2(cs, sn);
  };
  for (int m = tid; m < Ma; m += nth) {
    double2 b = make_double2(0.0, 0.0);
    if (m <= A - 1) { b = chirp_of(m); b.y = -b.y; }
    else if (Ma - m <= L - 1) { b = chirp_of(Ma - m); b.y = -b.y; }
    st2(&buf[swz(m)], b);
  }
  for (int j = tid; j < L; j += nth) st2(&chirp[j], chirp_of(j));
  lds_barrier();
  double2 v[P];
  auto nothing = []() {};
  fft_line<-1, LR, SHORT, false, false, true>(v, f, n16, false, 0, nothing);
  for (int m = tid; m < Ma; m += nth) st2(&bspec[m], ld2(&buf[swz(m)]));
}

__global__ __launch_bounds__(256) void fftrf_twiddle_kernel(double2* __restrict__ twg) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < FFT_TW_LEN / 2) {
    double s, c;
    sincospi(2.0 * (double)k / (double)FFT_TW_LEN, &s, &c);
    twg[k] = make_double2(c, -s);
  }
}

// ---- per-field mean and corrected std: two reductions in a fixed order (FRF_PARTS chunks per field, 256 strided
//      accumulators and a tree per chunk, the partials summed left to right) ------------------------------------------
// part[field][0][b] = sum over chunk b of R;  second: part[field][1][b] = sum over chunk b of (R - mean)^2
__global__ __launch_bounds__(256) void fftrf_sum_kernel(const double* __restrict__ R, int64_t r_fs, int64_t n,
                                                       double* part, int second) {
  __shared__ double s[256];
  const int fld = blockIdx.y, b = blockIdx.x;
  const double* Rf = R + (int64_t)fld * r_fs;
  double* pf = part + (int64_t)fld * r_fs;
  double mean = 0.0;
  if (second) {
    for (int i = 0; i < FRF_PARTS; ++i) mean += pf[i];
    mean /= (double)n;
  }
  const int64_t chunk = (n + FRF_PARTS - 1) / FRF_PARTS;
  const int64_t i0 = (int64_t)b * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
  double acc = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const double t = Rf[i] - mean;
    acc += second ? t * t : t;
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) pf[second * FRF_PARTS + b] = s[0];
}

// dst[(r - row0) + field ldd] = dk (R[r] - mean) / std + k0 for r in [row0, row0 + nloc)   (FFTRF.jl:94-98)
__global__ __launch_bounds__(256) void fftrf_normalise_kernel(const double* __restrict__ R, int64_t r_fs, int64_t n,
                                                             const double* __restrict__ part, double k0, double dk,
                                                             double* __restrict__ dst, int64_t ldd, int64_t row0, int64_t nloc) {
  const int fld = blockIdx.y;
  const double* Rf = R + (int64_t)fld * r_fs;
  const double* pf = part + (int64_t)fld * r_fs;
  double mean = 0.0, ss = 0.0;
  for (int i = 0; i < FRF_PARTS; ++i) mean += pf[i];
  mean /= (double)n;
  for (int i = 0; i < FRF_PARTS; ++i) ss += pf[FRF_PARTS + i];
  const double sd = sqrt(ss / (double)(n - 1));          // zero or non-finite: NaN fields, as the reference returns
  double* df = dst + (int64_t)fld * ldd;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nloc; r += (int64_t)gridDim.x * 256)
    df[r] = dk * (Rf[row0 + r] - mean) / sd + k0;
}

static int frf_ilog2(int64_t v) { int r = 0; while (((int64_t)1 << r) < v) ++r; return r; }

void fftrf_geometry(int ndims, const int64_t* N, FftrfGeom* g) {
  g->d = ndims;
  g->A[0] = N[1]; g->A[1] = N[0]; g->A[2] = (ndims == 3) ? N[2] : 1;
  g->Mtot = 1; g->n = 1;
  for (int a = 0; a < 3; ++a) {
    const bool real_axis = a < ndims;
    g->L[a] = real_axis ? 2 * g->A[a] : 1;
    const int64_t L = g->L[a];
    g->blue[a] = real_axis && (L & (L - 1)) != 0;
    int64_t P = L;
    if (g->blue[a]) { P = 1; while (P < L + g->A[a] - 1) P <<= 1; }
    g->P[a] = P;
    g->Mtot *= L;
    g->n *= g->A[a];
  }
}

// plan: [FFT_TW_LEN doubles of twiddles | per Bluestein axis: chirp (L complex), spectrum (P complex)]
static size_t frf_axis_offset(const FftrfGeom& g, int axis) {
  size_t off = FFT_TW_LEN;
  for (int a = 0; a < axis; ++a) if (g.blue[a]) off += 2 * (size_t)(g.L[a] + g.P[a]);
  return off;
}
size_t fftrf_plan_doubles(const FftrfGeom& g) { return frf_axis_offset(g, 3); }
// per field of a batch: phi (Mtot) | W (A_0 L_1 L_2 complex = Mtot doubles) | R (n) | partial sums
size_t fftrf_field_doubles(const FftrfGeom& g) { return (size_t)(2 * g.Mtot + g.n + 2 * FRF_PARTS); }

template <class K>
static void frf_allow_lds(K kernel, std::atomic<uint64_t>& mask) {
  if (first_use_on_this_device(mask))
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
}

template <int LR, bool SHORT>
static void frf_chirp_k(hipStream_t st, int threads, size_t shmem, int P, int L, int A, const double2* twg, double2* chirp,
                        double2* bspec) {
  static std::atomic<uint64_t> mask{0};
  frf_allow_lds(fftrf_chirp_kernel<LR, SHORT>, mask);
  hipLaunchKernelGGL((fftrf_chirp_kernel<LR, SHORT>), dim3(1), dim3(threads), shmem, st, P, frf_ilog2(P), L, A, twg, chirp, bspec);
}

void fftrf_twiddles(hipStream_t st, double* twg) {
  hipLaunchKernelGGL(fftrf_twiddle_kernel, dim3(FFT_TW_LEN / 2 / 256), dim3(256), 0, st, reinterpret_cast<double2*>(twg));
}
void fftrf_plan(hipStream_t st, const FftrfGeom& g, double* plan) {
  double2* twg = reinterpret_cast<double2*>(plan);
  fftrf_twiddles(st, plan);
  for (int a = 0; a < g.d; ++a) {
    if (!g.blue[a]) continue;
    const int P = (int)g.P[a], L = (int)g.L[a], A = (int)g.A[a];
    double2* chirp = reinterpret_cast<double2*>(plan + frf_axis_offset(g, a));
    double2* bspec = chirp + L;
    const int tpl = P >= 16 ? P / 16 : 1;
    const int threads = (tpl + 63) / 64 * 64;
    const int ntabB = P >= 128 ? P / 128 : 1;
    const size_t shmem = ((size_t)64 + ntabB + P) * sizeof(double2);
    const int lr = frf_ilog2(P) & 3;
    if (P < 16) frf_chirp_k<3, true>(st, threads, shmem, P, L, A, twg, chirp, bspec);       // P = 8: the only short Bluestein line
    else if (lr == 0) frf_chirp_k<0, false>(st, threads, shmem, P, L, A, twg, chirp, bspec);
    else if (lr == 1) frf_chirp_k<1, false>(st, threads, shmem, P, L, A, twg, chirp, bspec);
    else if (lr == 2) frf_chirp_k<2, false>(st, threads, shmem, P, L, A, twg, chirp, bspec);
    else frf_chirp_k<3, false>(st, threads, shmem, P, L, A, twg, chirp, bspec);
  }
}

struct FrfLaunch {
  hipStream_t st;
  int threads, nb, tiles;
  size_t shmem;
  const double* phi; double2* W; double* R;
  const double2 *twg, *chirp, *bspec;
  int64_t phi_fs, w_fs, r_fs;
  double beta4, scale;
};

template <int KIND, bool BLUE, int LR, bool SHORT>
static void frf_launch_k(const FrfLaunch& q, const FrfPass& ps) {
  static std::atomic<uint64_t> mask{0};
  frf_allow_lds(fftrf_line_kernel<KIND, BLUE, LR, SHORT>, mask);
  hipLaunchKernelGGL((fftrf_line_kernel<KIND, BLUE, LR, SHORT>), dim3((unsigned)((int64_t)q.tiles * q.nb)), dim3(q.threads), q.shmem,
                     q.st, ps, q.phi, q.W, q.R, q.twg, q.chirp, q.bspec, q.phi_fs, q.w_fs, q.r_fs, q.tiles, q.beta4, q.scale);
}
// the kernel is specialised on the last radix (log2 Ma mod 4), on lines shorter than 16 points and on Bluestein / direct.
// Short lines: a direct line of 2, 4 or 8 points, or the 8-point Bluestein line of N = 3 (P >= 3 N - 1 leaves no other).
template <int KIND, bool BLUE>
static void frf_launch_kb(const FrfLaunch& q, const FrfPass& ps) {
  const int lr = ps.log2Ma & 3;
  if (ps.Ma < 16) {
    if (BLUE) {
      if (ps.Ma != 8) throw std::runtime_error("fftrf_sample: a Bluestein line shorter than 8 points");
      frf_launch_k<KIND, BLUE, 3, true>(q, ps);
    } else {
      if (lr == 1) frf_launch_k<KIND, false, 1, true>(q, ps);
      else if (lr == 2) frf_launch_k<KIND, false, 2, true>(q, ps);
      else frf_launch_k<KIND, false, 3, true>(q, ps);
    }
  } else {
    if (lr == 0) frf_launch_k<KIND, BLUE, 0, false>(q, ps);
    else if (lr == 1) frf_launch_k<KIND, BLUE, 1, false>(q, ps);
    else if (lr == 2) frf_launch_k<KIND, BLUE, 2, false>(q, ps);
    else frf_launch_k<KIND, BLUE, 3, false>(q, ps);
  }
}

// lines per tile.  Contiguous lines need no neighbours: up to 32 within 64 KB of LDS.  Strided lines want long segments: up
// to 16 neighbours (256 bytes).  Both within 8192 points = 16 per thread x 512 threads (short lines: one thread per line).
int fftrf_tile_lines(int Ma, bool contiguous, int64_t nl0) {
  const int tpl = Ma >= 16 ? Ma / 16 : 1;
  int T = 512 / tpl;
  if (contiguous) {
    const int lds = (4096 / Ma > 1) ? 4096 / Ma : 1;
    if (T > lds) T = lds;
    if (T > 32) T = 32;
  } else {
    if (T > 16) T = 16;
  }
  if (T > nl0) T = (int)nl0;
  return T < 1 ? 1 : T;
}

static void frf_pass(hipStream_t st, const FftrfGeom& g, int axis, int nb, const double* plan, double* ws_phi, double* ws_w,
                     double* ws_r, int64_t fs, double beta) {
  const int64_t* A = g.A;
  const int64_t* L = g.L;
  FrfPass ps;
  ps.L = (int)L[axis]; ps.A = (int)A[axis];
  ps.Ma = (int)g.P[axis];
  ps.log2Ma = frf_ilog2(ps.Ma);
  ps.invP = 1.0 / (double)ps.Ma;
  ps.L1 = (uint32_t)L[1]; ps.L2 = (uint32_t)L[2];
  const bool last = (axis == g.d - 1);
  ps.contig = (axis == 0);
  ps.ls1 = 0; ps.os1 = 0; ps.nl1 = 1;
  if (axis == 0) {                    // phi (L0, L1, L2) -> W (A0, L1, L2)
    ps.nl0 = (uint32_t)(L[1] * L[2]); ps.ls0 = (uint32_t)L[0]; ps.ks = 1; ps.os0 = (uint32_t)A[0]; ps.oks = 1;
  } else if (axis == 1) {             // lines (i, h): element k at i + A0 k + A0 L1 h
    ps.nl0 = (uint32_t)A[0]; ps.nl1 = (uint32_t)L[2]; ps.ls0 = 1; ps.ls1 = (uint32_t)(A[0] * L[1]); ps.ks = (uint32_t)A[0];
    ps.os0 = ps.ls0; ps.os1 = ps.ls1; ps.oks = ps.ks;
    if (last) { ps.os0 = (uint32_t)A[1]; ps.os1 = 0; ps.oks = 1; }                    // finalk[j, i] at j + N_1 i
  } else {                            // lines (i, j): element k at i + A0 j + A0 L1 k
    ps.nl0 = (uint32_t)A[0]; ps.nl1 = (uint32_t)A[1]; ps.ls0 = 1; ps.ls1 = (uint32_t)A[0]; ps.ks = (uint32_t)(A[0] * L[1]);
    ps.os0 = (uint32_t)A[1]; ps.os1 = 1; ps.oks = (uint32_t)(A[1] * A[0]);            // finalk[j, i, h] at j + N_1 (i + N_2 h)
  }
  ps.drain_kfast = (ps.contig || (last && ps.oks == 1)) ? 1 : 0;
  const int T = fftrf_tile_lines(ps.Ma, ps.contig != 0, ps.nl0);
  ps.T = T;
  ps.lstride = ps.Ma + ((!ps.contig && T >= 2) ? ((16 / T > 1) ? 16 / T : 1) : 0);
  const int tpl = ps.Ma >= 16 ? ps.Ma / 16 : 1;
  FrfLaunch q;
  q.st = st; q.nb = nb;
  q.threads = (T * tpl + 63) / 64 * 64;
  if (q.threads > 512) throw std::runtime_error("fftrf_sample: tile exceeds 16 points per thread");
  const int ntabB = ps.Ma >= 128 ? ps.Ma / 128 : 1;
  q.shmem = ((size_t)64 + ntabB + (size_t)T * ps.lstride) * sizeof(double2);
  const int64_t tiles = (int64_t)((ps.nl0 + T - 1) / T) * ps.nl1;
  if (tiles * nb >= ((int64_t)1 << 31)) throw std::runtime_error("fftrf_sample: too many work items");
  q.tiles = (int)tiles;
  q.phi = ws_phi; q.W = reinterpret_cast<double2*>(ws_w); q.R = ws_r;
  q.phi_fs = fs; q.w_fs = fs / 2; q.r_fs = fs;        // fs doubles per field in every section: W counts in complex elements
  q.twg = reinterpret_cast<const double2*>(plan);
  q.chirp = reinterpret_cast<const double2*>(plan + frf_axis_offset(g, axis));
  q.bspec = q.chirp + L[axis];
  q.beta4 = 0.25 * beta;
  q.scale = 1.0 / (double)g.Mtot;
  const bool blue = g.blue[axis] != 0;
  if (axis == 0) { if (blue) frf_launch_kb<FRF_FIRST, true>(q, ps); else frf_launch_kb<FRF_FIRST, false>(q, ps); }
  else if (!last) { if (blue) frf_launch_kb<FRF_MIDDLE, true>(q, ps); else frf_launch_kb<FRF_MIDDLE, false>(q, ps); }
  else { if (blue) frf_launch_kb<FRF_LAST, true>(q, ps); else frf_launch_kb<FRF_LAST, false>(q, ps); }
}

// nb fields whose phi sits in ws (field b at ws + b fs): the passes, the statistics and the normalising write of rows
// [row0, row0 + nloc) into dst (column b at dst + b ldd).  fs = fftrf_field_doubles rounded up to an even count.
void fftrf_sample(hipStream_t st, const FftrfGeom& g, const double* plan, double* ws, int64_t fs, int nb, double k0, double dk,
                  double beta, double* dst, int64_t ldd, int64_t row0, int64_t nloc) {
  double* ws_phi = ws;
  double* ws_w = ws + g.Mtot;
  double* ws_r = ws + 2 * g.Mtot;
  double* part = ws + 2 * g.Mtot + g.n;
  for (int a = 0; a < g.d; ++a) frf_pass(st, g, a, nb, plan, ws_phi, ws_w, ws_r, fs, beta);
  hipLaunchKernelGGL(fftrf_sum_kernel, dim3(FRF_PARTS, nb), dim3(256), 0, st, ws_r, fs, g.n, part, 0);
  hipLaunchKernelGGL(fftrf_sum_kernel, dim3(FRF_PARTS, nb), dim3(256), 0, st, ws_r, fs, g.n, part, 1);
  if (nloc > 0) {
    int64_t gx = (nloc + 255) / 256;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(fftrf_normalise_kernel, dim3((unsigned)gx, nb), dim3(256), 0, st, ws_r, fs, g.n, part, k0, dk, dst, ldd,
                       row0, nloc);
  }
}

}}  // namespace gsi::hipk
