// fft_line.hpp -- the line transform of the FFT kernels: complex helpers, the LDS-only barrier, the bank swizzle and the
// radix-16 Stockham transform of one line held in LDS and registers.  Shared by fft_cov.hip (the covariance products) and
// fftrf_sample.hip (the FFTRF field sampler); device code only, every function forced inline.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gsi { namespace hipk {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 csqr(double2 a) { return make_double2(a.x * a.x - a.y * a.y, (a.x + a.x) * a.y); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
// Loads and stores by component: an assignment of the double2 STRUCT between address spaces becomes an llvm.memcpy,
// and an array that is the source or target of one stays in scratch memory instead of registers.
__device__ __forceinline__ double2 ld2(const double2* p) { return make_double2(p->x, p->y); }
__device__ __forceinline__ void st2(double2* p, double2 v) { p->x = v.x; p->y = v.y; }

constexpr int FFT_TW_LEN = 8192;     // longest supported line; the plan stores exp(-2 pi i k / 8192), k < 4096

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt -- every global load and store in
// flight -- which is exactly what the persistent pass must not do: the next item's loads and the previous item's
// stores are meant to stay in flight across the butterflies.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---- the transform of one line: Stockham autosort, radix 16 in registers -------------------------------------------
// A thread owns 16 points of its line: slot s <-> position jt + s * Ma/16 (jt = the thread's index within the line).
// Every stage of a Stockham decimation-in-time transform reads exactly those positions whatever its radix R (the
// inputs of butterfly jb = jt + c Ma/16, c < 16/R, are jb + r Ma/R = jt + (c + r 16/R) Ma/16), so a stage is
//     load 16 slots | twiddle, 16/R R-point DFTs in registers | barrier | scatter to (jb - k) R + k + m Ns | barrier
// with k = jb mod Ns, Ns = the product of the earlier radices.  Ma = 16^a * {1, 2, 4, 8}: a radix-16 stages and at
// most one smaller one LAST, so a 2048-point line is three LDS round trips (the radix-2/4 butterflies this replaces
// took six, and 60 % of their LDS cycles were bank conflicts).  Natural order in and out: no bit reversal anywhere,
// and the last stage of a forward transform leaves the thread holding the very slots the first stage of the inverse
// wants -- the fused pass multiplies by the spectrum in registers in between.
// LDS banking: element i of a line lives at i ^ ((i >> 4) & 15) (16-byte elements, 16 to a 256-byte bank row).  The
// loads are aligned runs of 16 consecutive elements per 16 lanes (a permutation within the row: conflict-free); the
// scatter of the first stage (lane stride 16 elements) lands in 16 different rows at 16 different columns; later
// stages scatter aligned runs again.
__device__ __forceinline__ int swz(int i) { return i ^ ((i >> 4) & 15); }
// A value the optimiser may not treat as loop-invariant: the per-element offsets and masks of an item's fill and drain
// are cheap to recompute, and hoisted out of the persistent loop they occupied (and spilled) ~100 registers.
__device__ __forceinline__ int opaque(int x) { asm volatile("" : "+v"(x)); return x; }

// W_16^(sgn * i) for i < 8, folded at compile time once the caller's loops are unrolled
__device__ __forceinline__ double2 mul_w16(double2 v, int i, int sgn) {
  if (i == 0) return v;
  if (i == 4) return sgn > 0 ? make_double2(-v.y, v.x) : make_double2(v.y, -v.x);
  const double C1 = 0.92387953251128673848, S1 = 0.38268343236508977173, H = 0.70710678118654752440;
  const double c = (i == 1) ? C1 : (i == 2) ? H : (i == 3) ? S1 : (i == 5) ? -S1 : (i == 6) ? -H : -C1;
  const double sa = (i == 1 || i == 7) ? S1 : (i == 2 || i == 6) ? H : C1;
  const double s = sgn > 0 ? sa : -sa;
  return make_double2(v.x * c - v.y * s, v.x * s + v.y * c);
}

// R-point DFT of a[0..R), natural order in and out: decimation in frequency, then the even/odd halves interleaved
// (register renaming once everything is unrolled)
template <int R, int SGN>
__device__ __forceinline__ void dft_regs(double2* a) {
  if constexpr (R > 1) {
    constexpr int H = R / 2;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const double2 t = csub(a[i], a[i + H]);
      a[i] = cadd(a[i], a[i + H]);
      a[i + H] = mul_w16(t, i * (16 / R), SGN);
    }
    dft_regs<H, SGN>(a);
    dft_regs<H, SGN>(a + H);
    double2 t[R];
#pragma unroll
    for (int i = 0; i < H; ++i) { t[2 * i] = a[i]; t[2 * i + 1] = a[i + H]; }
#pragma unroll
    for (int i = 0; i < R; ++i) a[i] = t[i];
  }
}

struct FftLine {            // what a thread knows about its line
  double2* x;               // the line in LDS
  const double2* tabA;      // W_Ma^a, a < 64 (forward sign)
  const double2* tabB;      // W_Ma^(64 b)
  int jt, tpl, L;           // index within the line, threads per line (Ma / points per thread), log2 Ma
  bool act;                 // writes anything at all (a thread past the tile's lines only keeps the barriers company)
  int wpl;                  // waves per line (1: a wave holds whole lines)
};

// Barrier between the stages of ONE line (round 4).  A line belongs to tpl = Ma / 16 threads -- one wave at 1024 points, two at
// 2048 -- and a stage boundary only orders the LDS traffic of that line's own waves.  With one wave per line (or several lines
// per wave) there is nothing to wait for: the LDS executes a wave's instructions in order, a later ds_read of any lane sees
// an earlier ds_write of any lane; only the compiler must not reorder them.  Measured at 512^3 (1024-point lines: 9 of the
// fused item's 12 workgroup barriers gone): 134.5 -> 131.1 ms per 16 columns -- 2.6 %, which says the barriers were never
// what the pass waits for.  With two waves per line an arrival counter in LDS (ds_add, poll) was built and measured SLOWER than
// s_barrier (1000^2: 6.68 -> 6.95 ms) and removed: lines that span waves keep the workgroup barrier.
// Fills and drains of a strided tile touch every line from every thread and keep the workgroup barrier too.
__device__ __forceinline__ void line_barrier(const FftLine& f) {
  if (f.wpl <= 1) { asm volatile("" ::: "memory"); return; }
  lds_barrier();
}

// twiddle and NB R-point DFTs over the slots c + r NB.  Ns = 1 << lNs.
template <int R, int NB, int SGN>
__device__ __forceinline__ void stage_compute(double2 (&v)[R * NB], const FftLine& f, int lNs) {
  constexpr int LR = (R == 16) ? 4 : (R == 8) ? 3 : (R == 4) ? 2 : 1;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    double2 a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = v[c + r * NB];
    if (lNs > 0) {
      const int jb = f.jt + c * f.tpl;
      const int k = jb & ((1 << lNs) - 1);
      const int t = k << (f.L - lNs - LR);                // W_{Ns R}^k = W_Ma^t
      double2 w1 = cmul(ld2(&f.tabA[t & 63]), ld2(&f.tabB[t >> 6]));
      if (SGN > 0) w1.y = -w1.y;
      // W^r from the binary powers W, W^2, W^4, W^8 as it is needed: few live registers, short dependency chains
      double2 pw[4];
      pw[0] = w1;
#pragma unroll
      for (int b = 1; b < LR; ++b) pw[b] = csqr(pw[b - 1]);
#pragma unroll
      for (int r = 1; r < R; ++r) {
        double2 wr = make_double2(1.0, 0.0);
        bool have = false;
#pragma unroll
        for (int b = 0; b < LR; ++b)
          if (r & (1 << b)) { wr = have ? cmul(wr, pw[b]) : pw[b]; have = true; }
        a[r] = cmul(a[r], wr);
      }
    }
    dft_regs<R, SGN>(a);
#pragma unroll
    for (int m = 0; m < R; ++m) v[c + m * NB] = a[m];
  }
}
template <int R, int NB>
__device__ __forceinline__ void stage_scatter(const double2 (&v)[R * NB], const FftLine& f, int lNs) {
  constexpr int LR = (R == 16) ? 4 : (R == 8) ? 3 : (R == 4) ? 2 : 1;
  if (!f.act) return;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const int jb = f.jt + c * f.tpl;
    const int k = jb & ((1 << lNs) - 1);
    const int base = ((jb - k) << LR) + k;
#pragma unroll
    for (int m = 0; m < R; ++m) st2(&f.x[swz(base + (m << lNs))], v[c + m * NB]);
  }
}
// positions >= nin are zero padding that was never written (zpad: the first stage of a forward transform)
template <int P>
__device__ __forceinline__ void stage_gather(double2 (&v)[P], const FftLine& f, bool zpad, int nin) {
#pragma unroll
  for (int s = 0; s < P; ++s) {
    const int pos = f.jt + s * f.tpl;
    const double2 t = ld2(&f.x[swz(pos)]);
    v[s] = (zpad && pos >= nin) ? make_double2(0.0, 0.0) : t;
  }
}
// The whole line transform: n16 radix-16 stages, then (LR > 0) one of radix 2^LR.  A thread holds P = 16 points, or the
// whole line when it is shorter (SHORT: n16 = 0, P = 2^LR).  IN_REGS: the slots are already in v; OUT_REGS: leave the
// result in the slots (else the line ends up in LDS, behind a barrier).
// `late` runs once, just before the final stage's butterflies (the pass issues the next item's loads there when it
// cannot afford to hold them through the whole transform).
// FULL_END: the barrier behind the final scatter is the workgroup's (a strided tile is drained by every thread).
template <int SGN, int LR, bool SHORT, bool IN_REGS, bool OUT_REGS, bool FULL_END, class Late>
__device__ __forceinline__ void fft_line(double2 (&v)[SHORT ? (1 << LR) : 16], const FftLine& f, int n16, bool zpad, int nin,
                                         Late late) {
  constexpr int P = SHORT ? (1 << LR) : 16;
  constexpr int RF = (LR == 0) ? 16 : (1 << LR);           // the final stage
  const int nfull = (LR == 0) ? n16 - 1 : n16;            // radix-16 stages that go back to LDS
  int lNs = 0;
  if constexpr (!SHORT) {
    for (int s = 0; s < nfull; ++s) {
      if (!(IN_REGS && s == 0)) stage_gather<16>(v, f, zpad && s == 0, nin);
      stage_compute<16, 1, SGN>(v, f, lNs);
      line_barrier(f);          // every thread of the line has gathered: it may be overwritten
      stage_scatter<16, 1>(v, f, lNs);
      line_barrier(f);
      lNs += 4;
    }
  }
  if (!(IN_REGS && nfull == 0)) stage_gather<P>(v, f, zpad && nfull == 0, nin);
  late();
  stage_compute<RF, P / RF, SGN>(v, f, lNs);
  if (!OUT_REGS) {
    line_barrier(f);
    stage_scatter<RF, P / RF>(v, f, lNs);
    if (FULL_END) lds_barrier(); else line_barrier(f);
  }
}

}}  // namespace gsi::hipk
