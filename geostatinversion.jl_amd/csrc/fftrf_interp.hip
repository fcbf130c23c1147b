// fftrf_interp.hip -- FFTRF.interpolate (FFTRF.jl:107-129): a batch of structured fields read at scattered points.
//
// The coordinate lookup is done once on the host (fftrf_points.hpp): per point the vec() index of its cell's lower corner
// and one fraction f per axis.  Here one thread owns one point: it reads its plan entry once and walks the batch's fields,
// FRI_UNROLL fields at a time so that the 2^d gathers of all of them are in flight before the first is used.  Neighbouring
// threads own neighbouring points: the plan reads and the stores are coalesced, the gathers are not and cannot be (the
// points come in the caller's order; the field of a batch stays in L2 / the Infinity Cache while its points are served).
// With few points and many fields the fields are also spread over blockIdx.y; a value depends on neither split.
//
// value = nested two-term sums (1 - f_a) A + f_a B, axis 0 innermost: every product and sum is rounded on its own (no
// fused multiply-add), so the result equals the numpy restatement of tests/fftrf_interp_model.py bit for bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdexcept>
#include "hip_common.hpp"

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

constexpr int FRI_THREADS = 256;
constexpr int FRI_UNROLL = 4;

template <int D>
__device__ __forceinline__ void fri_gather(const double* __restrict__ Vf, int64_t b, int64_t s1, int64_t s2, double (&c)[1 << D]) {
  c[0] = Vf[b];
  c[1] = Vf[b + 1];
  c[2] = Vf[b + s1];
  c[3] = Vf[b + s1 + 1];
  if (D == 3) {
    c[4] = Vf[b + s2];
    c[5] = Vf[b + s2 + 1];
    c[6] = Vf[b + s2 + s1];
    c[7] = Vf[b + s2 + s1 + 1];
  }
}

template <int D>
__device__ __forceinline__ double fri_value(const double (&c)[1 << D], double f0, double g0, double f1, double g1, double f2,
                                            double g2) {
  const double x0 = g0 * c[0] + f0 * c[1];
  const double x1 = g0 * c[2] + f0 * c[3];
  const double y0 = g1 * x0 + f1 * x1;
  if (D == 2) return y0;
  const double x2 = g0 * c[4] + f0 * c[5];
  const double x3 = g0 * c[6] + f0 * c[7];
  const double y1 = g1 * x2 + f1 * x3;
  return g2 * y0 + f2 * y1;
}

// fields [blockIdx.y fpb, min(nb, (blockIdx.y + 1) fpb)) at point blockIdx.x FRI_THREADS + threadIdx.x
template <int D>
__global__ __launch_bounds__(FRI_THREADS) void fftrf_interp_kernel(const int32_t* __restrict__ base, const double* __restrict__ frac,
                                                                  int64_t m, int64_t s1, int64_t s2, const double* __restrict__ V,
                                                                  int64_t v_fs, int nb, int fpb, double* __restrict__ dst,
                                                                  int64_t ldd) {
  const int64_t p = (int64_t)blockIdx.x * FRI_THREADS + threadIdx.x;
  if (p >= m) return;
  const int64_t b = base[p];
  const double f0 = frac[p], f1 = frac[m + p], f2 = (D == 3) ? frac[2 * m + p] : 0.0;
  const double g0 = 1.0 - f0, g1 = 1.0 - f1, g2 = 1.0 - f2;
  int c = (int)blockIdx.y * fpb;
  const int c1 = (c + fpb < nb) ? c + fpb : nb;
  for (; c + FRI_UNROLL <= c1; c += FRI_UNROLL) {
    double v[FRI_UNROLL][1 << D];
#pragma unroll
    for (int u = 0; u < FRI_UNROLL; ++u) fri_gather<D>(V + (int64_t)(c + u) * v_fs, b, s1, s2, v[u]);
#pragma unroll
    for (int u = 0; u < FRI_UNROLL; ++u) dst[p + (int64_t)(c + u) * ldd] = fri_value<D>(v[u], f0, g0, f1, g1, f2, g2);
  }
  for (; c < c1; ++c) {
    double v[1 << D];
    fri_gather<D>(V + (int64_t)c * v_fs, b, s1, s2, v);
    dst[p + (int64_t)c * ldd] = fri_value<D>(v, f0, g0, f1, g1, f2, g2);
  }
}

void fftrf_interp(hipStream_t st, int d, const int32_t* base, const double* frac, int64_t m, int64_t s1, int64_t s2,
                  const double* V, int64_t v_fs, int nb, double* dst, int64_t ldd) {
  if (m <= 0 || nb <= 0) return;
  const int64_t gx = (m + FRI_THREADS - 1) / FRI_THREADS;
  if (gx >= ((int64_t)1 << 31)) throw std::runtime_error("fftrf_interp: too many points for one launch");
  // about 2048 workgroups (8 per CU) before a workgroup takes more than FRI_UNROLL fields
  int64_t gy = (2048 + gx - 1) / gx;
  const int64_t groups = ((int64_t)nb + FRI_UNROLL - 1) / FRI_UNROLL;
  if (gy > groups) gy = groups;
  const int fpb = (int)((groups + gy - 1) / gy) * FRI_UNROLL;
  gy = ((int64_t)nb + fpb - 1) / fpb;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (d == 3)
    hipLaunchKernelGGL(fftrf_interp_kernel<3>, grid, dim3(FRI_THREADS), 0, st, base, frac, m, s1, s2, V, v_fs, nb, fpb, dst, ldd);
  else
    hipLaunchKernelGGL(fftrf_interp_kernel<2>, grid, dim3(FRI_THREADS), 0, st, base, frac, m, s1, s2, V, v_fs, nb, fpb, dst, ldd);
}

}}  // namespace gsi::hipk
