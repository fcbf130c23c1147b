// pcga_forward.hip -- the sparse forward model on the device (gsi_fwd): the products
//   out[r, c] = sum over the nonzeros t of row r of vals[t] g(w[j_t] p(j_t, c))
// for the K + 3 columns p(:, c) of direct.jl:39-45 / lsqr.jl:37-43, which are evaluated element by element from s, X and
// the resident basis Z and never stored -- or, for gsi_fwd_apply, for the columns of a plain matrix.
//
// Two forms over one segment table (fwd_plan.hpp), both templated on the element type of Z:
//   lane   one lane = one segment x FWD_CL columns; lanes run along segments (rows), so the stores coalesce and neighbouring
//          observations share cache lines of Z.  For short rows: point samples, small stencils.
//   wave   one wave = one segment x FWD_CG columns; the lanes stride over the segment's nonzeros, read colidx / vals / s / w
//          once per nonzero and issue the FWD_CG loads Z[j + c ldz] together (coalesced wherever a row's column indices are
//          consecutive); one butterfly reduction per column at the end.
// A split row's segments write one partial sum each and fwd_reduce adds them in segment order: no atomics, two calls on the
// same inputs return the same bits.  All index arithmetic j + c ldz is 64-bit (n = 512^3, c >= 16 passes 2^31 elements).
#include "hip_common.hpp"
#include "backend.hpp"

namespace gsi { namespace hipk {

namespace {

constexpr int FWD_CL = 4;     // columns per lane, lane form
constexpr int FWD_CG = 16;    // columns per wave, wave form
constexpr int64_t FWD_GRID_Y = 65535;

struct FwdK {
  const int64_t* segptr;
  const int32_t* colidx;
  const double* vals;
  const double* w;
  const void* Z;
  const double* s;
  const double* X;
  double* dst;            // out (ld nobs) when no row is split, else the partial sums (ld nseg): indexed by segment
  int64_t nseg, ldz, K, ncols, ldd, cbase;
  double delta;
  int link;
};

// p(j, c): column c is uniform over a wave in both forms, so these branches do not diverge
template <typename T, bool PLAIN>
__device__ __forceinline__ double fwd_elem(const FwdK& a, int64_t j, int64_t c, double sj) {
  if (PLAIN) return (double)((const T*)a.Z)[j + c * a.ldz];
  if (c < a.K) return sj + a.delta * (double)((const T*)a.Z)[j + c * a.ldz];
  if (c == a.K) return sj + a.delta * a.X[j];
  if (c == a.K + 1) return sj + a.delta * sj;
  return sj;
}

__device__ __forceinline__ double fwd_term(double v, double wj, double p, int link) {
  double t = wj * p;
  if (link) t = exp(t);
  return v * t;
}

template <typename T, bool PLAIN>
__global__ __launch_bounds__(256) void fwd_lane_kernel(FwdK a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.nseg) return;
  const int64_t c0 = a.cbase + (int64_t)blockIdx.y * FWD_CL;
  const int64_t t0 = a.segptr[k], t1 = a.segptr[k + 1];
  double acc[FWD_CL];
#pragma unroll
  for (int q = 0; q < FWD_CL; ++q) acc[q] = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t j = a.colidx[t];
    const double v = a.vals[t];
    const double wj = a.w ? a.w[j] : 1.0;
    const double sj = PLAIN ? 0.0 : a.s[j];
#pragma unroll
    for (int q = 0; q < FWD_CL; ++q) {
      const int64_t c = c0 + q;
      if (c < a.ncols) acc[q] += fwd_term(v, wj, fwd_elem<T, PLAIN>(a, j, c, sj), a.link);
    }
  }
#pragma unroll
  for (int q = 0; q < FWD_CL; ++q) {
    const int64_t c = c0 + q;
    if (c < a.ncols) a.dst[k + c * a.ldd] = acc[q];
  }
}

template <typename T, bool PLAIN>
__global__ __launch_bounds__(256) void fwd_wave_kernel(FwdK a) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= a.nseg) return;                                   // the whole wave leaves
  const int64_t c0 = a.cbase + (int64_t)blockIdx.y * FWD_CG;
  const int64_t t0 = a.segptr[k], t1 = a.segptr[k + 1];
  double acc[FWD_CG];
#pragma unroll
  for (int q = 0; q < FWD_CG; ++q) acc[q] = 0.0;
  // all FWD_CG columns of this group are columns of Z: the loads of one nonzero are issued together
  const bool full = PLAIN ? (c0 + FWD_CG <= a.ncols) : (c0 + FWD_CG <= a.K);
  if (full) {
    const T* Zc = (const T*)a.Z + c0 * a.ldz;
    for (int64_t t = t0 + lane; t < t1; t += 64) {
      const int64_t j = a.colidx[t];
      const double v = a.vals[t];
      const double wj = a.w ? a.w[j] : 1.0;
      const double sj = PLAIN ? 0.0 : a.s[j];
      double z[FWD_CG];
#pragma unroll
      for (int q = 0; q < FWD_CG; ++q) z[q] = (double)Zc[j + (int64_t)q * a.ldz];
#pragma unroll
      for (int q = 0; q < FWD_CG; ++q) acc[q] += fwd_term(v, wj, PLAIN ? z[q] : sj + a.delta * z[q], a.link);
    }
  } else {                                                   // the ragged last group and the three special columns
    for (int64_t t = t0 + lane; t < t1; t += 64) {
      const int64_t j = a.colidx[t];
      const double v = a.vals[t];
      const double wj = a.w ? a.w[j] : 1.0;
      const double sj = PLAIN ? 0.0 : a.s[j];
#pragma unroll
      for (int q = 0; q < FWD_CG; ++q) {
        const int64_t c = c0 + q;
        if (c < a.ncols) acc[q] += fwd_term(v, wj, fwd_elem<T, PLAIN>(a, j, c, sj), a.link);
      }
    }
  }
  double mine = 0.0;
#pragma unroll
  for (int q = 0; q < FWD_CG; ++q) {
    double x = acc[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    if (lane == q) mine = x;
  }
  const int64_t c = c0 + lane;
  if (lane < FWD_CG && c < a.ncols) a.dst[k + c * a.ldd] = mine;
}

__global__ __launch_bounds__(256) void fwd_reduce_kernel(const double* __restrict__ part, int64_t nseg,
                                                         const int64_t* __restrict__ rowseg, int64_t nobs, int64_t ncols,
                                                         int64_t cbase, double* __restrict__ out, int64_t ldo) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = cbase + blockIdx.y;
  if (r >= nobs || c >= ncols) return;
  const double* p = part + c * nseg;
  double acc = 0.0;
  for (int64_t k = rowseg[r]; k < rowseg[r + 1]; ++k) acc += p[k];
  out[r + c * ldo] = acc;
}

FwdK fwd_args(const FwdProduct& a) {
  FwdK k;
  k.segptr = a.segptr; k.colidx = a.colidx; k.vals = a.vals; k.w = a.w; k.Z = a.Z; k.s = a.s; k.X = a.X;
  k.dst = a.rowseg ? a.partial : a.out;
  k.nseg = a.nseg; k.ldz = a.ldz; k.K = a.K; k.ncols = a.ncols();
  k.ldd = a.rowseg ? a.nseg : a.ldo;
  k.cbase = 0; k.delta = a.delta; k.link = a.link;
  return k;
}

// grid.y counts column groups of `per` columns; at most FWD_GRID_Y of them per launch
template <class Launch>
void fwd_column_chunks(int64_t ncols, int per, Launch&& launch) {
  const int64_t groups = (ncols + per - 1) / per;
  for (int64_t g0 = 0; g0 < groups; g0 += FWD_GRID_Y) {
    const int64_t g = groups - g0 < FWD_GRID_Y ? groups - g0 : FWD_GRID_Y;
    launch(g0 * per, (unsigned)g);
  }
}

}  // namespace

void fwd_lane(hipStream_t st, const FwdProduct& a) {
  FwdK k = fwd_args(a);
  if (k.nseg <= 0 || k.ncols <= 0) return;
  const unsigned gx = (unsigned)((k.nseg + 255) / 256);
  fwd_column_chunks(k.ncols, FWD_CL, [&](int64_t cbase, unsigned gy) {
    k.cbase = cbase;
    if (a.plain) hipLaunchKernelGGL((fwd_lane_kernel<double, true>), dim3(gx, gy), dim3(256), 0, st, k);
    else if (a.zbits == 32) hipLaunchKernelGGL((fwd_lane_kernel<float, false>), dim3(gx, gy), dim3(256), 0, st, k);
    else hipLaunchKernelGGL((fwd_lane_kernel<double, false>), dim3(gx, gy), dim3(256), 0, st, k);
  });
}

void fwd_wave(hipStream_t st, const FwdProduct& a) {
  FwdK k = fwd_args(a);
  if (k.nseg <= 0 || k.ncols <= 0) return;
  const unsigned gx = (unsigned)((k.nseg + 3) / 4);
  fwd_column_chunks(k.ncols, FWD_CG, [&](int64_t cbase, unsigned gy) {
    k.cbase = cbase;
    if (a.plain) hipLaunchKernelGGL((fwd_wave_kernel<double, true>), dim3(gx, gy), dim3(256), 0, st, k);
    else if (a.zbits == 32) hipLaunchKernelGGL((fwd_wave_kernel<float, false>), dim3(gx, gy), dim3(256), 0, st, k);
    else hipLaunchKernelGGL((fwd_wave_kernel<double, false>), dim3(gx, gy), dim3(256), 0, st, k);
  });
}

void fwd_reduce(hipStream_t st, const FwdProduct& a) {
  if (!a.rowseg || a.nobs <= 0) return;
  const int64_t ncols = a.ncols();
  const unsigned gx = (unsigned)((a.nobs + 255) / 256);
  fwd_column_chunks(ncols, 1, [&](int64_t cbase, unsigned gy) {
    hipLaunchKernelGGL(fwd_reduce_kernel, dim3(gx, gy), dim3(256), 0, st, a.partial, a.nseg, a.rowseg, a.nobs, ncols, cbase,
                       a.out, a.ldo);
  });
}

}}  // namespace gsi::hipk
