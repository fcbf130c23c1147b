// interp_adjoint.hip -- the adjoint of FFTRF.interpolate: G = W' X, point values spread onto the nodes of the structured grid
// (DESIGN.md 4.6g).  W is the m x n multilinear interpolation matrix that fftrf_interp.hip applies.
//
// No atomics: the host has inverted the points plan once (interp_adjoint_plan.hpp) into, per node, the list of the
// (point, corner) pairs that reach it, in ascending point order.  One thread owns one node: it walks its list, recomputes each
// weight from the point's fractions and the corner code, and accumulates IADJ_COLS columns of X at a time, so that the list and
// the fractions are read once per IADJ_COLS columns.  Neighbouring threads own neighbouring nodes: the stores are coalesced,
// the list reads nearly so (a node's few entries follow its neighbour's); the reads of X and frac are gathers in the
// caller's point order.  blockIdx.y walks the column groups: workgroups are dispatched x-fastest, so at any time the
// machine works on a few groups -- IADJ_COLS columns of 10^6 points are 64 MB, inside the Infinity Cache with the plan.
//
// A list longer than the plan's chunk limit (a refined mesh, points clamped onto the boundary) is left out of the node pass:
// one thread per CHUNK sums its at most `chunk` contributions in list order (iadj_chunk_kernel), and one thread per
// (long node, column) adds the chunk sums in chunk order (iadj_long_kernel).  The order of every sum is the plan's alone:
// a column of G depends on neither nf nor the launch.  Every product and sum is rounded on its own (no fused multiply-add).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdexcept>
#include "hip_common.hpp"

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

constexpr int IADJ_THREADS = 256;
constexpr int IADJ_COLS = 8;

// contributions [e0, e1) of the index into acc, columns [0, nc) of X (already offset to the group's first column)
template <int D>
__device__ __forceinline__ void iadj_sum(const int32_t* __restrict__ point, const uint8_t* __restrict__ corner,
                                         const double* __restrict__ frac, int64_t m, int64_t e0, int64_t e1,
                                         const double* __restrict__ X, int64_t ldx, int nc, double (&acc)[IADJ_COLS]) {
#pragma unroll
  for (int c = 0; c < IADJ_COLS; ++c) acc[c] = 0.0;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t p = point[e];
    const int k = corner[e];
    const double f0 = frac[p], f1 = frac[m + p];
    double w = (k & 1) ? f0 : 1.0 - f0;
    w = w * ((k & 2) ? f1 : 1.0 - f1);
    if (D == 3) {
      const double f2 = frac[2 * m + p];
      w = w * ((k & 4) ? f2 : 1.0 - f2);
    }
#pragma unroll
    for (int c = 0; c < IADJ_COLS; ++c)
      if (c < nc) acc[c] = acc[c] + w * X[p + (int64_t)c * ldx];
  }
}

// node blockIdx.x IADJ_THREADS + threadIdx.x, columns [blockIdx.y IADJ_COLS, ...)
template <int D>
__global__ __launch_bounds__(IADJ_THREADS) void iadj_node_kernel(IadjDev pl, const double* __restrict__ X, int64_t ldx, int nf,
                                                                double* __restrict__ G, int64_t ldg) {
  const int64_t g = (int64_t)blockIdx.x * IADJ_THREADS + threadIdx.x;
  if (g >= pl.n) return;
  const int64_t e0 = pl.nodeptr[g], e1 = pl.nodeptr[g + 1];
  if (e1 - e0 > pl.chunk) return;                    // a long node: iadj_long_kernel writes it
  const int c0 = (int)blockIdx.y * IADJ_COLS;
  const int nc = (nf - c0 < IADJ_COLS) ? nf - c0 : IADJ_COLS;
  double acc[IADJ_COLS];
  iadj_sum<D>(pl.point, pl.corner, pl.frac, pl.m, e0, e1, X + (int64_t)c0 * ldx, ldx, nc, acc);
#pragma unroll
  for (int c = 0; c < IADJ_COLS; ++c)
    if (c < nc) G[g + (int64_t)(c0 + c) * ldg] = acc[c];
}

// chunk j = blockIdx.x IADJ_THREADS + threadIdx.x of the long nodes: partial[j + c nchunk]
template <int D>
__global__ __launch_bounds__(IADJ_THREADS) void iadj_chunk_kernel(IadjDev pl, const double* __restrict__ X, int64_t ldx, int nf,
                                                                 double* __restrict__ partial) {
  const int64_t j = (int64_t)blockIdx.x * IADJ_THREADS + threadIdx.x;
  if (j >= pl.nchunk) return;
  const int64_t e0 = pl.chunk_off[j], e1 = e0 + pl.chunk_len[j];
  const int c0 = (int)blockIdx.y * IADJ_COLS;
  const int nc = (nf - c0 < IADJ_COLS) ? nf - c0 : IADJ_COLS;
  double acc[IADJ_COLS];
  iadj_sum<D>(pl.point, pl.corner, pl.frac, pl.m, e0, e1, X + (int64_t)c0 * ldx, ldx, nc, acc);
#pragma unroll
  for (int c = 0; c < IADJ_COLS; ++c)
    if (c < nc) partial[j + (int64_t)(c0 + c) * pl.nchunk] = acc[c];
}

// long node i, column c: the chunk sums in chunk order
__global__ __launch_bounds__(IADJ_THREADS) void iadj_long_kernel(IadjDev pl, int nf, const double* __restrict__ partial,
                                                                double* __restrict__ G, int64_t ldg) {
  const int64_t t = (int64_t)blockIdx.x * IADJ_THREADS + threadIdx.x;
  if (t >= pl.nlong * (int64_t)nf) return;
  const int64_t i = t % pl.nlong, c = t / pl.nlong;
  const int64_t j0 = pl.long_chunk0[i], j1 = pl.long_chunk0[i + 1];
  const double* pc = partial + c * pl.nchunk;
  double s = pc[j0];
  for (int64_t j = j0 + 1; j < j1; ++j) s = s + pc[j];
  G[(int64_t)pl.long_node[i] + c * ldg] = s;
}

void interp_adjoint(hipStream_t st, const IadjDev& p, const double* X, int64_t ldx, int64_t nf, double* G, int64_t ldg,
                    double* partial) {
  if (p.n <= 0 || nf <= 0) return;
  const int64_t gy = (nf + IADJ_COLS - 1) / IADJ_COLS;
  const int64_t gx = (p.n + IADJ_THREADS - 1) / IADJ_THREADS;
  if (gy > 65535 || nf >= ((int64_t)1 << 31)) throw std::runtime_error("interp_adjoint: too many columns for one launch");
  if (p.nchunk > 0 && partial == nullptr) throw std::runtime_error("interp_adjoint: long nodes without a workspace");
  const int64_t lt = p.nlong * nf;
  if ((lt + IADJ_THREADS - 1) / IADJ_THREADS >= ((int64_t)1 << 31))
    throw std::runtime_error("interp_adjoint: too many long nodes x columns for one launch");
  const dim3 grid((unsigned)gx, (unsigned)gy), block(IADJ_THREADS);
  if (p.d == 3) hipLaunchKernelGGL(iadj_node_kernel<3>, grid, block, 0, st, p, X, ldx, (int)nf, G, ldg);
  else hipLaunchKernelGGL(iadj_node_kernel<2>, grid, block, 0, st, p, X, ldx, (int)nf, G, ldg);
  if (p.nchunk <= 0) return;
  const dim3 cgrid((unsigned)((p.nchunk + IADJ_THREADS - 1) / IADJ_THREADS), (unsigned)gy);
  if (p.d == 3) hipLaunchKernelGGL(iadj_chunk_kernel<3>, cgrid, block, 0, st, p, X, ldx, (int)nf, partial);
  else hipLaunchKernelGGL(iadj_chunk_kernel<2>, cgrid, block, 0, st, p, X, ldx, (int)nf, partial);
  hipLaunchKernelGGL(iadj_long_kernel, dim3((unsigned)((lt + IADJ_THREADS - 1) / IADJ_THREADS)), block, 0, st, p, (int)nf, partial,
                     G, ldg);
}

}}  // namespace gsi::hipk
