// fwd_adjoint.hip -- the adjoint of a sparse forward model: G (n x b) = H' V for the CSR matrix H (nobs x n, with its cell
// weights folded in) of a gsi_fwd and V (nobs x b) resident in HBM.
//
// No atomics: the host has inverted H once (fwd_adjoint_plan.hpp) into, per grid cell, the list of the (row, value) pairs
// that reach it, by ascending row.  One thread owns one cell: it walks its list and accumulates FADJ_COLS columns of V at a
// time, so that the list and its values are read once per FADJ_COLS columns.  Neighbouring threads own neighbouring cells:
// the stores are coalesced along j, the list reads nearly so (a cell's few entries follow its neighbour's); the reads of V
// are gathers by observation, from nobs x FADJ_COLS doubles that stay in cache.  blockIdx.y walks the column groups.
//
// A list longer than the plan's chunk limit (a cell many rays start in, a well every observation reads) is left out of the
// cell pass: one thread per CHUNK sums its at most `chunk` contributions in list order (fadj_chunk_kernel), and one thread
// per (long column, output column) adds the chunk sums in chunk order (fadj_long_kernel).  The order of every sum is the
// plan's alone: a column of G depends on neither b nor the launch.  Every product and sum is rounded on its own (no fused
// multiply-add).  All offsets j + c ld are 64-bit (n = 2^27 cells and 17 columns pass 2^31 elements).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <stdexcept>
#include "hip_common.hpp"
#include "backend.hpp"

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

namespace {

constexpr int FADJ_THREADS = 256;
constexpr int FADJ_COLS = 8;

struct FadjK {
  int64_t n, chunk, nlong, nchunk;
  const int64_t* colptr;
  const int32_t* row;
  const double* val;
  const int32_t* long_col;
  const int64_t* long_chunk0;
  const int64_t* chunk_off;
  const int32_t* chunk_len;
};

// contributions [e0, e1) of the index into acc, columns [0, nc) of V (already offset to the group's first column)
__device__ __forceinline__ void fadj_sum(const int32_t* __restrict__ row, const double* __restrict__ val, int64_t e0, int64_t e1,
                                         const double* __restrict__ V, int64_t ldv, int nc, double (&acc)[FADJ_COLS]) {
#pragma unroll
  for (int c = 0; c < FADJ_COLS; ++c) acc[c] = 0.0;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t r = row[e];
    const double h = val[e];
#pragma unroll
    for (int c = 0; c < FADJ_COLS; ++c)
      if (c < nc) acc[c] = acc[c] + h * V[r + (int64_t)c * ldv];
  }
}

// cell blockIdx.x FADJ_THREADS + threadIdx.x, columns [blockIdx.y FADJ_COLS, ...)
__global__ __launch_bounds__(FADJ_THREADS) void fadj_cell_kernel(FadjK pl, const double* __restrict__ V, int64_t ldv, int b,
                                                                double* __restrict__ G, int64_t ldg) {
  const int64_t j = (int64_t)blockIdx.x * FADJ_THREADS + threadIdx.x;
  if (j >= pl.n) return;
  const int64_t e0 = pl.colptr[j], e1 = pl.colptr[j + 1];
  if (e1 - e0 > pl.chunk) return;                    // a long column: fadj_long_kernel writes it
  const int c0 = (int)blockIdx.y * FADJ_COLS;
  const int nc = (b - c0 < FADJ_COLS) ? b - c0 : FADJ_COLS;
  double acc[FADJ_COLS];
  fadj_sum(pl.row, pl.val, e0, e1, V + (int64_t)c0 * ldv, ldv, nc, acc);
#pragma unroll
  for (int c = 0; c < FADJ_COLS; ++c)
    if (c < nc) G[j + (int64_t)(c0 + c) * ldg] = acc[c];
}

// chunk k = blockIdx.x FADJ_THREADS + threadIdx.x of the long columns: partial[k + c nchunk]
__global__ __launch_bounds__(FADJ_THREADS) void fadj_chunk_kernel(FadjK pl, const double* __restrict__ V, int64_t ldv, int b,
                                                                 double* __restrict__ partial) {
  const int64_t k = (int64_t)blockIdx.x * FADJ_THREADS + threadIdx.x;
  if (k >= pl.nchunk) return;
  const int64_t e0 = pl.chunk_off[k], e1 = e0 + pl.chunk_len[k];
  const int c0 = (int)blockIdx.y * FADJ_COLS;
  const int nc = (b - c0 < FADJ_COLS) ? b - c0 : FADJ_COLS;
  double acc[FADJ_COLS];
  fadj_sum(pl.row, pl.val, e0, e1, V + (int64_t)c0 * ldv, ldv, nc, acc);
#pragma unroll
  for (int c = 0; c < FADJ_COLS; ++c)
    if (c < nc) partial[k + (int64_t)(c0 + c) * pl.nchunk] = acc[c];
}

// long column i, output column c: the chunk sums in chunk order
__global__ __launch_bounds__(FADJ_THREADS) void fadj_long_kernel(FadjK pl, int b, const double* __restrict__ partial,
                                                                double* __restrict__ G, int64_t ldg) {
  const int64_t t = (int64_t)blockIdx.x * FADJ_THREADS + threadIdx.x;
  if (t >= pl.nlong * (int64_t)b) return;
  const int64_t i = t % pl.nlong, c = t / pl.nlong;
  const int64_t k0 = pl.long_chunk0[i], k1 = pl.long_chunk0[i + 1];
  const double* pc = partial + c * pl.nchunk;
  double s = pc[k0];
  for (int64_t k = k0 + 1; k < k1; ++k) s = s + pc[k];
  G[(int64_t)pl.long_col[i] + c * ldg] = s;
}

}  // namespace

void fwd_adjoint(hipStream_t st, const FwdAdjoint& a) {
  if (a.n <= 0 || a.b <= 0) return;
  const int64_t gy = (a.b + FADJ_COLS - 1) / FADJ_COLS;
  const int64_t gx = (a.n + FADJ_THREADS - 1) / FADJ_THREADS;
  if (a.b > FADJ_MAX_COLS || gy > 65535) throw std::runtime_error("fwd_adjoint: too many columns for one launch");
  if (gx >= ((int64_t)1 << 31)) throw std::runtime_error("fwd_adjoint: too many cells for one launch");
  if (a.ldv < a.nobs || a.ldg < a.n) throw std::runtime_error("fwd_adjoint: leading dimension too small");
  if (a.nchunk > 0 && a.partial == nullptr) throw std::runtime_error("fwd_adjoint: long columns without a workspace");
  const int64_t lt = a.nlong * a.b;
  if ((lt + FADJ_THREADS - 1) / FADJ_THREADS >= ((int64_t)1 << 31) ||
      (a.nchunk + FADJ_THREADS - 1) / FADJ_THREADS >= ((int64_t)1 << 31))
    throw std::runtime_error("fwd_adjoint: too many long columns for one launch");
  FadjK pl;
  pl.n = a.n; pl.chunk = a.chunk; pl.nlong = a.nlong; pl.nchunk = a.nchunk;
  pl.colptr = a.colptr; pl.row = a.row; pl.val = a.val;
  pl.long_col = a.long_col; pl.long_chunk0 = a.long_chunk0; pl.chunk_off = a.chunk_off; pl.chunk_len = a.chunk_len;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(FADJ_THREADS);
  hipLaunchKernelGGL(fadj_cell_kernel, grid, block, 0, st, pl, a.V, a.ldv, (int)a.b, a.G, a.ldg);
  if (a.nchunk <= 0) return;
  const dim3 cgrid((unsigned)((a.nchunk + FADJ_THREADS - 1) / FADJ_THREADS), (unsigned)gy);
  hipLaunchKernelGGL(fadj_chunk_kernel, cgrid, block, 0, st, pl, a.V, a.ldv, (int)a.b, a.partial);
  hipLaunchKernelGGL(fadj_long_kernel, dim3((unsigned)((lt + FADJ_THREADS - 1) / FADJ_THREADS)), block, 0, st, pl, (int)a.b,
                     a.partial, a.G, a.ldg);
}

}}  // namespace gsi::hipk
