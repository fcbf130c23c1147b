// bilinear_terms.hip -- the bilinear forms of the likelihood gradient, gfx950: with the resident
// n x b panels L, Y, R (column-major, leading dimension n) and V = Y + dd .* R (dd: n values, one per row; dd and R null: V = Y)
//   gram[a + g c] = sum_i L[i, a] V[i, c]    a, c < g           (the (1 + p) x (1 + p) matrix S_k of the gradient)
//   t[j - g]      = sum_i L[i, j] V[i, j]    g <= j < b         (one trace sample per probe)
// in ONE pass that reads every entry of L, Y and R once, with a summation order that is written down and restated by
// bilinear_terms_host.hpp and tests/bilinear_model.py, so the result is a pure function of the operands' bits:
//
//   * every product is rounded on its own (the file is compiled with fp contraction off): first d = dd[i] R[i, c], then
//     v = Y[i, c] + d, then p = L[i, a] v;
//   * the rows are cut into chunks of BILINEAR_CHUNK = 2048; within a chunk each output starts from 0.0 and adds its products
//     in ascending row order -- partial[chunk][o];
//   * a second kernel adds the chunks' partial sums in ascending chunk order, again from 0.0.  No atomics anywhere.
//
//   bilinear_partial_kernel  workgroup (chunk, group).  Group "gram" (present when g > 0): tiles of 64 rows of L[:, :g] and
//                            V[:, :g] go through LDS with whole-line loads (lanes along i); thread (a, c) of the 16 x 16
//                            then adds its 64 products in row order.  Groups of 32 probe columns: the PRODUCTS of a 64 x 32
//                            tile go to LDS (padded rows: no bank conflict), thread c < 32 adds column c's 64 in row order.
//                            Offsets i + c n are 64-bit; rows beyond n are never read and add nothing.
//   bilinear_sum_kernel      one thread per output: the chunks in order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

namespace {

constexpr int BL_BS = 256;
constexpr int BL_TR = 64;                 // rows per tile: one wave reads one line of a column
constexpr int BL_TC = 32;                 // probe columns per workgroup
constexpr int BL_G = 16;                  // the largest g
constexpr int BL_LANES_PER_ROWSET = BL_BS / BL_TR;    // columns loaded per step

__global__ __launch_bounds__(BL_BS) void bilinear_partial_kernel(int64_t n, int64_t b, int64_t g, const double* __restrict__ L,
                                                                 const double* __restrict__ Y, const double* __restrict__ R,
                                                                 const double* __restrict__ dd, double* __restrict__ partial) {
  __shared__ double sa[BL_TR * BL_G];              // gram: the L tile [r][a]
  __shared__ double sb[BL_TC * (BL_TR + 1)];       // gram: the V tile [r][c]; probe columns: the products [c][r], padded
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int64_t r0 = chunk * BILINEAR_CHUNK;
  const int64_t rend = (n - r0 < BILINEAR_CHUNK) ? n : r0 + BILINEAR_CHUNK;
  const int64_t nout = g * g + (b - g);
  double* out = partial + (size_t)chunk * (size_t)nout;
  const int grp = (int)blockIdx.y - (g > 0 ? 1 : 0);      // -1: the gram
  const int lr = tid % BL_TR, lc = tid / BL_TR;
  double s = 0.0;
  if (grp < 0) {
    const int a = tid % BL_G, c = tid / BL_G;
    const bool mine = a < g && c < g;
    for (int64_t t0 = r0; t0 < rend; t0 += BL_TR) {
      const int64_t i = t0 + lr;
      if (i < rend) {
        for (int col = lc; col < g; col += BL_LANES_PER_ROWSET) {
          const size_t off = (size_t)i + (size_t)col * (size_t)n;
          double v = Y[off];
          if (dd != nullptr) {
            const double d = dd[i] * R[off];
            v = v + d;
          }
          sa[lr * BL_G + col] = L[off];
          sb[lr * BL_G + col] = v;
        }
      }
      __syncthreads();
      const int rows = (rend - t0 < BL_TR) ? (int)(rend - t0) : BL_TR;
      if (mine) {
        for (int r = 0; r < rows; ++r) {
          const double p = sa[r * BL_G + a] * sb[r * BL_G + c];
          s = s + p;
        }
      }
      __syncthreads();
    }
    if (mine) out[a + g * c] = s;
  } else {
    const int64_t j0 = g + (int64_t)grp * BL_TC;
    const int ncol = (b - j0 < BL_TC) ? (int)(b - j0) : BL_TC;
    for (int64_t t0 = r0; t0 < rend; t0 += BL_TR) {
      const int64_t i = t0 + lr;
      if (i < rend) {
        for (int col = lc; col < ncol; col += BL_LANES_PER_ROWSET) {
          const size_t off = (size_t)i + (size_t)(j0 + col) * (size_t)n;
          double v = Y[off];
          if (dd != nullptr) {
            const double d = dd[i] * R[off];
            v = v + d;
          }
          const double p = L[off] * v;
          sb[col * (BL_TR + 1) + lr] = p;
        }
      }
      __syncthreads();
      const int rows = (rend - t0 < BL_TR) ? (int)(rend - t0) : BL_TR;
      if (tid < ncol) {
        for (int r = 0; r < rows; ++r) s = s + sb[tid * (BL_TR + 1) + r];
      }
      __syncthreads();
    }
    if (tid < ncol) out[g * g + (j0 - g) + tid] = s;
  }
}

__global__ __launch_bounds__(BL_BS) void bilinear_sum_kernel(int64_t chunks, int64_t nout, const double* __restrict__ partial,
                                                             double* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * BL_BS + threadIdx.x;
  if (o >= nout) return;
  double s = 0.0;
  for (int64_t k = 0; k < chunks; ++k) s = s + partial[(size_t)k * (size_t)nout + (size_t)o];
  out[o] = s;
}

inline int64_t bl_chunks(int64_t n) { return (n + BILINEAR_CHUNK - 1) / BILINEAR_CHUNK; }

}  // namespace

size_t bilinear_partial_doubles(int64_t n, int64_t b, int64_t g) { return (size_t)bl_chunks(n) * (size_t)(g * g + (b - g)); }

// out (g g + b - g doubles): the gram, then t.  The caller has checked 1 <= n, 1 <= b, 0 <= g <= min(b, 16), b - g <= 32 * 65534.
void bilinear_terms(hipStream_t st, int64_t n, int64_t b, int64_t g, const double* L, const double* Y, const double* R,
                    const double* dd, double* partial, double* out) {
  static_assert(BL_G * BL_G == BL_BS && BL_TR * BL_G <= BL_TC * (BL_TR + 1), "the gram tile shares the product tile's LDS");
  const int64_t chunks = bl_chunks(n), nout = g * g + (b - g);
  const int64_t groups = (g > 0 ? 1 : 0) + (b - g + BL_TC - 1) / BL_TC;
  hipLaunchKernelGGL(bilinear_partial_kernel, dim3((unsigned)chunks, (unsigned)groups), dim3(BL_BS), 0, st, n, b, g, L, Y, R, dd,
                     partial);
  hipLaunchKernelGGL(bilinear_sum_kernel, dim3((unsigned)((nout + BL_BS - 1) / BL_BS)), dim3(BL_BS), 0, st, chunks, nout, partial, out);
}

}}  // namespace gsi::hipk
