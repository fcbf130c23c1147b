// pivoted_chol.hip -- diagonal-pivoted Cholesky of a covariance that is read by entries (pchol_state.hpp states the
// contract): a rank-K factor L L' ~ A from K columns of A and one growing row-times-panel
// product, without a single operator product.
//
// Two launches per step, in stream order; nothing waits for the host:
//   step    one thread per row i: A(i, p) in one of three forms -- column p of a stored matrix, the grid-offset table, the
//           scattered-point generator of pointcov_gen.hpp --, the row's j earlier entries of L (column-major: neighbouring rows
//           are neighbouring lanes, every load of a wave is one 512-byte run) against row p of L, the new column, the new
//           d, and the workgroup's partial (max d, its lowest index, sum of the positive d, non-finite seen)
//   decide  one workgroup: the partials in index order (PC_BS chains of a fixed stride, then a fixed tree), the stopping
//           rules of pchol_state.hpp, the next pivot and sqrt(d_p) into the state block, and row p of L into `prow`
// Row p of L is staged once per step by `decide` (K <= 2048 doubles): every workgroup of the step then reads it at a
// wave-uniform address, i.e. through the scalar cache, and no lane spends a register or an LDS read on it.
// A step enqueued after the stop reads the state block and returns.  No float atomics, no grid-wide barrier: two calls
// give the same bits.  64-bit row indices throughout.
//
// Loop edges (tests/pivchol_cases.py): PC_BS rows per workgroup (n = 255, 256, 257); PC_UNROLL columns per trip of the
// row loop (j = 7, 8, 9, ... 32); PC_BS partials per sweep of `decide` (n > 256 * 256 rows).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "hip_common.hpp"
#include "pchol_state.hpp"
#include "pointcov_gen.hpp"      // (in front of the pragma: the generator is compiled as the tile loaders compile it)

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

namespace {
using namespace gsi::pchol;
constexpr int PC_BS = 256;
constexpr int PC_UNROLL = 8;

// all PC_BS threads; the same tree every time.  The result is valid in thread 0.
__device__ inline Red pc_block_reduce(Red v, Red* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Red o;
    o.dmax = __shfl_down(v.dmax, off, 64);
    o.idx = __shfl_down(v.idx, off, 64);
    o.possum = __shfl_down(v.possum, off, 64);
    o.bad = __shfl_down(v.bad, off, 64);
    red_join(v, o);
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  Red t = sh[0];
  red_join(t, sh[1]); red_join(t, sh[2]); red_join(t, sh[3]);
  __syncthreads();
  return t;
}

// A(i, p).  FORM 1: a stored matrix; 2: table[|dx| ny + |dy|] for grid points i = (i / ny, i % ny); 3: the generator
template <int FORM>
__device__ __forceinline__ double pc_entry(const PcholCol& a, int64_t i, int64_t p, const double* tab) {
  if (FORM == 1) return a.a[i + p * a.ld];
  if (FORM == 2) {
    const int ny = a.ny;                                            // (grid points are 31-bit: api.cpp refuses larger grids)
    const int ix = (int)i / ny, iy = (int)i - ix * ny;
    const int px = (int)p / ny, py = (int)p - px * ny;
    const int dx = ix > px ? ix - px : px - ix, dy = iy > py ? iy - py : py - iy;
    return a.a[(int64_t)dx * ny + dy];
  }
  const GenPointK gq = gen_point_setup(a.dim, a.kind);
  const int fl = gen_flags(gq.flags);
  const double2 pxy = *reinterpret_cast<const double2*>(a.a + 4 * i);
  const double qx = a.a[4 * p], qy = a.a[4 * p + 1];
  const double dx = pxy.x - qx, dy = pxy.y - qy;
  double s0 = fma(dx, dx, dy * dy);
  if (fl & 1) {
    const double dz = a.a[4 * i + 2] - a.a[4 * p + 2];
    s0 = fma(dz, dz, s0);
  }
  double v0, v1;
  gen_point_pair(gq, fl, s0, s0, tab, v0, v1);
  return v0 + ((i == p) ? a.nugget : 0.0);
}

// d_i = A(i, i) and the partials of the first decision
template <int FORM>
__global__ __launch_bounds__(PC_BS) void pc_diag_kernel(int64_t n, PcholCol a, double* __restrict__ d, double* __restrict__ part) {
  __shared__ double tab[64];
  __shared__ Red sh[4];
  if (FORM == 3) { gen_table_init(tab, threadIdx.x, a.sigma2); __syncthreads(); }
  const int64_t i = (int64_t)blockIdx.x * PC_BS + threadIdx.x;
  Red r = red_identity();
  if (i < n) {
    const double v = pc_entry<FORM>(a, i, i, tab);
    d[i] = v;
    red_row(r, v, i, false);
  }
  r = pc_block_reduce(r, sh);
  if (threadIdx.x == 0) {
    double* o = part + 4 * (int64_t)blockIdx.x;
    o[0] = r.dmax; o[1] = r.idx; o[2] = r.possum; o[3] = r.bad;
  }
}

template <int FORM>
__global__ __launch_bounds__(PC_BS) void pc_step_kernel(int64_t n, PcholCol a, double* __restrict__ L, int64_t ldl,
                                                        double* __restrict__ d, const double* __restrict__ s,
                                                        const double* __restrict__ prow, double* __restrict__ part) {
  __shared__ double tab[64];
  __shared__ Red sh[4];
  if (s[S_REASON] != 0.0) return;                                   // (uniform over the grid) stopped: nothing to do
  const int64_t j = (int64_t)s[S_STEP], p = (int64_t)s[S_PIVOT];
  const double root = s[S_ROOT];
  if (FORM == 3) { gen_table_init(tab, threadIdx.x, a.sigma2); __syncthreads(); }
  const int64_t i = (int64_t)blockIdx.x * PC_BS + threadIdx.x;
  Red r = red_identity();
  if (i < n) {
    const double aip = pc_entry<FORM>(a, i, p, tab);
    const double* Li = L + i;
    double sum = 0.0;
    int64_t c = 0;
    for (; c + PC_UNROLL <= j; c += PC_UNROLL) {                    // the loads of a trip are in flight together
      double v[PC_UNROLL];
#pragma unroll
      for (int u = 0; u < PC_UNROLL; ++u) v[u] = Li[(c + u) * ldl];
#pragma unroll
      for (int u = 0; u < PC_UNROLL; ++u) sum = sum + v[u] * prow[c + u];
    }
    for (; c < j; ++c) sum = sum + Li[c * ldl] * prow[c];
    const double l = (aip - sum) / root;
    L[i + j * ldl] = l;
    double di = d[i] - l * l;
    if (i == p) di = 0.0;
    d[i] = di;
    red_row(r, di, i, !is_fin(l));
  }
  r = pc_block_reduce(r, sh);
  if (threadIdx.x == 0) {
    double* o = part + 4 * (int64_t)blockIdx.x;
    o[0] = r.dmax; o[1] = r.idx; o[2] = r.possum; o[3] = r.bad;
  }
}

// one workgroup: the partials in a fixed order, the rules, the next pivot's row of L
__global__ __launch_bounds__(PC_BS) void pc_decide_kernel(int64_t nparts, const double* __restrict__ part, double* __restrict__ s,
                                                          const double* __restrict__ L, int64_t ldl, double* __restrict__ prow,
                                                          int first) {
  __shared__ Red sh[4];
  __shared__ int64_t nxt[2];
  if (s[S_REASON] != 0.0) return;                                   // (uniform)
  Red r = red_identity();
  for (int64_t k = threadIdx.x; k < nparts; k += PC_BS) {
    const double* o = part + 4 * k;
    red_join(r, Red{o[0], o[1], o[2], o[3]});
  }
  r = pc_block_reduce(r, sh);
  if (threadIdx.x == 0) {
    decide(s, r, first != 0);
    nxt[0] = (s[S_REASON] == 0.0) ? (int64_t)s[S_STEP] : 0;         // stopped: no row to stage
    nxt[1] = (int64_t)s[S_PIVOT];
  }
  __syncthreads();
  const int64_t j = nxt[0], p = nxt[1];
  for (int64_t c = threadIdx.x; c < j; c += PC_BS) prow[c] = L[p + c * ldl];
}

__global__ __launch_bounds__(PC_BS) void pc_begin_kernel(double* s, int64_t K, double tol) {
  if (threadIdx.x == 0) begin(s, K, tol);
}

// U (n x K, ld ldu): column k *= S[k]
__global__ __launch_bounds__(PC_BS) void pc_scale_cols_kernel(int64_t n, int64_t K, double* __restrict__ U, int64_t ldu,
                                                              const double* __restrict__ S) {
  for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
    const double sk = S[k];
    for (int64_t i = (int64_t)blockIdx.x * PC_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PC_BS) U[i + k * ldu] *= sk;
  }
}

inline int64_t pc_parts(int64_t n) { return (n + PC_BS - 1) / PC_BS; }
inline size_t up4(size_t x) { return (x + 3) & ~(size_t)3; }
struct PcWork { double *s, *prow, *part, *pts4; };
inline PcWork pc_carve(double* work, int64_t n, int64_t K) {
  PcWork w;
  w.s = work;
  w.prow = w.s + up4(state_doubles(K));
  w.part = w.prow + up4((size_t)K);
  w.pts4 = w.part + 4 * (size_t)pc_parts(n);                        // (32-byte records: every offset is a multiple of 4 doubles)
  return w;
}
}  // namespace

// work = [state | row p of L (K) | partials (4 per workgroup) | FORM 3: the points as 32-byte records (4 n)]
size_t pchol_work_doubles(int form, int64_t n, int64_t K) {
  return up4(state_doubles(K)) + up4((size_t)K) + 4 * (size_t)pc_parts(n) + (form == 3 ? 4 * (size_t)n : 0);
}
double* pchol_points(double* work, int64_t n, int64_t K) { return pc_carve(work, n, K).pts4; }

#define PC_FORMS(KERNEL, GRID, ...)                                                                      \
  do {                                                                                                   \
    if (a.form == 1) hipLaunchKernelGGL((KERNEL<1>), GRID, dim3(PC_BS), 0, st, __VA_ARGS__);             \
    else if (a.form == 2) hipLaunchKernelGGL((KERNEL<2>), GRID, dim3(PC_BS), 0, st, __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERNEL<3>), GRID, dim3(PC_BS), 0, st, __VA_ARGS__);                         \
  } while (0)

// d <- diag(A), the state of a fresh factorization, the first decision.  L only feeds the staging of row p (nothing at j = 0).
void pchol_begin(hipStream_t st, const PcholCol& a, int64_t n, int64_t K, double tol, const double* L, int64_t ldl, double* d,
                 double* work) {
  const PcWork w = pc_carve(work, n, K);
  const dim3 g((unsigned)pc_parts(n));
  hipLaunchKernelGGL(pc_begin_kernel, dim3(1), dim3(PC_BS), 0, st, w.s, K, tol);
  PC_FORMS(pc_diag_kernel, g, n, a, d, w.part);
  hipLaunchKernelGGL(pc_decide_kernel, dim3(1), dim3(PC_BS), 0, st, pc_parts(n), (const double*)w.part, w.s, L, ldl, w.prow, 1);
}
// one step and the decision behind it; a no-op once the state says stop
void pchol_step(hipStream_t st, const PcholCol& a, int64_t n, int64_t K, double* L, int64_t ldl, double* d, double* work) {
  const PcWork w = pc_carve(work, n, K);
  const dim3 g((unsigned)pc_parts(n));
  PC_FORMS(pc_step_kernel, g, n, a, L, ldl, d, (const double*)w.s, (const double*)w.prow, w.part);
  hipLaunchKernelGGL(pc_decide_kernel, dim3(1), dim3(PC_BS), 0, st, pc_parts(n), (const double*)w.part, w.s, (const double*)L, ldl,
                     w.prow, 0);
}
#undef PC_FORMS

void scale_cols(hipStream_t st, int64_t n, int64_t K, double* U, int64_t ldu, const double* S) {
  const int64_t gx = std::min<int64_t>((n + PC_BS - 1) / PC_BS, 1024);
  hipLaunchKernelGGL(pc_scale_cols_kernel, dim3((unsigned)gx, (unsigned)std::min<int64_t>(K, 64)), dim3(PC_BS), 0, st, n, K, U, ldu,
                     S);
}

}}  // namespace gsi::hipk
