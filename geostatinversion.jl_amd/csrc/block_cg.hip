// block_cg.hip -- the vector side of the multi-column conjugate-gradient solver (cg_state.hpp):
// three fused passes over the n x b panels per iteration and two one-workgroup scalar kernels that run cg_state.hpp's
// recurrences with one thread per column.  Nothing waits for the host.
//
//   pass 1  part_pq[j] <- partial sums of p_j'(q_j + d .* p_j)                        reads P, Q (and d)
//           after_pq for every column
//   pass 2  x_j += alpha_j p_j;  r_j -= alpha_j (q_j + d .* p_j);  part_rr[j] <- r_j'r_j    reads X, R, P, Q; writes X, R
//           after_rr for every column, after_iter for the batch
//   pass 3  p_j = r_j + beta_j p_j                                                    reads R, P; writes P
//
// q + d .* p is recomputed in pass 2, not written back in pass 1: pass 2 reads P and Q anyway (x += alpha p needs P), so
// recomputing costs the n doubles of d per column (cache-resident: every column reads the same vector), writing it back
// would cost a panel.  11 panel transfers per iteration for the columns that are still active; a column that has stopped is
// skipped by passes 2 and 3 (and by pass 1), so its x, r and p are not even read.
//
// Panels are column-major with ld = n.  A workgroup owns (row part, column): lanes run along rows, 16 bytes per lane
// where n is even and the panels are 16-byte aligned (8 otherwise), and loop over the columns blockIdx.y, + gridDim.y, ...
// Per-column sums are two-stage: a fixed grid of CG_PARTS row parts, each one block sum in a fixed order, summed in index
// order by the scalar kernels -- no float atomics, two calls give the same bits.  64-bit indices throughout.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"
#include "cg_state.hpp"

namespace gsi { namespace hipk {

namespace {
using namespace gsi::cgst;
constexpr int CG_PARTS = BLOCK_CG_PARTS;   // row parts = partial sums per column and reduction (128)
constexpr int CG_BS = 256;
constexpr int CG_COLS_Y = 16;       // gridDim.y: 128 x 16 = 2048 workgroups at most

__device__ inline double cg_block_sum(double v, double* sh) {       // all CG_BS threads; the same order every time
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return t;
}
__device__ inline double cg_sum_parts(const double* part) {
  double s = 0.0;
  for (int i = 0; i < CG_PARTS; ++i) s += part[i];
  return s;
}
__device__ inline bool cg_live(const double* s, int64_t j) {        // would after_pq advance this column?
  return colv(s, STOPPED, j) == 0.0 && colv(s, ITERS, j) < s[H_MAXITER] && s[H_BREAKDOWN] == 0.0;
}

// partial sums of v_j'v_j (the start: v = B)
template <bool VEC>
__global__ __launch_bounds__(CG_BS) void cg_sumsq_kernel(int64_t n, int64_t b, const double* __restrict__ V,
                                                         double* __restrict__ part) {
  __shared__ double sh[4];
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    const double* v = V + j * n;
    double acc = 0.0;
    if (VEC) {
      const double2* v2 = reinterpret_cast<const double2*>(v);
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n / 2; i += (int64_t)CG_PARTS * CG_BS) {
        const double2 a = v2[i];
        acc += a.x * a.x + a.y * a.y;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += (int64_t)CG_PARTS * CG_BS) acc += v[i] * v[i];
    }
    const double tot = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) part[j * CG_PARTS + blockIdx.x] = tot;
  }
}
__global__ __launch_bounds__(CG_BS) void cg_begin_kernel(double* __restrict__ s, const double* __restrict__ part, double tol,
                                                         int64_t maxiter, int64_t b) {
  __shared__ int tl[4];
  if (threadIdx.x == 0) { begin(s, b, tol, maxiter); tl[0] = tl[1] = tl[2] = 0; tl[3] = 0x7fffffff; }
  __syncthreads();
  for (int64_t j = threadIdx.x; j < b; j += CG_BS) {
    begin_col(s, j, cg_sum_parts(part + j * CG_PARTS));
    const Tally t = tally_col(s, j);
    if (t.active) atomicAdd(&tl[0], 1);
    if (t.converged) atomicAdd(&tl[1], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) after_iter(s, Tally{tl[0], tl[1], 0, 0x7fffffff});
}

// pass 1
template <bool VEC, bool HASD>
__global__ __launch_bounds__(CG_BS) void cg_pq_kernel(int64_t n, int64_t b, const double* __restrict__ P,
                                                      const double* __restrict__ Q, const double* __restrict__ d,
                                                      const double* __restrict__ s, double* __restrict__ part) {
  __shared__ double sh[4];
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    if (!cg_live(s, j)) continue;                                   // (uniform over the workgroup; after_pq ignores the sum)
    const double* p = P + j * n;
    const double* q = Q + j * n;
    double acc = 0.0;
    if (VEC) {
      const double2* p2 = reinterpret_cast<const double2*>(p);
      const double2* q2 = reinterpret_cast<const double2*>(q);
      const double2* d2 = reinterpret_cast<const double2*>(d);
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n / 2; i += (int64_t)CG_PARTS * CG_BS) {
        const double2 pv = p2[i];
        double2 w = q2[i];
        if (HASD) { const double2 dv = d2[i]; w.x += dv.x * pv.x; w.y += dv.y * pv.y; }
        acc += pv.x * w.x + pv.y * w.y;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += (int64_t)CG_PARTS * CG_BS) {
        const double pv = p[i];
        double w = q[i];
        if (HASD) w += d[i] * pv;
        acc += pv * w;
      }
    }
    const double tot = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) part[j * CG_PARTS + blockIdx.x] = tot;
  }
}
__global__ __launch_bounds__(CG_BS) void cg_after_pq_kernel(double* __restrict__ s, const double* __restrict__ part) {
  const int64_t b = (int64_t)s[H_NCOLS];
  for (int64_t j = threadIdx.x; j < b; j += CG_BS) after_pq(s, j, cg_sum_parts(part + j * CG_PARTS));
}

// pass 2
template <bool VEC, bool HASD>
__global__ __launch_bounds__(CG_BS) void cg_xr_kernel(int64_t n, int64_t b, const double* __restrict__ P,
                                                      const double* __restrict__ Q, const double* __restrict__ d,
                                                      double* __restrict__ X, double* __restrict__ R,
                                                      const double* __restrict__ s, double* __restrict__ part) {
  __shared__ double sh[4];
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    if (colv(s, APPLY, j) == 0.0) continue;                         // stopped or out of budget: x_j and r_j are not touched
    const double alpha = colv(s, ALPHA, j);
    const double* p = P + j * n;
    const double* q = Q + j * n;
    double* x = X + j * n;
    double* r = R + j * n;
    double acc = 0.0;
    if (VEC) {
      const double2* p2 = reinterpret_cast<const double2*>(p);
      const double2* q2 = reinterpret_cast<const double2*>(q);
      const double2* d2 = reinterpret_cast<const double2*>(d);
      double2* x2 = reinterpret_cast<double2*>(x);
      double2* r2 = reinterpret_cast<double2*>(r);
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n / 2; i += (int64_t)CG_PARTS * CG_BS) {
        const double2 pv = p2[i];
        double2 w = q2[i];
        if (HASD) { const double2 dv = d2[i]; w.x += dv.x * pv.x; w.y += dv.y * pv.y; }
        double2 xv = x2[i], rv = r2[i];
        xv.x += alpha * pv.x; xv.y += alpha * pv.y;
        rv.x -= alpha * w.x; rv.y -= alpha * w.y;
        x2[i] = xv; r2[i] = rv;
        acc += rv.x * rv.x + rv.y * rv.y;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += (int64_t)CG_PARTS * CG_BS) {
        const double pv = p[i];
        double w = q[i];
        if (HASD) w += d[i] * pv;
        x[i] += alpha * pv;
        const double rv = r[i] - alpha * w;
        r[i] = rv;
        acc += rv * rv;
      }
    }
    const double tot = cg_block_sum(acc, sh);
    if (threadIdx.x == 0) part[j * CG_PARTS + blockIdx.x] = tot;
  }
}
__global__ __launch_bounds__(CG_BS) void cg_after_rr_kernel(double* __restrict__ s, const double* __restrict__ part) {
  __shared__ int tl[4];
  const int64_t b = (int64_t)s[H_NCOLS];
  if (threadIdx.x == 0) { tl[0] = tl[1] = tl[2] = 0; tl[3] = 0x7fffffff; }
  __syncthreads();
  for (int64_t j = threadIdx.x; j < b; j += CG_BS) {
    after_rr(s, j, cg_sum_parts(part + j * CG_PARTS));
    const Tally t = tally_col(s, j);                                // (integer atomics: the sums do not depend on the order)
    if (t.active) atomicAdd(&tl[0], 1);
    if (t.converged) atomicAdd(&tl[1], 1);
    if (t.applied) atomicAdd(&tl[2], 1);
    if (t.first_breakdown != 0x7fffffff) atomicMin(&tl[3], t.first_breakdown);
  }
  __syncthreads();
  if (threadIdx.x == 0) after_iter(s, Tally{tl[0], tl[1], tl[2], tl[3]});
}

// pass 3
template <bool VEC>
__global__ __launch_bounds__(CG_BS) void cg_p_kernel(int64_t n, int64_t b, const double* __restrict__ R, double* __restrict__ P,
                                                     const double* __restrict__ s) {
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    if (colv(s, UPDP, j) == 0.0) continue;                          // a stopped column's p is left as it is
    const double beta = colv(s, BETA, j);
    const double* r = R + j * n;
    double* p = P + j * n;
    if (VEC) {
      const double2* r2 = reinterpret_cast<const double2*>(r);
      double2* p2 = reinterpret_cast<double2*>(p);
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n / 2; i += (int64_t)CG_PARTS * CG_BS) {
        const double2 rv = r2[i];
        double2 pv = p2[i];
        pv.x = rv.x + beta * pv.x; pv.y = rv.y + beta * pv.y;
        p2[i] = pv;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * CG_BS + threadIdx.x; i < n; i += (int64_t)CG_PARTS * CG_BS) p[i] = r[i] + beta * p[i];
    }
  }
}

inline dim3 cg_grid(int64_t b) { return dim3(CG_PARTS, (unsigned)(b < CG_COLS_Y ? b : CG_COLS_Y)); }
inline bool cg_vec(int64_t n, const void* a, const void* b2, const void* c, const void* d, const void* e) {
  auto al = [](const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; };
  return (n & 1) == 0 && al(a) && al(b2) && al(c) && al(d) && al(e);
}
}  // namespace

// work = [state | part_pq (b x CG_PARTS) | part_rr (b x CG_PARTS)]
static size_t cg_state_span(int64_t b) { return (state_doubles(b) + 7) & ~(size_t)7; }
size_t block_cg_work_doubles(int64_t b) { return cg_state_span(b) + 2 * (size_t)b * CG_PARTS; }

// R = P = B has been copied and X cleared by the caller: the columns' |b|^2 and the state of a fresh solve
void block_cg_begin(hipStream_t st, int64_t n, int64_t b, const double* B, double tol, int64_t maxiter, double* work) {
  double* part = work + cg_state_span(b);
  if (cg_vec(n, B, nullptr, nullptr, nullptr, nullptr))
    hipLaunchKernelGGL(cg_sumsq_kernel<true>, cg_grid(b), dim3(CG_BS), 0, st, n, b, B, part);
  else
    hipLaunchKernelGGL(cg_sumsq_kernel<false>, cg_grid(b), dim3(CG_BS), 0, st, n, b, B, part);
  hipLaunchKernelGGL(cg_begin_kernel, dim3(1), dim3(CG_BS), 0, st, work, part, tol, maxiter, b);
}

// passes 1 and 2 on their own: block_pcg.hip runs them in front of its preconditioner passes
bool block_cg_vec(int64_t n, const void* a, const void* b2, const void* c, const void* d, const void* e) {
  return cg_vec(n, a, b2, c, d, e);
}
#define CG_LAUNCH2(K, ...)                                                                                     \
  do {                                                                                                         \
    if (vec && d) hipLaunchKernelGGL((K<true, true>), g, bs, 0, st, __VA_ARGS__);                              \
    else if (vec) hipLaunchKernelGGL((K<true, false>), g, bs, 0, st, __VA_ARGS__);                             \
    else if (d) hipLaunchKernelGGL((K<false, true>), g, bs, 0, st, __VA_ARGS__);                               \
    else hipLaunchKernelGGL((K<false, false>), g, bs, 0, st, __VA_ARGS__);                                     \
  } while (0)
void block_cg_pass_pq(hipStream_t st, bool vec, int64_t n, int64_t b, const double* P, const double* Q, const double* d,
                      const double* s, double* part) {
  const dim3 g = cg_grid(b), bs(CG_BS);
  CG_LAUNCH2(cg_pq_kernel, n, b, P, Q, d, s, part);
}
void block_cg_pass_xr(hipStream_t st, bool vec, int64_t n, int64_t b, const double* P, const double* Q, const double* d,
                      double* X, double* R, const double* s, double* part) {
  const dim3 g = cg_grid(b), bs(CG_BS);
  CG_LAUNCH2(cg_xr_kernel, n, b, P, Q, d, X, R, s, part);
}
#undef CG_LAUNCH2

// everything of one iteration behind the operator product Q = A P
void block_cg_step(hipStream_t st, int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R, double* P,
                   double* work) {
  double* s = work;
  double* ppq = work + cg_state_span(b);
  double* prr = ppq + (size_t)b * CG_PARTS;
  const bool vec = cg_vec(n, Q, d, X, R, P);
  const dim3 g = cg_grid(b), bs(CG_BS);
  block_cg_pass_pq(st, vec, n, b, P, Q, d, s, ppq);
  hipLaunchKernelGGL(cg_after_pq_kernel, dim3(1), bs, 0, st, s, (const double*)ppq);
  block_cg_pass_xr(st, vec, n, b, P, Q, d, X, R, s, prr);
  hipLaunchKernelGGL(cg_after_rr_kernel, dim3(1), bs, 0, st, s, (const double*)prr);
  if (vec) hipLaunchKernelGGL(cg_p_kernel<true>, g, bs, 0, st, n, b, (const double*)R, P, (const double*)s);
  else hipLaunchKernelGGL(cg_p_kernel<false>, g, bs, 0, st, n, b, (const double*)R, P, (const double*)s);
}

}}  // namespace gsi::hipk
