// block_pcg.hip -- the multi-column conjugate-gradient solver of block_cg.hip preconditioned by P = Z Z' + diag(d + shift)
// (cg_state.hpp's pcg_* recurrences).  P^-1 = diag(e) - W W' with e = 1 / (d + shift) and
// W = diag(e) Z R^-1, R'R = I + Z' diag(e) Z: z = P^-1 r is a row scaling and two skinny contractions.  Built on
// block_cg.hip's scheme: the fixed grid of 128 row parts x up to 16 column slots, 16-byte lanes where n is even and the
// panels are aligned (8 otherwise), two-stage sums in a fixed order, no float atomics, 64-bit indices, nothing waits for
// the host.
//
//   pass 1   block_cg.hip's cg_pq_kernel as it is                                      reads P, Q (and d)
//            pcg_after_pq for every column
//   pass 2   block_cg.hip's cg_xr_kernel as it is                                      reads X, R, P, Q; writes X, R
//            pcg_after_rr for every column
//   (the caller:  S = W'R  (K x b, gemm_tn),  Y = W S  (n x b, gemm_nn) -- on all b columns, the contraction launchers)
//   pass 3a  part_rz[j] <- partial sums of r_j'(e .* r_j - y_j)                        reads R, Y (and e)
//            pcg_after_rz for every column, after_iter for the batch
//   pass 3b  p_j = (e .* r_j - y_j) + beta_j p_j                                       reads R, Y, P (and e); writes P
//
// r'z is summed from z itself: r'Er - |S_j|^2 is the same number with a cancellation of (lambda_1 + d) / d.  z is not
// stored: pass 3b recomputes it from R, Y and the cache-resident e, which costs what reading a stored z would.
// 16 panel transfers per iteration for the columns that are still active (pass 1: 2, pass 2: 6, the contractions: R read
// and Y written, pass 3a: 2, pass 3b: 4) and two reads of W, against 11 for plain CG.  Passes skip stopped columns.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"
#include "cg_state.hpp"

namespace gsi { namespace hipk {

namespace {
using namespace gsi::cgst;
constexpr int PCG_PARTS = BLOCK_CG_PARTS;
constexpr int PCG_BS = 256;
constexpr int PCG_COLS_Y = 16;

__device__ inline double pcg_block_sum(double v, double* sh) {      // all PCG_BS threads; the same order every time
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return t;
}
__device__ inline double pcg_sum_parts(const double* part) {
  double s = 0.0;
  for (int i = 0; i < PCG_PARTS; ++i) s += part[i];
  return s;
}

// the start: p_j = z0_j = e .* b_j - y_j, partial sums of b_j'b_j and b_j'z0_j, for every column
template <bool VEC>
__global__ __launch_bounds__(PCG_BS) void pcg_z0_kernel(int64_t n, int64_t b, const double* __restrict__ B,
                                                        const double* __restrict__ e, const double* __restrict__ Y,
                                                        double* __restrict__ P, double* __restrict__ part_bb,
                                                        double* __restrict__ part_bz) {
  __shared__ double sh[4];
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    const double* bj = B + j * n;
    const double* y = Y + j * n;
    double* p = P + j * n;
    double abb = 0.0, abz = 0.0;
    if (VEC) {
      const double2* b2 = reinterpret_cast<const double2*>(bj);
      const double2* y2 = reinterpret_cast<const double2*>(y);
      const double2* e2 = reinterpret_cast<const double2*>(e);
      double2* p2 = reinterpret_cast<double2*>(p);
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n / 2; i += (int64_t)PCG_PARTS * PCG_BS) {
        const double2 bv = b2[i], yv = y2[i], ev = e2[i];
        double2 z;
        z.x = ev.x * bv.x - yv.x; z.y = ev.y * bv.y - yv.y;
        p2[i] = z;
        abb += bv.x * bv.x + bv.y * bv.y;
        abz += bv.x * z.x + bv.y * z.y;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n; i += (int64_t)PCG_PARTS * PCG_BS) {
        const double bv = bj[i];
        const double z = e[i] * bv - y[i];
        p[i] = z;
        abb += bv * bv;
        abz += bv * z;
      }
    }
    const double tbb = pcg_block_sum(abb, sh);
    const double tbz = pcg_block_sum(abz, sh);
    if (threadIdx.x == 0) { part_bb[j * PCG_PARTS + blockIdx.x] = tbb; part_bz[j * PCG_PARTS + blockIdx.x] = tbz; }
  }
}
__global__ __launch_bounds__(PCG_BS) void pcg_begin_kernel(double* __restrict__ s, const double* __restrict__ part_bb,
                                                           const double* __restrict__ part_bz, double tol, int64_t maxiter,
                                                           int64_t b) {
  __shared__ int tl[4];
  if (threadIdx.x == 0) { begin(s, b, tol, maxiter); tl[0] = tl[1] = tl[2] = 0; tl[3] = 0x7fffffff; }
  __syncthreads();
  for (int64_t j = threadIdx.x; j < b; j += PCG_BS) {
    pcg_begin_col(s, j, pcg_sum_parts(part_bb + j * PCG_PARTS), pcg_sum_parts(part_bz + j * PCG_PARTS));
    const Tally t = tally_col(s, j);
    if (t.active) atomicAdd(&tl[0], 1);
    if (t.converged) atomicAdd(&tl[1], 1);
    if (t.first_breakdown != 0x7fffffff) atomicMin(&tl[3], t.first_breakdown);
  }
  __syncthreads();
  if (threadIdx.x == 0) after_iter(s, Tally{tl[0], tl[1], 0, tl[3]});
}

__global__ __launch_bounds__(PCG_BS) void pcg_after_pq_kernel(double* __restrict__ s, const double* __restrict__ part) {
  const int64_t b = (int64_t)s[H_NCOLS];
  for (int64_t j = threadIdx.x; j < b; j += PCG_BS) pcg_after_pq(s, j, pcg_sum_parts(part + j * PCG_PARTS));
}
__global__ __launch_bounds__(PCG_BS) void pcg_after_rr_kernel(double* __restrict__ s, const double* __restrict__ part) {
  const int64_t b = (int64_t)s[H_NCOLS];
  for (int64_t j = threadIdx.x; j < b; j += PCG_BS) pcg_after_rr(s, j, pcg_sum_parts(part + j * PCG_PARTS));
}

// pass 3a
template <bool VEC>
__global__ __launch_bounds__(PCG_BS) void pcg_rz_kernel(int64_t n, int64_t b, const double* __restrict__ R,
                                                        const double* __restrict__ Y, const double* __restrict__ e,
                                                        const double* __restrict__ s, double* __restrict__ part) {
  __shared__ double sh[4];
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    if (colv(s, UPDP, j) == 0.0) continue;                          // stopped: pcg_after_rz ignores the sum
    const double* r = R + j * n;
    const double* y = Y + j * n;
    double acc = 0.0;
    if (VEC) {
      const double2* r2 = reinterpret_cast<const double2*>(r);
      const double2* y2 = reinterpret_cast<const double2*>(y);
      const double2* e2 = reinterpret_cast<const double2*>(e);
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n / 2; i += (int64_t)PCG_PARTS * PCG_BS) {
        const double2 rv = r2[i], yv = y2[i], ev = e2[i];
        acc += rv.x * (ev.x * rv.x - yv.x) + rv.y * (ev.y * rv.y - yv.y);
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n; i += (int64_t)PCG_PARTS * PCG_BS) {
        const double rv = r[i];
        acc += rv * (e[i] * rv - y[i]);
      }
    }
    const double tot = pcg_block_sum(acc, sh);
    if (threadIdx.x == 0) part[j * PCG_PARTS + blockIdx.x] = tot;
  }
}
__global__ __launch_bounds__(PCG_BS) void pcg_after_rz_kernel(double* __restrict__ s, const double* __restrict__ part) {
  __shared__ int tl[4];
  const int64_t b = (int64_t)s[H_NCOLS];
  if (threadIdx.x == 0) { tl[0] = tl[1] = tl[2] = 0; tl[3] = 0x7fffffff; }
  __syncthreads();
  for (int64_t j = threadIdx.x; j < b; j += PCG_BS) {
    pcg_after_rz(s, j, pcg_sum_parts(part + j * PCG_PARTS));
    const Tally t = tally_col(s, j);                                // (integer atomics: the sums do not depend on the order)
    if (t.active) atomicAdd(&tl[0], 1);
    if (t.converged) atomicAdd(&tl[1], 1);
    if (t.applied) atomicAdd(&tl[2], 1);
    if (t.first_breakdown != 0x7fffffff) atomicMin(&tl[3], t.first_breakdown);
  }
  __syncthreads();
  if (threadIdx.x == 0) after_iter(s, Tally{tl[0], tl[1], tl[2], tl[3]});
}

// pass 3b
template <bool VEC>
__global__ __launch_bounds__(PCG_BS) void pcg_p_kernel(int64_t n, int64_t b, const double* __restrict__ R,
                                                       const double* __restrict__ Y, const double* __restrict__ e,
                                                       double* __restrict__ P, const double* __restrict__ s) {
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    if (colv(s, UPDP, j) == 0.0) continue;                          // a stopped column's p is left as it is
    const double beta = colv(s, BETA, j);
    const double* r = R + j * n;
    const double* y = Y + j * n;
    double* p = P + j * n;
    if (VEC) {
      const double2* r2 = reinterpret_cast<const double2*>(r);
      const double2* y2 = reinterpret_cast<const double2*>(y);
      const double2* e2 = reinterpret_cast<const double2*>(e);
      double2* p2 = reinterpret_cast<double2*>(p);
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n / 2; i += (int64_t)PCG_PARTS * PCG_BS) {
        const double2 rv = r2[i], yv = y2[i], ev = e2[i];
        double2 pv = p2[i];
        pv.x = (ev.x * rv.x - yv.x) + beta * pv.x; pv.y = (ev.y * rv.y - yv.y) + beta * pv.y;
        p2[i] = pv;
      }
    } else {
      for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n; i += (int64_t)PCG_PARTS * PCG_BS)
        p[i] = (e[i] * r[i] - y[i]) + beta * p[i];
    }
  }
}

// the preconditioner's setup: e holds d + shift (checked positive and finite by the caller)
__global__ __launch_bounds__(PCG_BS) void pcg_rows_kernel(int64_t n, double* __restrict__ e, double* __restrict__ sqe) {
  for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PCG_BS) {
    const double v = 1.0 / e[i];
    e[i] = v;
    sqe[i] = sqrt(v);
  }
}
__global__ __launch_bounds__(PCG_BS) void pcg_add_identity_kernel(double* __restrict__ C, int64_t K) {
  for (int64_t i = (int64_t)blockIdx.x * PCG_BS + threadIdx.x; i < K; i += (int64_t)gridDim.x * PCG_BS) C[i + i * K] += 1.0;
}

inline dim3 pcg_grid(int64_t b) { return dim3(PCG_PARTS, (unsigned)(b < PCG_COLS_Y ? b : PCG_COLS_Y)); }
size_t pcg_state_span(int64_t b) { return (pcg_state_doubles(b) + 7) & ~(size_t)7; }
}  // namespace

// work = [state | part_pq (b x PCG_PARTS) | part_rr | part_rz]; the start keeps b'b in part_pq and b'z0 in part_rr
size_t block_pcg_work_doubles(int64_t b) { return pcg_state_span(b) + 3 * (size_t)b * PCG_PARTS; }

void block_pcg_begin(hipStream_t st, int64_t n, int64_t b, const double* B, const double* e, const double* Y, double* P,
                     double tol, int64_t maxiter, double* work) {
  double* pbb = work + pcg_state_span(b);
  double* pbz = pbb + (size_t)b * PCG_PARTS;
  if (block_cg_vec(n, B, e, Y, P, nullptr))
    hipLaunchKernelGGL(pcg_z0_kernel<true>, pcg_grid(b), dim3(PCG_BS), 0, st, n, b, B, e, Y, P, pbb, pbz);
  else
    hipLaunchKernelGGL(pcg_z0_kernel<false>, pcg_grid(b), dim3(PCG_BS), 0, st, n, b, B, e, Y, P, pbb, pbz);
  hipLaunchKernelGGL(pcg_begin_kernel, dim3(1), dim3(PCG_BS), 0, st, work, (const double*)pbb, (const double*)pbz, tol, maxiter,
                     b);
}

void block_pcg_step_xr(hipStream_t st, int64_t n, int64_t b, const double* Q, const double* d, double* X, double* R,
                       const double* P, double* work) {
  double* s = work;
  double* ppq = work + pcg_state_span(b);
  double* prr = ppq + (size_t)b * PCG_PARTS;
  const bool vec = block_cg_vec(n, Q, d, X, R, P);
  block_cg_pass_pq(st, vec, n, b, P, Q, d, s, ppq);
  hipLaunchKernelGGL(pcg_after_pq_kernel, dim3(1), dim3(PCG_BS), 0, st, s, (const double*)ppq);
  block_cg_pass_xr(st, vec, n, b, P, Q, d, X, R, s, prr);
  hipLaunchKernelGGL(pcg_after_rr_kernel, dim3(1), dim3(PCG_BS), 0, st, s, (const double*)prr);
}

void block_pcg_step_p(hipStream_t st, int64_t n, int64_t b, const double* e, const double* R, const double* Y, double* P,
                      double* work) {
  double* s = work;
  double* prz = work + pcg_state_span(b) + 2 * (size_t)b * PCG_PARTS;
  const dim3 g = pcg_grid(b), bs(PCG_BS);
  if (block_cg_vec(n, e, R, Y, P, nullptr)) {
    hipLaunchKernelGGL(pcg_rz_kernel<true>, g, bs, 0, st, n, b, R, Y, e, (const double*)s, prz);
    hipLaunchKernelGGL(pcg_after_rz_kernel, dim3(1), bs, 0, st, s, (const double*)prz);
    hipLaunchKernelGGL(pcg_p_kernel<true>, g, bs, 0, st, n, b, R, Y, e, P, (const double*)s);
  } else {
    hipLaunchKernelGGL(pcg_rz_kernel<false>, g, bs, 0, st, n, b, R, Y, e, (const double*)s, prz);
    hipLaunchKernelGGL(pcg_after_rz_kernel, dim3(1), bs, 0, st, s, (const double*)prz);
    hipLaunchKernelGGL(pcg_p_kernel<false>, g, bs, 0, st, n, b, R, Y, e, P, (const double*)s);
  }
}

void pcg_precond_rows(hipStream_t st, int64_t n, double* e, double* sqe) {
  const int64_t blocks = (n + PCG_BS - 1) / PCG_BS;
  hipLaunchKernelGGL(pcg_rows_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(PCG_BS), 0, st, n, e, sqe);
}
void pcg_add_identity(hipStream_t st, double* C, int64_t K) {
  hipLaunchKernelGGL(pcg_add_identity_kernel, dim3((unsigned)((K + PCG_BS - 1) / PCG_BS)), dim3(PCG_BS), 0, st, C, K);
}

}}  // namespace gsi::hipk
