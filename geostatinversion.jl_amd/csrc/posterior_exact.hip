// posterior_exact.hip -- the device side of the exact posterior variance of linear inversion and kriging (DESIGN.md section
// 4.6m), gfx950: the row pass over the n x b panels T_J = C H' (L^-T)[:, J], and the two small kernels around the Cholesky
// factorization of the doubled trapezoid [M; Phi'; I].
//
//   px_rowdot_kernel   acc[i] += sum over c < b of A[i, c] B[i, c] for column-major panels with leading dimensions.  Lanes run
//                      along i, so every column access of a wave is whole lines; 16 bytes per lane where n and the leading
//                      dimensions are even and the bases 16-byte aligned, 8 otherwise (a resident matrix has ld = rows, so
//                      an odd n has every other column off the 16-byte grid).  PX_UNROLL columns' loads are issued before the first add.  The grid is capped at
//                      PX_MAX_BLOCKS workgroups and strided beyond that; offsets i + c ld are 64-bit.  One owner per row, no
//                      atomics.  The file is compiled with fp contraction off: every product is rounded on its own and added
//                      to the row's running sum, which starts from acc[i], in ascending c -- the result is a pure function
//                      of the operands' bits (posterior_exact_host.hpp and tests/posterior_exact_model.py state the same
//                      sums), and it does not depend on how the columns are cut into batches.  SAME: B is A, loaded once.
//   px_unit_kernel     E (nobs x b) <- zeros with a one at (c0 + c, c): the right-hand sides that make the operator's own
//                      product write columns [c0, c0 + b) of H C H'.
//   px_rows_kernel     the carried rows of the (2 nobs + p) x nobs trapezoid: diag onto the diagonal, rows [nobs, nobs + p)
//                      <- Phi', rows [nobs + p, 2 nobs + p) <- I.
//   px_carried_kernel  W_d (nobs x p) <- the transpose of the factored rows [nobs, nobs + p).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"

#pragma clang fp contract(off)

namespace gsi { namespace hipk {

namespace {

constexpr int PX_BS = 256;
constexpr int PX_UNROLL = 8;              // columns whose loads are in flight before the first add
constexpr int PX_MAX_BLOCKS = 1024;       // 4 workgroups per CU of an MI355X; longer panels are grid-strided
// (tests/test_posterior_exact_gpu.py places n just beyond PX_MAX_BLOCKS * PX_BS lanes: its SWEEP_* follow these two)

template <bool SAME, bool VEC>
__global__ __launch_bounds__(PX_BS) void px_rowdot_kernel(int64_t n, int64_t b, const double* __restrict__ A, int64_t lda,
                                                          const double* __restrict__ B, int64_t ldb, double* __restrict__ acc) {
  const int64_t first = (int64_t)blockIdx.x * PX_BS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * PX_BS;
  if (VEC) {
    const int64_t nv = n >> 1;
    for (int64_t v = first; v < nv; v += stride) {
      const size_t i = (size_t)v * 2;
      double2 s = *reinterpret_cast<const double2*>(acc + i);
      int64_t c = 0;
      for (; c + PX_UNROLL <= b; c += PX_UNROLL) {
        double2 a[PX_UNROLL], q[PX_UNROLL];
#pragma unroll
        for (int u = 0; u < PX_UNROLL; ++u) {
          a[u] = *reinterpret_cast<const double2*>(A + i + (size_t)(c + u) * (size_t)lda);
          if (!SAME) q[u] = *reinterpret_cast<const double2*>(B + i + (size_t)(c + u) * (size_t)ldb);
        }
#pragma unroll
        for (int u = 0; u < PX_UNROLL; ++u) {
          const double2 w = SAME ? a[u] : q[u];
          const double px = a[u].x * w.x, py = a[u].y * w.y;
          s.x = s.x + px;
          s.y = s.y + py;
        }
      }
      for (; c < b; ++c) {
        const double2 av = *reinterpret_cast<const double2*>(A + i + (size_t)c * (size_t)lda);
        const double2 w = SAME ? av : *reinterpret_cast<const double2*>(B + i + (size_t)c * (size_t)ldb);
        const double px = av.x * w.x, py = av.y * w.y;
        s.x = s.x + px;
        s.y = s.y + py;
      }
      *reinterpret_cast<double2*>(acc + i) = s;
    }
  } else {
    for (int64_t r = first; r < n; r += stride) {
      const size_t i = (size_t)r;
      double s = acc[i];
      int64_t c = 0;
      for (; c + PX_UNROLL <= b; c += PX_UNROLL) {
        double a[PX_UNROLL], q[PX_UNROLL];
#pragma unroll
        for (int u = 0; u < PX_UNROLL; ++u) {
          a[u] = A[i + (size_t)(c + u) * (size_t)lda];
          if (!SAME) q[u] = B[i + (size_t)(c + u) * (size_t)ldb];
        }
#pragma unroll
        for (int u = 0; u < PX_UNROLL; ++u) {
          const double pr = a[u] * (SAME ? a[u] : q[u]);
          s = s + pr;
        }
      }
      for (; c < b; ++c) {
        const double av = A[i + (size_t)c * (size_t)lda];
        const double pr = av * (SAME ? av : B[i + (size_t)c * (size_t)ldb]);
        s = s + pr;
      }
      acc[i] = s;
    }
  }
}

__global__ __launch_bounds__(PX_BS) void px_unit_kernel(double* __restrict__ E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) {
  const int64_t r = (int64_t)blockIdx.x * PX_BS + threadIdx.x;
  if (r >= nobs) return;
  for (int64_t c = blockIdx.y; c < b; c += gridDim.y) E[(size_t)r + (size_t)c * (size_t)ld] = (r == c0 + c) ? 1.0 : 0.0;
}

// thread (r, j), r in [0, p + nobs): row nobs + r of column j; the thread that writes the identity's one adds diag[j]
__global__ __launch_bounds__(PX_BS) void px_rows_kernel(double* __restrict__ T, int64_t ld, int64_t nobs, int64_t p,
                                                        const double* __restrict__ diag, const double* __restrict__ Phi,
                                                        int64_t ldphi) {
  const int64_t r = (int64_t)blockIdx.x * PX_BS + threadIdx.x;
  if (r >= nobs + p) return;
  for (int64_t j = blockIdx.y; j < nobs; j += gridDim.y) {
    double* cj = T + (size_t)j * (size_t)ld;
    if (r < p) {
      cj[nobs + r] = Phi[(size_t)j + (size_t)r * (size_t)ldphi];
    } else {
      const bool one = (r - p == j);
      cj[nobs + r] = one ? 1.0 : 0.0;
      if (one && diag != nullptr) cj[j] = cj[j] + diag[j];
    }
  }
}

__global__ __launch_bounds__(PX_BS) void px_carried_kernel(const double* __restrict__ T, int64_t ld, int64_t nobs, int64_t p,
                                                           double* __restrict__ Wd) {
  const int64_t j = (int64_t)blockIdx.x * PX_BS + threadIdx.x;
  if (j >= nobs) return;
  for (int64_t k = blockIdx.y; k < p; k += gridDim.y)
    Wd[(size_t)j + (size_t)k * (size_t)nobs] = T[(size_t)(nobs + k) + (size_t)j * (size_t)ld];
}

inline unsigned px_grid_y(int64_t cols) { return (unsigned)(cols < 32768 ? (cols > 0 ? cols : 1) : 32768); }

}  // namespace

void px_rowdot_acc(hipStream_t st, int64_t n, int64_t b, const double* A, int64_t lda, const double* B, int64_t ldb, double* acc) {
  if (n < 1 || b < 1) return;
  const bool same = (A == B && lda == ldb);
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = (n & 1) == 0 && (lda & 1) == 0 && (ldb & 1) == 0 && al(A) && al(B) && al(acc);
  const int64_t items = vec ? (n >> 1) : n;
  int64_t blocks = (items + PX_BS - 1) / PX_BS;
  if (blocks > PX_MAX_BLOCKS) blocks = PX_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks), block(PX_BS);
  if (same && vec) hipLaunchKernelGGL((px_rowdot_kernel<true, true>), grid, block, 0, st, n, b, A, lda, B, ldb, acc);
  else if (same) hipLaunchKernelGGL((px_rowdot_kernel<true, false>), grid, block, 0, st, n, b, A, lda, B, ldb, acc);
  else if (vec) hipLaunchKernelGGL((px_rowdot_kernel<false, true>), grid, block, 0, st, n, b, A, lda, B, ldb, acc);
  else hipLaunchKernelGGL((px_rowdot_kernel<false, false>), grid, block, 0, st, n, b, A, lda, B, ldb, acc);
}

void px_unit_panel(hipStream_t st, double* E, int64_t ld, int64_t nobs, int64_t b, int64_t c0) {
  if (nobs < 1 || b < 1) return;
  const dim3 grid((unsigned)((nobs + PX_BS - 1) / PX_BS), px_grid_y(b)), block(PX_BS);
  hipLaunchKernelGGL(px_unit_kernel, grid, block, 0, st, E, ld, nobs, b, c0);
}

void px_trapezoid_rows(hipStream_t st, double* T, int64_t ld, int64_t nobs, int64_t p, const double* diag, const double* Phi,
                       int64_t ldphi) {
  if (nobs < 1) return;
  const dim3 grid((unsigned)((nobs + p + PX_BS - 1) / PX_BS), px_grid_y(nobs)), block(PX_BS);
  hipLaunchKernelGGL(px_rows_kernel, grid, block, 0, st, T, ld, nobs, p, diag, Phi, ldphi);
}

void px_carried_rows(hipStream_t st, const double* T, int64_t ld, int64_t nobs, int64_t p, double* Wd) {
  if (nobs < 1 || p < 1) return;
  const dim3 grid((unsigned)((nobs + PX_BS - 1) / PX_BS), px_grid_y(p)), block(PX_BS);
  hipLaunchKernelGGL(px_carried_kernel, grid, block, 0, st, T, ld, nobs, p, Wd);
}

}}  // namespace gsi::hipk
