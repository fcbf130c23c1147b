// block_slq.hip -- what stochastic Lanczos quadrature adds to the multi-column solvers of block_cg.hip / block_pcg.hip
// (DESIGN.md section 4.6k):
//
//   slq_trace_begin_kernel   rho0 of every column, once, behind the solver's begin kernel           reads the state
//   slq_trace_kernel         alpha_k, beta_k of every column that advanced, once per iteration,      reads the state
//                            behind cg_after_rr_kernel / pcg_after_rz_kernel (cg_state.hpp's trace_col)
//   slq_quadrature_kernel    slq_state.hpp's quadrature, one thread per column
//   slq_sample_kernel        Zout = Y ./ e + G2 ./ sqrt(e): the panel pass of gsi_precond_sample
//
// The trace kernels are single blocks that only read the state block and write the trace: the solver's own kernels are not
// touched and a traced solve returns the bits of an untraced one.  The quadrature is serial per column (m^2 rotations or so
// on 3 m numbers); columns run along the lanes and every array is column-interleaved, so a wave's loads and stores are
// whole lines.  Nothing here indexes with 32 bits.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hip_common.hpp"
#include "cg_state.hpp"
#include "slq_state.hpp"

namespace gsi { namespace hipk {

namespace {
constexpr int SLQ_BS = 256;
constexpr int SLQ_QBS = 64;            // the quadrature: one wave per block, so that b columns spread over b / 64 CUs

__global__ __launch_bounds__(SLQ_BS) void slq_trace_begin_kernel(const double* __restrict__ s, double* __restrict__ tr,
                                                                 int64_t qmax) {
  const int64_t b = (int64_t)s[cgst::H_NCOLS];
  for (int64_t j = threadIdx.x; j < b; j += SLQ_BS) cgst::trace_begin_col(s, j, tr, qmax);
}
__global__ __launch_bounds__(SLQ_BS) void slq_trace_kernel(const double* __restrict__ s, double* __restrict__ tr, int64_t qmax) {
  const int64_t b = (int64_t)s[cgst::H_NCOLS];
  for (int64_t j = threadIdx.x; j < b; j += SLQ_BS) cgst::trace_col(s, j, tr, qmax);
}

// steps[j] (a whole number stored as a double, 0 .. qmax) entries of column j are used; work: 3 * qmax * b doubles
__global__ __launch_bounds__(SLQ_QBS) void slq_quadrature_kernel(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                 const double* __restrict__ steps, const double* __restrict__ rho0,
                                                                 int64_t qmax, int64_t b, double* __restrict__ work,
                                                                 double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * SLQ_QBS + threadIdx.x;
  if (j >= b) return;
  int64_t m = (int64_t)steps[j];
  if (m < 0) m = 0;
  if (m > qmax) m = qmax;
  double* d = work + j;
  double* e = d + qmax * b;
  double* z = e + qmax * b;
  out[j] = slq::quadrature_log(alpha + j, beta + j, m, rho0[j], b, d, e, z);
}

__global__ __launch_bounds__(SLQ_BS) void slq_sample_kernel(int64_t n, int64_t b, const double* __restrict__ e,
                                                            const double* __restrict__ Y, const double* __restrict__ G2,
                                                            double* __restrict__ Zout) {
  for (int64_t j = blockIdx.y; j < b; j += gridDim.y) {
    const double* y = Y + j * n;
    const double* g = G2 + j * n;
    double* zo = Zout + j * n;
    for (int64_t i = (int64_t)blockIdx.x * SLQ_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SLQ_BS) {
      const double ev = e[i];
      zo[i] = y[i] / ev + g[i] / sqrt(ev);
    }
  }
}
}  // namespace

void slq_trace_begin(hipStream_t st, const double* state, double* tr, int64_t qmax) {
  hipLaunchKernelGGL(slq_trace_begin_kernel, dim3(1), dim3(SLQ_BS), 0, st, state, tr, qmax);
}
void slq_trace_step(hipStream_t st, const double* state, double* tr, int64_t qmax) {
  hipLaunchKernelGGL(slq_trace_kernel, dim3(1), dim3(SLQ_BS), 0, st, state, tr, qmax);
}
void slq_quadrature(hipStream_t st, const double* alpha, const double* beta, const double* steps, const double* rho0,
                    int64_t qmax, int64_t b, double* work, double* out) {
  const int64_t blocks = (b + SLQ_QBS - 1) / SLQ_QBS;
  hipLaunchKernelGGL(slq_quadrature_kernel, dim3((unsigned)blocks), dim3(SLQ_QBS), 0, st, alpha, beta, steps, rho0, qmax, b, work,
                     out);
}
void slq_sample_rows(hipStream_t st, int64_t n, int64_t b, const double* e, const double* Y, const double* G2, double* Zout) {
  const int64_t bx = (n + SLQ_BS - 1) / SLQ_BS;
  hipLaunchKernelGGL(slq_sample_kernel, dim3((unsigned)(bx < 1024 ? bx : 1024), (unsigned)(b < 16 ? b : 16)), dim3(SLQ_BS), 0, st,
                     n, b, e, Y, G2, Zout);
}

}}  // namespace gsi::hipk
