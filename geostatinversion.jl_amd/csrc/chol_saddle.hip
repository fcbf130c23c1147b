// chol_saddle.hip -- the direct solve of pcgadirect's saddle-point system (direct.jl:56-58) on the device; DESIGN.md
// section 4.7c.  For a positive definite A = HQH + R = E E' + R the system [A HX; HX' 0] x = [b1; b2] is one Cholesky
// factorization A = L L', the forward substitutions w = L^-1 HX and v = L^-1 b1, the scalar beta = (w'v - b2) / (w'w) and
// one back substitution xi = L^-T (v - beta w).
//
//   cs_syrk_kernel    C_lower = beta C + alpha P P' (+ R) on the fp64 matrix cores, 64 x 64 tiles that touch the lower
//                     trapezoid only.  P is m x k column-major, so both MFMA operands are 16-row runs of columns of P: no
//                     transpose anywhere.  It forms A (P = E, k = K, R dense or diagonal) and does every trailing update
//                     (P = the panel just solved, k = 64, alpha = -1, beta = 1).
//   cs_potf2_kernel   the 64 x 64 diagonal block, one workgroup, in LDS.  A pivot that is not a positive finite number puts
//                     its 1-based column into the flag (first one wins) and the block is left as it was.
//   cs_trsm_kernel    the panel below the diagonal block, X L11' = A21: row-local, one lane per row, L11 in LDS.
//   cs_schur_kernel   w'w, w'v, beta and z = v - beta w from the two rows carried below the matrix.
//   cs_trsv_lt_kernel one 64-wide block of the back substitution L' xi = z.
// The workspace is an m x n trapezoid (m >= n): rows n .. m-1 are extra rows B that ride through the factorization and come
// out as (L^-1 B')', which is the forward substitution on the right-hand sides at no extra launch.  Every kernel behind a
// failed pivot returns at once on the flag, so no NaN reaches a later step.  No atomics on data (the flag is one
// compare-and-swap): two calls on the same inputs return the same bits.  All offsets are 64-bit.
#include "hip_common.hpp"

namespace gsi { namespace hipk {

namespace {

typedef double cs_double4 __attribute__((ext_vector_type(4)));
constexpr int CS_NB = 64;            // block width of the factorization
constexpr int CS_LD = CS_NB + 1;     // LDS leading dimension of a block held row by row

// rmode 0: nothing added; 1: R dense (lower triangle read, ld ldr); 2: R = the diagonal's entries
__global__ __launch_bounds__(256) void cs_syrk_kernel(double* C, int64_t ldc, int64_t mc, int64_t nc,
                                                      const double* __restrict__ P, int64_t ldp, int64_t k, double alpha,
                                                      double beta, const double* __restrict__ R, int64_t ldr, int rmode,
                                                      const int32_t* __restrict__ flag) {
  if (blockIdx.x < blockIdx.y) return;                 // a tile strictly above the diagonal
  if (*flag != 0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, jl = lane & 15, kk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * 64 + (wave & 1) * 32, c0 = (int64_t)blockIdx.y * 64 + (wave >> 1) * 32;
  if (r0 >= mc || c0 >= nc || r0 + 31 < c0) return;    // outside, or a 32 x 32 quarter above the diagonal
  int64_t rrow[2], crow[2];
  bool rok[2], cok[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    rrow[h] = r0 + 16 * h + jl;  rok[h] = rrow[h] < mc;  if (!rok[h]) rrow[h] = 0;
    crow[h] = c0 + 16 * h + jl;  cok[h] = crow[h] < nc;  if (!cok[h]) crow[h] = 0;
  }
  cs_double4 acc[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 2; ++g) acc[h][g] = (cs_double4){0.0, 0.0, 0.0, 0.0};
  for (int64_t k0 = 0; k0 < k; k0 += 16) {            // four k-steps of 4 per trip: their 16 loads are issued together
    double fr[4][2], fc[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t kc = k0 + 4 * u + kk;
      const bool kok = kc < k;
      const double* col = P + (kok ? kc : 0) * ldp;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        fr[u][h] = (kok && rok[h]) ? col[rrow[h]] : 0.0;
        fc[u][h] = (kok && cok[h]) ? col[crow[h]] : 0.0;
      }
    }
    // a-operand <-> column of C, b-operand <-> row of C: a lane's four results lie in one row, and 16 lanes cover 16
    // consecutive rows of one column of C (stores of 128 contiguous bytes)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int g = 0; g < 2; ++g)
          acc[h][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(fc[u][g], fr[u][h], acc[h][g], 0, 0, 0);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t row = r0 + 16 * h + jl;
    if (row >= mc) continue;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t cl = c0 + 16 * g + kk + 4 * reg;
        if (cl >= nc || cl > row) continue;
        double v = alpha * acc[h][g][reg];
        if (beta != 0.0) v += beta * C[row + cl * ldc];
        if (rmode == 1) v += R[row + cl * ldr];
        else if (rmode == 2 && cl == row) v += R[row];
        C[row + cl * ldc] = v;
      }
  }
}

// The diagonal block A[j0 : j0 + jb, j0 : j0 + jb] (jb <= 64) <- its lower Cholesky factor.
__global__ __launch_bounds__(256) void cs_potf2_kernel(double* A, int64_t ld, int64_t j0, int jb, int32_t* flag) {
  __shared__ double s[CS_NB * CS_LD];
  if (*flag != 0) return;
  const int tid = threadIdx.x;
  double* D = A + j0 + j0 * ld;
  for (int e = tid; e < CS_NB * CS_NB; e += 256) {
    const int r = e & 63, c = e >> 6;
    s[r * CS_LD + c] = (r < jb && c <= r) ? D[r + (int64_t)c * ld] : 0.0;
  }
  __syncthreads();
  const int i = tid & 63, q = tid >> 6;
  for (int c = 0; c < jb; ++c) {
    const double d = s[c * CS_LD + c];
    if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) {        // the same value in every lane: the exit is uniform
      if (tid == 0) atomicCAS(flag, 0, (int32_t)(j0 + c + 1));
      return;
    }
    const double r = sqrt(d);
    __syncthreads();
    if (q == 0) {
      if (i == c) s[c * CS_LD + c] = r;
      else if (i > c && i < jb) s[i * CS_LD + c] /= r;
    }
    __syncthreads();
    if (i < jb) {
      const double lic = s[i * CS_LD + c];
      for (int j = c + 1 + q; j <= i; j += 4) s[i * CS_LD + j] -= lic * s[j * CS_LD + c];
    }
    __syncthreads();
  }
  for (int e = tid; e < CS_NB * CS_NB; e += 256) {
    const int r = e & 63, c = e >> 6;
    if (r < jb && c <= r) D[r + (int64_t)c * ld] = s[r * CS_LD + c];
  }
}

// Rows [j0 + jb, m) of the block column: X L11' = A21 with L11 the factored diagonal block.  One lane per row.  The row's
// 64 entries sit in a column of LDS that only this lane touches (lane-major, so no bank conflicts and no barriers inside
// the solve); L11 is read from LDS at one address per wave.  (The row in 64 registers with the loops unrolled made the
// scheduler hoist the 2016 LDS reads of the solve and spill thousands of registers.)
constexpr int CS_TRSM_THREADS = 64;
__global__ __launch_bounds__(CS_TRSM_THREADS) void cs_trsm_kernel(double* A, int64_t ld, int64_t m, int64_t j0, int jb,
                                                                  const int32_t* __restrict__ flag) {
  __shared__ double Ls[CS_NB * CS_NB];                    // L11[c][t] at c * 64 + t
  __shared__ double xs[CS_NB * CS_TRSM_THREADS];          // this lane's x[c] at c * 64 + lane
  if (*flag != 0) return;
  const int tid = threadIdx.x;
  const double* D = A + j0 + j0 * ld;
  for (int e = tid; e < CS_NB * CS_NB; e += CS_TRSM_THREADS) {
    const int r = e & 63, c = e >> 6;
    Ls[r * CS_NB + c] = (r < jb && c <= r) ? D[r + (int64_t)c * ld] : 0.0;
  }
  const int64_t row = j0 + jb + (int64_t)blockIdx.x * CS_TRSM_THREADS + tid;
  const bool live = row < m;
  double* a = A + (live ? row : j0 + jb) + j0 * ld;
#pragma unroll 8
  for (int c = 0; c < jb; ++c) xs[c * CS_TRSM_THREADS + tid] = live ? a[(int64_t)c * ld] : 0.0;
  __syncthreads();
  for (int c = 0; c < jb; ++c) {
    const double* lc = Ls + c * CS_NB;
    double v0 = xs[c * CS_TRSM_THREADS + tid], v1 = 0.0;
    int t = 0;
#pragma unroll 4
    for (; t + 1 < c; t += 2) {
      v0 -= xs[t * CS_TRSM_THREADS + tid] * lc[t];
      v1 -= xs[(t + 1) * CS_TRSM_THREADS + tid] * lc[t + 1];
    }
    if (t < c) v0 -= xs[t * CS_TRSM_THREADS + tid] * lc[t];
    xs[c * CS_TRSM_THREADS + tid] = (v0 + v1) / lc[c];
  }
  if (!live) return;
#pragma unroll 8
  for (int c = 0; c < jb; ++c) a[(int64_t)c * ld] = xs[c * CS_TRSM_THREADS + tid];
}

// W[nobs, c] = HX[c], W[nobs + 1, c] = b[c]: the two right-hand sides as extra rows of the workspace
__global__ void cs_set_rows_kernel(double* W, int64_t ld, int64_t nobs, const double* __restrict__ HX,
                                   const double* __restrict__ b) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nobs) return;
  W[nobs + c * ld] = HX[c];
  W[nobs + 1 + c * ld] = b[c];
}

// With w = row nobs and v = row nobs + 1 of the factored workspace: beta = (w'v - b2) / (w'w), x[0 : nobs] = v - beta w,
// x[nobs] = beta; out3 = {w'w, beta, 1 if both are usable else 0}.  One workgroup, sums in a fixed order.
__global__ __launch_bounds__(1024) void cs_schur_kernel(const double* __restrict__ W, int64_t ld, int64_t nobs,
                                                        const double* __restrict__ b, double* __restrict__ x,
                                                        double* __restrict__ out3) {
  __shared__ double sw[1024], sv[1024];
  const int tid = threadIdx.x;
  double ww = 0.0, wv = 0.0;
  for (int64_t c = tid; c < nobs; c += 1024) {
    const double w = W[nobs + c * ld], v = W[nobs + 1 + c * ld];
    ww += w * w;
    wv += w * v;
  }
  sw[tid] = ww;
  sv[tid] = wv;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) { sw[tid] += sw[tid + off]; sv[tid] += sv[tid + off]; }
    __syncthreads();
  }
  ww = sw[0];
  wv = sv[0];
  const double beta = (wv - b[nobs]) / ww;
  const bool ok = ww > 0.0 && ww <= 1.79769313486231570815e308 && beta == beta && fabs(beta) <= 1.79769313486231570815e308;
  for (int64_t c = tid; c < nobs; c += 1024)
    x[c] = ok ? W[nobs + 1 + c * ld] - beta * W[nobs + c * ld] : 0.0;
  if (tid == 0) {
    x[nobs] = ok ? beta : 0.0;
    out3[0] = ww;
    out3[1] = beta;
    out3[2] = ok ? 1.0 : 0.0;
  }
}

// x[j0 : j0 + jb] <- L11^-T (x[j0 : j0 + jb] - tail), tail (or null) = L21' x[j0 + jb : n] from gemv_t
__global__ __launch_bounds__(64) void cs_trsv_lt_kernel(const double* __restrict__ A, int64_t ld, int64_t j0, int jb,
                                                        const double* __restrict__ tail, double* __restrict__ x) {
  __shared__ double s[CS_NB * CS_LD];
  __shared__ double rhs[CS_NB];
  const int tid = threadIdx.x;
  const double* D = A + j0 + j0 * ld;
  for (int e = tid; e < CS_NB * CS_NB; e += 64) {
    const int r = e & 63, c = e >> 6;
    s[r * CS_LD + c] = (r < jb && c <= r) ? D[r + (int64_t)c * ld] : 0.0;
  }
  if (tid < jb) rhs[tid] = x[j0 + tid] - (tail ? tail[tid] : 0.0);
  __syncthreads();
  for (int c = jb - 1; c >= 0; --c) {
    const double xc = rhs[c] / s[c * CS_LD + c];
    __syncthreads();
    if (tid == c) rhs[c] = xc;
    else if (tid < c) rhs[tid] -= s[c * CS_LD + tid] * xc;
    __syncthreads();
  }
  if (tid < jb) x[j0 + tid] = rhs[tid];
}

}  // namespace

void cs_syrk_lower(hipStream_t st, double* C, int64_t ldc, int64_t mc, int64_t nc, const double* P, int64_t ldp, int64_t k,
                   double alpha, double beta, const double* R, int64_t ldr, int rmode, const int32_t* flag) {
  if (mc <= 0 || nc <= 0) return;
  const dim3 grid((unsigned)((mc + 63) / 64), (unsigned)((nc + 63) / 64));
  hipLaunchKernelGGL(cs_syrk_kernel, grid, dim3(256), 0, st, C, ldc, mc, nc, P, ldp, k, alpha, beta, R, ldr, rmode, flag);
}

// 3 launches per block column (2 for the last one when m == n): diagonal block, panel, trailing update
void cs_chol_lower(hipStream_t st, double* A, int64_t m, int64_t n, int64_t ld, int32_t* flag) {
  for (int64_t j0 = 0; j0 < n; j0 += CS_NB) {
    const int jb = (int)((n - j0 < CS_NB) ? (n - j0) : CS_NB);
    const int64_t j1 = j0 + jb;
    hipLaunchKernelGGL(cs_potf2_kernel, dim3(1), dim3(256), 0, st, A, ld, j0, jb, flag);
    if (j1 < m) {
      const unsigned g = (unsigned)((m - j1 + CS_TRSM_THREADS - 1) / CS_TRSM_THREADS);
      hipLaunchKernelGGL(cs_trsm_kernel, dim3(g), dim3(CS_TRSM_THREADS), 0, st, A, ld, m, j0, jb, flag);
    }
    if (j1 < n) cs_syrk_lower(st, A + j1 + j1 * ld, ld, m - j1, n - j1, A + j1 + j0 * ld, ld, jb, -1.0, 1.0, nullptr, 0, 0, flag);
  }
}

void cs_set_rows(hipStream_t st, double* W, int64_t ld, int64_t nobs, const double* HX, const double* b) {
  hipLaunchKernelGGL(cs_set_rows_kernel, dim3((unsigned)((nobs + 255) / 256)), dim3(256), 0, st, W, ld, nobs, HX, b);
}

void cs_schur(hipStream_t st, const double* W, int64_t ld, int64_t nobs, const double* b, double* x, double* out3) {
  hipLaunchKernelGGL(cs_schur_kernel, dim3(1), dim3(1024), 0, st, W, ld, nobs, b, x, out3);
}

// L' xi = z in place in x (n entries), from the last block upward: per block gemv_t over the panel below it (two launches,
// slab sums added in index order) and the 64 x 64 triangular solve.  part: gemv_t_workspace_doubles(64) + 64 doubles.
void cs_backsolve(hipStream_t st, const double* A, int64_t n, int64_t ld, double* x, double* part) {
  double* tail = part + gemv_t_workspace_doubles(CS_NB);
  const int64_t nblk = (n + CS_NB - 1) / CS_NB;
  for (int64_t blk = nblk - 1; blk >= 0; --blk) {
    const int64_t j0 = blk * CS_NB;
    const int jb = (int)((n - j0 < CS_NB) ? (n - j0) : CS_NB);
    const int64_t j1 = j0 + jb;
    if (j1 < n) gemv_t(st, n - j1, jb, 1.0, A + j1 + j0 * ld, ld, x + j1, tail, part);
    hipLaunchKernelGGL(cs_trsv_lt_kernel, dim3(1), dim3(64), 0, st, A, ld, j0, jb, (j1 < n) ? tail : (const double*)nullptr, x);
  }
}
size_t cs_backsolve_workspace_doubles() { return gemv_t_workspace_doubles(CS_NB) + CS_NB; }

}}  // namespace gsi::hipk
