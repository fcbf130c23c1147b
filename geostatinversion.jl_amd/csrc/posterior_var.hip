// posterior_var.hip -- the row pass of the PCGA posterior variance, gfx950.
//
//   a[i] = sum_j ( sum_k Z[i,k] W[k,j] )^2        q[i] = sum_k Z[i,k]^2        t[i] = sum_k Z[i,k] u[k]
//
// for a basis Z (n x K, column-major, double or float widened on load) and W (K x ncols).  Z W is never written: the
// products run on the fp64 matrix cores (v_mfma_f64_16x16x4_f64) and are squared and summed while they are accumulators.
//
// Tiling.  A workgroup of 4 waves owns PV_ROWS = 64 rows, 16 per wave; a wave keeps the 16 x (16 NB) products of its rows
// with one column chunk of W in NB accumulator tiles.  NB = 8 (a chunk of 128 columns, 64 accumulator registers) in general,
// NB = 4 for ncols <= 64; the choice depends on ncols alone.  The pass is bound by memory latency, not by the matrix cores:
// what counts is how many waves a SIMD holds (2 with NB = 8; with NB = 16, one wave and one pass over k, the C5 shape took
// 3.1 ms against 2.3 ms, profiles/pcga_posterior.json has the latter).  W passes through LDS in slabs of PV_KS = 16 values of
// k, shared by the 4 waves and fetched one slab ahead into registers; the rows of Z (and u) go from memory straight into the
// operand registers, also one slab ahead.  Z comes from HBM once: with ncols <= 128 there is one pass over k, and a wider W
// is taken chunk by chunk, the workgroup's 64 x K block of Z then coming back from cache, and the chunks' sums are added to
// the rows' sums in chunk order.
//
// Operand maps (gemm_f64_kernel.inc.hpp): the instruction computes D (16 x 16) += A (16 x 4) B (4 x 16), lane l holding
// A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15] in register r.  W' is the A operand and Z' the B
// operand, so D[j][i] = (Z W)[i][j]: a lane's four registers of every tile belong to ONE row i = l & 15 of Z, the sum over j
// is a sum over the lane's own registers, and four lanes (l, l ^ 16, l ^ 32, l ^ 48) hold the four partial sums of a row.
// They are combined pairwise by two exchanges, the same tree in every lane: a row's three sums are a fixed function of that
// row of Z and of W, whatever n is and wherever the row falls in a tile -- no atomics, one owner per row.
//
// Triangular W (upper): W[k, j] with k > j is never read.  For chunk columns [c0, c1) the loop over k stops at min(K, c1),
// groups of four 16-column tiles are skipped in every slab that lies wholly below them, and the entries below the diagonal in
// the tiles that are multiplied are replaced by zeros when the slab is fetched.  q and t are accumulated over each k the first
// time a chunk reaches it; the k no chunk reaches (ncols < K) are read by a short loop at the end.
#include "hip_common.hpp"

namespace gsi { namespace hipk {

namespace {

constexpr int PV_ROWS = 64;                  // rows per workgroup (16 per wave)
constexpr int PV_SMALL = 64;                 // ncols up to this take the NB = 4 kernel
constexpr int PV_KS = 16;                    // values of k per LDS slab

typedef double double4_t __attribute__((ext_vector_type(4)));

// The loads are branch-free: outside the matrix the address falls back to element 0, which always exists and may always be
// read, and the value is replaced by zero.  A predicated load would put a branch around every load and make the compiler wait
// for all loads in flight at every slab.
template <typename T>
__device__ __forceinline__ double pv_load_z(const T* __restrict__ Z, int64_t ldz, int64_t row, int64_t n, int64_t k, int64_t K) {
  const bool ok = row < n && k < K;
  const size_t at = ok ? (size_t)k * (size_t)ldz + (size_t)row : (size_t)0;
  const double v = (double)Z[at];
  return ok ? v : 0.0;
}

__device__ __forceinline__ double pv_load_u(const double* __restrict__ u, int64_t k, int64_t K) {
  const double v = u[k < K ? k : 0];
  return k < K ? v : 0.0;
}

// one slab value: W[k, j], zero outside the matrix and below the diagonal of a triangular W (W[0, 0] is never below it)
__device__ __forceinline__ double pv_load_w(const double* __restrict__ W, int64_t ldw, int64_t k, int64_t K, int64_t j,
                                            int64_t ncols, bool upper) {
  const bool ok = k < K && j < ncols && (!upper || k <= j);
  const size_t at = ok ? (size_t)j * (size_t)ldw + (size_t)k : (size_t)0;
  const double v = W[at];
  return ok ? v : 0.0;
}

// One slab: tiles [BLO, BHI) of the chunk times the slab's PV_KS values of k, without a branch inside, so that the LDS reads
// run ahead of the products.  The caller rounds the tiles it may skip to groups of 4: a tile computed though it lies below
// the diagonal, or beyond the last column, multiplies the zeros the slab fetch put there.
template <int NB, int BLO, int BHI>
__device__ __forceinline__ void pv_slab(double4_t (&acc)[NB], const double* __restrict__ wbase, const double (&zf)[PV_KS / 4]) {
  constexpr int RS = 32 * NB + 4;
#pragma unroll
  for (int s = 0; s < PV_KS / 4; ++s) {
#pragma unroll
    for (int b = BLO; b < BHI; ++b)
      acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(wbase[2 * s * RS + 32 * b], zf[s], acc[b], 0, 0, 0);
  }
}

template <int NB, int BHI>
__device__ __forceinline__ void pv_slab_from(int glo, double4_t (&acc)[NB], const double* __restrict__ wbase,
                                             const double (&zf)[PV_KS / 4]) {
  if (glo <= 0) pv_slab<NB, 0, BHI>(acc, wbase, zf);
  else if (glo == 1) { if constexpr (BHI > 4) pv_slab<NB, 4, BHI>(acc, wbase, zf); }
  else if (glo == 2) { if constexpr (BHI > 8) pv_slab<NB, 8, BHI>(acc, wbase, zf); }
  else { if constexpr (BHI > 12) pv_slab<NB, 12, BHI>(acc, wbase, zf); }
}

// u: K readable doubles even when t is not wanted (the launcher passes W then), so that its loads need no branch
template <typename T, int NB>
__global__ __launch_bounds__(256) void pv_quadform_kernel(const T* __restrict__ Z, int64_t n, int64_t ldz, int64_t K,
                                                          const double* __restrict__ W, int64_t ldw, int64_t ncols, int upper,
                                                          const double* __restrict__ u, int want_t,
                                                          double* __restrict__ a, double* __restrict__ q,
                                                          double* __restrict__ t) {
  constexpr int CHUNK = 16 * NB;
  constexpr int RS = 2 * CHUNK + 4;            // doubles per LDS row: a row holds two values of k of every column, [j][k & 1];
                                               // + 4 puts the 8 rows of a slab on 8 different groups of 4 banks for the writes
  constexpr int WREGS = CHUNK * PV_KS / 256;   // slab values fetched per thread
  __shared__ double Ws[(PV_KS / 2) * RS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 15;            // the row of Z within the wave's 16 / the column of W within a tile
  const int lk = lane >> 4;            // k within a step of 4
  const int64_t row = (int64_t)blockIdx.x * PV_ROWS + wave * 16 + li;
  // the slab fetch: thread -> (k = tid & 15, columns (tid >> 4) + 16 r), 16 consecutive k of a column per 16 threads
  const int fk = tid & 15;
  const int fj = tid >> 4;
  const int fdst = (fk >> 1) * RS + (fk & 1);
  const double* wbase = Ws + (lk >> 1) * RS + (lk & 1) + 2 * li;

  double sa = 0.0, sq = 0.0, stt = 0.0;
  int64_t kdone = 0;                   // q and t hold the terms of every k below this

  for (int64_t c0 = 0; c0 < ncols; c0 += CHUNK) {
    const int64_t c1 = c0 + CHUNK < ncols ? c0 + CHUNK : ncols;
    const int64_t kend = upper ? (K < c1 ? K : c1) : K;
    double4_t acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = double4_t{0.0, 0.0, 0.0, 0.0};

    double wreg[WREGS];
#pragma unroll
    for (int r = 0; r < WREGS; ++r) wreg[r] = pv_load_w(W, ldw, fk, K, c0 + fj + 16 * r, ncols, upper != 0);

    // the rows of Z and the entries of u one slab ahead, like W
    double zn[PV_KS / 4], un[PV_KS / 4];
#pragma unroll
    for (int s = 0; s < PV_KS / 4; ++s) {
      zn[s] = pv_load_z(Z, ldz, row, n, 4 * s + lk, K);
      un[s] = pv_load_u(u, 4 * s + lk, K);
    }

    for (int64_t ks = 0; ks < kend; ks += PV_KS) {
      double zf[PV_KS / 4], uf[PV_KS / 4];
#pragma unroll
      for (int s = 0; s < PV_KS / 4; ++s) { zf[s] = zn[s]; uf[s] = un[s]; }
      __syncthreads();                                  // the previous slab has been read by every wave
#pragma unroll
      for (int r = 0; r < WREGS; ++r) Ws[fdst + 2 * (fj + 16 * r)] = wreg[r];
      __syncthreads();
      // the next slab of W, Z and u, without a branch: they arrive while this slab is multiplied.  Past the end of the loop
      // the guards of the loads return zeros or values nobody uses.
#pragma unroll
      for (int r = 0; r < WREGS; ++r) wreg[r] = pv_load_w(W, ldw, ks + PV_KS + fk, K, c0 + fj + 16 * r, ncols, upper != 0);
#pragma unroll
      for (int s = 0; s < PV_KS / 4; ++s) {
        zn[s] = pv_load_z(Z, ldz, row, n, ks + PV_KS + 4 * s + lk, K);
        un[s] = pv_load_u(u, ks + PV_KS + 4 * s + lk, K);
      }
      if (ks >= kdone) {
#pragma unroll
        for (int s = 0; s < PV_KS / 4; ++s) {
          sq = __builtin_fma(zf[s], zf[s], sq);
          stt = __builtin_fma(zf[s], uf[s], stt);
        }
      }
      // groups of 4 tiles wholly below the diagonal in this slab (columns < ks)
      int glo = 0;
      if (upper && ks > c0) glo = (int)((ks - c0) / 64);
      pv_slab_from<NB, NB>(glo, acc, wbase, zf);
    }
    if (kend > kdone) kdone = ((kend + PV_KS - 1) / PV_KS) * PV_KS;
    // the chunk's squares: one FMA per accumulator element, tiles in order, then onto the row's sum
    double sc = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      sc = __builtin_fma(acc[b][0], acc[b][0], sc);
      sc = __builtin_fma(acc[b][1], acc[b][1], sc);
      sc = __builtin_fma(acc[b][2], acc[b][2], sc);
      sc = __builtin_fma(acc[b][3], acc[b][3], sc);
    }
    sa += sc;
  }
  // the k no chunk reached (a W with fewer columns than rows, or a triangular one narrower than K)
  if (q != nullptr || want_t) {
    for (int64_t ks = kdone; ks < K; ks += 4) {
      const double z = pv_load_z(Z, ldz, row, n, ks + lk, K);
      sq = __builtin_fma(z, z, sq);
      stt = __builtin_fma(z, pv_load_u(u, ks + lk, K), stt);
    }
  }
  // the four lanes of a row: (p0 + p1) + (p2 + p3) in every one of them
  sa += __shfl_xor(sa, 16, 64);
  sa += __shfl_xor(sa, 32, 64);
  sq += __shfl_xor(sq, 16, 64);
  sq += __shfl_xor(sq, 32, 64);
  stt += __shfl_xor(stt, 16, 64);
  stt += __shfl_xor(stt, 32, 64);
  if (lk == 0 && row < n) {
    a[row] = sa;
    if (q != nullptr) q[row] = sq;
    if (want_t) t[row] = stt;
  }
}

__global__ __launch_bounds__(256) void pv_scale_rows_kernel(int64_t m, int64_t c, const double* __restrict__ d,
                                                            const double* __restrict__ src, int64_t lds,
                                                            double* __restrict__ dst, int64_t ldd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j = blockIdx.y;
  if (i < m && j < c) dst[(size_t)j * (size_t)ldd + (size_t)i] = d[i] * src[(size_t)j * (size_t)lds + (size_t)i];
}

template <typename T>
void pv_launch(hipStream_t st, const T* Z, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw, int64_t ncols,
               bool upper, const double* u, double* a, double* q, double* t) {
  const dim3 grid((unsigned)((n + PV_ROWS - 1) / PV_ROWS)), block(256);
  // without u the kernel still reads K doubles through its u pointer (and drops them): the first column of W serves
  const double* up = u ? u : W;
  const int want_t = u ? 1 : 0;
  if (ncols <= PV_SMALL)
    hipLaunchKernelGGL((pv_quadform_kernel<T, 4>), grid, block, 0, st, Z, n, ldz, K, W, ldw, ncols, upper ? 1 : 0, up, want_t, a,
                       q, t);
  else
    hipLaunchKernelGGL((pv_quadform_kernel<T, 8>), grid, block, 0, st, Z, n, ldz, K, W, ldw, ncols, upper ? 1 : 0, up, want_t, a,
                       q, t);
}

}  // namespace

void pv_quadform(hipStream_t st, const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw,
                 int64_t ncols, bool upper, const double* u, double* a, double* q, double* t) {
  if (n < 1) return;
  if (zbits == 32) pv_launch(st, (const float*)Z, n, ldz, K, W, ldw, ncols, upper, u, a, q, t);
  else pv_launch(st, (const double*)Z, n, ldz, K, W, ldw, ncols, upper, u, a, q, t);
}

void pv_scale_rows(hipStream_t st, int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst,
                   int64_t ldd) {
  if (m < 1 || c < 1) return;
  for (int64_t c0 = 0; c0 < c; c0 += 32768) {          // grid.y is limited to 65535
    const int64_t cb = c - c0 < 32768 ? c - c0 : 32768;
    const dim3 grid((unsigned)((m + 255) / 256), (unsigned)cb), block(256);
    hipLaunchKernelGGL(pv_scale_rows_kernel, grid, block, 0, st, m, cb, d, src + (size_t)c0 * (size_t)lds, lds,
                       dst + (size_t)c0 * (size_t)ldd, ldd);
  }
}

}}  // namespace gsi::hipk
