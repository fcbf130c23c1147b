// lowrank_power.hip -- the device side of randsvd's power steps in sample space (hip_backend.hip: lowrank_power_step,
// DESIGN.md section 4.11): the LU's interchanges composed into the step's index lists, and the two triangular solves
// U = c L11^-1 (S[perm(0:l)] T) and C = c T U^-1.  Everything here has a fixed order and uses no atomics on results.
#include "hip_common.hpp"
#include <climits>

namespace gsi { namespace hipk {

constexpr int LRP_MAXL = 384;            // the power step's limit of l (hip_backend.hip)
constexpr int LRP_THREADS = 256;         // the composing workgroup
constexpr int LRP_ITEMS = 3;             // candidates of a moved row per thread: 256 * 3 = 2 * LRP_MAXL

// ---- the interchanges, composed ----
// One workgroup.  P S = L U with LAPACK's interchanges piv[0:l) (0-based: step j exchanges rows j and piv[j] >= j) gives
// (P S)[i] = S[perm(i)], and perm differs from the identity on at most 2 l rows: the l positions on top and the positions
// >= l that a pivot named.  Applying the exchanges one after the other is a chain of l dependent steps; here every step
// looks up its predecessors instead.  Let A[j] be the row at position j just before step j.  A position x >= j holds, before
// step j, what the last earlier step that named it (piv[j'] = x, j' < j) left there, which is A[j'], or x itself.  So
//   A[j] = A[pa(j)],  pa(j) = the last j' < j with piv[j'] = j        (A[j] = j where there is none),
// a forest over the steps that pointer jumping resolves in log2(l) rounds, and with pb(j) = the last j' < j with
// piv[j'] = piv[j]:
//   perm(j) = A[pb(j)] (piv[j] itself where there is none) for an exchange, A[j] for piv[j] = j;
//   perm(x) = A[j] for a position x >= l, j the last step that named x.
// Thread j finds pa, pb and whether it is that last step in one pass over the pivots.  Then the lower positions are sorted
// (rank sort: they are distinct), the moved rows mv = {i : perm(i) != i} are counted in ascending order (a scan over
// [top; sorted lower]), and the three index lists of lr_gather_rows / lr_check_rows are written:
//   rows [0, 2l)                src = perm(mv[k]), sub = mv[k]      (D = S[perm(mv)] - S[mv]);   k >= nmv: S[0] - S[0] = 0
//   rows [o_chk, o_chk + nchk)  src = perm(chk[k]), sub = -1        chk = 0 .. l-1, then the splitmix64 sample of [l, n)
//   rows [o_sm, o_sm + 2l)      src = mv[k], sub = -1               (S[mv]);                      k >= nmv: S[0] - S[0] = 0
// and every row up to ldr that belongs to no block is S[0] - S[0] as well.  The offsets depend on (n, l) alone.
// verdict[0] = *info (the LU's), [1] = 1 where a pivot was out of range (r < j or r >= n; it is clamped to [j, n-1] first, so
// every index written is a row of S), [2] = nmv.
constexpr int LRP_PER = (LRP_MAXL + LRP_THREADS - 1) / LRP_THREADS;   // steps per thread

__global__ __launch_bounds__(LRP_THREADS) void lr_compose_kernel(const int32_t* __restrict__ piv, const int32_t* __restrict__ info,
                                                                 int64_t n, int l, int nchk, int64_t o_chk, int64_t o_sm,
                                                                 int64_t ldr, int64_t* __restrict__ src, int64_t* __restrict__ sub,
                                                                 int64_t* __restrict__ chk, int32_t* __restrict__ verdict) {
  __shared__ int32_t top[LRP_MAXL], pv[LRP_MAXL], up[LRP_MAXL], lk[LRP_MAXL], lv[LRP_MAXL], sk[LRP_MAXL], sv[LRP_MAXL];
  __shared__ int32_t scan[LRP_THREADS];
  __shared__ int32_t cnt_s, bad_s;
  const int tid = threadIdx.x;
  if (tid == 0) { cnt_s = 0; bad_s = 0; }
  __syncthreads();
  for (int j = tid; j < l; j += LRP_THREADS) {
    int64_t r = piv[j];
    if (r < j || r >= n) { bad_s = 1; r = r < j ? j : n - 1; }
    pv[j] = (int32_t)r;
  }
  __syncthreads();
  int pb[LRP_PER];
  bool last[LRP_PER];
#pragma unroll
  for (int u = 0; u < LRP_PER; ++u) {
    const int j = tid + u * LRP_THREADS;
    pb[u] = -1;
    last[u] = false;
    if (j < l) {
      const int r = pv[j];
      int pa = -1;
      bool lst = r >= l;                                // (asked of the lower positions only)
      for (int jp = 0; jp < j; ++jp) {
        const int v = pv[jp];
        if (v == j) pa = jp;
        if (v == r) pb[u] = jp;
      }
      for (int jp = j + 1; jp < l; ++jp)
        if (pv[jp] == r) lst = false;
      last[u] = lst;
      up[j] = pa >= 0 ? pa : j;
    }
  }
  __syncthreads();
  for (int span = 1; span < l; span <<= 1) {            // pointer jumping: up[j] <- the root of j's chain
    int q[LRP_PER];
#pragma unroll
    for (int u = 0; u < LRP_PER; ++u) {
      const int j = tid + u * LRP_THREADS;
      q[u] = j < l ? up[up[j]] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < LRP_PER; ++u) {
      const int j = tid + u * LRP_THREADS;
      if (j < l) up[j] = q[u];
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < LRP_PER; ++u) {
    const int j = tid + u * LRP_THREADS;
    if (j < l) {
      const int r = pv[j];
      top[j] = (r == j) ? up[j] : (pb[u] >= 0 ? up[pb[u]] : r);
      lk[j] = last[u] ? r : INT32_MAX;                  // one entry per lower position, at the last step that named it
      lv[j] = up[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < LRP_PER; ++u) {                   // rank sort of the lower positions
    const int j = tid + u * LRP_THREADS;
    if (j < l && lk[j] != INT32_MAX) {
      const int32_t key = lk[j];
      int rank = 0;
      for (int i = 0; i < l; ++i) rank += (lk[i] < key) ? 1 : 0;
      sk[rank] = key;
      sv[rank] = lv[j];
      atomicAdd(&cnt_s, 1);                             // (a count: the same whatever the order)
    }
  }
  __syncthreads();
  const int cnt = cnt_s;
  // candidates q < l + cnt in ascending position: pos(q) = q | sk[q - l], perm there = top[q] | sv[q - l]
  const int ncand = l + cnt;
  int mine = 0;
  for (int u = 0; u < LRP_ITEMS; ++u) {
    const int q = tid * LRP_ITEMS + u;
    if (q < ncand) mine += (q < l ? (top[q] != q) : (sv[q - l] != sk[q - l])) ? 1 : 0;
  }
  scan[tid] = mine;
  __syncthreads();
  for (int off = 1; off < LRP_THREADS; off <<= 1) {     // inclusive scan
    const int add = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const int nmv = scan[LRP_THREADS - 1];
  int k = scan[tid] - mine;
  for (int u = 0; u < LRP_ITEMS; ++u) {
    const int q = tid * LRP_ITEMS + u;
    if (q >= ncand) break;
    const int32_t pos = q < l ? q : sk[q - l], val = q < l ? top[q] : sv[q - l];
    if (val == pos) continue;
    src[k] = val; sub[k] = pos;
    src[o_sm + k] = pos; sub[o_sm + k] = -1;
    ++k;
  }
  for (int64_t i = tid; i < ldr; i += LRP_THREADS) {    // the rows of no block, and the blocks' rows past nmv: S[0] - S[0]
    const bool used = i < nmv || (i >= o_chk && i < o_chk + nchk) || (i >= o_sm && i < o_sm + nmv);
    if (!used) { src[i] = 0; sub[i] = 0; }
  }
  for (int c = tid; c < nchk; c += LRP_THREADS) {
    int64_t i = c;
    if (c >= l) {                                       // splitmix64 of the (c - l + 1)-th state after the seed
      uint64_t z = 0x9e3779b97f4a7c15ull * (uint64_t)(c - l + 2);
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      i = l + (int64_t)(z % (uint64_t)(n - l));
    }
    int64_t p = i;
    if (i < l) p = top[i];
    else {                                              // binary search of the sorted lower positions
      int lo = 0, hi = cnt;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sk[mid] < i) lo = mid + 1; else hi = mid;
      }
      if (lo < cnt && sk[lo] == i) p = sv[lo];
    }
    chk[c] = i;
    src[o_chk + c] = p; sub[o_chk + c] = -1;
  }
  if (tid == 0) { verdict[0] = info[0]; verdict[1] = bad_s; verdict[2] = nmv; verdict[3] = 0; }
}

void lr_compose(hipStream_t st, const int32_t* piv, const int32_t* info, int64_t n, int64_t l, int64_t nchk, int64_t o_chk,
                int64_t o_sm, int64_t ldr, int64_t* src, int64_t* sub, int64_t* chk, int32_t* verdict) {
  hipLaunchKernelGGL(lr_compose_kernel, dim3(1), dim3(LRP_THREADS), 0, st, piv, info, n, (int)l, (int)nchk, o_chk, o_sm, ldr,
                     src, sub, chk, verdict);
}

// ---- the triangular solves ----
// One wave solves M x = b for NC right-hand sides at once, M (m x m, ld ldm) lower triangular, column-major: lane i of block t
// owns row 64 t + i, so a column of M is one contiguous load.  The right-hand sides lie in LDS (xs[c][i]) and are replaced by
// the solutions.  Block by block: the rows of the block first take the solved blocks' contribution (left-looking; the solved
// x are broadcast reads of LDS), then the 64 x 64 diagonal block is solved inside the wave, x_j going from its lane to the
// others through v_readlane.  What the kernel waits for is memory, not arithmetic (m^2 / 2 * NC fused multiply-adds): the 64
// columns of a block are loaded together, before any is used, so a block row of M costs one round trip per block instead of
// one per few columns.  The l steps of the diagonal blocks are the other chain, so each is kept to a v_readlane pair and one
// multiply-add per right-hand side: a lane's part of the diagonal block is loaded with zeros on and above the diagonal, and
// where the diagonal is not 1 (UNIT = false) the row -- its right-hand side, after the update, and its entries in the block --
// is scaled by 1 / M_ii first.  A zero on the diagonal then makes the solution non-finite, which the step's check reads as a
// decline.  Lanes past the last row work on a copy of it and store nothing; columns past it are loaded as zeros.  The
// workgroup is this one wave: __syncthreads() orders its LDS traffic and costs nothing else.
__device__ __forceinline__ double lrp_readlane(double v, int srclane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
  return __hiloint2double(hi, lo);
}

template <int NC, bool UNIT>
__device__ __forceinline__ void lrp_lower_solve(const double* __restrict__ M, int64_t ldm, int m, double (*xs)[LRP_MAXL],
                                                int lane) {
  const int nb = (m + 63) >> 6;
  for (int t = 0; t < nb; ++t) {
    const int row = t * 64 + lane;
    const int rowc = row < m ? row : m - 1;
    const double* __restrict__ Mr = M + rowc;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = xs[c][rowc];
    for (int j0 = 0; j0 < t * 64; j0 += 64) {
      double a[64];
#pragma unroll
      for (int u = 0; u < 64; ++u) a[u] = Mr[(int64_t)(j0 + u) * ldm];
      __builtin_amdgcn_sched_barrier(0);                // (all 64 loads in flight before the first is used)
#pragma unroll
      for (int u = 0; u < 64; ++u)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = fma(-a[u], xs[c][j0 + u], acc[c]);
    }
    double a[64];
#pragma unroll
    for (int u = 0; u < 64; ++u) {
      const int col = t * 64 + u;
      a[u] = Mr[(int64_t)(col < m ? col : m - 1) * ldm];
    }
    const double d = UNIT ? 1.0 : M[rowc + (int64_t)rowc * ldm];
    __builtin_amdgcn_sched_barrier(0);
    if (!UNIT) {
      const double rd = 1.0 / d;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] *= rd;
#pragma unroll
      for (int u = 0; u < 64; ++u) a[u] *= rd;
    }
#pragma unroll
    for (int u = 0; u < 64; ++u) a[u] = (rowc > t * 64 + u) ? a[u] : 0.0;
#pragma unroll
    for (int u = 0; u < 64; ++u)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fma(-a[u], lrp_readlane(acc[c], u), acc[c]);
    if (row < m) {
#pragma unroll
      for (int c = 0; c < NC; ++c) xs[c][row] = acc[c];
    }
    __syncthreads();
  }
}

// Ut (l x l, ld l) <- U' on and below its diagonal, U = c L11^-1 Mp: workgroup b solves the columns [b NC, b NC + NC) of Mp
// (l x l, ld l) against the unit lower triangle on top of L (ld ldl) and writes them as rows.  U is upper triangular, so a
// column j needs its first j + 1 rows only; what L11^-1 Mp leaves below the diagonal is rounding and is not formed.
template <int NC>
__global__ __launch_bounds__(64) void lr_solve_u_kernel(const double* __restrict__ L, int64_t ldl, const double* __restrict__ Mp,
                                                        int l, double c, double* __restrict__ Ut) {
  __shared__ double xs[NC][LRP_MAXL];
  const int lane = threadIdx.x, col0 = blockIdx.x * NC;
  const int m = (col0 + NC < l) ? col0 + NC : l;
  double v[NC][LRP_MAXL / 64];
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) {
      const int i = ib * 64 + lane;
      v[cc][ib] = (i < m && col0 + cc < l) ? Mp[i + (int64_t)(col0 + cc) * l] : 0.0;
    }
  __builtin_amdgcn_sched_barrier(0);                    // (the loads together, then the stores to LDS)
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) xs[cc][ib * 64 + lane] = v[cc][ib];
  __syncthreads();
  lrp_lower_solve<NC, true>(L, ldl, m, xs, lane);
  for (int cc = 0; cc < NC; ++cc) {
    const int col = col0 + cc;
    if (col >= l) break;
    for (int i = lane; i <= col; i += 64) Ut[col + (int64_t)i * l] = c * xs[cc][i];
  }
}

// C (N x l, ld N) <- c T U^-1: row r of C solves U' x = T[r, :]', and Ut = U' is lower triangular with contiguous columns.
// Workgroup b takes the rows [b NC, b NC + NC) of T (N x l, ld N).
template <int NC>
__global__ __launch_bounds__(64) void lr_solve_c_kernel(const double* __restrict__ Ut, int l, const double* __restrict__ T,
                                                        int64_t N, double c, double* __restrict__ C) {
  __shared__ double xs[NC][LRP_MAXL];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * NC;
  double v[NC][LRP_MAXL / 64];
#pragma unroll
  for (int cc = 0; cc < NC; ++cc) {
    const int64_t r = r0 + cc < N ? r0 + cc : N - 1;
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) {
      const int i = ib * 64 + lane;
      v[cc][ib] = i < l ? T[r + (int64_t)i * N] : 0.0;
    }
  }
  __builtin_amdgcn_sched_barrier(0);                    // (the loads together, then the stores to LDS)
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) xs[cc][ib * 64 + lane] = v[cc][ib];
  __syncthreads();
  lrp_lower_solve<NC, false>(Ut, l, l, xs, lane);
  for (int cc = 0; cc < NC; ++cc) {
    if (r0 + cc >= N) break;
    for (int i = lane; i < l; i += 64) C[r0 + cc + (int64_t)i * N] = c * xs[cc][i];
  }
}

constexpr int LRP_NC_U = 2, LRP_NC_C = 4;

void lr_solve_u(hipStream_t st, const double* L, int64_t ldl, const double* Mp, int64_t l, double c, double* Ut) {
  hipLaunchKernelGGL(lr_solve_u_kernel<LRP_NC_U>, dim3((unsigned)((l + LRP_NC_U - 1) / LRP_NC_U)), dim3(64), 0, st, L, ldl, Mp,
                     (int)l, c, Ut);
}
void lr_solve_c(hipStream_t st, const double* Ut, int64_t l, const double* T, int64_t N, double c, double* C) {
  hipLaunchKernelGGL(lr_solve_c_kernel<LRP_NC_C>, dim3((unsigned)((N + LRP_NC_C - 1) / LRP_NC_C)), dim3(64), 0, st, Ut, (int)l, T,
                     N, c, C);
}

// ---- a panel factored in two column halves (hip_backend.hip: lowrank_split_*) ----
// The first l1 rows of U, [U11 | U12] = c L11^-1 Mp, from the l1 pivot rows of the left half: Mp (l1 x l, ld l1) = S[perm(0:l1)] T,
// L11 the unit lower triangle on top of the left half.  Workgroup b solves the columns [b NC, b NC + NC).  A column j < l1
// belongs to the upper triangular U11 and stops at row j; it is written as row j of Ut11 (l1 x l1, ld l1: U11', what
// lr_solve_c_kernel reads).  A column j >= l1 is a column of U12 (l1 x (l - l1), ld l1), written as it stands.
template <int NC>
__global__ __launch_bounds__(64) void lr_solve_u12_kernel(const double* __restrict__ L, int64_t ldl, const double* __restrict__ Mp,
                                                          int l1, int l, double c, double* __restrict__ Ut11,
                                                          double* __restrict__ U12) {
  __shared__ double xs[NC][LRP_MAXL];
  const int lane = threadIdx.x, col0 = blockIdx.x * NC;
  const int m = (col0 + NC < l1) ? col0 + NC : l1;
  double v[NC][LRP_MAXL / 64];
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) {
      const int i = ib * 64 + lane;
      v[cc][ib] = (i < m && col0 + cc < l) ? Mp[i + (int64_t)(col0 + cc) * l1] : 0.0;
    }
  __builtin_amdgcn_sched_barrier(0);                    // (the loads together, then the stores to LDS)
#pragma unroll
  for (int cc = 0; cc < NC; ++cc)
#pragma unroll
    for (int ib = 0; ib < LRP_MAXL / 64; ++ib) xs[cc][ib * 64 + lane] = v[cc][ib];
  __syncthreads();
  lrp_lower_solve<NC, true>(L, ldl, m, xs, lane);
  for (int cc = 0; cc < NC; ++cc) {
    const int col = col0 + cc;
    if (col >= l) break;
    if (col < l1) {
      for (int i = lane; i <= col; i += 64) Ut11[col + (int64_t)i * l1] = c * xs[cc][i];
    } else {
      for (int i = lane; i < l1; i += 64) U12[i + (int64_t)(col - l1) * l1] = c * xs[cc][i];
    }
  }
}

void lr_solve_u12(hipStream_t st, const double* L, int64_t ldl, const double* Mp, int64_t l1, int64_t l, double c, double* Ut11,
                  double* U12) {
  hipLaunchKernelGGL(lr_solve_u12_kernel<LRP_NC_U>, dim3((unsigned)((l + LRP_NC_U - 1) / LRP_NC_U)), dim3(64), 0, st, L, ldl, Mp,
                     (int)l1, (int)l, c, Ut11, U12);
}

// The interchanges of one half applied to nc columns of the other, X (ld ldx): X[sub[k]] <- X[src[k]] for the moved rows
// k < nmv = verdict[2] of lr_compose (src[k] = perm(sub[k]); at most maxmv).  Every moved row is read into tmp (ld ldt) before
// any is written -- two launches --, so the order among them does not matter and no column waits for a chain of exchanges.
// The second launch also writes zeros to the rows [0, nzero): the block above the right half's Schur complement.
__global__ __launch_bounds__(256) void lr_rows_out_kernel(const double* __restrict__ X, int64_t ldx, int nc,
                                                          const int64_t* __restrict__ src, const int32_t* __restrict__ verdict,
                                                          int maxmv, double* __restrict__ tmp, int64_t ldt) {
  const int nmv = verdict[2] < maxmv ? verdict[2] : maxmv;
  const int64_t total = (int64_t)nmv * nc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = e % nmv, c = e / nmv;
    tmp[k + c * ldt] = X[src[k] + c * ldx];
  }
}
__global__ __launch_bounds__(256) void lr_rows_in_kernel(double* __restrict__ X, int64_t ldx, int nc,
                                                         const int64_t* __restrict__ sub, const int32_t* __restrict__ verdict,
                                                         int maxmv, const double* __restrict__ tmp, int64_t ldt, int nzero) {
  const int nmv = verdict[2] < maxmv ? verdict[2] : maxmv;
  const int64_t rows = (int64_t)nmv + nzero, total = rows * nc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = e % rows, c = e / rows;
    if (k < nmv) {
      const int64_t r = sub[k];
      X[r + c * ldx] = r < nzero ? 0.0 : tmp[k + c * ldt];      // (a row both branches reach gets the same zero from both)
    } else {
      X[(k - nmv) + c * ldx] = 0.0;
    }
  }
}

void lr_move_rows(hipStream_t st, double* X, int64_t ldx, int64_t nc, const int64_t* src, const int64_t* sub,
                  const int32_t* verdict, int64_t maxmv, double* tmp, int64_t ldt, int64_t nzero) {
  if (nc < 1 || maxmv < 1) return;
  const unsigned g_out = (unsigned)((maxmv * nc + 255) / 256), g_in = (unsigned)(((maxmv + nzero) * nc + 255) / 256);
  hipLaunchKernelGGL(lr_rows_out_kernel, dim3(g_out), dim3(256), 0, st, X, ldx, (int)nc, src, verdict, (int)maxmv, tmp, ldt);
  hipLaunchKernelGGL(lr_rows_in_kernel, dim3(g_in), dim3(256), 0, st, X, ldx, (int)nc, sub, verdict, (int)maxmv, tmp, ldt,
                     (int)nzero);
}

// dst[j] <- piv[j] + add, j < cnt: the first half's interchanges kept while the second factorization reuses the workspace they
// lie in, then the second half's appended in the whole panel's row numbers
__global__ __launch_bounds__(256) void lr_pivots_kernel(const int32_t* __restrict__ piv, int cnt, int32_t add,
                                                        int32_t* __restrict__ dst) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < cnt) dst[j] = piv[j] + add;
}
void lr_pivots(hipStream_t st, const int32_t* piv, int64_t cnt, int64_t add, int32_t* dst) {
  hipLaunchKernelGGL(lr_pivots_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, piv, (int)cnt, (int32_t)add, dst);
}

// A zero pivot that a half's factorization flagged (info = its column + 1) is forgotten: the panel is factored again whole,
// and that factorization reports its own.  A lost exchange (info < 0) stays.
__global__ void lr_forget_zero_pivot_kernel(int32_t* __restrict__ info) {
  if (info[0] > 0) info[0] = 0;
}
void lr_forget_zero_pivot(hipStream_t st, int32_t* info) {
  hipLaunchKernelGGL(lr_forget_zero_pivot_kernel, dim3(1), dim3(1), 0, st, info);
}

}}  // namespace gsi::hipk
