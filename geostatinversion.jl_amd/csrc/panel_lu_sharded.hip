// panel_lu_sharded.hip -- the row-sharded form of `F = lu(Y); Q = F.L` ("sharded alternative"): every rank keeps
// only its rows [row0, row0 + mloc) of the panel; per pivot step the ranks exchange one record each {local max |value|, its
// global row, that row, row j} (pipeline.cpp:lu_panel_sharded runs the collectives), everything else is row-local.  The
// arithmetic per element is the register-resident kernel's, operation for operation (same blocks of 64, leaves of 8, the same
// forward substitution for U12, fma(-l, u, a) in the same order, the same rank-64 MFMA update: panel_lu_blocks.hip), so the
// result is bit-identical to the single-rank factorization -- tests/test_gpu_parity.py compares them on the GPU.
// Leaf columns live in HBM between the steps here (a step is host-sequenced around a collective, not a persistent launch).
// Record (doubles): [0] max |value| (-1: none), [1] global row (as a double), [2] 1.0 if this rank holds row j,
//                   [4, 4 + l) the candidate row, [4 + l, 4 + 2 l) row j.
// Also here, for the multi-rank persistent leaves (panel_lu_leaf.hip: lu2_leaf_mr): the interchanges of the columns outside a
// leaf across ranks (lus_swap_*), and the time-out flag's way through an all-reduce.
#include "panel_lu_dev.hpp"

namespace gsi { namespace hipk {

namespace {
constexpr int LUS_HDR = 4;

__global__ __launch_bounds__(256) void lus_cand_partial_kernel(const double* __restrict__ Y, int64_t ld, int64_t mloc,
                                                               int64_t row0, int64_t j, double* __restrict__ pval,
                                                               int64_t* __restrict__ pidx) {
  __shared__ double s_v[4];
  __shared__ int32_t s_i[4];
  double best = -1.0;
  int32_t besti = -1;
  for (int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x; li < mloc; li += (int64_t)gridDim.x * 256) {
    const int64_t gi = row0 + li;
    if (gi >= j) {
      const double av = fabs(Y[li + j * ld]);
      if (av > best) { best = av; besti = (int32_t)gi; }     // ascending rows per thread: the first maximum stays
    }
  }
  wave_argmax(best, besti);
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x < 64) {
    double v = (threadIdx.x < 4) ? s_v[threadIdx.x] : -1.0;
    int32_t i = (threadIdx.x < 4) ? s_i[threadIdx.x] : -1;
    wave_argmax8(v, i);
    if (threadIdx.x == 0) { pval[blockIdx.x] = v; pidx[blockIdx.x] = i; }
  }
}
__global__ __launch_bounds__(256) void lus_cand_final_kernel(const double* __restrict__ Y, int64_t ld, int64_t mloc,
                                                             int64_t row0, int64_t l, int64_t j, int nparts,
                                                             const double* __restrict__ pval, const int64_t* __restrict__ pidx,
                                                             double* __restrict__ rec) {
  __shared__ double s_v[4];
  __shared__ int32_t s_i[4];
  __shared__ int32_t s_win;
  double best = -1.0;
  int32_t besti = -1;
  for (int p = threadIdx.x; p < nparts; p += 256) {
    const double v = pval[p];
    const int32_t i = (int32_t)pidx[p];
    if (v > best || (v == best && (uint32_t)i < (uint32_t)besti)) { best = v; besti = i; }
  }
  wave_argmax(best, besti);
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x < 64) {
    double v = (threadIdx.x < 4) ? s_v[threadIdx.x] : -1.0;
    int32_t i = (threadIdx.x < 4) ? s_i[threadIdx.x] : -1;
    wave_argmax8(v, i);
    if (threadIdx.x == 0) {
      s_win = i;
      rec[0] = v;
      rec[1] = (double)i;
      rec[2] = (j >= row0 && j < row0 + mloc) ? 1.0 : 0.0;
      rec[3] = 0.0;
    }
  }
  __syncthreads();
  const int64_t wi = s_win;
  const bool has_j = (j >= row0 && j < row0 + mloc);
  for (int64_t c = threadIdx.x; c < l; c += 256) {
    rec[LUS_HDR + c] = (wi >= 0) ? Y[(wi - row0) + c * ld] : 0.0;
    rec[LUS_HDR + l + c] = has_j ? Y[(j - row0) + c * ld] : 0.0;
  }
}

// every workgroup reduces the ranks' records in rank order (same result everywhere), then: the rank that holds row j
// receives the pivot row there, the rank that holds row r the old row j, rows below j take the rank-1 update of the leaf
__global__ __launch_bounds__(256) void lus_apply_kernel(double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0,
                                                        int64_t m, int64_t l, int64_t j0, int s, int w,
                                                        const double* __restrict__ recs, int nranks,
                                                        int32_t* __restrict__ ipiv, int32_t* __restrict__ info,
                                                        double* __restrict__ pval, int64_t* __restrict__ pidx) {
  // pval / pidx != null: this launch also leaves the per-workgroup arg-max partials of the NEXT leaf column (s + 1, over the
  // values it has just updated) where lus_cand_final_kernel expects them -- one launch less per pivot step
  __shared__ double s_v4[4];
  __shared__ int32_t s_i4[4];
  __shared__ double s_u[LW], s_old[LW];
  __shared__ int32_t s_r;
  __shared__ int s_gw, s_go;
  __shared__ double s_bestv;
  const int64_t j = j0 + s;
  const int64_t reclen = LUS_HDR + 2 * l;
  if (threadIdx.x == 0) {
    double best = -1.0;
    int32_t besti = -1;
    int gw = -1, go = -1;
    for (int g = 0; g < nranks; ++g) {
      const double v = recs[g * reclen + 0];
      const int32_t i = (int32_t)recs[g * reclen + 1];
      if (i >= 0 && (v > best || (v == best && (uint32_t)i < (uint32_t)besti))) { best = v; besti = i; gw = g; }
      if (recs[g * reclen + 2] != 0.0) go = g;
    }
    const bool valid = (besti >= j && besti < m && gw >= 0);
    s_r = valid ? besti : (int32_t)j;
    s_gw = valid ? gw : go;
    s_go = go;
    s_bestv = best;
  }
  __syncthreads();
  const int32_t r = s_r;
  const double* prow = recs + (int64_t)s_gw * reclen + ((s_gw == s_go && r == j) ? LUS_HDR + l : LUS_HDR);   // the pivot row
  const double* orow = recs + (int64_t)s_go * reclen + LUS_HDR + l;                                          // the old row j
  if (threadIdx.x < LW) {
    s_u[threadIdx.x] = (threadIdx.x < w) ? prow[j0 + threadIdx.x] : 0.0;
    s_old[threadIdx.x] = (threadIdx.x < w) ? orow[j0 + threadIdx.x] : 0.0;
  }
  __syncthreads();
  const double piv = s_u[s];
  const double rpiv = (piv != 0.0) ? 1.0 / piv : 0.0;
  const bool has_j = (j >= row0 && j < row0 + mloc), has_r = (r >= row0 && r < row0 + mloc);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {                      // every rank keeps the whole pivot sequence
      if (ipiv != nullptr) ipiv[j] = r;
      if (!(s_bestv > 0.0)) atomicCAS(info, 0, (int32_t)(j + 1));
    }
    if (r != j) {
      for (int64_t c = threadIdx.x; c < l; c += 256) {
        const bool leafcol = (c >= j0 && c < j0 + w);
        if (has_j) Y[(j - row0) + c * ld] = prow[c];                 // the pivot row moves up (all columns)
        if (has_r && !leafcol) Y[(r - row0) + c * ld] = orow[c];     // the old row j moves down (its leaf part below)
      }
    }
  }
  double nbest = -1.0;
  int32_t nbesti = -1;
  for (int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x; li < mloc; li += (int64_t)gridDim.x * 256) {
    const int64_t gi = row0 + li;
    if (gi <= j) continue;
    double* row = Y + li + j0 * ld;
    const bool moved = (gi == r);
    double x[LW];
#pragma unroll
    for (int k = 0; k < LW; ++k) x[k] = moved ? s_old[k] : ((k >= s && k < w) ? row[k * ld] : 0.0);
    const double x0 = x[s];
    const double lij = (rpiv != 0.0) ? x0 * rpiv : x0;
    x[s] = lij;
#pragma unroll
    for (int k = 0; k < LW; ++k)
      if (k > s) x[k] -= lij * s_u[k];
#pragma unroll
    for (int k = 0; k < LW; ++k)
      if (k < w && (k >= s || moved)) row[k * ld] = x[k];
    if (pval != nullptr) {                        // candidate of column s + 1: ascending rows per thread, the first maximum stays
      double nv = 0.0;
#pragma unroll
      for (int k = 0; k < LW; ++k)
        if (k == s + 1) nv = fabs(x[k]);
      if (nv > nbest) { nbest = nv; nbesti = (int32_t)gi; }
    }
  }
  if (pval != nullptr) {                          // the reduction of lus_cand_partial_kernel, same order
    wave_argmax(nbest, nbesti);
    if ((threadIdx.x & 63) == 0) { s_v4[threadIdx.x >> 6] = nbest; s_i4[threadIdx.x >> 6] = nbesti; }
    __syncthreads();
    if (threadIdx.x < 64) {
      double v = (threadIdx.x < 4) ? s_v4[threadIdx.x] : -1.0;
      int32_t i = (threadIdx.x < 4) ? s_i4[threadIdx.x] : -1;
      wave_argmax8(v, i);
      if (threadIdx.x == 0) { pval[blockIdx.x] = v; pidx[blockIdx.x] = i; }
    }
  }
}

// rows [jb, j0) of the leaf columns -> U12 = L11^-1 A12 (kp x 8, [c * 8 + v]); the rank that holds those rows
__global__ __launch_bounds__(512) void lus_u12_leaf_kernel(const double* __restrict__ Y, int64_t ld, int64_t jb_local,
                                                           int kp, int64_t j0, int w, double* __restrict__ U12) {
  __shared__ double Ls[KPMAX * LSP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < kp * kp; e += 512) {
    const int r = e % kp, c = e / kp;
    Ls[r * LSP + c] = Y[(jb_local + r) + (int64_t)(j0 - kp + c) * ld];     // rows local, columns global jb .. j0
  }
  __syncthreads();
  for (int v = wave; v < LW; v += 8) {
    double x = (lane < kp && v < w) ? Y[(jb_local + lane) + (int64_t)(j0 + v) * ld] : 0.0;
    for (int cp = 0; cp < kp; ++cp) {
      const double xc = readlane_d(x, __builtin_amdgcn_readfirstlane(cp));
      if (lane > cp && lane < kp) x -= Ls[lane * LSP + cp] * xc;
    }
    if (lane < kp) U12[lane * LW + v] = x;
  }
}
__global__ __launch_bounds__(256) void lus_pending_kernel(double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0,
                                                          int64_t jb, int64_t j0, int w, const double* __restrict__ U12) {
  __shared__ double Us[KPMAX * LW];
  const int kp = (int)(j0 - jb);
  for (int e = threadIdx.x; e < kp * LW; e += 256) Us[e] = U12[e];
  __syncthreads();
  for (int64_t li = (int64_t)blockIdx.x * 256 + threadIdx.x; li < mloc; li += (int64_t)gridDim.x * 256) {
    if (row0 + li < j0) continue;
    double a[LW];
#pragma unroll
    for (int k = 0; k < LW; ++k) a[k] = (k < w) ? Y[li + (j0 + k) * ld] : 0.0;
    for (int c = 0; c < kp; ++c) {
      const double lv = Y[li + (jb + c) * ld];
#pragma unroll
      for (int k = 0; k < LW; ++k) a[k] -= lv * Us[c * LW + k];
    }
#pragma unroll
    for (int k = 0; k < LW; ++k)
      if (k < w) Y[li + (j0 + k) * ld] = a[k];
  }
}
__global__ void lu_flag_export_kernel(const int32_t* __restrict__ info, double* __restrict__ flag) {
  flag[0] = (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) ? 1.0 : 0.0;
}
__global__ void lu_flag_import_kernel(int32_t* __restrict__ info, const double* __restrict__ flag) {
  if (flag[0] > 0.0 && __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) atomicExch(info, -1);
}
__global__ void lus_finish_kernel(double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l) {
  const int64_t total = l * l;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e % l, c = e / l;
    if (r < row0 || r >= row0 + mloc) continue;
    if (r == c) Y[(r - row0) + c * ld] = 1.0;
    else if (r < c) Y[(r - row0) + c * ld] = 0.0;
  }
}
}  // namespace

int lus_grid(int64_t mloc) {
  int64_t g = (mloc + 255) / 256;
  if (g < 1) g = 1;
  if (g > 1024) g = 1024;
  return (int)g;
}
void lus_candidate(hipStream_t st, const double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j, double* rec,
                   double* pval, int64_t* pidx, bool partials_ready) {
  const int g = lus_grid(mloc);
  if (!partials_ready) hipLaunchKernelGGL(lus_cand_partial_kernel, dim3(g), dim3(256), 0, st, Y, ld, mloc, row0, j, pval, pidx);
  hipLaunchKernelGGL(lus_cand_final_kernel, dim3(1), dim3(256), 0, st, Y, ld, mloc, row0, l, j, g, pval, pidx, rec);
}
// next_pval / next_pidx (may be null): leave the partials of leaf column s + 1 for the next lus_candidate
void lus_apply(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l, int64_t j0, int s, int w,
               const double* recs, int nranks, int32_t* ipiv, int32_t* info, double* next_pval, int64_t* next_pidx) {
  hipLaunchKernelGGL(lus_apply_kernel, dim3(lus_grid(mloc)), dim3(256), 0, st, Y, ld, mloc, row0, m, l, j0, s, w, recs, nranks,
                     ipiv, info, next_pval, next_pidx);
}
void lus_u12_leaf(hipStream_t st, const double* Y, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12) {
  hipLaunchKernelGGL(lus_u12_leaf_kernel, dim3(1), dim3(512), 0, st, Y, ld, jb - row0, (int)(j0 - jb), j0, w, U12);
}
void lus_pending(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t jb, int64_t j0, int w,
                 const double* U12) {
  hipLaunchKernelGGL(lus_pending_kernel, dim3(lus_grid(mloc)), dim3(256), 0, st, Y, ld, mloc, row0, jb, j0, w, U12);
}
void lu_flag_export(hipStream_t st, const int32_t* info, double* flag) {
  hipLaunchKernelGGL(lu_flag_export_kernel, dim3(1), dim3(1), 0, st, info, flag);
}
void lu_flag_import(hipStream_t st, int32_t* info, const double* flag) {
  hipLaunchKernelGGL(lu_flag_import_kernel, dim3(1), dim3(1), 0, st, info, flag);
}
void lus_finish(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l) {
  int eb = (int)((l * l + 255) / 256);
  if (eb > 1024) eb = 1024;
  hipLaunchKernelGGL(lus_finish_kernel, dim3(eb), dim3(256), 0, st, Y, ld, mloc, row0, l);
}

// ---- the row interchanges of one leaf's pivots on the columns OUTSIDE the leaf, across ranks (LAPACK swaps whole rows; the
//      leaf kernel moved the leaf's own 8 columns in registers).  The <= 16 rows involved -- j0 .. j0 + w - 1 and the pivot
//      rows r_s -- are collected into a table (every rank contributes the rows it owns, zeros elsewhere; the host
//      all-reduces it), the w swaps are replayed on the table, every rank writes back the rows it owns.
//      Slot t < w: row j0 + t; slot w + s: pivot row r_s unless that row already has a slot (then the slot stays zero).
__device__ inline int lus_swap_slot(const int32_t* piv, int w, int32_t j0, int32_t row) {     // canonical slot of a row
  if (row >= j0 && row < j0 + w) return row - j0;
  for (int s2 = 0; s2 < w; ++s2)
    if (piv[s2] == row) return w + s2;
  return -1;
}
// slot of a row in the peer kernel's layout: t < LW: row j0 + t; LW + s: pivot r_s (first occurrence)
__device__ inline int lus_swap_slot_lw(const int32_t* piv, int w, int32_t j0, int32_t row) {
  if (row >= j0 && row < j0 + w) return row - j0;
  for (int s2 = 0; s2 < w; ++s2)
    if (piv[s2] == row) return LW + s2;
  return -1;
}
__global__ __launch_bounds__(256) void lus_swap_pack_kernel(const double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0,
                                                            int64_t l, int32_t j0, int w, const int32_t* __restrict__ ipiv,
                                                            double* __restrict__ table) {
  __shared__ int32_t piv[LW];
  if (threadIdx.x < LW) piv[threadIdx.x] = (threadIdx.x < (unsigned)w) ? ipiv[j0 + threadIdx.x] : -1;
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)2 * LW * l; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e / l);
    const int64_t c = e % l;
    double v = 0.0;
    if (t < 2 * w) {
      const int32_t row = (t < w) ? j0 + t : piv[t - w];
      const bool canonical = (t < w) || (lus_swap_slot(piv, w, j0, row) == t);
      if (canonical && row >= row0 && row < row0 + mloc && !(c >= j0 && c < j0 + w)) v = Y[(row - row0) + c * ld];
    }
    table[e] = v;
  }
}
__global__ __launch_bounds__(256) void lus_swap_apply_kernel(double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0,
                                                             int64_t l, int32_t j0, int w, const int32_t* __restrict__ ipiv,
                                                             const double* __restrict__ table) {
  __shared__ int32_t piv[LW];
  if (threadIdx.x < LW) piv[threadIdx.x] = (threadIdx.x < (unsigned)w) ? ipiv[j0 + threadIdx.x] : -1;
  __syncthreads();
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < l; c += (int64_t)gridDim.x * 256) {
    if (c >= j0 && c < j0 + w) continue;
    double v[2 * LW];
#pragma unroll
    for (int t = 0; t < 2 * LW; ++t) v[t] = table[(int64_t)t * l + c];
    for (int s2 = 0; s2 < w; ++s2) {                       // LAPACK's order: swap rows j0 + s and r_s
      const int b = lus_swap_slot(piv, w, j0, piv[s2]);
      if (b >= 0 && b != s2) {
        double va = 0.0, vb = 0.0;
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t) { if (t == s2) va = v[t]; if (t == b) vb = v[t]; }
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t) { if (t == s2) v[t] = vb; if (t == b) v[t] = va; }
      }
    }
#pragma unroll
    for (int t = 0; t < 2 * LW; ++t) {
      if (t < 2 * w) {
        const int32_t row = (t < w) ? j0 + t : piv[t - w];
        const bool canonical = (t < w) || (lus_swap_slot(piv, w, j0, row) == t);
        if (canonical && row >= row0 && row < row0 + mloc) Y[(row - row0) + c * ld] = v[t];
      }
    }
  }
}
// The same interchange WITHOUT a host-sequenced collective: every rank pushes the rows it owns into every other rank's table
// box (granule pairs tagged with the leaf's first epoch, system-scope stores into peer-mapped memory), polls its own box for
// the rows the others own, replays the swaps and writes back its rows.  One launch per leaf and rank, thread = one column.
// A rank that owns none of the <= 16 rows has nothing to write and leaves at once.
__global__ __launch_bounds__(256) void lus_swap_peer_kernel(double* __restrict__ Y, int64_t ld, int64_t mloc, int64_t row0,
                                                            int64_t l, int32_t j0, int w, const int32_t* __restrict__ ipiv,
                                                            LuMrArgs mr, unsigned long long* __restrict__ own, size_t box_off,
                                                            uint32_t tag, int64_t pad, int poll_limit,
                                                            int32_t* __restrict__ info) {
  __shared__ int32_t piv[LW];
  __shared__ int s_any;
  if (threadIdx.x == 0) s_any = 0;
  if (threadIdx.x < LW) piv[threadIdx.x] = (threadIdx.x < (unsigned)w) ? ipiv[j0 + threadIdx.x] : -1;
  __syncthreads();
  if (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;   // a timed-out factorization drains
  // canonical slots and their owners (the same on every rank)
  int32_t srow[2 * LW];
  bool scan[2 * LW], smine[2 * LW];
  bool any_mine = false;
#pragma unroll
  for (int t = 0; t < 2 * LW; ++t) {
    const int32_t row = (t < w) ? j0 + t : ((t >= LW && t - LW < w) ? piv[t - LW] : -1);
    srow[t] = row;
    bool canonical = row >= 0;
    if (canonical && t >= LW) {
      if (row >= j0 && row < j0 + w) canonical = false;
      for (int s2 = 0; s2 < t - LW; ++s2) if (piv[s2] == row) canonical = false;
    }
    scan[t] = canonical;
    smine[t] = canonical && row >= row0 && row < row0 + mloc;
    any_mine = any_mine || smine[t];
  }
  if (!any_mine) return;
  const size_t lq = (size_t)l;
  bool timed_out = false;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < l; c += (int64_t)gridDim.x * 256) {
    if (c >= j0 && c < j0 + w) continue;
    double v[2 * LW];
#pragma unroll
    for (int t = 0; t < 2 * LW; ++t) {           // my rows: read, push to everyone else
      v[t] = 0.0;
      if (smine[t]) {
        v[t] = Y[(srow[t] - row0) + c * ld];
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v[t]);
        const size_t off = box_off + ((size_t)t * lq + (size_t)c) * 2;
        for (int q = 0; q < mr.nranks; ++q) {
          if (q == mr.rank) continue;
          __hip_atomic_store(mr.peer[q] + off, ((unsigned long long)tag << 32) | (uint32_t)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(mr.peer[q] + off + 1, ((unsigned long long)tag << 32) | (uint32_t)(bits >> 32), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
    {                                            // the others' rows: poll my own box, all slots of a round in flight together
      unsigned long long lo[2 * LW], hi[2 * LW];
      int tries = timed_out ? poll_limit : 0;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t) {
          if (scan[t] && !smine[t]) {
            const size_t off = box_off + ((size_t)t * lq + (size_t)c) * 2;
            lo[t] = poll_granule<true>(own + off);
            hi[t] = poll_granule<true>(own + off + 1);
          }
        }
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t)
          if (scan[t] && !smine[t]) ok = ok && ((uint32_t)(lo[t] >> 32) == tag && (uint32_t)(hi[t] >> 32) == tag);
        if (ok) break;
        if (++tries > poll_limit) { timed_out = true; lu_timeout_note(info, 6, (int)c, tag, mr.rank * 1024 + (int)blockIdx.x); break; }
        __builtin_amdgcn_s_sleep(1);
      }
#pragma unroll
      for (int t = 0; t < 2 * LW; ++t)
        if (scan[t] && !smine[t])
          v[t] = __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi[t] << 32) | (uint32_t)lo[t]));
    }
    for (int s2 = 0; s2 < w; ++s2) {             // LAPACK's order: swap rows j0 + s and r_s
      const int b = lus_swap_slot_lw(piv, w, j0, piv[s2]);
      if (b >= 0 && b != s2) {
        double va = 0.0, vb = 0.0;
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t) { if (t == s2) va = v[t]; if (t == b) vb = v[t]; }
#pragma unroll
        for (int t = 0; t < 2 * LW; ++t) { if (t == s2) v[t] = vb; if (t == b) v[t] = va; }
      }
    }
#pragma unroll
    for (int t = 0; t < 2 * LW; ++t)
      if (smine[t]) Y[(srow[t] - row0) + c * ld] = v[t];
  }
  if (timed_out) atomicExch(info, -1);
}
void lus_swap_peer(hipStream_t st, const Lu2MrWork& w, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l,
                   int64_t j0, int wd, uint32_t epoch_base) {
  LuMrArgs a{};
  a.rank = w.rank; a.nranks = w.nranks; a.gbase = (int32_t)row0; a.mtot = (int32_t)m; a.us = nullptr;
  for (int q = 0; q < w.nranks; ++q) a.peer[q] = w.peer[q];
  const int64_t pad = (m + w.nranks - 1) / w.nranks;
  const size_t G = w.hier ? (size_t)w.grid + (size_t)w.nranks : (size_t)w.nranks * (size_t)w.grid;
  const size_t box = (size_t)2 * G * REC + (size_t)2 * (2 * KPMAX * LW) + (size_t)((epoch_base >> 3) & 1u) * ((size_t)2 * LW * 2 * LU2_MR_MAXL);
  const int poll_limit = w.poll_limit > 0 ? w.poll_limit : POLL_LIMIT;
  const int g = (int)std::min<int64_t>((l + 255) / 256, 64);
  hipLaunchKernelGGL(lus_swap_peer_kernel, dim3(g), dim3(256), 0, st, Y, ld, mloc, row0, l, (int32_t)j0, wd, w.ipiv, a, w.peer[w.rank], box,
                     epoch_base + 1u, pad, poll_limit, w.info);
}

void lus_swap_pack(hipStream_t st, const double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j0, int w,
                   const int32_t* ipiv, double* table) {
  const int g = (int)std::min<int64_t>((2 * LW * l + 255) / 256, 256);
  hipLaunchKernelGGL(lus_swap_pack_kernel, dim3(g), dim3(256), 0, st, Y, ld, mloc, row0, l, (int32_t)j0, w, ipiv, table);
}
void lus_swap_apply(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t l, int64_t j0, int w,
                    const int32_t* ipiv, const double* table) {
  const int g = (int)std::min<int64_t>((l + 255) / 256, 64);
  hipLaunchKernelGGL(lus_swap_apply_kernel, dim3(g), dim3(256), 0, st, Y, ld, mloc, row0, l, (int32_t)j0, w, ipiv, table);
}

}}  // namespace gsi::hipk
