// panel_lu_blocks.hip -- what happens BETWEEN the blocks (16 .. 64 columns each: lu_schedule.hpp) of `F = lu(Y); Q = F.L`,
// whichever form factors the leaves inside them (panel_lu_dev.hpp lists the forms).  Every instantiation of these kernels is
// compiled here and nowhere else.
//   * lu_leftlook_kernel + lu_urows_kernel: the LEFT-looking update of the single-rank forms (described further down).
//   * lu_u12_kernel + lu_rankk_kernel: the right-looking update (every trailing column re-read and rewritten after every
//     block), kept for the row-sharded form, the bit-identity reference, which reaches it through lus_u12_block / lus_rankk.
//   * lu_blocks: the loop over the blocks of a schedule that the resident (lu2_L) and the streamed (lu3_L) form run their
//     leaves in; lu2_extract_L_kernel ends it.
#include "panel_lu_dev.hpp"
#include <type_traits>

namespace gsi { namespace hipk {

// U12 = L11^-1 A12 for the K x K unit-lower block at (jb, jb) and the columns [c0, c1): out[k + (c - c0) ldo].
// Thread = one column; L11 in LDS (broadcast reads), the column in registers.
// (256 threads bring L11 in -- K^2 / 256 loads each instead of K^2 / 64: the kernel sits between two blocks of the
// factorization and is all latency -- then the first wave solves its 64 columns.)
// (256 threads) L11 into LDS as [row][col]: a row's multipliers are contiguous
template <int K>
__device__ inline void u12_stage_L11(double* L11, const double* __restrict__ Y, int64_t ld, int64_t jb, int64_t jbrow) {
#pragma unroll 8
  for (int e = threadIdx.x; e < K * K; e += 256) {
    const int r = e % K, c = e / K;
    L11[r * K + c] = Y[(jbrow + r) + (jb + c) * ld];
  }
}
// x <- L11^-1 x: the one scalar order (and fma contraction) every U12 of a factorization is solved in
template <int K>
__device__ inline void u12_solve(const double* L11, double (&x)[K]) {
#pragma unroll
  for (int r = 1; r < K; ++r) {
    double v = x[r];
#pragma unroll
    for (int p = 0; p < r; ++p) v -= L11[r * K + p] * x[p];
    x[r] = v;
  }
}

template <int K>
__global__ __launch_bounds__(256) void lu_u12_kernel(const double* __restrict__ Y, int64_t ld, int64_t jb, int64_t jbrow,
                                                     int64_t c0, int64_t c1, double* __restrict__ out, int64_t ldo) {
  // jb: the block's first COLUMN (global); jbrow: the row of Y that holds global row jb (jb - row0 for a row shard)
  __shared__ double L11[K * K];
  u12_stage_L11<K>(L11, Y, ld, jb, jbrow);
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int64_t c = c0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= c1) return;
  double x[K];
  const double* col = Y + jbrow + c * ld;
#pragma unroll
  for (int r = 0; r < K; ++r) x[r] = col[r];
  u12_solve<K>(L11, x);
  double* o = out + (c - c0) * ldo;
#pragma unroll
  for (int r = 0; r < K; ++r) o[r] = x[r];
}

// A22 -= L21 * U12: rows [r_begin, m), columns [c0, c0 + t), L21 = Y[:, jb:jb+K], U12 (K x t, ld K) from lu_u12_kernel.
// Workgroup = 4 waves x 32 rows; column chunk of <= RK_CHUNK columns per blockIdx.y (its U12 slice sits in LDS).
// MFMA operands swapped like the big contraction kernel: lane (jl = lane & 15, kk = lane >> 4) holds, for C row
// jl (+16 h), the columns kk + 4 reg of a 16-column tile.
template <int K, int DEPTH, int RK_CHUNK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RK_CHUNK == 64 ? 3 : 2, RK_CHUNK == 64 ? 3 : 4))) void lu_rankk_kernel(double* __restrict__ Y, int64_t ld, int64_t m, int64_t r_begin,
                                                       int64_t jb, int64_t c0, int64_t t,
                                                       const double* __restrict__ U12) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  constexpr int KP = K + 2;                     // padded k stride of the U image [col][k] (KP / 2 odd: conflict-free b64 reads)
  extern __shared__ double us[];                // RK_CHUNK * KP doubles
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jl = lane & 15, kk = lane >> 4;
  const int64_t rb = r_begin + ((int64_t)blockIdx.x * 4 + wave) * 32;
  // this wave's 32 rows of multipliers as MFMA fragments: fa[h][s] = L[rb + 16 h + jl, jb + 4 s + kk]
  double fa[2][K / 4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t rrow = rb + 16 * h + jl;
#pragma unroll
    for (int s = 0; s < K / 4; ++s) fa[h][s] = (rrow < m) ? Y[rrow + (jb + 4 * s + kk) * ld] : 0.0;
  }
  for (int64_t cc0 = 0; cc0 < t; cc0 += RK_CHUNK) {   // the workgroup walks ALL trailing columns: L21 is read once
    const int tc = (int)((t - cc0 < RK_CHUNK) ? (t - cc0) : RK_CHUNK);
    __syncthreads();                                  // the previous chunk's U image is no longer read
    for (int e = tid; e < RK_CHUNK * K; e += 256) {
      const int k = e % K, c = e / K;
      us[c * KP + k] = (c < tc) ? U12[k + (cc0 + c) * K] : 0.0;
    }
    __syncthreads();
    if (rb >= m) continue;
    const int ntile = (tc + 15) / 16;
    double cin[2][4];
    auto load_tile = [&](int tt, double (&dst)[2][4]) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t rrow = rb + 16 * h + jl;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int cl = 16 * tt + kk + 4 * reg;
          dst[h][reg] = (rrow < m && cl < tc) ? Y[rrow + (c0 + cc0 + cl) * ld] : 0.0;
        }
      }
    };
    load_tile(0, cin);
    double cin2[2][4];                                // DEPTH == 2: two tiles of C in flight
    if (DEPTH == 2 && ntile > 1) load_tile(1, cin2);
    for (int tt = 0; tt < ntile; ++tt) {
      double4_t acc[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) acc[h] = (double4_t){cin[h][0], cin[h][1], cin[h][2], cin[h][3]};
      if (DEPTH == 2) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) cin[h][reg] = cin2[h][reg];
        if (tt + 2 < ntile) load_tile(tt + 2, cin2);
      } else if (tt + 1 < ntile) load_tile(tt + 1, cin);     // next tile's C in flight behind this tile's MFMAs
#pragma unroll
      for (int s = 0; s < K / 4; ++s) {
        const double fb = -us[(16 * tt + jl) * KP + 4 * s + kk];
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb, fa[h][s], acc[h], 0, 0, 0);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t rrow = rb + 16 * h + jl;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int cl = 16 * tt + kk + 4 * reg;
          if (rrow < m && cl < tc) Y[rrow + (c0 + cc0 + cl) * ld] = acc[h][reg];
        }
      }
    }
  }
}

template <int K, int DEPTH, int CHUNK>
static void launch_rankk_v(hipStream_t st, unsigned grid, double* Y, int64_t ld, int64_t m, int64_t r_begin, int64_t jb,
                           int64_t c0, int64_t t, const double* U12) {
  constexpr size_t shmem = (size_t)CHUNK * (K + 2) * sizeof(double);
  static std::atomic<uint64_t> attr_mask{0};
  if (first_use_on_this_device(attr_mask))
    (void)hipFuncSetAttribute((const void*)lu_rankk_kernel<K, DEPTH, CHUNK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
  hipLaunchKernelGGL((lu_rankk_kernel<K, DEPTH, CHUNK>), dim3(grid), dim3(256), shmem, st, Y, ld, m, r_begin, jb, c0, t, U12);
}
// U12 columns staged per pass (its LDS image bounds the workgroups per CU: 128 columns = 67 KB = 2 workgroups, 64 = 4) and C
// tiles in flight per wave: A/B knobs GSI_LU_RK_CHUNK (64 | 128), GSI_LU_RK_DEPTH (1 | 2).
// Round 5: THREE waves per SIMD.  The kernel is a latency chain per wave (C tile in, 2 K / 4 MFMAs, C tile out) at 44 % of the
// matrix pipe and 0.54 of the HBM peak; with 164 VGPRs + 16 AGPRs it ran two waves per SIMD whatever the chunk.  Told to fit
// three (amdgpu_waves_per_eu on the 64-column instantiations: 160 VGPRs, no AGPR copies, no spills) and with 64-column chunks
// (34 KB of LDS: three workgroups per CU) the four updates of a factorization take 2.4 instead of 2.8 ms: LU 29.4 -> 27.7 - 28.4 ms
// per step in alternating runs (profiles/r05_lu_rankk_occupancy.log).  Four waves (128 VGPRs) spill 46 registers: 32.6.  The
// same 64-column chunks at two waves per SIMD were "noise" in round 3 (tools/ab_rankk.sh): it was the occupancy, not the chunk.
template <int K>
static void launch_rankk(hipStream_t st, unsigned grid, double* Y, int64_t ld, int64_t m, int64_t r_begin, int64_t jb,
                         int64_t c0, int64_t t, const double* U12) {
  static const int depth = getenv("GSI_LU_RK_DEPTH") ? atoi(getenv("GSI_LU_RK_DEPTH")) : 1;
  static const int chunk = getenv("GSI_LU_RK_CHUNK") ? atoi(getenv("GSI_LU_RK_CHUNK")) : 64;
  if (chunk == 64 && depth == 2) launch_rankk_v<K, 2, 64>(st, grid, Y, ld, m, r_begin, jb, c0, t, U12);
  else if (chunk == 64) launch_rankk_v<K, 1, 64>(st, grid, Y, ld, m, r_begin, jb, c0, t, U12);
  else if (depth == 2) launch_rankk_v<K, 2, 128>(st, grid, Y, ld, m, r_begin, jb, c0, t, U12);
  else launch_rankk_v<K, 1, 128>(st, grid, Y, ld, m, r_begin, jb, c0, t, U12);
}

// ---- left-looking order between blocks (the single-rank factorizations; the row-sharded form stays right-looking) ----------
// Block i's columns are left alone until block i is next; then ONE pass brings rows [jb, m) of them up to date with every
// finished block to their left, and after its leaves the U rows of block i (rows [jb, jb + NB) of all trailing columns) are
// brought up to date the same way and solved.  The solved U rows of every block are kept as the strict block upper triangle of
// an l x l matrix, U(p, c) = U[p + c ldu], ldu = l: nothing in it depends on where the block boundaries are.
// The blocks need not be equally wide (lu_schedule.hpp chooses the widths): the kernels walk the finished columns 0 .. jb in
// 16-column tiles, whatever blocks they were factored in, and are instantiated for the width of the block they update.
// Every element sees the MFMAs of lu_rankk_kernel -- operands -U12 (A) and L (B) in its lane mapping, k in groups of four,
// in ascending order -- on an accumulator that stays in registers instead of crossing HBM between the blocks (an fp64
// store + reload is exact), and the U rows are solved by lu_u12_kernel's own u12_solve: the factors are bit for bit the
// right-looking ones (the row-sharded form is the reference), and the same bits for every schedule: an element's k terms come
// in the same order wherever a block ends.  Passes over the panel for the update before a b-column block at jb: jb (L) + 2 b (C).
constexpr int LL_WAVES = 12;                                   // 12 waves x 16 rows: three waves per SIMD, one workgroup per CU
constexpr int LL_BS = 64 * LL_WAVES;
constexpr int LL_UNIT = 64;                                    // finished columns per -U image and per L fragment set
constexpr int LL_KP = LL_UNIT + 2;                             // padded k stride of an image (LL_KP / 2 odd, as in lu_rankk_kernel)
constexpr int LL_GROUP = 4;                                    // images per launch: 256 finished columns
constexpr size_t LL_LDS = (size_t)LL_GROUP * 64 * LL_KP * sizeof(double);   // -U images of up to 256 finished columns (132 KB)

// a uniform pointer the compiler may not re-derive from its start: one 64-bit SGPR pair walks the columns instead of one
// hoisted base per column (32 of them ran the kernel out of SGPRs and into spills)
__device__ __forceinline__ char* ll_advance(char* p, int64_t step) {
  p += step;
  asm volatile("" : "+s"(p));
  return p;
}

// A[jb:m, jb:jb+tc] -= L[jb:m, p0:p1] U(p0:p1, jb:jb+tc): the tc <= NB columns of the block at jb against the finished columns
// [p0, p1) (p0 a multiple of 64, p1 - p0 a multiple of 16 and <= 256; more finished columns: one launch per 256, ascending).
// Persistent: the workgroup stages the -U images once -- one per 64 finished columns, LDS [(u NB + c) KP + k]; the last may
// hold 16, 32 or 48 -- then every wave walks 16-row chunks on its own, no barrier: C tile (16 rows x NB columns) in registers
// for the whole chunk, the L fragments of the next 64 columns in flight behind the NB / 16 x 16 MFMAs of these 64 (64 cycles
// each: one LDS read per MFMA is far below the LDS rate).  Addressing: a 32-bit per-lane offset (row, and kk columns over) set
// once per chunk + one walking uniform column pointer -- no vector address arithmetic between the MFMAs.
// WIDE: panels whose 3 ld * 8 bytes do not fit that offset (ld > 1.7e8 rows) take 64-bit per-lane offsets.
template <int NB, bool WIDE>
__global__ __launch_bounds__(LL_BS) void lu_leftlook_kernel(double* __restrict__ Y, int64_t ld, int64_t m, int64_t jb, int tc,
                                                            int p0, int p1, const double* __restrict__ U, int64_t ldu) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type off_t;
  constexpr int KP = LL_KP, NT = NB / 16, NS = LL_UNIT / 4;
  typedef std::integral_constant<int, NS> whole_t;
  extern __shared__ double us[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jl = lane & 15, kk = lane >> 4;
  const int np = p1 - p0, nfull = np / LL_UNIT, rem = np % LL_UNIT;
  for (int c = wave; c < NB; c += LL_WAVES) {         // a wave per block column, the lanes along k
    const double* ucol = U + p0 + (jb + c) * ldu;
    for (int k = lane; k < np; k += 64) us[((k / LL_UNIT) * NB + c) * KP + k % LL_UNIT] = (c < tc) ? -ucol[k] : 0.0;
  }
  __syncthreads();
  const int lb = jl * KP + kk;                      // this lane's fb: -U(64 u + 4 s + kk, 16 tt + jl)
  const int64_t nch = (m - jb + 15) / 16;
  const int64_t cs = ld * (int64_t)sizeof(double);  // bytes per column
  for (int64_t ch = (int64_t)blockIdx.x * LL_WAVES + wave; ch < nch; ch += (int64_t)gridDim.x * LL_WAVES) {
    const int64_t rb = jb + ch * 16;
    // lane (jl, kk): row rb + jl (rows beyond m read row m - 1 and are never stored), column kk further on
    const int64_t r = (rb + jl < m) ? rb + jl : m - 1;
    const off_t vo = (off_t)((r - rb) * (int64_t)sizeof(double) + kk * cs);
    auto at = [&](char* colp) -> double* { return reinterpret_cast<double*>(colp + vo); };
    char* const cbase = reinterpret_cast<char*>(Y + rb + jb * ld);
    double4_t acc[NT];                              // C column jb + 16 tt + 4 reg + kk
    {
      char* p = cbase;
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          acc[tt][reg] = (16 * tt + 4 * reg + kk < tc) ? *at(p) : 0.0;
          p = ll_advance(p, 4 * cs);
        }
    }
    double fa[NS], fn[NS];
    char* pf = reinterpret_cast<char*>(Y + rb + (int64_t)p0 * ld);   // walks the L columns p0 .. p1
    auto load_frag = [&](auto n, double (&f)[NS]) {  // the next 4 n columns
#pragma unroll
      for (int s = 0; s < decltype(n)::value; ++s) {
        f[s] = *at(pf);
        pf = ll_advance(pf, 4 * cs);
      }
    };
    auto run = [&](auto n, const double (&f)[NS], int u) {
      const double* ub = us + u * NB * KP + lb;
#pragma unroll
      for (int s = 0; s < decltype(n)::value; ++s)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
          acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ub[16 * tt * KP + 4 * s], f[s], acc[tt], 0, 0, 0);
    };
    // the 16, 32 or 48 columns behind the last whole 64 (rem is uniform: scalar branches)
    auto load_rest = [&](double (&f)[NS]) {
      if (rem == 16) load_frag(std::integral_constant<int, 4>{}, f);
      else if (rem == 32) load_frag(std::integral_constant<int, 8>{}, f);
      else if (rem == 48) load_frag(std::integral_constant<int, 12>{}, f);
    };
    auto run_rest = [&](const double (&f)[NS]) {
      if (rem == 16) run(std::integral_constant<int, 4>{}, f, nfull);
      else if (rem == 32) run(std::integral_constant<int, 8>{}, f, nfull);
      else if (rem == 48) run(std::integral_constant<int, 12>{}, f, nfull);
    };
    if (nfull > 0) {
      load_frag(whole_t{}, fa);
      int u = 0;
      for (; u + 1 < nfull; ++u) {                    // (the last whole 64 peeled: the prefetch is unconditional in the loop)
        load_frag(whole_t{}, fn);
        run(whole_t{}, fa, u);
#pragma unroll
        for (int s = 0; s < NS; ++s) fa[s] = fn[s];
      }
      load_rest(fn);
      run(whole_t{}, fa, u);
      run_rest(fn);
    } else {
      load_rest(fa);
      run_rest(fa);
    }
    const bool live = rb + jl < m;
    char* p = cbase;
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (live && 16 * tt + 4 * reg + kk < tc) *at(p) = acc[tt][reg];
        p = ll_advance(p, 4 * cs);
      }
  }
}

// The U rows of the K-column block at jb: rows [jb, jb + K) of the trailing columns [c0, c1) brought up to date with the
// finished columns 0 .. jb (the sequence above, -U read from L2: a few MB per factorization), then solved by u12_solve as in
// lu_u12_kernel and written into U: U[(jb + k) + c ldu].  Workgroup = 64 columns; waves 0 .. K / 16 - 1 hold 16 rows x 64
// columns each.
template <int K>
__global__ __launch_bounds__(256) void lu_urows_kernel(const double* __restrict__ Y, int64_t ld, int64_t jb, int64_t c0,
                                                       int64_t c1, double* U, int64_t ldu) {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  constexpr int TP = K + 1;                    // [col][row] image of the updated rows, padded
  __shared__ double L11[K * K];
  __shared__ double T[64 * TP];
  u12_stage_L11<K>(L11, Y, ld, jb, jb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jl = lane & 15, kk = lane >> 4;
  const int64_t cb = c0 + (int64_t)blockIdx.x * 64;
  if (wave < K / 16) {
    const int64_t row = jb + 16 * wave + jl;
    double4_t acc[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t c = cb + 16 * tt + kk + 4 * reg;
        acc[tt][reg] = (c < c1) ? Y[row + c * ld] : 0.0;
      }
    for (int64_t p = 0; p < jb; p += 16) {       // (jb is a multiple of 16: only a last block is ragged)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t k = p + 4 * s + kk;
        const double fa = Y[row + k * ld];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const int64_t c = cb + 16 * tt + jl;
          const double fb = (c < c1) ? -U[k + c * ldu] : 0.0;
          acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb, fa, acc[tt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) T[(16 * tt + kk + 4 * reg) * TP + 16 * wave + jl] = acc[tt][reg];
  }
  __syncthreads();
  if (tid >= 64) return;
  const int64_t c = cb + tid;
  if (c >= c1) return;
  double x[K];
#pragma unroll
  for (int r = 0; r < K; ++r) x[r] = T[tid * TP + r];
  u12_solve<K>(L11, x);
  double* o = U + jb + c * ldu;
#pragma unroll
  for (int r = 0; r < K; ++r) o[r] = x[r];
}

// f(std::integral_constant<int, W>) for the kernel width W = 16, 32, 48 or 64 that holds w columns
template <class F>
static void lu_for_width(int w, F&& f) {
  if (w <= 16) f(std::integral_constant<int, 16>{});
  else if (w <= 32) f(std::integral_constant<int, 32>{});
  else if (w <= 48) f(std::integral_constant<int, 48>{});
  else f(std::integral_constant<int, 64>{});
}

template <int NB, bool WIDE>
static void launch_leftlook_v(hipStream_t st, unsigned grid, double* Y, int64_t ld, int64_t m, int64_t jb, int tc,
                              const double* U, int64_t ldu) {
  static std::atomic<uint64_t> attr_mask{0};
  if (first_use_on_this_device(attr_mask))
    (void)hipFuncSetAttribute((const void*)lu_leftlook_kernel<NB, WIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LL_LDS);
  for (int64_t p0 = 0; p0 < jb; p0 += LL_GROUP * LL_UNIT) {     // (more than 256 finished columns: one launch per 256)
    const int64_t p1 = std::min<int64_t>(jb, p0 + LL_GROUP * LL_UNIT);
    const size_t shmem = (size_t)((p1 - p0 + LL_UNIT - 1) / LL_UNIT) * NB * LL_KP * sizeof(double);
    hipLaunchKernelGGL((lu_leftlook_kernel<NB, WIDE>), dim3(grid), dim3(LL_BS), shmem, st, Y, ld, m, jb, tc, (int)p0, (int)p1, U, ldu);
  }
}
// Step 1 of block [jb, jb + b) (jb > 0, a multiple of 16): its columns, rows [jb, m), brought up to date with every column to
// their left.
static void lu_ll_update(hipStream_t st, double* Y, int64_t ld, int64_t m, int64_t l, int64_t jb, int b, const double* u12) {
  if (jb == 0 || m <= jb) return;
  int dev = 0, ncu = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) ncu = 256;
  const int64_t chunks = (m - jb + 15) / 16;
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + LL_WAVES - 1) / LL_WAVES, ncu);   // one workgroup per CU
  const bool wide = (3 * ld + 32) * (int64_t)sizeof(double) >= ((int64_t)1 << 32);
  lu_for_width(b, [&](auto w) {
    constexpr int NB = decltype(w)::value;
    if (wide) launch_leftlook_v<NB, true>(st, grid, Y, ld, m, jb, b, u12, l);
    else launch_leftlook_v<NB, false>(st, grid, Y, ld, m, jb, b, u12, l);
  });
}
// Step 3 of the block [jb, jb + b) (after its leaves): its U rows for every trailing column [jb + b, l).  Only a block of 16,
// 32, 48 or 64 columns has columns to its right.
static void lu_ll_urows(hipStream_t st, const double* Y, int64_t ld, int64_t l, int64_t jb, int b, double* u12) {
  const int64_t c0 = jb + b;
  if (c0 >= l) return;
  const unsigned gu = (unsigned)((l - c0 + 63) / 64);
  lu_for_width(b, [&](auto w) {
    constexpr int K = decltype(w)::value;
    if (jb == 0) hipLaunchKernelGGL(lu_u12_kernel<K>, dim3(gu), dim3(256), 0, st, Y, ld, jb, jb, c0, l, u12 + c0 * l, l);
    else hipLaunchKernelGGL(lu_urows_kernel<K>, dim3(gu), dim3(256), 0, st, Y, ld, jb, c0, l, u12, l);
  });
}

// top l x l: unit diagonal, zero strict upper triangle (what Julia's F.L returns)
__global__ void lu2_extract_L_kernel(double* __restrict__ Y, int64_t ld, int64_t l) {
  const int64_t total = l * l;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e % l, c = e / l;
    if (r == c) Y[r + c * ld] = 1.0;
    else if (r < c) Y[r + c * ld] = 0.0;
  }
}

void lu_blocks(hipStream_t st, double* Y, int64_t ld, int64_t m, int64_t l, const std::vector<int>& widths, double* u12,
               const LuLeafFn& leaf) {
  if (!lu_schedule_valid(l, widths)) throw std::runtime_error("lu_blocks: the block widths do not fit the panel");
  int64_t jb = 0;
  for (const int b : widths) {
    lu_ll_update(st, Y, ld, m, l, jb, b, u12);             // left-looking: this block's columns, once, before its leaves
    for (int64_t j0 = jb; j0 < jb + b; j0 += LW) leaf(jb, b, j0, (int)((jb + b - j0 < LW) ? (jb + b - j0) : LW));
    lu_ll_urows(st, Y, ld, l, jb, b, u12);                 // (the last block has no columns to its right)
    jb += b;
  }
  int eb = (int)((l * l + 255) / 256);
  if (eb > 1024) eb = 1024;
  hipLaunchKernelGGL(lu2_extract_L_kernel, dim3(eb), dim3(256), 0, st, Y, ld, l);
}

// the row-sharded form's block update: right-looking, on this rank's rows [row0, row0 + mloc)
void lus_u12_block(hipStream_t st, const double* Y, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                   double* U12) {
  const unsigned gu = (unsigned)((c1 - c0 + 63) / 64);
  if (b == 64) hipLaunchKernelGGL(lu_u12_kernel<64>, dim3(gu), dim3(256), 0, st, Y, ld, jb, jb - row0, c0, c1, U12, (int64_t)64);
  else hipLaunchKernelGGL(lu_u12_kernel<32>, dim3(gu), dim3(256), 0, st, Y, ld, jb, jb - row0, c0, c1, U12, (int64_t)32);
}
void lus_rankk(hipStream_t st, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
               const double* U12) {
  int64_t rbeg = c0 - row0;             // first local row below the block
  if (rbeg < 0) rbeg = 0;
  const int64_t mr = mloc - rbeg;
  if (mr <= 0) return;
  const unsigned gr = (unsigned)((mr + 127) / 128);
  if (b == 64) launch_rankk<64>(st, gr, Y, ld, mloc, rbeg, jb, c0, t, U12);
  else launch_rankk<32>(st, gr, Y, ld, mloc, rbeg, jb, c0, t, U12);
}

}}  // namespace gsi::hipk
