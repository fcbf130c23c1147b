// panel_lu_leaf.hip -- the register-resident form of `F = lu(Y); Q = F.L` (RandMatFact.jl:60-61, 68-69, 72-73)
// for panels of up to 4096 rows per CU (n = 10^6 at l = 320 is the case it is built for).  Same pivots as
// LAPACK dgetrf (first maximal |entry| wins), L in pivoted row order; what this form is about is how
// often the panel crosses HBM.
//
// Per-column sweeps (the first implementation, kept as tools/rejected_kernels/panel_lu_round1_sweeps.hip.txt) read and
// write the <= 8 live columns of a leaf once PER COLUMN: 88 column passes per 8-column leaf, and the blocks in between are
// brought up to date by K = 8/16/32 products that the big contraction kernel runs at 1.3-1.7 TB/s.  Here:
//   * lu_leaf_kernel: ONE persistent launch per 8-column leaf.  Every thread keeps its rows' 8 leaf values in
//     registers for all 8 pivot steps (10^6 x 8 doubles = 64 MB = half of the chip's register file), so a leaf costs
//     one read and one write of its columns.  The launch is also LEFT-LOOKING inside its 64-column block: on load it
//     applies the pending update of the block's earlier columns (reads kp = j0 - jb columns of L, U12 = L11^-1 A12
//     is a kp x 8 solve done redundantly by every workgroup, one wave per leaf column), so no in-block trailing
//     update is ever written back.  Per 64-column block: 8 (0 + 8 + ... + 56) + 128 = 352 column passes.
//     One exchange per pivot step: every workgroup publishes {max |value|, row, that row's 8 values} (workgroup 0
//     also row j's values) as one 256-byte record with write-through (sc1) stores, a drained flag store after them;
//     every workgroup polls all flags, reads all records and reduces them in the same fixed order, so the pivot row's
//     values are known everywhere without touching rows another workgroup owns (MI355X_MICROARCH.md, "Valid forms":
//     sc1 payload -> vmcnt(0) -> sc1 flag, sc1 polls and loads; no fences, no atomics).  Two record sets by parity of
//     the step: a workgroup can publish step s+2 only after it has seen every record of step s+1, which its owner
//     wrote after it had read step s.
//   * between the blocks: panel_lu_blocks.hip (left-looking; lu2_L runs its leaves inside that file's block loop).
// Column passes at l = 320, NB = 64: 5 * 352 + sum_b (64 b + 128) = 1760 + 1152 = 2912 (23.3 GB at n = 10^6) against 3296
// right-looking and ~52 GB with per-column sweeps.
#include "panel_lu_dev.hpp"
#include <cstdio>

namespace gsi { namespace hipk {

namespace {
#ifdef GSI_LU_TRACE
// debug build only (hipcc -DGSI_LU_TRACE): 100 MHz wall-clock stamps of the phases of every pivot step of the kp = 0
// leaves, for 4 workgroups; dumped by lu2_L to $GSI_LU_TRACE
__device__ unsigned long long g_lu_trace[4 * 8 * 8];
#define LU_STAMP(ph)                                                                                    \
  do {                                                                                                  \
    if (tid == 0 && kp == 0) {                                                                          \
      const int tw = (g == 0) ? 0 : (g == 1) ? 1 : (g == G / 2) ? 2 : (g == G - 1) ? 3 : -1;              \
      if (tw >= 0) g_lu_trace[(tw * 8 + s) * 8 + (ph)] = wall_clock64();                                   \
    }                                                                                                   \
  } while (0)
#else
#define LU_STAMP(ph) do { } while (0)
#endif
}  // namespace

// One leaf [j0, j0 + w) of the block that starts at column jb (kp = j0 - jb columns of the block already factored).
// Grid: G workgroups of BS threads, all resident (G <= number of CUs).  Rows j0 .. j0+7 (the leaf's diagonal block:
// the rows that become pivot rows) are held by threads 0..7 of workgroup 0 in `d`; every other row i >= j0 + 8 by
// thread (g, tid) as row j0 + 8 + (g R + rr) BS + tid, rr < R, in `a` -- those rows are active in every step and
// never final, so the code that touches the 8 x R register-resident values is straight-line: no per-row bookkeeping,
// no control-flow joins (a first version with early exits and per-step conditions made the compiler copy all of them
// at every join: 2x the registers, 900 spills at R = 8).
// Few fat waves on purpose: a pivot step is a chain of short dependent phases, and what it costs is the instruction
// stream per SIMD (a version with 16 waves per CU spent 10 us per step issuing ~1800 instructions per wave).
//
// Exchange format.  A record is 18 "units" (doubles): [0] max |value|, [1] row, [2..10) that row's leaf values,
// [10..18) row j's leaf values (workgroup 0 only).  Every unit travels as two 8-byte granules {32 value bits, 32-bit
// step tag}, each written by ONE sc1 store: a granule is the unit of atomicity, so a reader that sees the tag of this
// step in a granule has the data of this step -- no flag, no drain wait, no second round trip behind a flag.
// Two hops: the LEADER (last workgroup) reads every record, reduces them in a fixed order and publishes ONE result
// record {max, pivot row, its 8 values, row j's 8 values}; every other workgroup polls only that result (36 granules,
// one wave).  (Every workgroup sweeping all 256 records itself pulled 10 MB of write-through lines across the fabric
// per step and measured slower.)
// A leaf narrower than 8 columns (the panel's last) still runs 8 steps; steps s >= w see zero columns and are
// gated: no pivot is recorded, nothing is interchanged, the update multiplies zeros.
// MR (several ranks, one launch per rank): this rank holds rows [gbase, gbase + m) of the mtot-row panel in Y
// (local indices), its workgroups are records [rank * G, (rank + 1) * G) of the exchange, and every record is written
// into EVERY rank's record buffer (peer-mapped memory, system-scope stores; pollers read their own memory only).  Rank 0
// owns the diagonal block.  U12 of the pending update comes ready-made (rank 0 solved it, the host sequenced an
// all-reduce); the interchange of the columns outside the leaf is done after the launch (panel_lu_sharded.hip: lus_swap_*).
// MR, hier (shards of more than 256 / nranks workgroups: weak scaling, 10^6 rows per rank): TWO hops.  A workgroup publishes
// into its OWN rank's buffer only (slots 0 .. grid - 1) and every workgroup reduces its rank's records exactly as the
// single-GPU kernel does; workgroup 0 of each rank then writes the rank's result {max, row, its 8 values, row j's 8 values}
// into every rank's buffer (slots grid + rank), and every workgroup polls those nranks records: one more store latency
// across the fabric per pivot step, and the number of records a workgroup polls stays <= 256.
// OV: the panel (or, with MR, this rank's shard) is TALLER than the grid's registers hold.  Rows beyond the resident window -- [ovb, m),
// ovb = j0 + 8 + grid * R * BS -- stay in HBM with their STORED leaf values and are evaluated lazily, as the streamed
// leaves (panel_lu_streamed.hip) do it: the pending update is applied to them once on the way in (written back), every pivot step
// re-derives their candidates from the stored values and the pivot rows so far (s_u), the leaf's last act turns them into
// multipliers.  An overflow row that wins a pivot step hands its values over through the record like any other row and
// receives the old row j's CURRENT values in exchange -- those are already eliminated through the steps before, which a
// small list (s_lr, s_ll: row, first step still to apply) remembers.  Same operations on the same values in the same
// order as the resident rows see: bit-identical factors.  What it is for: the panels just above 4096 rows per CU, whose
// few overflow rows sit in L2 / Infinity Cache between the steps (1.2e6 rows: 9 instead of 14.7 ms).
template <int BS, int R, bool MR, bool OV = false>
__global__ __launch_bounds__(BS) void lu_leaf_kernel(double* __restrict__ Y, int64_t ld, int32_t m, int32_t l,
                                                     int32_t jb, int32_t j0, int w, unsigned long long* __restrict__ recs,
                                                     uint32_t epoch_base, int32_t* __restrict__ ipiv,
                                                     int32_t* __restrict__ info, int onehop, int poll_limit,
                                                     uint32_t mute_epoch, LuMrArgs mr) {
  constexpr int NW = BS / 64;
  constexpr int LPR = BS / 256;               // leader: consumer lanes per record (G <= 256 records)
  constexpr int GPL = (2 * (2 + LW)) / LPR;   // leader: granules per consumer lane
  static_assert(GPL * LPR == 2 * (2 + LW), "record does not divide over its consumer lanes");
  static_assert(LW == 8, "the step list below is written out for 8-column leaves");
  __shared__ double Ls[KPMAX * LSP];
  __shared__ double Us[KPMAX * LW];
  __shared__ double s_val[NW];
  __shared__ int32_t s_idx[NW];
  __shared__ double s_cand[NW][LW];
  __shared__ double s_oldpub[LW];
  __shared__ double c_val[NW];
  __shared__ int32_t c_idx[NW];
  __shared__ uint32_t c_rowbits[NW][2 * LW];  // the wave-local winner's 8 row values as 16 halves
  __shared__ uint32_t c_oldbits[2 * LW];
  __shared__ int32_t c_slot[NW];
  __shared__ int s_abort;
  __shared__ double s_u[OV ? LW * LW : 1];      // OV: the leaf's pivot rows so far (u_t) and 1 / u_tt
  __shared__ double s_rp[OV ? LW : 1];
  __shared__ int32_t s_lr[OV ? LW : 1];         // OV: overflow rows that hold values eliminated through step s_ll - 1
  __shared__ int32_t s_ll[OV ? LW : 1];
  __shared__ int32_t s_nl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int Gl = gridDim.x;                                 // this rank's workgroups
  const bool hier = MR && mr.hier != 0;
  const int G = MR ? mr.slots : Gl;                         // record slots of the exchange (layout of the buffer)
  const int GP = hier ? Gl : G;                             // records a workgroup polls in the (first) hop
  const int gslot = MR ? (hier ? g : mr.rank * Gl + g) : g; // this workgroup's record
  const int32_t gbase = MR ? mr.gbase : 0;                  // global index of local row 0
  const int32_t mtot = MR ? mr.mtot : m;
  const int kp = j0 - jb;
  // a launch that follows a timed-out one (info < 0, same stream) drains without polling: one time-out per factorization
  if (tid == 0) s_abort = (__hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) ? 1 : 0;

  // addressing: one uniform 64-bit column base (SGPRs) + a 32-bit per-thread byte offset, so no 64-bit per-element
  // address stays live in VGPRs between the load at the top and the store at the bottom (m < 2^28 rows)
  auto colbase = [&](int32_t c) -> char* { return reinterpret_cast<char*>(Y + (int64_t)c * ld); };
  auto elem = [&](char* base, int32_t i) -> double* { return reinterpret_cast<double*>(base + (uint32_t)i * 8u); };
  // regular rows: local row0 + rr BS (global gbase + that); on a rank > 0 every local row is below the diagonal block
  const int32_t row0 = ((gbase == 0) ? j0 + LW : 0) + g * (R * BS) + tid;
  const int32_t grow0 = gbase + row0;
  const bool isdiag = (g == 0 && tid < LW && gbase == 0);  // holds row j0 + tid of the diagonal block in d
  const int32_t drow = j0 + tid;
  double a[R][LW];
  double d[LW];
#pragma unroll
  for (int k = 0; k < LW; ++k) {
    char* cb = colbase(j0 + (k < w ? k : 0));
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const int32_t i = row0 + rr * BS;
      a[rr][k] = (i < m && k < w) ? *elem(cb, i) : 0.0;   // rows beyond m, columns beyond w: zeros
    }
    d[k] = (isdiag && drow < m && k < w) ? *elem(cb, drow) : 0.0;
  }

  // ---- pending update of the block's earlier columns: a -= L[:, jb:j0] * (L11^-1 A12) ----------------------
  if (kp > 0) {
    // U12 = L11^-1 A12 lives in rows jb .. j0 of the block: on rank 0 when the panel is sharded.  Rank 0 solves it like
    // the single-rank kernel (every workgroup for itself) and its workgroup 0 pushes the kp x 8 values, tagged with this
    // leaf's first epoch, into the other ranks' U mailboxes; they poll their own memory.
    const bool solve_here = !MR || gbase == 0;
    if (solve_here) {
    {
      // all of a thread's elements of the kp x kp block are requested before the first one is used: as a plain loop this
      // was one HBM / L2 round trip per iteration (up to KPMAX^2 / BS of them) at the head of every leaf
      constexpr int NLS = (KPMAX * KPMAX + BS - 1) / BS;
      double lsv[NLS];
#pragma unroll
      for (int i = 0; i < NLS; ++i) {
        const int e = tid + i * BS;
        const int ec = e < kp * kp ? e : 0;
        const int r = ec % kp, c = ec / kp;
        lsv[i] = Y[(jb + r) + (int64_t)(jb + c) * ld];
      }
#pragma unroll
      for (int i = 0; i < NLS; ++i) {
        const int e = tid + i * BS;
        if (e < kp * kp) Ls[(e % kp) * LSP + e / kp] = lsv[i];
      }
    }
    __syncthreads();
    for (int v = wave; v < LW; v += NW) {          // one wave per leaf column: forward substitution along the lanes
      double x = (lane < kp && v < w) ? Y[(jb + lane) + (int64_t)(j0 + v) * ld] : 0.0;
      for (int cp = 0; cp < kp; ++cp) {
        const double xc = readlane_d(x, __builtin_amdgcn_readfirstlane(cp));
        if (lane > cp && lane < kp) x -= Ls[lane * LSP + cp] * xc;
      }
      if (lane < kp) Us[lane * LW + v] = x;
    }
    __syncthreads();
    }
    if constexpr (MR) {
      const uint32_t utag = epoch_base + 1u;
      const size_t ubox = (size_t)2 * (size_t)G * REC + (size_t)((epoch_base >> 3) & 1u) * (size_t)(2 * KPMAX * LW);
      if (gbase == 0) {
        if (g == 0) {
          for (int e = tid; e < kp * LW; e += BS) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(Us[e]);
            for (int q = 0; q < mr.nranks; ++q) {
              if (q == mr.rank) continue;
              __hip_atomic_store(mr.peer[q] + ubox + 2 * e, ((unsigned long long)utag << 32) | (uint32_t)bits, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
              __hip_atomic_store(mr.peer[q] + ubox + 2 * e + 1, ((unsigned long long)utag << 32) | (uint32_t)(bits >> 32),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
          }
        }
      } else {
        __syncthreads();                          // s_abort (set by thread 0 at the top) is read below
        for (int e = tid; e < kp * LW; e += BS) {
          unsigned long long lo = 0, hi = 0;
          int tries = s_abort ? poll_limit : 0;
          for (;;) {
            lo = poll_granule<true>(recs + ubox + 2 * e);
            hi = poll_granule<true>(recs + ubox + 2 * e + 1);
            if ((uint32_t)(lo >> 32) == utag && (uint32_t)(hi >> 32) == utag) break;
            if (++tries > poll_limit) { s_abort = 1; lu_timeout_note(info, 1, e, utag, mr.rank * 1024 + g); break; }
            __builtin_amdgcn_s_sleep(1);
          }
          Us[e] = __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
        }
        __syncthreads();
      }
    }
    for (int c = 0; c < kp; c += 2) {              // kp is a multiple of the leaf width
      double lv[2][R];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        char* cb = colbase(jb + c + cc);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
          const int32_t i = row0 + rr * BS;
          lv[cc][rr] = (i < m) ? *elem(cb, i) : 0.0;
        }
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        double u[LW];
#pragma unroll
        for (int k = 0; k < LW; ++k) u[k] = Us[(c + cc) * LW + k];
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
          for (int k = 0; k < LW; ++k) a[rr][k] -= lv[cc][rr] * u[k];
      }
    }
    if (isdiag && drow < m) {                      // (8 threads of the grid) the diagonal block's rows
      for (int c = 0; c < kp; ++c) {
        const double lvd = *elem(colbase(jb + c), drow);
#pragma unroll
        for (int k = 0; k < LW; ++k) d[k] -= lvd * Us[c * LW + k];
      }
    }
  }

  // ---- OV: the rows beyond the resident window ---------------------------------------------------------------
  const int32_t ovb = ((gbase == 0) ? j0 + LW : 0) + Gl * (R * BS);   // first overflow row (LOCAL index, as every i below)
  const int32_t ovstride = Gl * BS;
  const int32_t ov0 = ovb + g * BS + tid;                   // this thread's overflow rows: ov0 + k ovstride < m
  // first step still to apply to overflow row i (0 unless it received an old row j during this leaf)
  auto ov_level = [&](int32_t i) -> int {
    int lev = 0;
    const int nl = s_nl;
    for (int q = 0; q < nl; ++q) if (s_lr[q] == i) lev = s_ll[q];
    return lev;
  };
  if constexpr (OV) {
    if (tid == 0) s_nl = 0;
    if (kp > 0) {                                           // pending update, written back (as lu3_open_kernel)
      for (int32_t i = ov0; i < m; i += ovstride) {
        double x[LW];
#pragma unroll
        for (int k = 0; k < LW; ++k) x[k] = (k < w) ? *elem(colbase(j0 + k), i) : 0.0;
        for (int c = 0; c < kp; c += 4) {
          double lv4[4];
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) lv4[cc] = *elem(colbase(jb + c + cc), i);
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
#pragma unroll
            for (int k = 0; k < LW; ++k) x[k] -= lv4[cc] * Us[(c + cc) * LW + k];
        }
#pragma unroll
        for (int k = 0; k < LW; ++k) if (k < w) *elem(colbase(j0 + k), i) = x[k];
      }
    }
    __syncthreads();                                        // s_nl
  }

  // Row interchanges of the columns OUTSIDE the leaf (LAPACK swaps whole rows): column c belongs to workgroup
  // c % G, thread c / G.  Pipelined one step behind: the two loads of step s are issued when its pivot is known and
  // stored swapped at step s + 1, so their latency hides behind the next exchange (same thread, program order:
  // a later load of the same element sees the earlier store).
  const int32_t swc = g + Gl * tid;
  const bool has_col = !MR && swc < l && !(swc >= j0 && swc < j0 + w);
  double* const swcol = Y + (int64_t)(has_col ? swc : 0) * ld;
  bool pend = false;
  double pa0 = 0.0, pa1 = 0.0;
  int32_t pj = 0, pr = 0;

  // one pivot step; S = leaf column (compile time: register index)
  auto step = [&](auto S_) {
    constexpr int s = decltype(S_)::value;
    const bool live = s < w;
    const int32_t j = j0 + s;
    const uint32_t epoch = epoch_base + (uint32_t)s + 1u;
    const size_t set_off = (size_t)(epoch & 1u) * (size_t)G * REC;
    unsigned long long* rec_set = recs + set_off;
    LU_STAMP(0);
    // (a) this thread's, this wave's, this workgroup's candidate for column s; lowest rows first, strict >
    double best = -1.0;
    int32_t besti = -1;
    if (isdiag && tid >= s) { best = fabs(d[s]); besti = drow; }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const double av = fabs(a[rr][s]);
      if (av > best && (!MR || row0 + rr * BS < m)) { best = av; besti = grow0 + rr * BS; }   // MR: rows beyond the shard are no candidates
    }
    if constexpr (OV) {                         // overflow rows: current value in column s from the stored values, lazily
      if (live) {
        for (int32_t i = ov0; i < m; i += ovstride) {
          const int lev = ov_level(i);
          double x[s + 1];
#pragma unroll
          for (int k = 0; k <= s; ++k) x[k] = *elem(colbase(j0 + k), i);
#pragma unroll
          for (int t = 0; t < s; ++t) {
            if (t >= lev) {
              const double rp = s_rp[t];
              const double lt = (rp != 0.0) ? x[t] * rp : x[t];
#pragma unroll
              for (int k = t + 1; k <= s; ++k) x[k] -= lt * s_u[t * LW + k];
            }
          }
          const double av = fabs(x[s]);
          if (av > best) { best = av; besti = gbase + i; }
        }
      }
    }
    double wv = best;
    int32_t wi = besti;
    wave_argmax(wv, wi);
    if (lane == 0) { s_val[wave] = wv; s_idx[wave] = wi; }
    if (besti >= 0 && besti == wi) {            // the ONE lane of the wave that owns its candidate row: one copy per
      if (isdiag && besti == drow) {            // wave (~40 instructions) is cheaper than two more barriers
#pragma unroll
        for (int k = 0; k < LW; ++k) s_cand[wave][k] = d[k];
      }
      if constexpr (OV) {
        if (besti - gbase >= ovb) {             // an overflow row: all 8 of its current values
          const int32_t bl = besti - gbase;
          const int lev = ov_level(bl);
          double x[LW];
#pragma unroll
          for (int k = 0; k < LW; ++k) x[k] = (k < w) ? *elem(colbase(j0 + k), bl) : 0.0;
#pragma unroll
          for (int t = 0; t < s; ++t) {
            if (t >= lev) {
              const double rp = s_rp[t];
              const double lt = (rp != 0.0) ? x[t] * rp : x[t];
              x[t] = lt;
#pragma unroll
              for (int k = t + 1; k < LW; ++k) x[k] -= lt * s_u[t * LW + k];
            }
          }
#pragma unroll
          for (int k = 0; k < LW; ++k) s_cand[wave][k] = x[k];
        }
      }
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (grow0 + rr * BS == besti) {
#pragma unroll
          for (int k = 0; k < LW; ++k) s_cand[wave][k] = a[rr][k];
        }
    }
    if (isdiag && tid == s) {                   // row j itself (the row the pivot row will be exchanged with)
#pragma unroll
      for (int k = 0; k < LW; ++k) s_oldpub[k] = d[k];
    }
    __syncthreads();
    LU_STAMP(1);
    // (b) wave 0 reduces the waves' candidates and publishes the workgroup's record: one granule per lane
    if (wave == 0) {
      double pv = (lane < NW) ? s_val[lane] : -1.0;
      int32_t pi = (lane < NW) ? s_idx[lane] : -1;
      const int32_t mywi = pi;
      static_assert(NW <= 8, "wave_argmax8 reduces lanes 0..7");
      wave_argmax8(pv, pi);
      const unsigned long long own = __ballot(lane < NW && pi >= 0 && mywi == pi);
      const int ww = own ? (__ffsll((long long)own) - 1) : 0;
      const int unit = lane >> 1;
      // mute_epoch != 0 (tests only): the last workgroup stays silent at that step, as a workgroup that never got a CU
      // would -- everyone else runs out of polls and the launch ends with info = -1
      const bool muted = (mute_epoch != 0u && epoch == mute_epoch && gslot == G - 1);
      if (!muted && (unit < 2 + LW || (gslot == 0 && unit < 2 + 2 * LW))) {
        unsigned long long bits;
        if (unit == 0) bits = (unsigned long long)__double_as_longlong(pv);
        else if (unit == 1) bits = (unsigned long long)(long long)pi;
        else if (unit < 2 + LW) bits = (unsigned long long)__double_as_longlong(s_cand[ww][unit - 2]);
        else bits = (unsigned long long)__double_as_longlong(s_oldpub[unit - 2 - LW]);
        const uint32_t half = (lane & 1) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
        if constexpr (MR) {
          if (hier) {                              // first hop stays on this rank
            __hip_atomic_store(rec_set + (size_t)gslot * REC + lane, ((unsigned long long)epoch << 32) | half, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
          } else {
            for (int q = 0; q < mr.nranks; ++q)    // one copy into every rank's buffer: remote stores, local polls
              __hip_atomic_store(mr.peer[q] + set_off + (size_t)gslot * REC + lane, ((unsigned long long)epoch << 32) | half,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        } else {
          __hip_atomic_store(rec_set + (size_t)g * REC + lane, ((unsigned long long)epoch << 32) | half,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    // (c) the exchange.  Two protocols (GSI_LU_ONEHOP selects):
    //  one hop (default): every workgroup reads the (value, row) head of every record itself (3 granules each: 6 KB per
    //            workgroup and round), reduces, then fetches the winner's row values (landed long before) and row j;
    //            measured 5.6-6.5 us per step, LU 7.35 ms at n = 1e6, l = 320;
    //  two hops: a leader sweeps all WHOLE records, reduces, publishes the result; everyone else polls the result:
    //            6.5-7.5 us per step (7.7 ms).  (Every workgroup sweeping all whole records -- 40 KB each -- 14.7 us.)
    const bool leader = (g == G - 1) && !onehop;           // (MR launches always use the one-hop protocol)
    // the result is published in LU2_RES_COPIES copies on lines of their own; workgroup g polls copy g % LU2_RES_COPIES
    // (255 workgroups polling the same three lines serialise on one memory channel)
    unsigned long long* res = recs + (size_t)2 * (size_t)G * REC + (size_t)(epoch & 1u) * (size_t)LU2_RES_COPIES * REC;
    if (onehop) {
      const int ncw1 = (GP + 63) / 64;                                     // one lane per record
      if (wave < ncw1) {
        const bool mine = tid < GP;
        const unsigned long long* src = rec_set + (size_t)(mine ? tid : 0) * REC;
        const bool extra = tid < 2 * LW;                                    // workgroup 0's copy of row j
        const unsigned long long* xsrc = rec_set + 2 * (2 + LW) + (extra ? tid : 0);
        unsigned long long g0 = 0, g1 = 0, g2 = 0, gx = 0;
        int tries = s_abort ? poll_limit : 0;
        bool ok;
        for (;;) {
          if (mine) {
            g0 = poll_granule<MR>(src + 0);
            g1 = poll_granule<MR>(src + 1);
            g2 = poll_granule<MR>(src + 2);
          }
          if (extra) gx = poll_granule<MR>(xsrc);
          ok = !mine || ((uint32_t)(g0 >> 32) == epoch && (uint32_t)(g1 >> 32) == epoch && (uint32_t)(g2 >> 32) == epoch);
          if (extra) ok = ok && ((uint32_t)(gx >> 32) == epoch);
          if (__all(ok)) break;
          if (++tries > poll_limit) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (!__all(ok)) { s_abort = 1; if (!ok) lu_timeout_note(info, 2, tid, epoch, (MR ? mr.rank : 0) * 1024 + g); }
        LU_STAMP(2);
        if (extra) c_oldbits[tid] = (uint32_t)gx;
        double cv = -1.0;
        int32_t ci = -1;
        if (mine) {
          cv = __longlong_as_double((long long)(((unsigned long long)(uint32_t)g1 << 32) | (uint32_t)g0));
          ci = (int32_t)(uint32_t)g2;
        }
        double rv = cv;
        int32_t ri = ci;
        wave_argmax(rv, ri);
        if (mine && ri >= 0 && ci == ri) c_slot[wave] = tid;              // the record that holds the wave's winner
        if (lane == 0) { c_val[wave] = rv; c_idx[wave] = ri; }
      }
      __syncthreads();
      if (wave == 0) {
        double fv = (lane < ncw1) ? c_val[lane] : -1.0;
        int32_t fi = (lane < ncw1) ? c_idx[lane] : -1;
        const int32_t myfi = fi;
        wave_argmax8(fv, fi);
        const unsigned long long own = __ballot(lane < ncw1 && fi >= 0 && myfi == fi);
        const int fw = own ? (__ffsll((long long)own) - 1) : 0;
        const int gw = (fi >= 0) ? c_slot[fw] : 0;
        // the winner's 8 row values: granules 4 .. 20 of its record, one per lane (they were stored with the head)
        const bool mine = lane < 2 * LW;
        const unsigned long long* rsrc = rec_set + (size_t)gw * REC + 4 + (mine ? lane : 0);
        unsigned long long gv = 0;
        int tries = s_abort ? poll_limit : 0;
        bool ok;
        for (;;) {
          if (mine) gv = poll_granule<MR>(rsrc);
          ok = !mine || ((uint32_t)(gv >> 32) == epoch);
          if (__all(ok)) break;
          if (++tries > poll_limit) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (!__all(ok)) { s_abort = 1; if (!ok) lu_timeout_note(info, 3, gw, epoch, (MR ? mr.rank : 0) * 1024 + g); }
        LU_STAMP(3);
        if (mine) c_rowbits[0][lane] = (uint32_t)gv;
        if (lane == 0) { c_val[0] = fv; c_idx[0] = fi; }
      }
      __syncthreads();
      if constexpr (MR) {
        if (hier) {                               // second hop: the ranks' results (slots Gl .. Gl + nranks - 1 of every buffer)
          if (wave == 0) {
            if (g == 0) {                         // this rank's result, one granule per lane, into every rank's buffer
              const int unit = lane >> 1;
              if (unit < 2 + 2 * LW) {
                unsigned long long bits;
                if (unit == 0) bits = (unsigned long long)__double_as_longlong(c_val[0]);
                else if (unit == 1) bits = (unsigned long long)(long long)c_idx[0];
                else if (unit < 2 + LW) bits = reinterpret_cast<const unsigned long long*>(c_rowbits[0])[unit - 2];
                else bits = reinterpret_cast<const unsigned long long*>(c_oldbits)[unit - 2 - LW];
                const uint32_t half = (lane & 1) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
                for (int q = 0; q < mr.nranks; ++q)
                  __hip_atomic_store(mr.peer[q] + set_off + (size_t)(Gl + mr.rank) * REC + lane, ((unsigned long long)epoch << 32) | half,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              }
            }
            const bool rmine = lane < mr.nranks;
            const unsigned long long* src = rec_set + (size_t)(Gl + (rmine ? lane : 0)) * REC;
            unsigned long long g0 = 0, g1 = 0, g2 = 0;
            int tries = s_abort ? poll_limit : 0;
            bool ok;
            for (;;) {
              if (rmine) {
                g0 = poll_granule<true>(src + 0);
                g1 = poll_granule<true>(src + 1);
                g2 = poll_granule<true>(src + 2);
              }
              ok = !rmine || ((uint32_t)(g0 >> 32) == epoch && (uint32_t)(g1 >> 32) == epoch && (uint32_t)(g2 >> 32) == epoch);
              if (__all(ok)) break;
              if (++tries > poll_limit) break;
              __builtin_amdgcn_s_sleep(1);
            }
            if (!__all(ok)) { s_abort = 1; if (!ok) lu_timeout_note(info, 4, lane, epoch, mr.rank * 1024 + g); }
            double cv = -1.0;
            int32_t ci = -1;
            if (rmine) {
              cv = __longlong_as_double((long long)(((unsigned long long)(uint32_t)g1 << 32) | (uint32_t)g0));
              ci = (int32_t)(uint32_t)g2;
            }
            double rv = cv;
            int32_t ri = ci;
            wave_argmax(rv, ri);
            const unsigned long long own = __ballot(rmine && ri >= 0 && ci == ri);
            const int qw = own ? (__ffsll((long long)own) - 1) : 0;
            // the winner's 8 row values (its rank's record) and row j's (rank 0's record): 16 granules each, one per lane
            const bool vmine = lane < 2 * LW, omine = lane >= 32 && lane < 32 + 2 * LW;
            const unsigned long long* vsrc = rec_set + (size_t)(Gl + qw) * REC + 4 + (vmine ? lane : 0);
            const unsigned long long* osrc = rec_set + (size_t)Gl * REC + 2 * (2 + LW) + (omine ? lane - 32 : 0);
            unsigned long long gv = 0;
            tries = s_abort ? poll_limit : 0;
            for (;;) {
              if (vmine) gv = poll_granule<true>(vsrc);
              if (omine) gv = poll_granule<true>(osrc);
              ok = !(vmine || omine) || ((uint32_t)(gv >> 32) == epoch);
              if (__all(ok)) break;
              if (++tries > poll_limit) break;
              __builtin_amdgcn_s_sleep(1);
            }
            if (!__all(ok)) { s_abort = 1; if (!ok) lu_timeout_note(info, 5, qw, epoch, mr.rank * 1024 + g); }
            if (vmine) c_rowbits[0][lane] = (uint32_t)gv;
            if (omine) c_oldbits[lane - 32] = (uint32_t)gv;
            if (lane == 0) { c_val[0] = rv; c_idx[0] = ri; }
          }
          __syncthreads();
        }
      }
    } else
    {
    const int ncw = leader ? (G * LPR + 63) / 64 : 1;                     // waves that hold entries of the reduction
    if (leader) {
      const int slot = tid / LPR, part = tid % LPR;
      const bool mine = slot < G;
      const unsigned long long* src = rec_set + (size_t)(mine ? slot : 0) * REC + part * GPL;
      const bool extra = tid < 2 * LW;                                    // workgroup 0's copy of row j
      const unsigned long long* xsrc = rec_set + 2 * (2 + LW) + (extra ? tid : 0);
      if (wave < ncw) {
        unsigned long long gl[GPL], gx = 0;
        int tries = s_abort ? poll_limit : 0;   // a timed-out launch drains without polling again
        bool ok;
        for (;;) {
#pragma unroll
          for (int i = 0; i < GPL; ++i) gl[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (extra) gx = __hip_atomic_load(xsrc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = true;
          if (mine) {
#pragma unroll
            for (int i = 0; i < GPL; ++i) ok = ok && ((uint32_t)(gl[i] >> 32) == epoch);
          }
          if (extra) ok = ok && ((uint32_t)(gx >> 32) == epoch);
          if (__all(ok)) break;
          if (++tries > poll_limit) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (!__all(ok)) s_abort = 1;
        LU_STAMP(2);
        if (extra) c_oldbits[tid] = (uint32_t)gx;
        // candidate (value, row) sits in the record's first four granules = part 0's gl[0..4)
        double cv = -1.0;
        int32_t ci = -1;
        if (mine && part == 0) {
          cv = __longlong_as_double((long long)(((unsigned long long)(uint32_t)gl[1] << 32) | (uint32_t)gl[0]));
          ci = (int32_t)(uint32_t)gl[2];
        }
        double rv = cv;
        int32_t ri = ci;
        wave_argmax(rv, ri);
        // the lanes of the wave-local winner's record drop its row values (granules 4..20) into LDS
        const int32_t myi = __shfl(ci, lane - part);       // the record's row, known to all of its lanes
        if (mine && ri >= 0 && myi == ri) {
#pragma unroll
          for (int i = 0; i < GPL; ++i) {
            const int gi = part * GPL + i;
            if (gi >= 4) c_rowbits[wave][gi - 4] = (uint32_t)gl[i];
          }
        }
        if (lane == 0) { c_val[wave] = rv; c_idx[wave] = ri; }
      }
      __syncthreads();
      if (wave == 0) {                          // finish the reduction and publish the result: one granule per lane
        double fv = (lane < ncw) ? c_val[lane] : -1.0;
        int32_t fi = (lane < ncw) ? c_idx[lane] : -1;
        const int32_t myfi = fi;
        wave_argmax8(fv, fi);
        const unsigned long long own = __ballot(lane < ncw && fi >= 0 && myfi == fi);
        const int fw = own ? (__ffsll((long long)own) - 1) : 0;
        const int unit = lane >> 1;
        unsigned long long bits = 0;
        if (unit < 2 + 2 * LW) {
          if (unit == 0) bits = (unsigned long long)__double_as_longlong(fv);
          else if (unit == 1) bits = (unsigned long long)(long long)fi;
          else if (unit < 2 + LW) bits = reinterpret_cast<const unsigned long long*>(c_rowbits[fw])[unit - 2];
          else bits = reinterpret_cast<const unsigned long long*>(c_oldbits)[unit - 2 - LW];
          const uint32_t half = (lane & 1) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
#pragma unroll
          for (int cpy = 0; cpy < LU2_RES_COPIES; ++cpy)
            __hip_atomic_store(res + (size_t)cpy * REC + lane, ((unsigned long long)epoch << 32) | half, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        LU_STAMP(3);
        // the leader's own threads read the result from slot 0, like everybody else
        if (lane == 0) { c_val[0] = fv; c_idx[0] = fi; }
        if (unit >= 2 && unit < 2 + LW && (lane & 1) == 0) reinterpret_cast<unsigned long long*>(c_rowbits[0])[unit - 2] = bits;
      }
      __syncthreads();
    } else {
      if (wave == 0) {                          // poll the leader's result: granule `lane`
        const bool mine = lane < 2 * (2 + 2 * LW);
        unsigned long long gv = 0;
        int tries = s_abort ? poll_limit : 0;
        bool ok;
        for (;;) {
          if (mine) gv = __hip_atomic_load(res + (size_t)(g % LU2_RES_COPIES) * REC + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = !mine || ((uint32_t)(gv >> 32) == epoch);
          if (__all(ok)) break;
          if (++tries > poll_limit) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (!__all(ok)) s_abort = 1;
        LU_STAMP(3);
        // lay the result out exactly as the leader's own LDS image: c_val / c_idx [0], c_rowbits[0], c_oldbits
        if (lane < 2) reinterpret_cast<uint32_t*>(&c_val[0])[lane] = (uint32_t)gv;
        else if (lane == 2) c_idx[0] = (int32_t)(uint32_t)gv;
        else if (lane >= 4 && lane < 4 + 2 * LW) c_rowbits[0][lane - 4] = (uint32_t)gv;
        else if (lane >= 4 + 2 * LW && lane < 4 + 4 * LW) c_oldbits[lane - 4 - 2 * LW] = (uint32_t)gv;
      }
      __syncthreads();
    }
    }
    LU_STAMP(4);
    // (d) the result: slot 0 of the LDS image
    const double bestv = c_val[0];
    int32_t r = c_idx[0];
    const bool valid = live && (r >= j && r < mtot);
    if (!valid) r = j;                           // all-NaN column (or a gated step): no interchange
    const double* c_old = reinterpret_cast<const double*>(c_oldbits);
    const double* c_row = reinterpret_cast<const double*>(c_rowbits[0]);
    double u[LW];
#pragma unroll
    for (int k = 0; k < LW; ++k) u[k] = valid ? c_row[k] : c_old[k];
    const double piv = u[s];
    const double rpiv = (piv != 0.0) ? 1.0 / piv : 0.0;
    if constexpr (OV) {
      if (live) {
        if (tid == 0) {                         // (unrolled: u[] indexed by the thread id would live in scratch)
#pragma unroll
          for (int k = 0; k < LW; ++k) s_u[s * LW + k] = u[k];
          s_rp[s] = rpiv;
        }
        const int32_t rl = r - gbase;           // (local index; on another rank's rows this is out of [ovb, m))
        if (rl >= ovb && rl < m && r != j) {    // the pivot row was one of MY overflow rows: the old row j moves there, already
          if (tid == 2 * LW) { const int q = s_nl; s_lr[q] = rl; s_ll[q] = s; s_nl = q + 1; }    // eliminated through step s - 1
          if ((rl - ovb) % ovstride == g * BS + tid) {
#pragma unroll
            for (int k = 0; k < LW; ++k) if (k < w) *elem(colbase(j0 + k), rl) = c_old[k];
          }
        }
      }
      __syncthreads();                          // s_u / the list before the next step's lazy evaluations
    }
    // (e) bookkeeping by workgroup 0; pipelined interchange of this thread's column outside the leaf
    if (g == 0 && tid == 0 && live) {
      ipiv[j] = r;
      if (!(bestv > 0.0)) atomicCAS(info, 0, j + 1);
    }
    if (has_col) {
      if (pend) { swcol[pj] = pa1; swcol[pr] = pa0; }
      pend = (r != j);
      if (pend) { pa0 = swcol[j]; pa1 = swcol[r]; pj = j; pr = r; }
    }
    // (f) rank-1 update in registers: regular rows are all active, none is row j
    bool hit = false;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) hit = hit || (grow0 + rr * BS == r);
    if (hit) {                                   // (one thread of the whole grid) the old row j moves here
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
        if (grow0 + rr * BS == r) {
#pragma unroll
          for (int k = 0; k < LW; ++k) a[rr][k] = c_old[k];
        }
    }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const double x0 = a[rr][s];
      const double lij = (rpiv != 0.0) ? x0 * rpiv : x0;
      a[rr][s] = lij;
#pragma unroll
      for (int k = s + 1; k < LW; ++k) a[rr][k] -= lij * u[k];
    }
    if (isdiag && tid >= s) {                    // the diagonal block's rows (8 threads of the grid)
      if (tid == s) {                            // this position receives the pivot row and is final
#pragma unroll
        for (int k = 0; k < LW; ++k) d[k] = u[k];
      } else {
        if (drow == r) {                         // the old row j moves here
#pragma unroll
          for (int k = 0; k < LW; ++k) d[k] = c_old[k];
        }
        const double x0 = d[s];
        const double lij = (rpiv != 0.0) ? x0 * rpiv : x0;
        d[s] = lij;
#pragma unroll
        for (int k = s + 1; k < LW; ++k) d[k] -= lij * u[k];
      }
    }
    LU_STAMP(5);
  };

  // straight-line step list
  {
    using std::integral_constant;
    step(integral_constant<int, 0>{});
    step(integral_constant<int, 1>{});
    step(integral_constant<int, 2>{});
    step(integral_constant<int, 3>{});
    step(integral_constant<int, 4>{});
    step(integral_constant<int, 5>{});
    step(integral_constant<int, 6>{});
    step(integral_constant<int, 7>{});
  }
  if constexpr (OV) {                           // the overflow rows' multipliers
    for (int32_t i = ov0; i < m; i += ovstride) {
      const int lev = ov_level(i);
      double x[LW];
#pragma unroll
      for (int k = 0; k < LW; ++k) x[k] = (k < w) ? *elem(colbase(j0 + k), i) : 0.0;
#pragma unroll
      for (int t = 0; t < LW; ++t) {
        if (t >= lev && t < w) {
          const double rp = s_rp[t];
          const double lt = (rp != 0.0) ? x[t] * rp : x[t];
          x[t] = lt;
#pragma unroll
          for (int k = t + 1; k < LW; ++k) x[k] -= lt * s_u[t * LW + k];
        }
      }
#pragma unroll
      for (int k = 0; k < LW; ++k) if (k < w) *elem(colbase(j0 + k), i) = x[k];
    }
  }
  if (s_abort && tid == 0) atomicExch(info, -1);
  if (has_col && pend) { swcol[pj] = pa1; swcol[pr] = pa0; }
#pragma unroll
  for (int k = 0; k < LW; ++k) {
    if (k < w) {
      char* cb = colbase(j0 + k);
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        const int32_t i = row0 + rr * BS;
        if (i < m) *elem(cb, i) = a[rr][k];
      }
      if (isdiag && drow < m) *elem(cb, drow) = d[k];
    }
  }
}

bool lu2_config(int64_t m, int ncus, int* bs, int* rpt, int* grid) {
  if (ncus < 1) return false;
  if (ncus > 256) ncus = 256;               // the leader reads one record per workgroup with <= 2 lanes each
  static const int cfg[4][2] = {{256, 1}, {256, 4}, {512, 4}, {512, 8}};
  for (int c = 0; c < 4; ++c) {
    const int64_t per = (int64_t)cfg[c][0] * cfg[c][1];
    if (m <= (int64_t)ncus * per) { *bs = cfg[c][0]; *rpt = cfg[c][1]; *grid = (int)((m + per - 1) / per); return true; }
  }
  return false;
}

template <int BS, int R>
static void launch_leaf(hipStream_t st, int grid, double* Y, int64_t ld, int64_t m, int64_t l, int64_t jb, int64_t j0,
                        int w, const Lu2Work& wk, uint32_t epoch_base) {
  static const int onehop = getenv("GSI_LU_ONEHOP") ? atoi(getenv("GSI_LU_ONEHOP")) : 1;   // A/B knob; 0 = two hops via a leader
  const int poll_limit = wk.poll_limit > 0 ? wk.poll_limit : POLL_LIMIT;
  LuMrArgs none{};
  if constexpr (BS == 512 && R == 8) {
    if (wk.ov) {                          // taller than the grid's registers: overflow rows evaluated lazily
      hipLaunchKernelGGL((lu_leaf_kernel<512, 8, false, true>), dim3(grid), dim3(512), 0, st, Y, ld, (int32_t)m, (int32_t)l,
                         (int32_t)jb, (int32_t)j0, w, wk.recs, epoch_base, wk.ipiv, wk.info, 1, poll_limit, wk.mute_epoch, none);
      return;
    }
  }
  if (!wk.cooperative) {
    hipLaunchKernelGGL((lu_leaf_kernel<BS, R, false>), dim3(grid), dim3(BS), 0, st, Y, ld, (int32_t)m, (int32_t)l, (int32_t)jb,
                       (int32_t)j0, w, wk.recs, epoch_base, wk.ipiv, wk.info, onehop, poll_limit, wk.mute_epoch, none);
    return;
  }
  // cooperative launch: the runtime guarantees that all `grid` workgroups are resident together (and refuses the launch
  // otherwise) -- what the spin-waits between workgroups rely on when the device is shared with other queues
  int32_t m32 = (int32_t)m, l32 = (int32_t)l, jb32 = (int32_t)jb, j032 = (int32_t)j0;
  int oh = onehop, pl = poll_limit;
  uint32_t eb = epoch_base, mute = wk.mute_epoch;
  unsigned long long* recs = wk.recs;
  int32_t* ipiv = wk.ipiv;
  int32_t* info = wk.info;
  void* args[] = {&Y, &ld, &m32, &l32, &jb32, &j032, &w, &recs, &eb, &ipiv, &info, &oh, &pl, &mute, &none};
  (void)hipLaunchCooperativeKernel((const void*)lu_leaf_kernel<BS, R, false>, dim3(grid), dim3(BS), args, 0, st);
}

// How many workgroups of a leaf kernel (bs threads) one CU holds (registers, LDS, waves), 0 if the query fails: the persistent
// launch needs grid <= that x CUs, or its spin-waits would wait for workgroups that cannot start.
static int leaf_resident_per_cu(const void* kernel, int bs) {
  int nblk = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nblk, kernel, bs, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return nblk;
}
int lu2_resident_per_cu_ov() { return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 8, false, true>, 512); }
int lu2_resident_per_cu(int bs, int rpt) {
  if (bs == 256 && rpt == 1) return leaf_resident_per_cu((const void*)lu_leaf_kernel<256, 1, false>, 256);
  if (bs == 256) return leaf_resident_per_cu((const void*)lu_leaf_kernel<256, 4, false>, 256);
  if (rpt == 4) return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 4, false>, 512);
  return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 8, false>, 512);
}

// ---- the leaf launch of the MULTI-RANK factorization: this rank's rows, G = w.grid workgroups per rank, records exchanged
//      through every rank's peer-mapped buffer.  Launch geometry for shards of at most `pad` rows on `nranks` ranks:
//      nranks * grid <= 256 records, every rank the same (bs, rpt, grid).
bool lu2_mr_config(int64_t pad, int nranks, int ncus, int* bs, int* rpt, int* grid, int* hier, int* ov, int force) {
  *ov = 0;
  if (nranks < 1 || nranks > LU2_MAX_RANKS) return false;
  if (force == 2) {                        // (self-test) two workgroups per rank, the rest of the shard as overflow rows
    if (nranks < 2 || pad <= 2 * 4096 || ncus < 2) return false;
    *bs = 512; *rpt = 8; *grid = 2; *hier = 1; *ov = 1;
    return true;
  }
  // GSI_LU_MR_OV_GRID=k (tests): at most k workgroups per rank, the rest of the shard as overflow rows
  static const int ov_cap = getenv("GSI_LU_MR_OV_GRID") ? atoi(getenv("GSI_LU_MR_OV_GRID")) : 0;
  static const int64_t ov_max = getenv("GSI_LU_OV_MAX") ? atoll(getenv("GSI_LU_OV_MAX")) : ((int64_t)5 << 20);
  if (ov_cap > 0 && nranks > 1 && pad > (int64_t)ov_cap * 4096 && ov_cap <= std::min(256 - nranks, ncus)) {
    *bs = 512; *rpt = 8; *grid = ov_cap; *hier = 1; *ov = 1;
    return true;
  }
  static const int cfg[4][2] = {{256, 1}, {256, 4}, {512, 4}, {512, 8}};
  static const char* he = getenv("GSI_LU_MR_HIER");              // 1: always two hops (tests), 0: never
  const bool force_hier = (he != nullptr && he[0] == '1') || force == 1, no_hier = he != nullptr && he[0] == '0' && force != 1;
  // one hop: every workgroup of every rank is a record of the exchange (nranks * grid <= 256)
  const int gmax = std::min(256 / nranks, ncus);
  for (int c = 0; c < 4 && !force_hier; ++c) {
    const int64_t per = (int64_t)cfg[c][0] * cfg[c][1];
    const int64_t g = (pad + per - 1) / per;
    if (g <= gmax) { *bs = cfg[c][0]; *rpt = cfg[c][1]; *grid = (int)std::max<int64_t>(g, 1); *hier = 0; return true; }
  }
  // two hops: a rank's workgroups reduce among themselves first (grid + nranks <= 256 record slots)
  const int gmax2 = std::min(256 - nranks, ncus);
  for (int c = 0; c < 4 && !no_hier && nranks > 1; ++c) {
    const int64_t per = (int64_t)cfg[c][0] * cfg[c][1];
    const int64_t g = (pad + per - 1) / per;
    if (g <= gmax2) { *bs = cfg[c][0]; *rpt = cfg[c][1]; *grid = (int)std::max<int64_t>(g, 1); *hier = 1; return true; }
  }
  // taller still (up to GSI_LU_OV_MAX rows per rank): every CU a <512, 8> workgroup, two hops, the rows beyond the resident
  // window evaluated lazily (OV)
  if (!no_hier && nranks > 1 && gmax2 >= 1 && pad <= ov_max && !(getenv("GSI_LU_OV") != nullptr && getenv("GSI_LU_OV")[0] == '0')) {
    *bs = 512; *rpt = 8; *grid = gmax2; *hier = 1; *ov = 1;
    return true;
  }
  return false;
}
template <int BS, int R>
static void launch_leaf_mr_t(hipStream_t st, const Lu2MrWork& w, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m,
                             int64_t l, int64_t jb, int64_t j0, int wd, const double* us, uint32_t epoch_base) {
  LuMrArgs a{};
  a.rank = w.rank; a.nranks = w.nranks; a.gbase = (int32_t)row0; a.mtot = (int32_t)m; a.us = us;
  a.hier = w.hier; a.slots = w.hier ? w.grid + w.nranks : w.nranks * w.grid;
  for (int q = 0; q < w.nranks; ++q) a.peer[q] = w.peer[q];
  const int poll_limit = w.poll_limit > 0 ? w.poll_limit : POLL_LIMIT;
  if constexpr (BS == 512 && R == 8) {
    if (w.ov) {                           // shards taller than the grid's registers: overflow rows evaluated lazily
      hipLaunchKernelGGL((lu_leaf_kernel<512, 8, true, true>), dim3(w.grid), dim3(512), 0, st, Y, ld, (int32_t)mloc, (int32_t)l,
                         (int32_t)jb, (int32_t)j0, wd, w.peer[w.rank], epoch_base, w.ipiv, w.info, 1, poll_limit, 0u, a);
      return;
    }
  }
  hipLaunchKernelGGL((lu_leaf_kernel<BS, R, true>), dim3(w.grid), dim3(BS), 0, st, Y, ld, (int32_t)mloc, (int32_t)l, (int32_t)jb,
                     (int32_t)j0, wd, w.peer[w.rank], epoch_base, w.ipiv, w.info, 1, poll_limit, 0u, a);
}
void lu2_leaf_mr(hipStream_t st, const Lu2MrWork& w, double* Y, int64_t ld, int64_t mloc, int64_t row0, int64_t m, int64_t l,
                 int64_t jb, int64_t j0, int wd, const double* us, uint32_t epoch_base) {
  if (w.bs == 256 && w.rpt == 1) launch_leaf_mr_t<256, 1>(st, w, Y, ld, mloc, row0, m, l, jb, j0, wd, us, epoch_base);
  else if (w.bs == 256) launch_leaf_mr_t<256, 4>(st, w, Y, ld, mloc, row0, m, l, jb, j0, wd, us, epoch_base);
  else if (w.rpt == 4) launch_leaf_mr_t<512, 4>(st, w, Y, ld, mloc, row0, m, l, jb, j0, wd, us, epoch_base);
  else launch_leaf_mr_t<512, 8>(st, w, Y, ld, mloc, row0, m, l, jb, j0, wd, us, epoch_base);
}
int lu2_mr_resident_per_cu_ov() { return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 8, true, true>, 512); }
int lu2_mr_resident_per_cu(int bs, int rpt) {
  if (bs == 256 && rpt == 1) return leaf_resident_per_cu((const void*)lu_leaf_kernel<256, 1, true>, 256);
  if (bs == 256) return leaf_resident_per_cu((const void*)lu_leaf_kernel<256, 4, true>, 256);
  if (rpt == 4) return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 4, true>, 512);
  return leaf_resident_per_cu((const void*)lu_leaf_kernel<512, 8, true>, 512);
}
// a rank's exchange buffer: two parity sets of records, two U mailboxes (kp x 8 doubles as granule pairs), two table boxes
// (16 rows x l <= LU2_MR_MAXL columns as granule pairs) for the rows a leaf's pivots exchange between ranks
size_t lu2_mr_record_granules(int nranks, int grid) {
  return (size_t)2 * (size_t)nranks * (size_t)grid * REC + (size_t)2 * (2 * KPMAX * LW) + (size_t)2 * ((size_t)2 * LW * 2 * LU2_MR_MAXL);
}

// lu2_L's workspace: both record sets (the candidates of `grid` workgroups, then the result copies), U12 of every block and
// the pivot rows, in that order
static size_t lu2_record_bytes(int grid) { return sizeof(unsigned long long) * 2 * ((size_t)grid + LU2_RES_COPIES) * REC; }
size_t lu2_work_bytes(int64_t l, int grid) {
  return lu2_record_bytes(grid) + sizeof(double) * (size_t)l * (size_t)l + sizeof(int32_t) * (size_t)(l + 4) + 256;
}
void lu2_carve(Lu2Work& w, int64_t l, void* work) {
  char* base = (char*)work;
  w.recs = (unsigned long long*)base; base += lu2_record_bytes(w.grid);
  w.u12 = (double*)base; base += sizeof(double) * (size_t)l * (size_t)l;   // the U rows of every block, whatever the schedule
  w.ipiv = (int32_t*)base;
}

void lu2_L(hipStream_t st, double* Y, int64_t m, int64_t l, int64_t ld, const Lu2Work& w) {
  // the record tags count pivot steps from 1: clear both record sets
  (void)hipMemsetAsync(w.recs, 0, lu2_record_bytes(w.grid), st);
  uint32_t epoch = 0;
  lu_blocks(st, Y, ld, m, l, w.widths, w.u12, [&](int64_t jb, int, int64_t j0, int wd) {
    // every leaf keeps the same grid: workgroups whose rows lie beyond m still take part in the exchange
    if (w.bs == 256 && w.rpt == 1) launch_leaf<256, 1>(st, w.grid, Y, ld, m, l, jb, j0, wd, w, epoch);
    else if (w.bs == 256) launch_leaf<256, 4>(st, w.grid, Y, ld, m, l, jb, j0, wd, w, epoch);
    else if (w.rpt == 4) launch_leaf<512, 4>(st, w.grid, Y, ld, m, l, jb, j0, wd, w, epoch);
    else launch_leaf<512, 8>(st, w.grid, Y, ld, m, l, jb, j0, wd, w, epoch);
    epoch += (uint32_t)LW;            // a narrow last leaf still runs (gated) 8 steps
  });
#ifdef GSI_LU_TRACE
  if (const char* path = getenv("GSI_LU_TRACE")) {
    unsigned long long h[4 * 8 * 8];
    (void)hipStreamSynchronize(st);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lu_trace), sizeof(h));
    if (FILE* f = fopen(path, "w")) {
      for (int tw = 0; tw < 4; ++tw)
        for (int s = 0; s < 8; ++s) {
          fprintf(f, "wg%d step%d", tw, s);
          for (int ph = 0; ph < 6; ++ph) fprintf(f, " %llu", h[(tw * 8 + s) * 8 + ph]);
          fprintf(f, "\n");
        }
      fclose(f);
    }
  }
#endif
}

}}  // namespace gsi::hipk
