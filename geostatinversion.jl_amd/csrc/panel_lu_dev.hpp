// panel_lu_dev.hpp -- what the forms of `F = lu(Y); Q = F.L` (RandMatFact.jl:60-61, 68-69, 72-73) share.  Internal: only the
// panel_lu_*.hip files include it (the public declarations are in hip_common.hpp).
//   panel_lu_leaf.hip      resident leaves: one persistent launch per 8-column leaf, the leaf's values in registers
//   panel_lu_streamed.hip  streamed leaves: panels taller than the register file
//   panel_lu_blocks.hip    the updates between the blocks (16 .. 64 columns: lu_schedule.hpp), and the block loop the two forms above run their leaves in
//   panel_lu_sharded.hip   step primitives of the row-sharded form, the interchanges across ranks
// Every form finds LAPACK dgetrf's pivots (first maximal |entry| wins), leaves L in pivoted row order and does the same
// operations on the same values in the same order: the factors are bit-identical between the forms.
// The device helpers sit in an unnamed namespace: every file that includes this compiles (and inlines) its own.
#pragma once
#include "hip_common.hpp"
#include "lu_schedule.hpp"
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <vector>

namespace gsi { namespace hipk {

namespace {

constexpr int LW = LU2_LEAF;           // leaf width (columns kept in registers)
constexpr int KPMAX = LU2_NB - LW;     // deepest pending update inside a block
constexpr int LSP = KPMAX + 1;         // padded row stride of the L11 image
constexpr int REC = LU2_REC_GRANULES;  // 8-byte granules per published record (512 B): unit u = granules 2u (low half), 2u + 1
constexpr int POLL_LIMIT = 4000000;    // default poll budget (~ seconds): a record that never arrives ends the launch with info = -1

__device__ inline double readlane_d(double x, int srclane) {   // srclane wave-uniform
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_readlane(lo, srclane);
  hi = __builtin_amdgcn_readlane(hi, srclane);
  return __hiloint2double(hi, lo);
}
// idamax over the wave: the largest value (values are >= 0 or the "no candidate" marker -1, never NaN), then the
// SMALLEST row among the lanes that hold it (first maximal entry wins, like LAPACK); "no candidate" rows are -1 =
// 0xFFFFFFFF and lose every tie.  All lanes end with the result.  DPP row shifts / broadcasts (register-file speed:
// the whole reduction is ~40 VALU instructions), not ds_bpermute shuffles -- 12 dependent LDS round trips measured
// 0.66 us per reduction, 2-3 of them on the critical path of every pivot step.
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_fmax(double v) {
  // the two halves move as 32-bit integers (the builtin is an integer builtin: a double argument would be VALUE-converted);
  // lanes without a source lane keep the identity -1.0 = 0xbff00000'00000000
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)0xbff00000, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return fmax(v, __hiloint2double(hi, lo));
}
template <int CTRL, int ROW_MASK>
__device__ inline uint32_t dpp_umin(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, CTRL, ROW_MASK, 0xf, false);
  return o < v ? o : v;
}
__device__ inline void wave_argmax(double& v, int32_t& i) {
  double mx = v;
  mx = dpp_fmax<0x111, 0xf>(mx);   // row_shr:1
  mx = dpp_fmax<0x112, 0xf>(mx);   // row_shr:2
  mx = dpp_fmax<0x114, 0xf>(mx);   // row_shr:4
  mx = dpp_fmax<0x118, 0xf>(mx);   // row_shr:8   -> lane 15 of every row holds the row's maximum
  mx = dpp_fmax<0x142, 0xa>(mx);   // row_bcast:15 into rows 1 and 3
  mx = dpp_fmax<0x143, 0xc>(mx);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's maximum
  mx = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mx), 63), __builtin_amdgcn_readlane(__double2loint(mx), 63));
  uint32_t key = (v == mx) ? (uint32_t)i : 0xFFFFFFFFu;
  key = dpp_umin<0x111, 0xf>(key);
  key = dpp_umin<0x112, 0xf>(key);
  key = dpp_umin<0x114, 0xf>(key);
  key = dpp_umin<0x118, 0xf>(key);
  key = dpp_umin<0x142, 0xa>(key);
  key = dpp_umin<0x143, 0xc>(key);
  v = mx;
  i = (int32_t)__builtin_amdgcn_readlane((int)key, 63);
}

// the same over entries that sit in lanes 0 .. 7 only (per-wave candidates of a workgroup, <= 8 waves): three
// shifts inside row 0, result read from lane 7
__device__ inline void wave_argmax8(double& v, int32_t& i) {
  double mx = v;
  mx = dpp_fmax<0x111, 0xf>(mx);
  mx = dpp_fmax<0x112, 0xf>(mx);
  mx = dpp_fmax<0x114, 0xf>(mx);
  mx = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(mx), 7), __builtin_amdgcn_readlane(__double2loint(mx), 7));
  uint32_t key = (v == mx) ? (uint32_t)i : 0xFFFFFFFFu;
  key = dpp_umin<0x111, 0xf>(key);
  key = dpp_umin<0x112, 0xf>(key);
  key = dpp_umin<0x114, 0xf>(key);
  v = mx;
  i = (int32_t)__builtin_amdgcn_readlane((int)key, 7);
}

// a record granule as a poller reads it: agent scope within one GPU, system scope when peers on other GPUs wrote it
template <bool MR>
__device__ inline unsigned long long poll_granule(const unsigned long long* p) {
  if constexpr (MR) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What a poll that ran out was waiting for: written once per factorization into info[2 .. 5] = {phase, slot, epoch, who}
// (phase 1: U mailbox of rank 0, 2: record heads, 3: the winner's row values, 4: the ranks' result heads (two-hop exchange),
// 5: their row values, 6: row boxes of the interchange kernel; who = rank * 1024 + workgroup).  take_error puts it into
// the message: "never launched" (epoch of a leaf's first step) and "stopped mid-leaf" are different bugs.
__device__ inline void lu_timeout_note(int32_t* info, int phase, int slot, uint32_t epoch, int who) {
  if (atomicCAS(info + 2, 0, phase) == 0) { info[3] = slot; info[4] = (int32_t)epoch; info[5] = who; }
}

}  // namespace

// what a multi-rank launch (the leaf kernel, the interchange kernel of panel_lu_sharded.hip) knows about the other ranks
struct LuMrArgs {
  int rank, nranks;
  int hier;                                  // two-hop exchange for shards too tall for nranks x grid <= 256 records (lu_leaf_kernel)
  int slots;                                 // record slots of the exchange: nranks * grid, or (hier) grid + nranks
  int32_t gbase, mtot;
  const double* us;                          // kp x LW, [c * LW + k]
  unsigned long long* peer[LU2_MAX_RANKS];   // every rank's record buffer (peer[rank] == recs)
};

// The block loop of the single-rank forms (panel_lu_blocks.hip).  Every block [jb, jb + b) of the schedule `widths`
// (lu_schedule.hpp: lu_schedule_valid): brought up to date with the columns to its left, leaf(jb, b, j0, wd) for each of its
// leaves [j0, j0 + wd) of <= LW columns in turn, its U rows for every trailing column (u12: l * l doubles, the U rows of the
// panel at [row + column * l]).  Then the top l x l becomes L's (unit diagonal, zeros above).
using LuLeafFn = std::function<void(int64_t jb, int b, int64_t j0, int wd)>;
void lu_blocks(hipStream_t st, double* Y, int64_t ld, int64_t m, int64_t l, const std::vector<int>& widths, double* u12,
               const LuLeafFn& leaf);

}}  // namespace gsi::hipk
