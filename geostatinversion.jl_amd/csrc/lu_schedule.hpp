// lu_schedule.hpp -- the block widths of the single-rank panel LU (panel_lu_blocks.hip: lu_blocks).  Host only, no HIP: the
// driver (hip_backend_panels.hip) and the C ABI's gsi_lu_schedule (api.cpp) share it.
//
// A schedule cuts the l columns into blocks; every block but the last is 16, 32, 48 or 64 columns wide (the left-looking
// kernels between the blocks walk the finished columns in 16-column tiles), the last takes what is left, 1 .. 64 columns.
// The chooser minimises the pass model of DESIGN.md 4.2 -- one pass = one read or one write of one panel column -- with
// 8-column leaves, left-looking inside and between the blocks:
//   * a block of s columns: its leaves re-read the kp = 0, 8, 16, ... finished columns of the block: 4 nl (nl - 1), nl = ceil(s / 8)
//     (= s (s / 8 - 1) / 2 for whole leaves);
//   * the update before a block of s columns at column jb > 0: jb columns of L read, the s columns read and written: jb + 2 s;
//   * every block after the first: LU_BLOCK_PASSES for its two launches (below).
// The reads and writes of the leaves' own columns (2 l) are the same for every schedule and left out.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gsi {

constexpr int LU_SCHED_MAX_W = 64;    // widest block (hipk::LU2_NB: the leaf kernel's L11 image)
constexpr int LU_SCHED_TILE = 16;     // every block but the last is a multiple of this

// What one more block costs beside its passes, in passes of the headline panel (10^6 rows).  The kernel trace of the
// uniform-64 build (profiles/r11_bench_kernel_stats.csv) prices the two launches a block adds at one lu_urows_kernel<64> of
// 32.8 us plus the start of one more lu_leftlook_kernel -- about 25 passes IF they were exposed and as long as the 64-column
// ones.  They are neither: the lu phase of the headline step under 18 forced schedules of its 160-column halves
// (profiles/r14_lu_schedule_sweep.jsonl) fits passes x 2.19 us + blocks x (-5.7 us) with 12 us rms, a block
// constant of -2.6 +- 5.6 passes: the stream runs ahead of the device, the U rows of a narrow block take a fraction of the
// 64-row launch (r14_bench_kernel_stats.csv), and a leaf's own latency (its kp x 8 solve) shrinks with the block.  The number
// kept is the floor two back-to-back launches cannot go under, 2 x 2.5 us of dispatch + 8 us of the shortest lu_urows_kernel
// = 13 us = 6 passes; it lies inside the fit's error, and only breaks ties between lists the measurement cannot tell apart.
constexpr int LU_BLOCK_PASSES = 6;

inline int64_t lu_inblock_passes(int s) {
  const int64_t nl = (s + 7) / 8;
  return 4 * nl * (nl - 1);
}
// the cost of a block of s columns that starts at column jb
inline int64_t lu_block_passes(int64_t jb, int s) {
  return lu_inblock_passes(s) + (jb > 0 ? jb + 2 * (int64_t)s + LU_BLOCK_PASSES : 0);
}
inline int64_t lu_schedule_passes(const std::vector<int>& w) {
  int64_t jb = 0, sum = 0;
  for (int s : w) { sum += lu_block_passes(jb, s); jb += s; }
  return sum;
}
// widths a driver can run on an l-column panel: they sum to l, every one 1 .. 64, all but the last multiples of 16
inline bool lu_schedule_valid(int64_t l, const std::vector<int>& w) {
  int64_t sum = 0;
  for (size_t i = 0; i < w.size(); ++i) {
    if (w[i] < 1 || w[i] > LU_SCHED_MAX_W) return false;
    if (i + 1 < w.size() && w[i] % LU_SCHED_TILE != 0) return false;
    sum += w[i];
  }
  return !w.empty() && sum == l;
}
// uniform blocks of nb columns, a narrower last one
inline void lu_schedule_uniform(int64_t l, int nb, std::vector<int>& out) {
  out.clear();
  for (int64_t jb = 0; jb < l; jb += nb) out.push_back((int)((l - jb < nb) ? (l - jb) : nb));
}
// the minimum of the model over all valid schedules; among equal sums the list that is smallest in dictionary order
inline void lu_schedule_model(int64_t l, std::vector<int>& out) {
  out.clear();
  if (l < 1) return;
  // g[t]: the cheapest way to finish from column 16 t on (t = 0 .. T: blocks start on multiples of 16 only)
  const int64_t T = (l - 1) / LU_SCHED_TILE;                    // the last block starts at 16 t for some t <= T
  std::vector<int64_t> g((size_t)T + 1);
  auto step = [&](int64_t t, int s) -> int64_t {               // a block of s columns at 16 t, then the best rest; -1: not possible
    const int64_t jb = t * LU_SCHED_TILE, end = jb + s;
    if (end > l) return -1;
    if (end == l) return lu_block_passes(jb, s);
    if (s % LU_SCHED_TILE != 0) return -1;
    return lu_block_passes(jb, s) + g[(size_t)(end / LU_SCHED_TILE)];
  };
  auto widths = [&](int64_t t, int (&w)[5]) -> int {            // candidates at 16 t, ascending: 16 .. 64 and a ragged last block
    const int64_t left = l - t * LU_SCHED_TILE;
    int n = 0;
    for (int s = LU_SCHED_TILE; s <= LU_SCHED_MAX_W && s <= left; s += LU_SCHED_TILE) w[n++] = s;
    if (left <= LU_SCHED_MAX_W && left % LU_SCHED_TILE != 0) {
      int i = n++;
      for (; i > 0 && w[i - 1] > left; --i) w[i] = w[i - 1];
      w[i] = (int)left;
    }
    return n;
  };
  for (int64_t t = T; t >= 0; --t) {
    int w[5];
    const int n = widths(t, w);
    int64_t best = -1;
    for (int i = 0; i < n; ++i) {
      const int64_t c = step(t, w[i]);
      if (c >= 0 && (best < 0 || c < best)) best = c;
    }
    g[(size_t)t] = best;
  }
  for (int64_t t = 0; t * LU_SCHED_TILE < l;) {
    int w[5];
    const int n = widths(t, w);
    for (int i = 0; i < n; ++i)
      if (step(t, w[i]) == g[(size_t)t]) {
        out.push_back(w[i]);
        t = (t * LU_SCHED_TILE + w[i] + LU_SCHED_TILE - 1) / LU_SCHED_TILE;
        break;
      }
  }
}
// "48,48,64" -> widths; false: not a list of numbers
inline bool lu_schedule_parse(const char* s, std::vector<int>& out) {
  out.clear();
  while (*s) {
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (end == s || v < 1 || v > 1 << 20) return false;
    out.push_back((int)v);
    s = end;
    if (*s == ',') { ++s; if (!*s) return false; }
    else if (*s) return false;
  }
  return !out.empty();
}
// What the driver runs on an l-column panel, knobs read per call:
//   GSI_LU_SCHEDULE=48,48,64  that list, for the panels whose width it sums to (other panels: as if it were not set)
//   GSI_LU_NB=32|64           uniform blocks
//   neither                   the model's minimum
// false: GSI_LU_SCHEDULE is set and is not a list of widths a schedule may hold.
inline bool lu_schedule_choose(int64_t l, std::vector<int>& out) {
  if (const char* e = getenv("GSI_LU_SCHEDULE")) {
    std::vector<int> w;
    if (!lu_schedule_parse(e, w)) return false;
    int64_t sum = 0;
    for (int s : w) sum += s;
    if (!lu_schedule_valid(sum, w)) return false;
    if (sum == l) { out = w; return true; }
  }
  const int nb = getenv("GSI_LU_NB") ? atoi(getenv("GSI_LU_NB")) : 0;
  if (nb == 32 || nb == 64) lu_schedule_uniform(l, nb, out);
  else lu_schedule_model(l, out);
  return true;
}

}  // namespace gsi
