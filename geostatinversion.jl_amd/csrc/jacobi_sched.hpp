// jacobi_sched.hpp -- the block-pair order of the block Jacobi SVD (jacobi_svd.hip): the round-robin tournament and the
// host-built schedule of a sparse sweep.  Plain C++ (no HIP header needed), so that a host program can test it on its own
// (tests/host/jacobi_sched_main.cpp).
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define GSI_SCHED_HD __device__ __host__
#else
#define GSI_SCHED_HD
#endif

namespace gsi { namespace hipk {

// round-robin ("circle") tournament on n (even) players: pair q of round r
GSI_SCHED_HD inline void rr_pair(int n, int r, int q, int* a, int* b) {
  if (q == 0) { *a = n - 1; *b = r % (n - 1); }
  else {
    *a = (r + q) % (n - 1);
    *b = ((r - q) % (n - 1) + (n - 1)) % (n - 1);
  }
}

// One sparse sweep.  flags: one int per block pair ba <= bb, row-major over the upper triangle (what jacobi_activity_kernel
// writes); non-zero = the pair still holds a column pair to rotate.  Out: the active cross pairs packed greedily into rounds
// of disjoint block pairs, sched = (ba, bb, cross_only) per entry, round after round; round_sizes = entries per round.
// A block whose own (diagonal) pair is active gets its intra-block sweep exactly once: cross_only = 0 sweeps both blocks and
// the cross pairs, so an entry gets it only while neither of its blocks has had that sweep already, and a block that is
// still waiting after the flagged cross pairs are placed is paired with another such block, or else with a block whose own
// pair is clean (sweeping that one again is harmless; such a partner exists, or the waiting blocks come in pairs: nblk is
// even and every other entry with cross_only = 0 took two flagged blocks).  At most npairs = nblk (nblk + 1) / 2 entries.
inline void jacobi_sparse_schedule(const std::vector<int32_t>& flags, int nblk, std::vector<int32_t>& sched,
                                   std::vector<int>& round_sizes) {
  std::vector<char> diag((size_t)nblk, 0), wait((size_t)nblk, 0);
  std::vector<std::array<int32_t, 3>> edges;
  for (int ba = 0, pi = 0; ba < nblk; ++ba)
    for (int bb = ba; bb < nblk; ++bb, ++pi) {
      if (!flags[(size_t)pi]) continue;
      if (ba == bb) { diag[(size_t)ba] = 1; wait[(size_t)ba] = 1; }
      else edges.push_back({ba, bb, 1});
    }
  std::vector<std::vector<std::array<int32_t, 3>>> rounds;
  std::vector<std::vector<char>> used;
  auto place = [&](std::array<int32_t, 3> e) {
    size_t r = 0;
    for (; r < rounds.size(); ++r)
      if (!used[r][(size_t)e[0]] && !used[r][(size_t)e[1]]) break;
    if (r == rounds.size()) { rounds.emplace_back(); used.emplace_back((size_t)nblk, 0); }
    rounds[r].push_back(e);
    used[r][(size_t)e[0]] = 1; used[r][(size_t)e[1]] = 1;
  };
  auto swept = [&](int b) { return diag[(size_t)b] && !wait[(size_t)b]; };   // flagged, and its intra-block sweep is placed
  for (auto& e : edges) {
    if ((wait[(size_t)e[0]] || wait[(size_t)e[1]]) && !swept(e[0]) && !swept(e[1])) {
      e[2] = 0; wait[(size_t)e[0]] = 0; wait[(size_t)e[1]] = 0;
    }
    place(e);
  }
  for (int b = 0; b < nblk; ++b)
    if (wait[(size_t)b]) {                                   // no cross pair brought its sweep along: a partner of its own
      int partner = -1;
      for (int c = b + 1; c < nblk && partner < 0; ++c)
        if (wait[(size_t)c]) partner = c;
      for (int k = 1; k < nblk && partner < 0; ++k)
        if (!diag[(size_t)((b + k) % nblk)]) partner = (b + k) % nblk;
      if (partner < 0) partner = (b + 1) % nblk;             // (not reached: see above)
      wait[(size_t)b] = 0; wait[(size_t)partner] = 0;
      place({std::min(b, partner), std::max(b, partner), 0});
    }
  sched.clear();
  round_sizes.clear();
  for (auto& rd : rounds) {
    round_sizes.push_back((int)rd.size());
    for (auto& e : rd) { sched.push_back(e[0]); sched.push_back(e[1]); sched.push_back(e[2]); }
  }
}

}}  // namespace gsi::hipk
