// The block-pair order of the Jacobi SVD (csrc/jacobi_sched.hpp) checked on the host, on its own: compiled and run by
// tests/test_jacobi_svd_model.py with the address and undefined-behaviour sanitizers.  Exit status 0 and "jacobi-sched-ok" on
// success; the first violated property is printed and ends the run with status 1.
#include "jacobi_sched.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

using gsi::hipk::jacobi_sparse_schedule;
using gsi::hipk::rr_pair;

static int g_checks = 0;

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    ++g_checks;                                              \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "FAILED %s: ", #cond);            \
      std::fprintf(stderr, __VA_ARGS__);                     \
      std::fprintf(stderr, "\n");                            \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

// the tournament meets every block pair exactly once, and every round is disjoint
static void check_tournament(int nblk) {
  std::vector<int> met((size_t)nblk * nblk, 0);
  for (int r = 0; r < nblk - 1; ++r) {
    std::vector<char> used((size_t)nblk, 0);
    for (int q = 0; q < nblk / 2; ++q) {
      int a = -1, b = -1;
      rr_pair(nblk, r, q, &a, &b);
      REQUIRE(a >= 0 && a < nblk && b >= 0 && b < nblk && a != b, "nblk %d round %d slot %d -> (%d, %d)", nblk, r, q, a, b);
      REQUIRE(!used[(size_t)a] && !used[(size_t)b], "nblk %d round %d: block of (%d, %d) twice in the round", nblk, r, a, b);
      used[(size_t)a] = used[(size_t)b] = 1;
      ++met[(size_t)std::min(a, b) * nblk + std::max(a, b)];
    }
  }
  for (int a = 0; a < nblk; ++a)
    for (int b = a + 1; b < nblk; ++b)
      REQUIRE(met[(size_t)a * nblk + b] == 1, "nblk %d: pair (%d, %d) met %d times", nblk, a, b, met[(size_t)a * nblk + b]);
}

static uint64_t mix(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

static void check_schedule(int nblk, const std::vector<int32_t>& flags, const char* what) {
  const int npairs = nblk * (nblk + 1) / 2;
  std::vector<int32_t> sched;
  std::vector<int> round_sizes;
  jacobi_sparse_schedule(flags, nblk, sched, round_sizes);
  REQUIRE((int)sched.size() <= 3 * npairs, "%s nblk %d: %zu ints for %d pairs", what, nblk, sched.size(), npairs);
  REQUIRE(sched.size() % 3 == 0, "%s nblk %d: %zu ints", what, nblk, sched.size());
  size_t total = 0;
  for (int rs : round_sizes) { REQUIRE(rs >= 1, "%s nblk %d: empty round", what, nblk); total += (size_t)rs; }
  REQUIRE(3 * total == sched.size(), "%s nblk %d: rounds hold %zu entries, schedule %zu ints", what, nblk, total, sched.size());
  std::map<std::pair<int, int>, int> seen;
  std::vector<int> full((size_t)nblk, 0);                     // cross_only = 0 entries a block is inside
  size_t off = 0;
  for (int rs : round_sizes) {
    std::vector<char> used((size_t)nblk, 0);
    for (int k = 0; k < rs; ++k, off += 3) {
      const int a = sched[off], b = sched[off + 1], co = sched[off + 2];
      REQUIRE(a >= 0 && a < b && b < nblk && (co == 0 || co == 1), "%s nblk %d: entry (%d, %d, %d)", what, nblk, a, b, co);
      REQUIRE(!used[(size_t)a] && !used[(size_t)b], "%s nblk %d: a block of (%d, %d) twice in one round", what, nblk, a, b);
      used[(size_t)a] = used[(size_t)b] = 1;
      ++seen[std::make_pair(a, b)];
      if (co == 0) { ++full[(size_t)a]; ++full[(size_t)b]; }
    }
  }
  for (int a = 0, pi = 0; a < nblk; ++a)
    for (int b = a; b < nblk; ++b, ++pi) {
      if (!flags[(size_t)pi]) continue;
      if (a == b) {
        REQUIRE(full[(size_t)a] == 1, "%s nblk %d: flagged diagonal block %d inside %d full entries", what, nblk, a, full[(size_t)a]);
      } else {
        const int times = seen[std::make_pair(a, b)];
        REQUIRE(times == 1, "%s nblk %d: flagged pair (%d, %d) scheduled %d times", what, nblk, a, b, times);
      }
    }
}

static size_t pair_index(int nblk, int a, int b) {            // a <= b, row-major over the upper triangle
  return (size_t)a * (size_t)nblk - (size_t)a * (size_t)(a - 1) / 2 + (size_t)(b - a);
}

int main() {
  for (int nblk : {2, 4, 6, 38, 76, 150, 626, 2500}) check_tournament(nblk);
  for (int nblk = 2; nblk <= 44; nblk += 2) {
    const int npairs = nblk * (nblk + 1) / 2;
    std::vector<int32_t> flags((size_t)npairs, 1);
    check_schedule(nblk, flags, "all");
    std::fill(flags.begin(), flags.end(), 0);
    check_schedule(nblk, flags, "none");
    for (int b = 0; b < nblk; ++b) flags[pair_index(nblk, b, b)] = 1;
    check_schedule(nblk, flags, "diagonals only");
    for (int b = 0; b < nblk; ++b) {
      std::fill(flags.begin(), flags.end(), 0);
      flags[pair_index(nblk, b, b)] = 1;
      check_schedule(nblk, flags, "single diagonal");
    }
    std::fill(flags.begin(), flags.end(), 0);                 // everything the last block is part of
    for (int a = 0; a < nblk; ++a) flags[pair_index(nblk, a, nblk - 1)] = 1;
    check_schedule(nblk, flags, "last block only");
  }
  // 2,000 hashed flag sets: the width and the density (1/2 ... 1/64 of the pairs, the diagonals on their own) from the hash too
  for (int s = 0; s < 2000; ++s) {
    const uint64_t h = mix(0x9E3779B97F4A7C15ull * (uint64_t)(s + 1));
    const int nblk = 2 + 2 * (int)(h % 22);                   // 2 ... 44
    const int npairs = nblk * (nblk + 1) / 2;
    const uint64_t den_cross = 2ull << ((h >> 8) % 6), den_diag = 1ull << ((h >> 16) % 4);
    std::vector<int32_t> flags((size_t)npairs, 0);
    for (int a = 0, pi = 0; a < nblk; ++a)
      for (int b = a; b < nblk; ++b, ++pi) {
        const uint64_t g = mix(h + 0xD1B54A32D192ED03ull * (uint64_t)(pi + 1));
        flags[(size_t)pi] = (g % (a == b ? den_diag : den_cross)) == 0 ? 1 : 0;
      }
    check_schedule(nblk, flags, "hashed");
  }
  std::printf("jacobi-sched-ok %d checks\n", g_checks);
  return 0;
}
