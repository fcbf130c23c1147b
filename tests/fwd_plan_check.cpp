// Stand-alone check of the segment planner (csrc/fwd_plan.hpp), built by tests/test_pcga_forward_cpu.py with the address and
// undefined-behaviour sanitizers and run as a child process.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fwd_plan.hpp"

static int fails = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++fails; } } while (0)

static void check_plan(const std::vector<int64_t>& lengths, int64_t limit) {
  const int64_t nobs = (int64_t)lengths.size();
  std::vector<int64_t> rowptr((size_t)nobs + 1, 0);
  for (int64_t r = 0; r < nobs; ++r) rowptr[(size_t)r + 1] = rowptr[(size_t)r] + lengths[(size_t)r];
  const int64_t nnz = rowptr[(size_t)nobs];
  const gsi::FwdPlan p = gsi::fwd_plan(rowptr.data(), nobs, limit);
  CHECK((int64_t)p.rowseg.size() == nobs + 1 && p.rowseg[0] == 0, "rowseg shape, limit %lld", (long long)limit);
  CHECK(p.rowseg[(size_t)nobs] == p.nseg(), "rowseg does not end at nseg");
  CHECK(p.segptr[0] == 0 && p.segptr[(size_t)p.nseg()] == nnz, "segments do not span [0, nnz)");
  std::vector<unsigned char> seen((size_t)nnz, 0);
  int64_t nsplit = 0, maxlen = 0;
  for (int64_t r = 0; r < nobs; ++r) {
    const int64_t k0 = p.rowseg[(size_t)r], k1 = p.rowseg[(size_t)r + 1], len = lengths[(size_t)r];
    CHECK(k1 > k0, "row %lld has no segment", (long long)r);
    if (len <= limit) CHECK(k1 - k0 == 1, "unsplit row %lld has %lld segments", (long long)r, (long long)(k1 - k0));
    else CHECK(k1 - k0 == (len + limit - 1) / limit, "row %lld: %lld segments", (long long)r, (long long)(k1 - k0));
    if (k1 - k0 > 1) ++nsplit;
    // contiguous and in order: the first starts at the row's start, each starts where the one before ended
    CHECK(p.segptr[(size_t)k0] == rowptr[(size_t)r], "row %lld: first segment does not start the row", (long long)r);
    CHECK(p.segptr[(size_t)k1] == rowptr[(size_t)r + 1], "row %lld: last segment does not end the row", (long long)r);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t a = p.segptr[(size_t)k], b = p.segptr[(size_t)k + 1];
      CHECK(b >= a && b - a <= limit, "segment %lld has %lld nonzeros, limit %lld", (long long)k, (long long)(b - a),
            (long long)limit);
      if (k1 - k0 > 1) CHECK(b > a, "empty segment %lld in a split row", (long long)k);
      if (b - a > maxlen) maxlen = b - a;
      for (int64_t t = a; t < b; ++t) seen[(size_t)t] += 1;
    }
  }
  for (int64_t t = 0; t < nnz; ++t)
    if (seen[(size_t)t] != 1) { CHECK(false, "nonzero %lld lies in %d segments", (long long)t, (int)seen[(size_t)t]); break; }
  CHECK(nsplit == p.nsplit, "split rows: counted %lld, planner says %lld", (long long)nsplit, (long long)p.nsplit);
  CHECK(maxlen == p.maxlen, "longest segment: %lld against %lld", (long long)maxlen, (long long)p.maxlen);
}

int main() {
  const std::vector<int64_t> lengths = {0, 1, 3, 63, 64, 65, 200, 1000, 1000000, 0, 100, 101, 64, 1};
  for (int64_t limit : {(int64_t)1, (int64_t)64, (int64_t)100, (int64_t)4096}) check_plan(lengths, limit);
  check_plan({0}, 64);
  check_plan({0, 0, 0}, 1);
  check_plan({7}, 7);
  check_plan({8}, 7);
  if (fails) { std::printf("%d planner checks failed\n", fails); return 1; }
  std::printf("planner ok\n");
  return 0;
}
