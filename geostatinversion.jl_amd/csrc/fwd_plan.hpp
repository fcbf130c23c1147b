// fwd_plan.hpp -- the segment table of a sparse forward model (gsi_fwd).  Host only, no backend:
// the kernels of pcga_forward.hip, the host path of pcga.cpp and a stand-alone test program read the same table.
//
// The nonzeros of the CSR rows are cut into SEGMENTS of at most `limit` nonzeros.  A row of at most `limit` nonzeros
// (an empty one too) is one segment; a longer row of L nonzeros becomes ceil(L / limit) segments of nearly equal length,
// contiguous and in order.  Segments follow each other in row order, so segment k covers nonzeros
// [segptr[k], segptr[k + 1]) and row r owns segments [rowseg[r], rowseg[r + 1]).
#pragma once
#include <cstdint>
#include <vector>

namespace gsi {

struct FwdPlan {
  std::vector<int64_t> segptr;   // nseg + 1
  std::vector<int64_t> rowseg;   // nobs + 1
  int64_t nsplit = 0;            // rows cut into more than one segment
  int64_t maxlen = 0;            // nonzeros of the longest segment
  int64_t nseg() const { return (int64_t)segptr.size() - 1; }
};

// rowptr: nobs + 1 non-decreasing offsets, rowptr[0] = 0 (the caller has checked that); limit >= 1
inline FwdPlan fwd_plan(const int64_t* rowptr, int64_t nobs, int64_t limit) {
  FwdPlan p;
  if (limit < 1) limit = 1;
  p.rowseg.reserve((size_t)nobs + 1);
  p.segptr.reserve((size_t)nobs + 1);
  p.rowseg.push_back(0);
  for (int64_t r = 0; r < nobs; ++r) {
    const int64_t b = rowptr[r], len = rowptr[r + 1] - b;
    const int64_t parts = len <= limit ? 1 : (len + limit - 1) / limit;
    if (parts > 1) p.nsplit += 1;
    // part q of a split row: [b + q len / parts, b + (q + 1) len / parts) -- lengths differ by at most one and none
    // exceeds ceil(len / parts) <= limit
    for (int64_t q = 0; q < parts; ++q) {
      const int64_t s0 = b + (q * len) / parts, s1 = b + ((q + 1) * len) / parts;
      p.segptr.push_back(s0);
      if (s1 - s0 > p.maxlen) p.maxlen = s1 - s0;
    }
    p.rowseg.push_back((int64_t)p.segptr.size());
  }
  p.segptr.push_back(rowptr[nobs]);
  return p;
}

}  // namespace gsi
