// fwd_adjoint_plan.hpp -- the inverted index (CSC) of a sparse forward model (gsi_fwd): which nonzeros of the CSR matrix H
// reach each grid cell.  It is what the adjoint G = H' V of fwd_adjoint.hip walks instead of scattering with atomics
// (DESIGN.md 4.6l).  Host only, no backend: the kernels (through the arrays built here), the host path of
// fwd_adjoint_host.hpp and a stand-alone test program read the same index; tests/fwd_adjoint_model.py restates it in numpy
// and the two agree entry for entry.
//
// Nonzero t of row r, column j = colidx[t], contributes (row r, value fl(vals[t] * w[j])) to cell j -- the value rounded once,
// here; without weights it is vals[t] itself.  Repeated indices inside a row stay separate contributions.
//   colptr (n + 1)      contributions [colptr[j], colptr[j + 1]) belong to cell j; 64-bit
//   row, val (nnz)      of every contribution; within a cell by ASCENDING ROW and, within a row, in storage order (the
//                       counting sort below visits the nonzeros in storage order, so this is what comes out)
// A list of more than FADJ_CHUNK contributions is a LONG column: it is cut into chunks of exactly FADJ_CHUNK contributions
// and, where the length is no multiple of it, one shorter remainder, in order.  Each chunk is summed on its own, in list
// order, and the chunk sums are added in chunk order; that fixes the rounding of every output value whatever the launch
// looks like.  A list of at most FADJ_CHUNK contributions is summed in list order and has no entry in the tables below.
//   long_col (nlong)    the long columns, ascending
//   long_chunk0 (nlong + 1)   chunks [long_chunk0[i], long_chunk0[i + 1]) belong to long column i
//   chunk_off, chunk_len (nchunk)   where each chunk starts in row / val, and how many contributions it has
//
// FADJ_CHUNK.  One lane walks one list, so a wave of the cell pass runs as long as the longest list among its 64 cells and
// a wave of the chunk pass as long as its longest chunk: the limit bounds the serial walk of any wave.  The split rule for
// sums through an inverted index -- cut lists longer than a quarter of one wave's share of the contributions -- gives, for
// 4096 rays of 1024 cells over 10^6 cells (4.2 10^6 contributions, 8192 waves in flight), 512 contributions per wave and a
// limit of 128 per WAVE; a lane's walk is serial where a wave's is 64 wide, so the limit per lane has to sit well below
// that, and above the lists that ordinary geometries produce (ray and block models: a few to a few tens per cell), which
// should take the single pass.  32 does both: a chunk is at most 4 to 8 average cell-pass walks at that shape.
#pragma once
#include <cstdint>
#include <vector>

namespace gsi {

constexpr int64_t FADJ_CHUNK = 32;

struct FwdAdjointPlan {
  int64_t n = 0, nobs = 0, nnz = 0;
  int64_t chunk = FADJ_CHUNK;
  std::vector<int64_t> colptr;       // n + 1
  std::vector<int32_t> row;          // nnz
  std::vector<double> val;           // nnz
  std::vector<int32_t> long_col;     // nlong
  std::vector<int64_t> long_chunk0;  // nlong + 1
  std::vector<int64_t> chunk_off;    // nchunk
  std::vector<int32_t> chunk_len;    // nchunk
  int64_t maxlen = 0;                // contributions of the longest list
  int64_t nlong() const { return (int64_t)long_col.size(); }
  int64_t nchunk() const { return (int64_t)chunk_off.size(); }
};

// rowptr (nobs + 1), colidx / vals (rowptr[nobs]) as gsi_fwd_linear_create has checked them (indices in [0, n), nobs and
// n < 2^31); w: n weights or null.  `chunk` (>= 1): the chunk limit; the library uses FADJ_CHUNK, the test program also
// smaller ones.  O(nnz + n).
inline FwdAdjointPlan fwd_adjoint_plan(int64_t nobs, int64_t n, const int64_t* rowptr, const int32_t* colidx,
                                       const double* vals, const double* w, int64_t chunk = FADJ_CHUNK) {
  FwdAdjointPlan ap;
  if (chunk < 1) chunk = 1;
  const int64_t nnz = rowptr[nobs];
  ap.n = n; ap.nobs = nobs; ap.nnz = nnz; ap.chunk = chunk;
  // counting sort by cell; rows are visited in ascending order and a row's nonzeros in storage order
  ap.colptr.assign((size_t)n + 1, 0);
  for (int64_t t = 0; t < nnz; ++t) ap.colptr[(size_t)colidx[t] + 1] += 1;
  for (int64_t j = 0; j < n; ++j) ap.colptr[(size_t)j + 1] += ap.colptr[(size_t)j];
  std::vector<int64_t> cursor(ap.colptr.begin(), ap.colptr.end() - 1);
  ap.row.assign((size_t)nnz, 0);
  ap.val.assign((size_t)nnz, 0.0);
  for (int64_t r = 0; r < nobs; ++r)
    for (int64_t t = rowptr[r]; t < rowptr[r + 1]; ++t) {
      const int64_t j = colidx[t];
      const int64_t at = cursor[(size_t)j]++;
      ap.row[(size_t)at] = (int32_t)r;
      volatile double v = w ? vals[t] * w[j] : vals[t];     // (volatile: one rounding to double, whatever the host's flags)
      ap.val[(size_t)at] = v;
    }
  ap.long_chunk0.push_back(0);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t b = ap.colptr[(size_t)j], len = ap.colptr[(size_t)j + 1] - b;
    if (len > ap.maxlen) ap.maxlen = len;
    if (len <= chunk) continue;
    ap.long_col.push_back((int32_t)j);
    for (int64_t o = 0; o < len; o += chunk) {
      ap.chunk_off.push_back(b + o);
      ap.chunk_len.push_back((int32_t)(len - o < chunk ? len - o : chunk));
    }
    ap.long_chunk0.push_back((int64_t)ap.chunk_off.size());
  }
  return ap;
}

}  // namespace gsi
