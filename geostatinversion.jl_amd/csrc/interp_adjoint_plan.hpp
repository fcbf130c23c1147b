// interp_adjoint_plan.hpp -- the inverted index of a points plan (fftrf_points.hpp): which (point, corner) pairs reach each
// grid node.  It is what the spread W' X of interp_adjoint.hip walks instead of scattering with atomics.
// Host only, no backend: the kernels (through the arrays built here), api.cpp and a stand-alone test program read the same
// index; tests/interp_adjoint_model.py restates it in numpy and the two agree entry for entry.
//
// Point p with lower corner base[p] reaches 2^d nodes: corner code k (bit a set = the upper neighbour along axis a) is node
//   g = base[p] + (k & 1) + (k >> 1 & 1) N[0] + (k >> 2 & 1) N[0] N[1],   weight prod_a (k bit a ? f_a : 1 - f_a).
// Every N[a] >= 2, so the 2^d nodes of a point are distinct: a point reaches a node through at most one corner.
//   nodeptr (n + 1)     contributions [nodeptr[g], nodeptr[g + 1]) belong to node g; 64-bit: there are 2^d m of them
//   point, corner       of every contribution; within a node in ASCENDING POINT ORDER.  Weights are not stored: the kernel
//                       recomputes them from frac and the corner code.
// A list of more than IADJ_CHUNK contributions is a LONG node: it is cut into chunks of exactly IADJ_CHUNK contributions
// and, where the length is no multiple of it, one shorter remainder, in order.  Each chunk is summed on its own, in list
// order, and the chunk sums are added in chunk order; that fixes the rounding of every output value whatever the launch
// looks like.  A list of at most IADJ_CHUNK contributions is summed in list order and has no entry in the tables below.
//   long_node (nlong)   the long nodes, ascending
//   long_chunk0 (nlong + 1)   chunks [long_chunk0[i], long_chunk0[i + 1]) belong to long node i
//   chunk_off, chunk_len (nchunk)   where each chunk starts in point / corner, and how many contributions it has
#pragma once
#include <cstdint>
#include <vector>
#include "fftrf_points.hpp"

namespace gsi {

constexpr int64_t IADJ_CHUNK = 64;

struct InterpAdjointPlan {
  int ndims = 0;
  int64_t N[3] = {1, 1, 1};
  int64_t n = 0, m = 0;
  int64_t chunk = IADJ_CHUNK;
  std::vector<int64_t> nodeptr;      // n + 1
  std::vector<int32_t> point;        // 2^d m
  std::vector<uint8_t> corner;       // 2^d m
  std::vector<int32_t> long_node;    // nlong
  std::vector<int64_t> long_chunk0;  // nlong + 1
  std::vector<int64_t> chunk_off;    // nchunk
  std::vector<int32_t> chunk_len;    // nchunk
  int64_t maxlen = 0;                // contributions of the longest list
  int64_t nlong() const { return (int64_t)long_node.size(); }
  int64_t nchunk() const { return (int64_t)chunk_off.size(); }
};

// the node a corner of a cell reaches
inline int64_t interp_adjoint_node(int64_t base, int k, int64_t s1, int64_t s2) {
  return base + (k & 1) + ((k >> 1) & 1) * s1 + ((k >> 2) & 1) * s2;
}

// `chunk` (>= 1): the chunk limit; the library uses IADJ_CHUNK, the test program also smaller ones.
inline InterpAdjointPlan interp_adjoint_plan(const FftrfPointsPlan& pts, int64_t chunk = IADJ_CHUNK) {
  InterpAdjointPlan ip;
  if (chunk < 1) chunk = 1;
  const int d = pts.ndims, nc = 1 << d;
  const int64_t m = pts.m_local, s1 = pts.N[0], s2 = pts.N[0] * pts.N[1];
  const int64_t n = pts.N[0] * pts.N[1] * (d == 3 ? pts.N[2] : 1);
  ip.ndims = d; ip.N[0] = pts.N[0]; ip.N[1] = pts.N[1]; ip.N[2] = (d == 3) ? pts.N[2] : 1;
  ip.n = n; ip.m = m; ip.chunk = chunk;
  // counting sort by node; points are visited in ascending order, so every list comes out in ascending point order
  ip.nodeptr.assign((size_t)n + 1, 0);
  for (int64_t p = 0; p < m; ++p)
    for (int k = 0; k < nc; ++k) ip.nodeptr[(size_t)interp_adjoint_node(pts.base[(size_t)p], k, s1, s2) + 1] += 1;
  for (int64_t g = 0; g < n; ++g) ip.nodeptr[(size_t)g + 1] += ip.nodeptr[(size_t)g];
  std::vector<int64_t> cursor(ip.nodeptr.begin(), ip.nodeptr.end() - 1);
  ip.point.assign((size_t)nc * (size_t)m, 0);
  ip.corner.assign((size_t)nc * (size_t)m, 0);
  for (int64_t p = 0; p < m; ++p)
    for (int k = 0; k < nc; ++k) {
      const int64_t at = cursor[(size_t)interp_adjoint_node(pts.base[(size_t)p], k, s1, s2)]++;
      ip.point[(size_t)at] = (int32_t)p;
      ip.corner[(size_t)at] = (uint8_t)k;
    }
  ip.long_chunk0.push_back(0);
  for (int64_t g = 0; g < n; ++g) {
    const int64_t b = ip.nodeptr[(size_t)g], len = ip.nodeptr[(size_t)g + 1] - b;
    if (len > ip.maxlen) ip.maxlen = len;
    if (len <= chunk) continue;
    ip.long_node.push_back((int32_t)g);
    for (int64_t o = 0; o < len; o += chunk) {
      ip.chunk_off.push_back(b + o);
      ip.chunk_len.push_back((int32_t)(len - o < chunk ? len - o : chunk));
    }
    ip.long_chunk0.push_back((int64_t)ip.chunk_off.size());
  }
  return ip;
}

}  // namespace gsi
