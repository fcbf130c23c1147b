// Stand-alone driver of the inverted-index planner (csrc/interp_adjoint_plan.hpp), built by tests/test_interp_adjoint_model.py
// with the address and undefined-behaviour sanitizers and run as a child process:
//   interp_adjoint_check --chunk                       prints the library's chunk limit (IADJ_CHUNK)
//   interp_adjoint_check <case file> <index file> [chunk]
//
// case file: as for fftrf_points_check (8 int64: ndims, N[0], N[1], N[2], m, has_box, row0, m_local; the points; the box).
// index file: 7 int64 (n, m, contributions, nlong, nchunk, maxlen, chunk), then nodeptr (n + 1 int64), point (int32),
// corner (uint8), long_node (int32), long_chunk0 (nlong + 1 int64), chunk_off (int64), chunk_len (int32).
// The program itself checks that every (point, corner) pair appears exactly once, at the node it reaches, and that every
// list is in ascending point order; exit status 1 if not.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "interp_adjoint_plan.hpp"

template <class T>
static void put(const std::vector<T>& v, std::FILE* out) {      // (an empty vector's data() may be null)
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), out);
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "--chunk") == 0) { std::printf("%lld\n", (long long)gsi::IADJ_CHUNK); return 0; }
  if (argc != 3 && argc != 4) { std::printf("usage: interp_adjoint_check <case file> <index file> [chunk]\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int64_t h[8];
  if (std::fread(h, sizeof(int64_t), 8, in) != 8) { std::printf("short header\n"); return 2; }
  const int ndims = (int)h[0];
  const int64_t N[3] = {h[1], h[2], h[3]};
  const int64_t m = h[4], has_box = h[5], row0 = h[6], m_local = h[7];
  const size_t npts = (m > 0 && ndims > 0) ? (size_t)m * (size_t)ndims : 0;
  std::vector<double> pts(npts > 0 ? npts : 1, 0.0), box(has_box && ndims > 0 ? 2 * (size_t)ndims : 1, 0.0);
  if (npts && std::fread(pts.data(), sizeof(double), npts, in) != npts) { std::printf("short points\n"); return 2; }
  if (has_box && std::fread(box.data(), sizeof(double), box.size(), in) != box.size()) { std::printf("short box\n"); return 2; }
  std::fclose(in);
  gsi::FftrfPointsPlan plan;
  const char* why = gsi::fftrf_points_plan(ndims, N, pts.data(), m, has_box ? box.data() : nullptr, row0, m_local, &plan);
  if (why) { std::printf("refused: %s\n", why); return 0; }
  const int64_t chunk = argc == 4 ? std::atoll(argv[3]) : gsi::IADJ_CHUNK;
  const gsi::InterpAdjointPlan ip = gsi::interp_adjoint_plan(plan, chunk);

  const int nc = 1 << ndims;
  const int64_t total = (int64_t)nc * m_local, s1 = plan.N[0], s2 = plan.N[0] * plan.N[1];
  if ((int64_t)ip.nodeptr.size() != ip.n + 1 || ip.nodeptr[0] != 0 || ip.nodeptr[(size_t)ip.n] != total ||
      (int64_t)ip.point.size() != total || (int64_t)ip.corner.size() != total) { std::printf("index shape\n"); return 1; }
  std::vector<uint8_t> seen((size_t)total, 0);
  for (int64_t g = 0; g < ip.n; ++g) {
    if (ip.nodeptr[(size_t)g + 1] < ip.nodeptr[(size_t)g]) { std::printf("nodeptr decreases at %lld\n", (long long)g); return 1; }
    for (int64_t e = ip.nodeptr[(size_t)g]; e < ip.nodeptr[(size_t)g + 1]; ++e) {
      const int64_t p = ip.point[(size_t)e];
      const int k = ip.corner[(size_t)e];
      if (p < 0 || p >= m_local || k >= nc) { std::printf("entry %lld out of range\n", (long long)e); return 1; }
      if (gsi::interp_adjoint_node(plan.base[(size_t)p], k, s1, s2) != g) { std::printf("entry %lld at the wrong node\n", (long long)e); return 1; }
      if (seen[(size_t)(p * nc + k)]++) { std::printf("pair (%lld, %d) twice\n", (long long)p, k); return 1; }
      if (e > ip.nodeptr[(size_t)g] && ip.point[(size_t)e - 1] >= p) { std::printf("list of node %lld out of order\n", (long long)g); return 1; }
    }
  }
  for (int64_t e = 0; e < total; ++e)
    if (!seen[(size_t)e]) { std::printf("pair %lld missing\n", (long long)e); return 1; }

  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::printf("cannot write %s\n", argv[2]); return 2; }
  const int64_t head[7] = {ip.n, ip.m, total, ip.nlong(), ip.nchunk(), ip.maxlen, ip.chunk};
  std::fwrite(head, sizeof(int64_t), 7, out);
  put(ip.nodeptr, out);
  put(ip.point, out);
  put(ip.corner, out);
  put(ip.long_node, out);
  put(ip.long_chunk0, out);
  put(ip.chunk_off, out);
  put(ip.chunk_len, out);
  std::fclose(out);
  std::printf("indexed %lld contributions, %lld long nodes, %lld chunks\n", (long long)total, (long long)ip.nlong(),
              (long long)ip.nchunk());
  return 0;
}
