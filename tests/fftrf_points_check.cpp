// Stand-alone driver of the point planner (csrc/fftrf_points.hpp), built by tests/test_fftrf_interp_model.py with the address
// and undefined-behaviour sanitizers and run as a child process:  fftrf_points_check <case file> <plan file>
//
// case file (native endianness):  8 int64: ndims, N[0], N[1], N[2], m, has_box, row0, m_local;  ndims m doubles of points
// (column-major, point i = column i);  2 ndims doubles of box when has_box.
// plan file:  m_local int32 of base, then ndims m_local doubles of frac.  A refusal prints "refused: <reason>" and writes no
// plan file; either way the exit status is 0 unless the files cannot be read or written.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fftrf_points.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::printf("usage: fftrf_points_check <case file> <plan file>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int64_t h[8];
  if (std::fread(h, sizeof(int64_t), 8, in) != 8) { std::printf("short header\n"); return 2; }
  const int ndims = (int)h[0];
  const int64_t N[3] = {h[1], h[2], h[3]};
  const int64_t m = h[4], has_box = h[5], row0 = h[6], m_local = h[7];
  // the planner must refuse m < 1 and a bad ndims itself: hand it exactly what the file holds, never more than that
  const size_t npts = (m > 0 && ndims > 0) ? (size_t)m * (size_t)ndims : 0;
  std::vector<double> pts(npts > 0 ? npts : 1, 0.0), box(has_box && ndims > 0 ? 2 * (size_t)ndims : 1, 0.0);
  if (npts && std::fread(pts.data(), sizeof(double), npts, in) != npts) { std::printf("short points\n"); return 2; }
  if (has_box && std::fread(box.data(), sizeof(double), box.size(), in) != box.size()) { std::printf("short box\n"); return 2; }
  std::fclose(in);
  gsi::FftrfPointsPlan plan;
  const char* why = gsi::fftrf_points_plan(ndims, N, pts.data(), m, has_box ? box.data() : nullptr, row0, m_local, &plan);
  if (why) {
    std::printf("refused: %s\n", why);
    if (!plan.base.empty() || !plan.frac.empty()) { std::printf("a refusal allocated\n"); return 1; }
    return 0;
  }
  if ((int64_t)plan.base.size() != m_local || (int64_t)plan.frac.size() != m_local * ndims) { std::printf("plan shape\n"); return 1; }
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) { std::printf("cannot write %s\n", argv[2]); return 2; }
  std::fwrite(plan.base.data(), sizeof(int32_t), plan.base.size(), out);
  std::fwrite(plan.frac.data(), sizeof(double), plan.frac.size(), out);
  std::fclose(out);
  std::printf("planned %lld points\n", (long long)m_local);
  return 0;
}
