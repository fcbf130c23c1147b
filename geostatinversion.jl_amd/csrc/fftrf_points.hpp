// fftrf_points.hpp -- where scattered points fall on a structured FFTRF grid: the coordinate lookup of FFTRF.interpolate
// (FFTRF.jl:107-129).  Host only, no backend: api.cpp, the kernel of fftrf_interp.hip (through the
// arrays built here) and a stand-alone test program read the same plan.
//
// Axis a of the N[0] x N[1] (x N[2]) field belongs to row a of `points` (d x m, column-major: point i = column i).
//   lo_a, hi_a = the extrema of row a over ALL m points (FFTRF.jl:117), or box[a], box[ndims + a] when a box is given;
//   step_a = (hi_a - lo_a) / (N[a] - 1);
//   t = (x - lo_a) / step_a,  clamped to [0, N[a] - 1]  (the reference's Flat() extrapolation);
//   i = min(floor(t), N[a] - 2),  f = t - i  in [0, 1]: the value is (1 - f) (cell i) + f (cell i + 1) along that axis.
// Every operation is one IEEE double operation in this order; tests/fftrf_interp_model.py restates it in numpy and the
// two plans agree bit for bit.  For the points [row0, row0 + m_local): base[p] = i_0 + N[0] (i_1 + N[1] i_2), the vec()
// index of the cell's lower corner, and frac[a * m_local + p] = f of axis a.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace gsi {

struct FftrfPointsPlan {
  int ndims = 0;
  int64_t N[3] = {1, 1, 1};
  int64_t m_local = 0;
  std::vector<int32_t> base;     // m_local
  std::vector<double> frac;      // ndims x m_local, axis-major
};

// Returns null and fills *plan, or the reason for refusing (nothing has been allocated then).
inline const char* fftrf_points_plan(int ndims, const int64_t* N, const double* points, int64_t m, const double* box,
                                     int64_t row0, int64_t m_local, FftrfPointsPlan* plan) {
  if (ndims != 2 && ndims != 3) return "FFTRF points: unsupported dimension (ndims must be 2 or 3)";
  if (!N || !points || !plan) return "FFTRF points: NULL argument";
  int64_t n = 1;
  for (int a = 0; a < ndims; ++a) {
    if (N[a] < 2) return "FFTRF points: interpolation needs N[a] >= 2 grid points on every axis";
    if (N[a] > (((int64_t)1 << 31) - 1) / n) return "FFTRF points: the grid must have fewer than 2^31 points";
    n *= N[a];
  }
  if (m < 1) return "FFTRF points: need m >= 1 points";
  if (row0 < 0 || m_local < 0 || row0 > m || m_local > m - row0) return "FFTRF points: rows [row0, row0 + m_local) must lie within the m points";
  double lo[3], hi[3], step[3];
  for (int a = 0; a < ndims; ++a) { lo[a] = points[a]; hi[a] = points[a]; }
  for (int64_t i = 0; i < m; ++i)
    for (int a = 0; a < ndims; ++a) {
      const double x = points[i * ndims + a];
      if (!std::isfinite(x)) return "FFTRF points: coordinates must be finite";
      if (x < lo[a]) lo[a] = x;
      if (x > hi[a]) hi[a] = x;
    }
  if (box) {
    for (int a = 0; a < 2 * ndims; ++a)
      if (!std::isfinite(box[a])) return "FFTRF points: box entries must be finite";
    for (int a = 0; a < ndims; ++a) {
      if (box[ndims + a] < box[a]) return "FFTRF points: box must have hi >= lo on every axis";
      lo[a] = box[a];
      hi[a] = box[ndims + a];
    }
  }
  for (int a = 0; a < ndims; ++a) {
    const double ext = hi[a] - lo[a];
    step[a] = ext / (double)(N[a] - 1);
    if (!(ext > 0.0) || !std::isfinite(ext) || !(step[a] > 0.0))
      return "FFTRF points: the extent hi - lo of every axis must be positive and finite";
  }
  plan->ndims = ndims;
  plan->N[0] = N[0]; plan->N[1] = N[1]; plan->N[2] = (ndims == 3) ? N[2] : 1;
  plan->m_local = m_local;
  plan->base.assign((size_t)m_local, 0);
  plan->frac.assign((size_t)m_local * ndims, 0.0);
  for (int64_t p = 0; p < m_local; ++p) {
    int64_t idx = 0, stride = 1;
    for (int a = 0; a < ndims; ++a) {
      const double top = (double)(N[a] - 1);
      double t = (points[(row0 + p) * ndims + a] - lo[a]) / step[a];
      t = t > 0.0 ? t : 0.0;
      t = t < top ? t : top;
      double fl = std::floor(t);
      if (fl > top - 1.0) fl = top - 1.0;
      plan->frac[(size_t)a * m_local + p] = t - fl;
      idx += (int64_t)fl * stride;
      stride *= N[a];
    }
    plan->base[(size_t)p] = (int32_t)idx;
  }
  return nullptr;
}

}  // namespace gsi
