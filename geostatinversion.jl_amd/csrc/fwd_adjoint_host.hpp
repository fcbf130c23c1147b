// fwd_adjoint_host.hpp -- G = H' V on the host, in the order of the plan of fwd_adjoint_plan.hpp: what runs when the
// backend has no adjoint kernels or GSI_FWD_HOST=1, and the restatement the kernels of fwd_adjoint.hip
// are held to, bit for bit.  Every product and every sum is rounded on its own.
#pragma once
#include <cstdint>
#include "fwd_adjoint_plan.hpp"

namespace gsi { namespace fwd_adjoint_host {

// contributions [e0, e1) of the index against column v of V, from 0.0, in list order
inline double list_sum(const FwdAdjointPlan& ap, int64_t e0, int64_t e1, const double* v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double acc = 0.0;
  for (int64_t e = e0; e < e1; ++e) {
    volatile double p = ap.val[(size_t)e] * v[ap.row[(size_t)e]];     // (volatile: the product is rounded before it is added)
    acc = acc + p;
  }
  return acc;
}

// G (n x b, ld ldg) = H' V (nobs x b, ld ldv), host arrays; every entry of G is written
inline void apply(const FwdAdjointPlan& ap, const double* V, int64_t ldv, int64_t b, double* G, int64_t ldg) {
  for (int64_t c = 0; c < b; ++c) {
    const double* v = V + c * ldv;
    double* g = G + c * ldg;
    for (int64_t j = 0; j < ap.n; ++j) {
      const int64_t e0 = ap.colptr[(size_t)j], e1 = ap.colptr[(size_t)j + 1];
      if (e1 - e0 <= ap.chunk) g[j] = list_sum(ap, e0, e1, v);
    }
    for (int64_t i = 0; i < ap.nlong(); ++i) {
      const int64_t k0 = ap.long_chunk0[(size_t)i], k1 = ap.long_chunk0[(size_t)i + 1];
      double s = list_sum(ap, ap.chunk_off[(size_t)k0], ap.chunk_off[(size_t)k0] + ap.chunk_len[(size_t)k0], v);
      for (int64_t k = k0 + 1; k < k1; ++k)
        s = s + list_sum(ap, ap.chunk_off[(size_t)k], ap.chunk_off[(size_t)k] + ap.chunk_len[(size_t)k], v);
      g[ap.long_col[(size_t)i]] = s;
    }
  }
}

}}  // namespace gsi::fwd_adjoint_host
