// The quadrature of stochastic Lanczos quadrature (slq_state.hpp) and the coefficient trace (cg_state.hpp's trace_col) as a
// program of its own, for the address and undefined-behaviour sanitizers: every array is a heap block of exactly the size the
// interface promises, on the smallest and the odd shapes (no step, one step, two, a stride of one and of many, a trace that
// stops exactly at qmax and one that goes beyond it), checked against identities that need no eigensolver:
//   * one step: rho0 log(1 / alpha_0);
//   * sum tau_i^2 = 1 and sum tau_i^2 lambda_i = T[0, 0], sum lambda_i = trace T (the QL keeps them);
//   * CG on a diagonal matrix with k distinct entries started from a vector with equal weights: after k steps the rule is
//     exact, rho0 sum_i w_i log(lambda_i).
// tests/test_op_logdet_cpu.py builds and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cg_state.hpp"
#include "slq_state.hpp"

namespace sq = gsi::slq;
namespace cg = gsi::cgst;

static int g_bad = 0;
static void expect(bool ok, const char* what, double a, double b) {
  if (!ok) { std::printf("FAILED %s (%.17g, %.17g)\n", what, a, b); ++g_bad; }
}

// plain CG on diag(lam) from z through cg_state.hpp, b columns (all the same system), traced with qmax
struct Run { std::vector<double> tr, st; int64_t b, qmax; };
static Run traced_cg(const std::vector<double>& lam, const std::vector<double>& z, int64_t b, int64_t qmax, int64_t maxiter) {
  using namespace cg;
  const int64_t n = (int64_t)lam.size();
  Run R;
  R.b = b; R.qmax = qmax;
  R.st.assign(state_doubles(b), 0.0);
  R.tr.assign(trace_doubles(b, qmax), 0.0);
  double* s = R.st.data();
  begin(s, b, 1e-13, maxiter);
  std::vector<std::vector<double>> x(b, std::vector<double>(n, 0.0)), r(b, z), p(b, z), w(b, std::vector<double>(n, 0.0));
  for (int64_t j = 0; j < b; ++j) {
    double bb = 0.0;
    for (int64_t i = 0; i < n; ++i) bb += z[i] * z[i];
    if (j == 1) { for (auto& v : r[j]) v = 0.0; p[j] = r[j]; bb = 0.0; }       // a zero column
    begin_col(s, j, bb);
    trace_begin_col(s, j, R.tr.data(), qmax);
  }
  after_iter(s);
  while (s[H_ACTIVE] > 0.0) {
    for (int64_t j = 0; j < b; ++j) {
      double pq = 0.0, rr = 0.0;
      for (int64_t i = 0; i < n; ++i) { w[j][i] = lam[i] * p[j][i]; pq += p[j][i] * w[j][i]; }
      after_pq(s, j, pq);
      if (colv(s, APPLY, j) != 0.0)
        for (int64_t i = 0; i < n; ++i) { x[j][i] += colv(s, ALPHA, j) * p[j][i]; r[j][i] -= colv(s, ALPHA, j) * w[j][i]; rr += r[j][i] * r[j][i]; }
      after_rr(s, j, rr);
      trace_col(s, j, R.tr.data(), qmax);
      if (colv(s, UPDP, j) != 0.0)
        for (int64_t i = 0; i < n; ++i) p[j][i] = r[j][i] + colv(s, BETA, j) * p[j][i];
    }
    after_iter(s);
  }
  return R;
}

static double quad_of(Run& R, int64_t j) {
  const int64_t b = R.b, qmax = R.qmax;
  std::vector<double> work(sq::work_doubles(b, qmax), 0.0);
  int64_t m = (int64_t)cg::colv(R.st.data(), cg::ITERS, j);
  if (m > qmax) m = qmax;
  double* tr = R.tr.data();
  return sq::quadrature_log(cg::trace_alpha(tr, b, qmax) + j, cg::trace_beta(tr, b, qmax) + j, m, cg::trace_rho0(tr, b, qmax)[j], b,
                            work.data() + j, work.data() + qmax * b + j, work.data() + 2 * qmax * b + j);
}

int main() {
  // no step, one step
  {
    std::vector<double> a(1, 0.25), be(1, 0.0), d(1), e(1), z(1);
    expect(sq::quadrature_log(a.data(), be.data(), 0, 3.0, 1, d.data(), e.data(), z.data()) == 0.0, "zero steps", 0, 0);
    const double v = sq::quadrature_log(a.data(), be.data(), 1, 3.0, 1, d.data(), e.data(), z.data());
    expect(v == 3.0 * std::log(1.0 / 0.25), "one step", v, 3.0 * std::log(4.0));
  }
  // the invariants of the QL on random coefficients, stride 1 and stride 5 (column 3 of 5)
  for (int64_t stride : {1, 5})
    for (int64_t m : {2, 3, 17, 64}) {
      const int64_t off = stride == 1 ? 0 : 3;
      std::vector<double> a((size_t)(m * stride), 0.0), be((size_t)(m * stride), 0.0), d((size_t)(m * stride), 0.0),
          e((size_t)(m * stride), 0.0), z((size_t)(m * stride), 0.0);
      uint64_t g = 88172645463325252ull + (uint64_t)(m * 7 + stride);
      auto rnd = [&]() { g ^= g << 13; g ^= g >> 7; g ^= g << 17; return 0.05 + (double)(g >> 11) / 9007199254740992.0; };
      for (int64_t k = 0; k < m; ++k) { a[(size_t)(k * stride + off)] = rnd(); be[(size_t)(k * stride + off)] = rnd(); }
      sq::tridiagonal(a.data() + off, be.data() + off, m, stride, d.data() + off, e.data() + off);
      double tr = 0.0;
      for (int64_t k = 0; k < m; ++k) tr += d[(size_t)(k * stride + off)];
      const double t00 = d[(size_t)off];
      expect(sq::ql_first_row(d.data() + off, e.data() + off, z.data() + off, m, stride), "ql settles", (double)m, (double)stride);
      double s0 = 0.0, s1 = 0.0, sl = 0.0;
      for (int64_t k = 0; k < m; ++k) {
        const double t = z[(size_t)(k * stride + off)], l = d[(size_t)(k * stride + off)];
        s0 += t * t; s1 += t * t * l; sl += l;
        expect(l > 0.0, "a positive eigenvalue", l, (double)k);
      }
      expect(std::fabs(s0 - 1.0) <= 1e-13, "sum tau^2 = 1", s0, (double)m);
      expect(std::fabs(s1 - t00) <= 1e-12 * std::fabs(t00), "sum tau^2 lambda = T00", s1, t00);
      expect(std::fabs(sl - tr) <= 1e-12 * std::fabs(tr), "sum lambda = trace", sl, tr);
      if (stride == 5)
        for (int64_t k = 0; k < m * stride; ++k)
          if (k % stride != off) expect(d[(size_t)k] == 0.0 && e[(size_t)k] == 0.0 && z[(size_t)k] == 0.0, "a neighbour's word", (double)k, 0);
    }
  // the exact rule: 6 distinct eigenvalues with multiplicities, equal weights
  {
    const double vals[6] = {0.5, 1.0, 2.0, 3.5, 7.0, 11.0};
    std::vector<double> lam, z;
    for (int i = 0; i < 30; ++i) { lam.push_back(vals[i % 6]); z.push_back(1.0); }
    double want = 0.0;
    for (int i = 0; i < 30; ++i) want += std::log(lam[(size_t)i]);
    for (int64_t qmax : {6, 8, 3}) {
      Run R = traced_cg(lam, z, 3, qmax, 100);
      const int64_t it = (int64_t)cg::colv(R.st.data(), cg::ITERS, 0);
      expect(it == 6, "six distinct eigenvalues, six iterations", (double)it, 6);
      expect(cg::colv(R.st.data(), cg::ITERS, 1) == 0.0 && quad_of(R, 1) == 0.0, "a zero column", 0, 0);
      expect(cg::trace_rho0(R.tr.data(), 3, qmax)[0] == 30.0, "rho0", cg::trace_rho0(R.tr.data(), 3, qmax)[0], 30);
      const double v0 = quad_of(R, 0), v2 = quad_of(R, 2);
      expect(v0 == v2, "equal columns", v0, v2);
      if (qmax >= 6) expect(std::fabs(v0 - want) <= 1e-12 * std::fabs(want), "the exact rule", v0, want);
      else expect(std::isfinite(v0) && std::fabs(v0 - want) > 1e-6, "a truncated rule is another number", v0, want);
    }
  }
  if (g_bad) { std::printf("%d checks FAILED\n", g_bad); return 1; }
  std::printf("slq host ok\n");
  return 0;
}
