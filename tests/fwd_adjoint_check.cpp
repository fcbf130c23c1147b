// fwd_adjoint_check.cpp -- stand-alone check of the inverted index of a forward model (csrc/fwd_adjoint_plan.hpp) and of the
// host sum in its order (csrc/fwd_adjoint_host.hpp), built by tests/test_fwd_adjoint_model.py with the address and
// undefined-behaviour sanitizers.  Host code only.
//   fwd_adjoint_check --chunk            prints FADJ_CHUNK
//   fwd_adjoint_check --self             random and crafted CSR inputs, chunk limits 1, 2, 3 and FADJ_CHUNK, against an
//                                        O(nnz n) brute force; prints "checked <cases>"
//   fwd_adjoint_check case.bin out.bin [chunk]
//       case.bin: int64 nobs, n, nnz, has_w; int64 rowptr[nobs + 1]; int64 colidx[nnz]; double vals[nnz]; double w[n] if has_w
//       out.bin:  int64 nlong, nchunk, maxlen; colptr; row (as int64); val; long_col (as int64); long_chunk0; chunk_off;
//                 chunk_len (as int64)                                       prints "indexed <nnz>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "fwd_adjoint_host.hpp"

using namespace gsi;

static int fail(const std::string& what) {
  std::fprintf(stderr, "fwd_adjoint_check: %s\n", what.c_str());
  return 1;
}

struct Csr {
  int64_t nobs = 0, n = 0;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> colidx;
  std::vector<double> vals, w;
};

// every property of the index, against a scan of all nonzeros per cell; then the host sum against the same scan
static int check(const Csr& H, int64_t chunk, std::mt19937_64& rng) {
  const double* w = H.w.empty() ? nullptr : H.w.data();
  const FwdAdjointPlan ap = fwd_adjoint_plan(H.nobs, H.n, H.rowptr.data(), H.colidx.data(), H.vals.data(), w, chunk);
  const int64_t nnz = H.rowptr[(size_t)H.nobs];
  if (ap.n != H.n || ap.nobs != H.nobs || ap.nnz != nnz || ap.chunk != chunk) return fail("sizes");
  if ((int64_t)ap.colptr.size() != H.n + 1 || ap.colptr[0] != 0 || ap.colptr[(size_t)H.n] != nnz) return fail("colptr ends");
  if ((int64_t)ap.row.size() != nnz || (int64_t)ap.val.size() != nnz) return fail("row / val sizes");
  if ((int64_t)ap.long_chunk0.size() != ap.nlong() + 1 || ap.chunk_len.size() != ap.chunk_off.size()) return fail("table sizes");
  const int b = 3;
  std::normal_distribution<double> nd;
  std::vector<double> V((size_t)H.nobs * b), G((size_t)H.n * b, -7.0);
  for (double& v : V) v = nd(rng);
  fwd_adjoint_host::apply(ap, V.data(), H.nobs, b, G.data(), H.n);
  int64_t ilong = 0, maxlen = 0;
  for (int64_t j = 0; j < H.n; ++j) {
    // brute force: the contributions of cell j by ascending row and, within a row, in storage order
    std::vector<int32_t> rows;
    std::vector<double> vals;
    for (int64_t r = 0; r < H.nobs; ++r)
      for (int64_t t = H.rowptr[(size_t)r]; t < H.rowptr[(size_t)r + 1]; ++t)
        if (H.colidx[(size_t)t] == j) {
          rows.push_back((int32_t)r);
          volatile double v = w ? H.vals[(size_t)t] * w[j] : H.vals[(size_t)t];
          vals.push_back((double)v);
        }
    const int64_t len = (int64_t)rows.size(), e0 = ap.colptr[(size_t)j];
    if (ap.colptr[(size_t)j + 1] - e0 != len) return fail("list length of cell " + std::to_string(j));
    for (int64_t e = 0; e < len; ++e)
      if (ap.row[(size_t)(e0 + e)] != rows[(size_t)e] || std::memcmp(&ap.val[(size_t)(e0 + e)], &vals[(size_t)e], 8) != 0)
        return fail("entry " + std::to_string(e) + " of cell " + std::to_string(j));
    if (len > maxlen) maxlen = len;
    if (len > chunk) {
      if (ilong >= ap.nlong() || ap.long_col[(size_t)ilong] != j) return fail("long column " + std::to_string(j) + " not listed");
      const int64_t k0 = ap.long_chunk0[(size_t)ilong], k1 = ap.long_chunk0[(size_t)ilong + 1];
      if (k1 - k0 != (len + chunk - 1) / chunk) return fail("chunk count of cell " + std::to_string(j));
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t o = (k - k0) * chunk;
        if (ap.chunk_off[(size_t)k] != e0 + o || ap.chunk_len[(size_t)k] != (len - o < chunk ? len - o : chunk))
          return fail("chunk " + std::to_string(k - k0) + " of cell " + std::to_string(j));
      }
      ilong += 1;
    }
    // the sum: each chunk from 0.0 in list order, the chunk sums in chunk order (one chunk when the list is short)
    for (int c = 0; c < b; ++c) {
      double s = 0.0;
      for (int64_t o = 0; o < len || o == 0; o += chunk) {
        double acc = 0.0;
        for (int64_t e = o; e < len && e < o + chunk; ++e) {
          volatile double p = vals[(size_t)e] * V[(size_t)rows[(size_t)e] + (size_t)c * H.nobs];
          acc = acc + p;
        }
        s = (o == 0) ? acc : s + acc;
      }
      const double got = G[(size_t)j + (size_t)c * H.n];
      if (std::memcmp(&got, &s, 8) != 0) return fail("sum of cell " + std::to_string(j) + " column " + std::to_string(c));
      if (len == 0 && (got != 0.0 || std::signbit(got))) return fail("an untouched cell is not +0.0");
    }
  }
  if (ilong != ap.nlong()) return fail("more long columns listed than there are");
  if (maxlen != ap.maxlen) return fail("maxlen");
  return 0;
}

static Csr random_csr(int64_t nobs, int64_t n, int64_t maxrow, bool weights, std::mt19937_64& rng, int64_t hot = -1) {
  Csr H;
  H.nobs = nobs; H.n = n;
  H.rowptr.push_back(0);
  std::normal_distribution<double> nd;
  for (int64_t r = 0; r < nobs; ++r) {
    const int64_t len = (r % 5 == 3) ? 0 : (int64_t)(rng() % (uint64_t)(maxrow + 1));       // every fifth row is empty
    for (int64_t t = 0; t < len; ++t) {
      int64_t j = (int64_t)(rng() % (uint64_t)n);
      if (hot >= 0 && t % 2 == 0) j = hot;                                                   // half of the row in one cell
      if (t == len - 1 && len >= 3) j = H.colidx[H.colidx.size() - 2];                       // a repeated index
      H.colidx.push_back((int32_t)j);
      H.vals.push_back(nd(rng));
    }
    H.rowptr.push_back((int64_t)H.colidx.size());
  }
  if (weights) for (int64_t j = 0; j < n; ++j) H.w.push_back(1.0 + 0.1 * nd(rng));
  return H;
}

static int self_check() {
  std::mt19937_64 rng(20240611);
  const int64_t chunks[4] = {1, 2, 3, FADJ_CHUNK};
  int cases = 0;
  for (int64_t chunk : chunks) {
    for (int rep = 0; rep < 3; ++rep) {
      const int64_t nobs = 1 + (int64_t)(rng() % 60), n = 1 + (int64_t)(rng() % 50);
      for (int weights = 0; weights < 2; ++weights) {
        if (check(random_csr(nobs, n, 9, weights != 0, rng), chunk, rng)) return 1;
        if (check(random_csr(nobs, n, 9, weights != 0, rng, n / 2), chunk, rng)) return 1;
        cases += 2;
      }
    }
    // crafted: nothing at all; one row, one cell; every row in cell 0 and in the last cell; 3 chunk + 5 rows in one cell
    Csr E; E.nobs = 4; E.n = 3; E.rowptr.assign(5, 0);
    if (check(E, chunk, rng)) return 1;
    Csr one; one.nobs = 1; one.n = 1; one.rowptr = {0, 2}; one.colidx = {0, 0}; one.vals = {1.5, -0.25};
    if (check(one, chunk, rng)) return 1;
    Csr fan; fan.nobs = 3 * chunk + 5; fan.n = 7;
    fan.rowptr.push_back(0);
    for (int64_t r = 0; r < fan.nobs; ++r) {
      fan.colidx.push_back(6); fan.vals.push_back(1.0 + (double)r);
      fan.colidx.push_back(0); fan.vals.push_back(-2.0);
      if (r < chunk) { fan.colidx.push_back(3); fan.vals.push_back(0.5); }          // exactly chunk: not long
      if (r <= chunk) { fan.colidx.push_back(4); fan.vals.push_back(0.25); }        // chunk + 1: two chunks
      fan.rowptr.push_back((int64_t)fan.colidx.size());
    }
    if (check(fan, chunk, rng)) return 1;
    const FwdAdjointPlan ap = fwd_adjoint_plan(fan.nobs, fan.n, fan.rowptr.data(), fan.colidx.data(), fan.vals.data(), nullptr, chunk);
    if (ap.nlong() != 3 || ap.long_col[0] != 0 || ap.long_col[1] != 4 || ap.long_col[2] != 6) return fail("crafted long columns");
    const int64_t per_fan = (3 * chunk + 5 + chunk - 1) / chunk;
    if (ap.nchunk() != 2 * per_fan + 2 || ap.maxlen != 3 * chunk + 5) return fail("crafted chunk count");
    cases += 3;
  }
  std::printf("checked %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--chunk") { std::printf("%lld\n", (long long)FADJ_CHUNK); return 0; }
  if (argc == 2 && std::string(argv[1]) == "--self") return self_check();
  if (argc < 3) return fail("usage: fwd_adjoint_check --chunk | --self | case.bin out.bin [chunk]");
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open the case file");
  int64_t head[4];
  if (std::fread(head, 8, 4, f) != 4) return fail("short case file");
  Csr H;
  H.nobs = head[0]; H.n = head[1];
  const int64_t nnz = head[2];
  H.rowptr.resize((size_t)H.nobs + 1);
  std::vector<int64_t> ci((size_t)nnz);
  H.vals.resize((size_t)nnz);
  if (head[3]) H.w.resize((size_t)H.n);
  if (std::fread(H.rowptr.data(), 8, H.rowptr.size(), f) != H.rowptr.size() || std::fread(ci.data(), 8, ci.size(), f) != ci.size() ||
      std::fread(H.vals.data(), 8, H.vals.size(), f) != H.vals.size() || std::fread(H.w.data(), 8, H.w.size(), f) != H.w.size())
    return fail("short case file");
  std::fclose(f);
  for (int64_t v : ci) H.colidx.push_back((int32_t)v);
  const int64_t chunk = argc > 3 ? std::atoll(argv[3]) : FADJ_CHUNK;
  std::mt19937_64 rng(1);
  if (check(H, chunk, rng)) return 1;
  const FwdAdjointPlan ap = fwd_adjoint_plan(H.nobs, H.n, H.rowptr.data(), H.colidx.data(), H.vals.data(),
                                             H.w.empty() ? nullptr : H.w.data(), chunk);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return fail("cannot open the output file");
  auto put64 = [&](const std::vector<int64_t>& v) { if (!v.empty()) std::fwrite(v.data(), 8, v.size(), o); };
  auto widen = [](const std::vector<int32_t>& v) { return std::vector<int64_t>(v.begin(), v.end()); };
  put64({ap.nlong(), ap.nchunk(), ap.maxlen});
  put64(ap.colptr);
  put64(widen(ap.row));
  if (!ap.val.empty()) std::fwrite(ap.val.data(), 8, ap.val.size(), o);
  put64(widen(ap.long_col));
  put64(ap.long_chunk0);
  put64(ap.chunk_off);
  put64(widen(ap.chunk_len));
  std::fclose(o);
  std::printf("indexed %lld\n", (long long)nnz);
  return 0;
}
