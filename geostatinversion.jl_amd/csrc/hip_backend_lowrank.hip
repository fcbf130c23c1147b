// hip_backend_lowrank.hip -- HipBackend's LowRankCovMatrix chains in sample space: the Gram matrix of the samples, randsvd's tail,
// its power steps, and the panel of a power step factored in two column halves (DESIGN.md sections 4.10 - 4.12).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hip_backend_impl.hpp"

namespace gsi {

namespace {

// The shapes the sample-space chains take: what lowrank_tail, lowrank_power_step and lowrank_split_ok all ask of (n, N, l).
// l <= 384 is the limit of the kernels of lowrank_power.hip and of the l x l chains, N <= 4096 that of the N x N products'
// sizing, n >= 2 l leaves rows below the pivot block (and is the first CholeskyQR tier's own gate).
bool sample_space_ok(int64_t n, int64_t N, int64_t l) { return l >= 1 && l <= 384 && N >= 1 && N <= 4096 && n >= 2 * l; }
// ... and what the functions that compose row lists ask besides (the power step, the halves): row numbers are 32-bit there.
// The tail composes none and has never had this bound.
bool row_lists_ok(int64_t n, int64_t N, int64_t l) { return sample_space_ok(n, N, l) && n < ((int64_t)1 << 31); }

// The layout of the row lists hipk::lr_compose writes (ld ldr) for `moved` rows that the interchanges may move and `chk`
// check rows: [0, moved) the moved rows' differences, [o_chk, o_chk + chk) the check rows, [o_sm, o_sm + moved) S[mv]; every
// block starts on a multiple of 8 rows, except that without check rows S[mv] follows the moved rows directly.
struct RowLists { int64_t o_chk, o_sm, ldr; };
RowLists row_lists(int64_t moved, int64_t chk) {
  RowLists r;
  r.o_chk = chk > 0 ? (int64_t)Carve::up8(moved) : moved;
  r.o_sm = r.o_chk + (int64_t)Carve::up8(chk);
  r.ldr = (int64_t)Carve::up8(r.o_sm + moved);
  return r;
}

// Both constants were measured at the headline: with 8 or 16 CUs left free the first kernel behind the
// fork waited for the whole side product; forked at B0 and with the refinement rounds by series, 0.46 n rows at 224 CUs end
// 0.4 ms before M is ready and 0.52 n 0.2 ms after it (in that bracket 0.40, 0.52, 0.58 and 0.64 were slower; with the fork
// alone, a longer chain, 0.52 and 0.58 were the faster ones).
constexpr double TAIL_OVERLAP_FRACTION = 0.46;
constexpr int TAIL_RESERVE_CUS = 32;
constexpr int64_t SPLIT_MAX_L1 = 192;

}  // namespace

// G = S'S of a LowRankCovMatrix's samples: the upper tiles of the general contraction (fixed K split: the same bits on
// every call), mirrored.  2 n N^2 flop less the skipped lower tiles, once per operator (pipeline.cpp caches it).
bool HipBackend::sample_gram(const double* S, int64_t ld, int64_t n, int64_t N, double* G) {
  bind();
  if (n < 1 || N < 1) return false;
  const GemmWs ws = gemm_ws(hipk::gemm_syrk_workspace_doubles(N, n) + 64);
  gemm_syrk_upper("sample_gram", ws, N, n, S, ld, G, N);
  hipk::mirror_upper(st_, G, N);
  check_launch("sample_gram");
  return true;
}
// randsvd after its last panel LU, in sample space (Backend::lowrank_tail).  With A = c S S',
// T = S'L and G = S'S every tall panel of the deferred path is S times an N x l coefficient matrix:
//   Y = S A0, A0 = c T;   CholeskyQR2 of Y: Gram A0'(G A0) -> R1, X1;  A1 = A0 X1 (Q1 = S A1);  Gram A1'(G A1) -> R2, X2
//   W = A'Q1 = S B0, B0 = c G A1;  CholeskyQR2 of W: B0'(G B0) -> RW1, XW1;  B1 = B0 XW1;  B1'(G B1) -> RW2, XW2
//   svd(RW2 RW1 X2) = U S V';  Z = S C,  C = B1 (XW2 U sqrt(S))[:, 0:K]
// -- the operations of qr_thinQ_deferred + op_mul_t + svd_tall_fused with the tall products replaced by N x l ones; one tall
// product (Z, K = N) is left.  Each Gram matrix is the exact one of its panel up to eps |M|^2 |G| (against eps |S M|^2 when
// the panel is formed): the second rounds' check catches a panel whose coefficients grew too large for that to hold.
//
// The overlap.  Between the second Gram round and M = (XW2 U sqrt(S))[:, 0:K] lies a chain of small dependent launches (the
// Gram rounds of W, the Jacobi sweeps) on a few workgroups, and behind it the one tall product.  C = B1 M = B0 (XW1 M), and B0
// = c G A1 is known behind the first product of the second round: Y_f = S[0:n_f] B0 (n_f x l) is formed on the side stream
// while the chain runs, on all but TAIL_RESERVE_CUS CUs (hipk::gemm_f64_nn_capped), and those rows of Z then cost a reduction
// of length l instead of N: Z[0:n_f] = Y_f (XW1 M).  (Not forked earlier: from G A0 the coefficient carries X1, and cond(R1)
// goes into the rows -- 6e-10 in the model of DESIGN.md.  GSI_LOWRANK_TAIL_FORK=late: from B1, behind the fourth round.)  The
// last l - K columns of Z are cleared on the side stream behind the product.  The rows
// from n_f on are the row block of today's product (the same tiles in the same order: the same bits).  n_f is a multiple of
// the contraction's row tile fixed by (n, the fraction), so repeated calls give the same bits.  Y_f goes into `scratch` (the
// caller's dead panel) or a pooled temporary.  On by default where the capped product runs persistent;
// GSI_LOWRANK_TAIL_OVERLAP=0 switches it off, =<fraction in (0, 1)> forces that row fraction on any shape the capped
// launch takes.
bool HipBackend::lowrank_tail(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T, int64_t l,
                              int64_t K, double c, double* Z, int64_t ldz, double* Sv, double* scratch, size_t scratch_doubles) {
  bind();
  if (!cholqr_gate(n, l) || !sample_space_ok(n, N, l) || l > N - 1 || K < 1 || K > l) return false;
  // < 0: the default gate; 0: off; in (0, 1): forced
  static const double ov_env = [] {
    const char* e = getenv("GSI_LOWRANK_TAIL_OVERLAP");
    if (e == nullptr || e[0] == 0) return -1.0;
    const double v = atof(e);
    return (v > 0.0 && v < 1.0) ? v : 0.0;
  }();
  static const int reserve = [] {                          // experiments: the CUs left to the main stream
    const char* e = getenv("GSI_LOWRANK_TAIL_RESERVE_CUS");
    const int v = e ? atoi(e) : TAIL_RESERVE_CUS;
    return (v >= 8 && (v & 7) == 0) ? v : TAIL_RESERVE_CUS;
  }();
  static const bool trace = (getenv("GSI_LOWRANK_POWER_TRACE") != nullptr || getenv("GSI_CQ_SERIES_TRACE") != nullptr);
  static const bool series_off = (getenv("GSI_CQ_SERIES") != nullptr && getenv("GSI_CQ_SERIES")[0] == '0');
  // experiments and the tests: "late" forks where B1 is known (behind the fourth round) instead of at B0
  static const bool fork_late = [] {
    const char* e = getenv("GSI_LOWRANK_TAIL_FORK");
    return e != nullptr && strcmp(e, "late") == 0;
  }();
  const size_t Nl = (size_t)N * l, ll = (size_t)l * l;
  Carve cv;
  const size_t o_A0 = cv.take(Nl), o_A1 = cv.take(Nl), o_P = cv.take(Nl), o_B0 = cv.take(Nl);
  size_t o_Gr[4], o_X[4];
  for (int i = 0; i < 4; ++i) o_Gr[i] = cv.take(ll);
  for (int i = 0; i < 4; ++i) o_X[i] = cv.take(ll);
  const size_t o_R = cv.take(ll), o_Rf = cv.take(ll), o_U = cv.take(ll), o_Mm = cv.take(ll), o_Np = cv.take(ll);
  Scratch buf(this, cv.total);
  const int cap = std::max(8, ((ncus_ - reserve) / 8) * 8);
  int64_t nf = 0;
  if (ov_env != 0.0) {
    nf = (int64_t)((ov_env > 0.0 ? ov_env : TAIL_OVERLAP_FRACTION) * (double)n) / 128 * 128;
    if (nf >= n) nf = (n - 1) / 128 * 128;
  }
  double* A0 = buf.p + o_A0;          // c T
  double* A1 = buf.p + o_A1;          // A0 X1; then B1
  double* P = buf.p + o_P;            // G times the current coefficients; then C
  double* B0 = buf.p + o_B0;          // c G A1: the side stream reads it from the fork to the join, nothing else goes there
  double* Gr[4];                      // the four Gram matrices, each R in place afterwards
  for (int i = 0; i < 4; ++i) Gr[i] = buf.p + o_Gr[i];
  double* X[4];                       // X1, X2, XW1, XW2
  for (int i = 0; i < 4; ++i) X[i] = buf.p + o_X[i];
  double* R = buf.p + o_R;
  double* Rf = buf.p + o_Rf;
  double* U = buf.p + o_U;
  double* Mm = buf.p + o_Mm;
  double* Np = buf.p + o_Np;          // XW1 M (l x K): what Y_f = S[0:n_f] B0 is multiplied by
  size_t gmax = hipk::gemm_workspace_doubles(N, l, N);
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(l, l, N));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, l));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(l, l, l));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(l, K, l));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, K, l));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(n, K, N));
  const double* side_B = fork_late ? A1 : B0;             // the coefficients the side product reads
  if (nf >= 128) {
    // (the capped launch reads its operands' alignment)
    hipk::GemmPlan plan = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool takes = hipk::gemm_f64_nn_capped(st_, nf, l, N, Sm, lds, side_B, N, A1, nf, cap, true, &plan);
    if (!takes || (ov_env < 0.0 && plan.persistent == 0)) nf = 0;
  } else {
    nf = 0;
  }
  Scratch own(this, (nf > 0 && (scratch == nullptr || scratch_doubles < (size_t)nf * (size_t)l)) ? (size_t)nf * (size_t)l : 0);
  double* Yf = (nf > 0) ? (own.p != nullptr ? own.p : scratch) : nullptr;      // nf x l, ld nf
  if (nf > 0) gmax = std::max(gmax, hipk::gemm_workspace_doubles(nf, K, l));
  const GemmWs ws = gemm_ws(gmax + 64);
  SideJoin side(this);                                    // (after every buffer the side stream touches: joined before they go)
  auto fork_side = [&] {
    side.fork();
    (void)hipk::gemm_f64_nn_capped(st2_, nf, l, N, Sm, lds, side_B, N, Yf, nf, cap);     // Y_f = S[0:n_f] B0 (late: B1)
    check_launch("lowrank_tail (side product)");
  };
  // one round on the panel S M: P = G M, Gram = M'P, R = chol(Gram) in place, X = R^-1
  auto round = [&](const double* M, int i, bool check) {
    gemm("lowrank_tail", ws, false, N, l, N, 1.0, G, N, M, N, 0.0, P, N);
    if (i == 1) {
      hipk::scal_copy(st_, (int64_t)N * l, c, P, B0);                                      // W = A'Q1 = S (c G A1) = S B0
      if (nf > 0 && !fork_late) fork_side();
    }
    gemm("lowrank_tail", ws, true, l, l, N, 1.0, M, N, P, N, 0.0, Gr[i], l);
    // (a refinement round: R and X by their series where the Gram matrix is the identity to 6e-6; Rf is free until the SVD)
    (void)hipk::cq_gram_round(st_, Gr[i], l, X[i], check, flags_ + FLAG_CHOLQR, flags_ + FLAG_CQ_SERIES, Rf);
    if (check && trace && !series_off) {                   // (GSI_CQ_SERIES=0: nobody measures the norm)
      double nrm = 0.0;
      HIP_CHECK(hipMemcpyAsync(&nrm, flags_ + FLAG_CQ_SERIES + 2, sizeof(double), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      fprintf(stderr, "lowrank_tail: n %lld N %lld l %lld, refinement round %d: |Gram - I|_F = %.3e (series form up to 6e-6)\n",
              (long long)n, (long long)N, (long long)l, i, nrm);
    }
  };
  phase_begin(PH_QR);
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CQ_SERIES, 0, 4 * sizeof(int32_t), st_));
  hipk::scal_copy(st_, (int64_t)N * l, c, T, A0);                                          // Y = S A0
  round(A0, 0, false);
  gemm("lowrank_tail", ws, false, N, l, l, 1.0, A0, N, X[0], l, 0.0, A1, N);               // Q1 = Y R1^-1 = S A1
  round(A1, 1, true);                                                                       // X2 = R2^-1: Q = Q1 X2; B0, the fork
  round(B0, 2, false);
  gemm("lowrank_tail", ws, false, N, l, l, 1.0, B0, N, X[2], l, 0.0, A1, N);               // W RW1^-1 = S B1
  round(A1, 3, true);
  check_launch("lowrank_tail");
  if (nf > 0 && fork_late) fork_side();
  // (the verdict and the count of series rounds in one copy: FLAG_CHOLQR .. FLAG_CQ_SERIES)
  int32_t verdict[FLAG_CQ_SERIES - FLAG_CHOLQR + 1];
  HIP_CHECK(hipMemcpyAsync(verdict, flags_ + FLAG_CHOLQR, sizeof(verdict), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  if (verdict[0] != 0) {
    side.join();
    phase_end(PH_QR);
    return false;                                         // nothing of Z or Sv written: the caller's path takes over
  }
  // the last l - K columns of Z are zero by definition (RandMatFact.jl:87); nobody else touches them: behind the side product
  // where there is one
  auto clear_rest = [&](hipStream_t st) {
    if (K < l) HIP_CHECK(hipMemsetAsync(Z + (size_t)K * ldz, 0, sizeof(double) * ((size_t)(l - K - 1) * ldz + n), st));
  };
  if (nf > 0) clear_rest(st2_);
  hipk::tri_product(st_, Gr[3], Gr[2], l, R);                                               // R_W = RW2 RW1
  gemm("lowrank_tail", ws, false, l, l, l, 1.0, R, l, X[1], l, 0.0, Rf, l);                // svd(W X2) = svd(R_W X2)
  phase_end(PH_QR);
  n_cholqr_ += 2;
  n_tail_series_rounds_ += verdict[FLAG_CQ_SERIES - FLAG_CHOLQR];
  phase_begin(PH_SVD);
  svd_small(Rf, l, U, Sv);
  hipk::scale_cols_sqrt(st_, U, l, Sv, K);
  phase_end(PH_SVD);
  phase_begin(PH_SMALL_GEMM);
  gemm("lowrank_tail", ws, false, l, K, l, 1.0, X[3], l, U, l, 0.0, Mm, l);                // M = XW2 U sqrt(S), first K columns
  gemm("lowrank_tail", ws, false, N, K, l, 1.0, A1, N, Mm, l, 0.0, P, N);                  // C = B1 M
  if (nf > 0) {
    const double* Mf = Mm;
    if (!fork_late) {
      gemm("lowrank_tail", ws, false, l, K, l, 1.0, X[2], l, Mm, l, 0.0, Np, l);           // B1 M = B0 (XW1 M)
      Mf = Np;
    }
    side.join();
    gemm("lowrank_tail", ws, false, nf, K, l, 1.0, Yf, nf, Mf, l, 0.0, Z, ldz);            // Z[0:n_f] = Y_f (XW1 M) (late: Y_f M)
    gemm_rowblock("lowrank_tail", ws, n, nf, n - nf, K, N, Sm, lds, P, N, Z, ldz);         // Z[n_f:n] = S[n_f:n] C
    ++n_tail_overlaps_;
  } else {
    gemm("lowrank_tail", ws, false, n, K, N, 1.0, Sm, lds, P, N, 0.0, Z, ldz);             // Z = S C
    clear_rest(st_);
  }
  check_launch("lowrank_tail");
  phase_end(PH_SMALL_GEMM);
  return true;
}
// gsi_cq_gram_round: one round of the tail on a Gram matrix of the caller's (the kernel tests)
void HipBackend::cq_gram_round_view(double* Gm, int64_t l, double* X, bool check, int32_t* out2, double* norm_out) {
  bind();
  Scratch tmp(this, (size_t)l * (size_t)l);
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CQ_SERIES, 0, 4 * sizeof(int32_t), st_));
  if (!hipk::cq_gram_round(st_, Gm, l, X, check, flags_ + FLAG_CHOLQR, flags_ + FLAG_CQ_SERIES, tmp.p))
    throw Error(GSI_ERR_ARG, "cq_gram_round: l is beyond the fused Cholesky kernel");
  check_launch("cq_gram_round");
  int32_t w[FLAG_CQ_SERIES - FLAG_CHOLQR + 4];
  HIP_CHECK(hipMemcpyAsync(w, flags_ + FLAG_CHOLQR, sizeof(w), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  out2[0] = w[0];
  out2[1] = w[FLAG_CQ_SERIES - FLAG_CHOLQR + 1];
  memcpy(norm_out, w + (FLAG_CQ_SERIES - FLAG_CHOLQR + 2), sizeof(double));
}
// One power step of the range finder in sample space (Backend::lowrank_power_step).  The LU of
// Y = c S T gives L = P Y U^-1 = (P S) C, C = c T U^-1, so S'L = S'P S C = G C + S'(P - I) S C, and P - I is non-zero on
// the <= 2 l rows the interchanges move.  The factorization keeps its U12 blocks in a workspace, so U is re-formed from the
// l pivot rows: U = L11^-1 (P Y)[0:l] = c L11^-1 S[perm(0:l)] T.  Launches: the interchanges composed into the index lists
// (one workgroup, lowrank_power.hip), one gather (the moved rows' differences D, the check rows -- the pivot rows first --,
// S[mv]), S_piv T (l x l x N), the forward solve for U against the L11 on top of the panel, the solve C U = c T, E =
// [D; S_chk] C, the check, G C (N x l x N), S[mv]' E (N x l x 2l).  The host never sees the pivots: the blocks of moved rows
// are padded to 2 l rows with zero rows, so every offset and launch shape follows from (n, N, l).  One host sync, at the end:
// the check's partial maxima, the LU's info and the invalid-pivot flag in one copy (the caller overwrites the panel that
// holds L after a `true`, so the verdict has to be known).  Fixed shapes and orders, no atomics: repeated calls give the
// same bits.
bool HipBackend::lowrank_power_step(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T,
                                    const int32_t* ipiv, const double* L, int64_t ldl, int64_t l, double c, double* Tn) {
  bind();
  static const bool trace = (getenv("GSI_LOWRANK_POWER_TRACE") != nullptr);
  constexpr int64_t NSAMPLE = 256;        // rows below the pivot block that the check also reads
  constexpr int NPARTS = 128;             // workgroups of the check (partial maxima)
  constexpr double CHECK_MAX = 1e-8;      // |(P S) C - L|max above this: the coefficients no longer reproduce L (declined)
  if (!row_lists_ok(n, N, l)) return false;
  const int64_t ns = std::min<int64_t>(NSAMPLE, n - l), nchk = l + ns;
  // gathered rows (ld ldr): [0, 2l) D = S[perm(mv)] - S[mv]; [o_chk, o_chk + nchk)
  // (P S) of the check rows; [o_sm, o_sm + 2l) S[mv].  Rows past the nmv moved ones, and padding rows, are S[0] - S[0] = 0.
  const RowLists rl = row_lists(2 * l, nchk);
  const int64_t o_chk = rl.o_chk, o_sm = rl.o_sm, nr = o_sm + 2 * l, ldr = rl.ldr;
  const size_t nidx = (size_t)(2 * ldr + nchk);
  // (the index lists, the partial maxima and the verdict lie packed: the read-back below copies the last two as one Verdict)
  Carve cv;
  const size_t o_Mp = cv.take((size_t)l * l), o_Ut = cv.take((size_t)l * l), o_C = cv.take((size_t)N * l),
               o_R = cv.take((size_t)ldr * (size_t)N), o_E = cv.take((size_t)ldr * (size_t)l), o_idx = cv.packed(nidx),
               o_part = cv.packed(NPARTS), o_verdict = cv.packed(2);
  Scratch buf(this, cv.total);
  double* Mp = buf.p + o_Mp;              // S[perm(0:l)] T
  double* Ut = buf.p + o_Ut;              // U' = (c L11^-1 Mp)', on and below its diagonal
  double* C = buf.p + o_C;                // c T U^-1
  double* R = buf.p + o_R;                // the gathered rows
  double* E = buf.p + o_E;                // rows [0, o_chk + nchk) of R times C
  int64_t* idx_dev = reinterpret_cast<int64_t*>(buf.p + o_idx);         // src, sub (ldr each), chk
  double* part = buf.p + o_part;
  int32_t* verdict = reinterpret_cast<int32_t*>(buf.p + o_verdict);     // LU info, invalid pivot, nmv, 0
  const int64_t me = o_chk + nchk;
  size_t gmax = hipk::gemm_workspace_doubles(l, l, N);
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(me, l, N));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, N));
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, 2 * l));
  const GemmWs ws = gemm_ws(gmax + 64);
  struct Verdict { double parts[NPARTS]; int32_t v[4]; };
  if (pin_power_ == nullptr) HIP_CHECK(hipHostMalloc(&pin_power_, sizeof(Verdict), hipHostMallocDefault));
  hipk::lr_compose(st_, ipiv, flags_ + FLAG_LU_INFO, n, l, nchk, o_chk, o_sm, ldr, idx_dev, idx_dev + ldr, idx_dev + 2 * ldr, verdict);
  hipk::lr_gather_rows(st_, Sm, lds, N, idx_dev, idx_dev + ldr, nr, R, ldr);
  gemm("lowrank_power_step", ws, false, l, l, N, 1.0, R + o_chk, ldr, T, N, 0.0, Mp, l);     // S[perm(0:l)] T
  hipk::lr_solve_u(st_, L, ldl, Mp, l, c, Ut);                                               // U = c L11^-1 Mp
  hipk::lr_solve_c(st_, Ut, l, T, N, c, C);                                                  // C U = c T
  gemm("lowrank_power_step", ws, false, me, l, N, 1.0, R, ldr, C, N, 0.0, E, ldr);           // [D; (P S)_chk] C
  hipk::lr_check_rows(st_, E + o_chk, ldr, L, ldl, idx_dev + 2 * ldr, nchk, l, part, NPARTS);
  gemm("lowrank_power_step", ws, false, N, l, N, 1.0, G, N, C, N, 0.0, Tn, N);               // G C
  gemm("lowrank_power_step", ws, true, N, l, 2 * l, 1.0, R + o_sm, ldr, E, ldr, 1.0, Tn, N); // + S[mv]' (D C)
  check_launch("lowrank_power_step");
  const Verdict* h = static_cast<const Verdict*>(pin_power_);
  HIP_CHECK(hipMemcpyAsync(pin_power_, part, sizeof(Verdict), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  double mx = 0.0;
  bool finite = true;
  for (int p = 0; p < NPARTS; ++p) {
    if (!std::isfinite(h->parts[p])) finite = false;
    else mx = std::max(mx, h->parts[p]);
  }
  if (!finite) mx = INFINITY;
  if (trace) fprintf(stderr, "lowrank_power_step: n %lld N %lld l %lld, %lld moved rows, check max |(P S) C - L| = %.3e\n",
                     (long long)n, (long long)N, (long long)l, (long long)h->v[2], mx);
  if (h->v[0] != 0 || h->v[1] != 0) return false;   // a zero pivot (or a lost exchange): the entry point reports it
  return finite && mx <= CHECK_MAX;
}
// ---- the panel of a power step factored in two column halves (Backend::lowrank_split_*) ----
// What the three steps hand to each other lies in ws_split_: the l interchanges of the whole panel, the verdicts of the two
// compositions, and the first half's index lists.  Nothing comes to the host: every launch shape follows from (n, N, l, l1).
struct HipBackend::SplitWs { int32_t* piv; int32_t* verdict1; int32_t* verdict2; int64_t* idx1; int64_t o_chk, o_sm, ldr; };
HipBackend::SplitWs HipBackend::split_ws(int64_t l1) {
  // lr_compose's lists for the first half: the moved rows at 0, its l1 pivot rows at o_chk (no sampled rows), S[mv] at o_sm
  const RowLists rl = row_lists(2 * l1, l1);
  SplitWs w;
  w.o_chk = rl.o_chk; w.o_sm = rl.o_sm; w.ldr = rl.ldr;
  // in bytes: the interchanges [2 SPLIT_MAX_L1], a spare 64, the two verdicts (4 words each) in a slot that ends at 2048,
  // the lists src, sub (up to up8(5 SPLIT_MAX_L1 + 16) rows each) and chk (l1)
  Carve cv;
  const size_t o_piv = cv.take(sizeof(int32_t) * 2 * SPLIT_MAX_L1);
  cv.take(64);
  const size_t o_verdict = cv.take(448);
  const size_t o_idx = cv.take(sizeof(int64_t) * (2 * Carve::up8(5 * SPLIT_MAX_L1 + 16) + SPLIT_MAX_L1));
  grow(ws_split_, cv.total);
  char* base = (char*)ws_split_.p;
  w.piv = (int32_t*)(base + o_piv);
  w.verdict1 = (int32_t*)(base + o_verdict);
  w.verdict2 = w.verdict1 + 4;
  w.idx1 = (int64_t*)(base + o_idx);
  return w;
}
bool HipBackend::lowrank_split_ok(int64_t n, int64_t N, int64_t l, int64_t l1) {
  bind();
  if (l1 < 1 || l1 > SPLIT_MAX_L1 || l <= l1 || l > 2 * l1 || l - l1 < 8 || !row_lists_ok(n, N, l)) return false;
  hipk::Lu2Work w;
  return lu2_takes(n, &w) && lu2_takes(n - l1, &w);
}
void HipBackend::lowrank_split_schur(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* T, const int32_t* ipiv1,
                                     const double* P, int64_t ldp, int64_t l, int64_t l1, double c, double* Tt) {
  bind();
  const int64_t l2 = l - l1;
  const SplitWs w = split_ws(l1);
  const int64_t ld1 = (int64_t)Carve::up8(l1);
  // ([U11' | U12] share one slot of l1 l + 8 doubles: U12 starts on a multiple of 8 behind U11')
  Carve cv;
  const size_t o_R = cv.take((size_t)ld1 * (size_t)N), o_Mp = cv.take((size_t)l1 * l), o_U = cv.take(Carve::up8((size_t)l1 * l) + 8),
               o_C1 = cv.take((size_t)N * l1);
  Scratch buf(this, cv.total);
  double* R = buf.p + o_R;                // S[perm(0:l1)] (l1 x N, ld up8(l1))
  double* Mp = buf.p + o_Mp;              // R T (l1 x l)
  double* Ut11 = buf.p + o_U;             // U11' (l1 x l1), then U12 (l1 x l2)
  double* U12 = Ut11 + Carve::up8((size_t)l1 * l1);
  double* C1 = buf.p + o_C1;              // c T1 U11^-1 (N x l1)
  size_t gmax = hipk::gemm_workspace_doubles(l1, l, N);
  gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l2, l1));
  const GemmWs ws = gemm_ws(gmax + 64);
  int64_t* src = w.idx1, * sub = w.idx1 + w.ldr, * chk = w.idx1 + 2 * w.ldr;
  hipk::lr_compose(st_, ipiv1, flags_ + FLAG_LU_INFO, n, l1, l1, w.o_chk, w.o_sm, w.ldr, src, sub, chk, w.verdict1);
  hipk::lr_pivots(st_, ipiv1, l1, 0, w.piv);                                                  // (the next LU reuses ws_lu_)
  hipk::lr_gather_rows(st_, Sm, lds, N, src + w.o_chk, sub + w.o_chk, l1, R, ld1);
  gemm("lowrank_split_schur", ws, false, l1, l, N, 1.0, R, ld1, T, N, 0.0, Mp, l1);           // S[perm(0:l1)] T
  hipk::lr_solve_u12(st_, P, ldp, Mp, l1, l, c, Ut11, U12);                                   // [U11 | U12] = c L11^-1 Mp
  hipk::lr_solve_c(st_, Ut11, l1, T, N, c, C1);                                               // C1 U11 = c T1
  hipk::scal_copy(st_, N * l2, c, T + (size_t)N * l1, Tt);
  gemm("lowrank_split_schur", ws, false, N, l2, l1, -1.0, C1, N, U12, l1, 1.0, Tt, N);        // c T2 - C1 U12
  check_launch("lowrank_split_schur");
}
void HipBackend::lowrank_split_rows(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1) {
  bind();
  (void)n;
  const int64_t l2 = l - l1;
  const SplitWs w = split_ws(l1);
  Scratch tmp(this, (size_t)(2 * l1) * (size_t)l2);
  hipk::lr_move_rows(st_, P + (size_t)l1 * ldp, ldp, l2, w.idx1, w.idx1 + w.ldr, w.verdict1, 2 * l1, tmp.p, 2 * l1, l1);
  check_launch("lowrank_split_rows");
}
void HipBackend::lowrank_split_join(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1, const int32_t* ipiv2,
                                    int32_t** ipiv) {
  bind();
  const int64_t l2 = l - l1;
  const SplitWs w = split_ws(l1);
  const RowLists rl = row_lists(2 * l2, 0);                // the moved rows at 0 and S[mv] at 2 l2; no check rows
  const int64_t ldr = rl.ldr;
  Carve cv;
  const size_t o_src = cv.take(ldr), o_sub = cv.take(ldr), o_chk = cv.take(8), o_tmp = cv.packed((size_t)(2 * l2) * (size_t)l1);
  Scratch buf(this, cv.total);
  int64_t* src = reinterpret_cast<int64_t*>(buf.p + o_src), * sub = reinterpret_cast<int64_t*>(buf.p + o_sub),
         * chk = reinterpret_cast<int64_t*>(buf.p + o_chk);
  double* tmp = buf.p + o_tmp;
  hipk::lr_compose(st_, ipiv2, flags_ + FLAG_LU_INFO, n - l1, l2, 0, rl.o_chk, rl.o_sm, ldr, src, sub, chk, w.verdict2);
  hipk::lr_pivots(st_, ipiv2, l2, l1, w.piv + l1);
  hipk::lr_move_rows(st_, P + l1, ldp, l1, src, sub, w.verdict2, 2 * l2, tmp, 2 * l2, 0);
  check_launch("lowrank_split_join");
  *ipiv = w.piv;
}
void HipBackend::lowrank_split_undo() {
  bind();
  hipk::lr_forget_zero_pivot(st_, flags_ + FLAG_LU_INFO);
  check_launch("lowrank_split_undo");
}

}  // namespace gsi
