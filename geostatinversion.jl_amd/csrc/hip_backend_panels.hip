// hip_backend_panels.hip -- HipBackend's panel factorizations: the panel LU on one rank and sharded over ranks, the three QR tiers,
// the fused tall SVD, and the small factorizations behind them (Jacobi SVD, Cholesky, triangular solve).
#include <algorithm>
#include <cstdlib>
#include "hip_backend_impl.hpp"
#include "lu_schedule.hpp"

namespace gsi {

// ---- panels ----
void HipBackend::lu_L(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host) {
  lu_L_impl(Y, m, l, ld, ipiv_host, nullptr);
}
// every form below leaves its interchanges in ws_lu_ (untouched until the next factorization): no form declines
bool HipBackend::lu_L_keep(double* Y, int64_t m, int64_t l, int64_t ld, int32_t** ipiv_dev) {
  if (ipiv_dev == nullptr) return false;
  lu_L_impl(Y, m, l, ld, nullptr, ipiv_dev);
  return true;
}
void HipBackend::lu_L_impl(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host, int32_t** ipiv_dev_out) {
  bind();
  // Panels of up to 4096 rows per CU: leaves held in registers (panel_lu_leaf.hip), left-looking updates between the
  // blocks (panel_lu_blocks.hip).  Everything else takes the streamed leaves below (panel_lu_streamed.hip).
  hipk::Lu2Work w2;
  // Panels taller than the register file holds (up to GSI_LU_OV_MAX rows, default 5 x 2^20): the resident kernel on all
  // CUs with the rows beyond its window evaluated lazily out of L2 / Infinity Cache / HBM; beyond that the streamed leaves
  // win (measured cross-over: 6e6 rows at l = 320).  GSI_LU_OV=0 switches it off (A/B).
  static const int64_t ov_max = getenv("GSI_LU_OV_MAX") ? atoll(getenv("GSI_LU_OV_MAX")) : ((int64_t)5 << 20);
  static const bool ov_off = (getenv("GSI_LU_OV") != nullptr && getenv("GSI_LU_OV")[0] == '0');
  bool fits = lu2_takes(m, &w2);
  if (!fits && lu2_resident_ok() && !ov_off && m <= ov_max && ncus_ >= 1) {
    const int g = std::min(ncus_, 256);
    if (m > (int64_t)g * 4096) {
      if (lu2_ov_resident_ < 0) lu2_ov_resident_ = hipk::lu2_resident_per_cu_ov();
      if ((int64_t)lu2_ov_resident_ * ncus_ >= g) { w2.bs = 512; w2.rpt = 8; w2.grid = g; w2.ov = true; fits = true; }
    }
  }
  int32_t* ipiv_dev = nullptr;
  if (fits) {
    // test / A-B knobs, read per call: GSI_LU_POLL_LIMIT (polls before a workgroup gives up), GSI_LU_TEST_MUTE_EPOCH
    // (one workgroup stays silent at that pivot step: exercises the info = -1 path), GSI_LU_COOPERATIVE=1
    if (const char* e = getenv("GSI_LU_POLL_LIMIT")) w2.poll_limit = atoi(e);
    if (const char* e = getenv("GSI_LU_TEST_MUTE_EPOCH")) w2.mute_epoch = (uint32_t)atoi(e);
    if (const char* e = getenv("GSI_LU_COOPERATIVE")) w2.cooperative = (e[0] == '1');
    // the block widths: GSI_LU_SCHEDULE=48,48,64 (a list for the panels it sums to), GSI_LU_NB=32|64 (uniform), else the
    // minimum of the pass model (lu_schedule.hpp)
    if (!lu_schedule_choose(l, w2.widths)) throw Error(GSI_ERR_ARG, "lu: GSI_LU_SCHEDULE is not a list of block widths (16, 32, 48, 64; a last block of 1 .. 64)");
    grow(ws_lu_, hipk::lu2_work_bytes(l, w2.grid));
    hipk::lu2_carve(w2, l, ws_lu_.p);
    w2.info = flags_ + FLAG_LU_INFO;
    hipk::lu2_L(st_, Y, m, l, ld, w2);
    check_launch("lu2_L");
    ipiv_dev = w2.ipiv;
  } else {
    // Everything the resident kernel does not take -- panels the register file cannot hold (more than 4096 rows per CU), a
    // context that lost co-residency once, a leaf grid that does not fit the chip: streamed leaves with lazily evaluated
    // candidates (same blocks, pivots and arithmetic; no spin-waits between workgroups).  GSI_LU_TALL=1 forces it for any
    // height (tests: bit-identical to the resident kernel).  (Round 1's per-column sweeps, the fall-back behind these through
    // round 4, are kept as tools/rejected_kernels/panel_lu_round1_sweeps.hip.txt.)
    if (m >= ((int64_t)1 << 31)) throw Error(GSI_ERR_ARG, "lu: panels of 2^31 rows and more are not supported");
    grow(ws_lu_, hipk::lu3_work_bytes(l));
    hipk::lu3_L(st_, Y, m, l, ld, ws_lu_.p, flags_ + FLAG_LU_INFO, &ipiv_dev);
    check_launch("lu3_L");
  }
  if (ipiv_dev_out) *ipiv_dev_out = ipiv_dev;
  if (ipiv_host) {
    HIP_CHECK(hipMemcpyAsync(ipiv_host, ipiv_dev, sizeof(int32_t) * l, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
}
// Ranks that SHARE this device (the RCCL-free communicators, one-GPU rehearsals of a multi-GPU job) each factor their
// replicated panel with a whole-chip grid of their own: the grids cannot all be resident, so the persistent kernels are
// not candidates at all (seen: 2 rank processes on one GPU, gathered 10^6 x 320 panel: a poll time-out on some runs).
bool HipBackend::lu2_resident_ok() const {
  static const bool tall_first = (getenv("GSI_LU_TALL") != nullptr && getenv("GSI_LU_TALL")[0] == '1');
  return !tall_first && !lu2_lost_ && ranks_sharing_device_ <= 1;
}
bool HipBackend::lu2_takes(int64_t m, hipk::Lu2Work* w) {
  return lu2_resident_ok() && hipk::lu2_config(m, ncus_, &w->bs, &w->rpt, &w->grid) && lu2_fits(w->bs, w->rpt, w->grid);
}
// The persistent leaf kernel spins on records of ALL its workgroups: the grid must fit the chip at this kernel's
// occupancy (registers, LDS, waves).  Queried once per instantiation; a panel that does not fit takes the streamed leaves.
bool HipBackend::lu2_fits(int bs, int rpt, int grid) {
  const int key = bs * 16 + rpt;
  auto it = lu2_resident_.find(key);
  if (it == lu2_resident_.end()) it = lu2_resident_.emplace(key, hipk::lu2_resident_per_cu(bs, rpt)).first;
  return (int64_t)it->second * ncus_ >= grid;
}
// ---- row-sharded LU primitives ----
struct HipBackend::LusWs { double* pval; int64_t* pidx; int32_t* ipiv; };
HipBackend::LusWs HipBackend::lus_ws(int64_t, int64_t l) {
  // fixed layout, in bytes: pivots (l <= 8188), then the per-workgroup partial arg-maxes (<= 1024 workgroups), 64 spare
  if (l > 8188) throw Error(GSI_ERR_ARG, "sharded lu: sketch width too large");
  Carve c;
  const size_t o_ipiv = c.take(32768), o_pval = c.take(sizeof(double) * 1024), o_pidx = c.take(sizeof(int64_t) * 1024);
  c.take(64);
  grow(ws_lus_, c.total);
  char* base = (char*)ws_lus_.p;
  LusWs w;
  w.ipiv = (int32_t*)(base + o_ipiv);
  w.pval = (double*)(base + o_pval);
  w.pidx = (int64_t*)(base + o_pidx);
  return w;
}
void HipBackend::lus_u12_leaf(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12) {
  bind();
  hipk::lus_u12_leaf(st_, Yloc, ld, row0, jb, j0, w, U12);
  check_launch("lus_u12_leaf");
}
void HipBackend::lus_pending(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w,
                             const double* U12) {
  bind();
  if (mloc > 0) hipk::lus_pending(st_, Yloc, ld, mloc, row0, jb, j0, w, U12);
  check_launch("lus_pending");
}
void HipBackend::lus_candidate(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j, double* rec) {
  bind();
  LusWs w = lus_ws(mloc, l);
  // the previous pivot step's apply kernel may already have left this column's per-workgroup partials (same panel, same rows)
  const bool ready = (lus_part_col_ == j && lus_part_Y_ == Yloc && lus_part_mloc_ == mloc);
  lus_part_col_ = -1;
  hipk::lus_candidate(st_, Yloc, ld, mloc, row0, l, j, rec, w.pval, w.pidx, ready);
  check_launch("lus_candidate");
}
void HipBackend::lus_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t j0, int s, int w,
                           const double* recs, int nranks) {
  bind();
  LusWs ws = lus_ws(mloc, l);
  static const bool fuse = (getenv("GSI_LUS_NO_FUSE") == nullptr);      // A/B knob
  const bool next = fuse && (s + 1 < w) && mloc > 0;
  hipk::lus_apply(st_, Yloc, ld, mloc, row0, m, l, j0, s, w, recs, nranks, ws.ipiv, flags_ + FLAG_LU_INFO, next ? ws.pval : nullptr,
                  next ? ws.pidx : nullptr);
  check_launch("lus_apply");
  lus_part_col_ = next ? j0 + s + 1 : -1;
  lus_part_Y_ = Yloc;
  lus_part_mloc_ = mloc;
}
void HipBackend::lus_u12_block(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                               double* U12) {
  bind();
  hipk::lus_u12_block(st_, Yloc, ld, row0, jb, b, c0, c1, U12);
  check_launch("lus_u12_block");
}
void HipBackend::lus_rankk(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
                           const double* U12) {
  bind();
  hipk::lus_rankk(st_, Yloc, ld, mloc, row0, jb, b, c0, t, U12);
  check_launch("lus_rankk");
}
void HipBackend::lus_finish(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l) {
  bind();
  hipk::lus_finish(st_, Yloc, ld, mloc, row0, l);
}
bool HipBackend::lus_mr_begin(Comm* comm, int64_t m, int64_t l) {
  bind();
  auto no = [&](const std::string& why) { mr_reason_ = why; return false; };
  if (comm == nullptr) return no("no communicator");
  // First use over this communicator: the record buffer is created and exchanged BEFORE any rank-local veto below, so
  // that every rank enters the collective inside share_pointers (a rank that skipped it would leave its peers in it).
  if (mr_comm_ != comm && !mr_share_tried_) {
    mr_share_tried_ = true;
    if (comm->nranks <= hipk::LU2_MAX_RANKS) {
      if (mr_recs_ == nullptr) {
        const size_t bytes = sizeof(unsigned long long) * hipk::lu2_mr_record_granules(1, 256);   // 256 records + mailboxes
        if (hipExtMallocWithFlags((void**)&mr_recs_, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
          (void)hipGetLastError();
          HIP_CHECK(hipMalloc((void**)&mr_recs_, bytes));
        }
        HIP_CHECK(hipMemsetAsync(mr_recs_, 0, bytes, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
        mr_epoch_ = 0;
      }
      void* all[hipk::LU2_MAX_RANKS] = {nullptr};
      if (comm->share_pointers(mr_recs_, 0, all)) {
        for (int g = 0; g < comm->nranks; ++g) mr_peer_[g] = (unsigned long long*)all[g];
        mr_comm_ = comm;
      } else {
        mr_disabled_ = true;
        mr_why_disabled_ = "the ranks' record buffers could not be mapped into each other (share_pointers)";
      }
    }
    lus_ws(1, 1);                        // the pivot / partial-arg-max workspace exists before any leaf is launched
  }
  static const bool off = (getenv("GSI_LU_NO_MR") != nullptr);
  if (off) return no("GSI_LU_NO_MR is set");
  if (mr_disabled_) return no("switched off on this context: " + mr_why_disabled_);
  if (mr_comm_ != comm) return no("another communicator owns this context's record buffers");
  if (comm->nranks > hipk::LU2_MAX_RANKS) return no("more than " + std::to_string(hipk::LU2_MAX_RANKS) + " ranks");
  if (m >= ((int64_t)1 << 28) || l > hipk::LU2_MR_MAXL) return no("panel too tall (2^28 rows) or too wide (" + std::to_string(hipk::LU2_MR_MAXL) + " columns)");
  const int G = comm->nranks;
  const int64_t pad = (m + G - 1) / G;
  hipk::Lu2MrWork w{};
  // Ranks that share this device (possible only with the RCCL-free communicators): ALL their leaf grids must be resident
  // together, and residency is decided per SHADER ENGINE (8 CUs; 4 per XCD) -- the workgroups of a launch are dealt
  // round-robin over the 8 XCDs and, inside an XCD, over its 4 engines, so a grid of g one-per-CU workgroups puts
  // ceil(ceil(g / 8) / 4) on the first engines.  Measured with rank processes on one GPU: 2 x 123, 4 x 62, 3 x 40, 2 x 100
  // workgroups run; 3 x 74, 3 x 80 and 3 x 82 time out (3 x 3 = 9 workgroups on engines of 8 CUs) although 222-246 <= 256.
  const int sharing = std::max(comm->ranks_on_my_device(), 1);
  const int se_cus = std::max(ncus_ / 32, 1);                        // CUs per shader engine (8)
  const int per_se = sharing > 1 ? std::max(se_cus / sharing, 0) : se_cus;
  if (per_se < 1)
    return no(std::to_string(sharing) + " ranks share this device, more than the " + std::to_string(se_cus) +
              " CUs of a shader engine: their persistent leaf grids cannot all be resident");
  if (!hipk::lu2_mr_config(pad, G, sharing > 1 ? per_se * 32 : ncus_, &w.bs, &w.rpt, &w.grid, &w.hier, &w.ov, mr_force_))
    return no("no launch geometry for shards of " + std::to_string(pad) + " rows on " + std::to_string(G) + " ranks (" +
              std::to_string(sharing) + " sharing this device)");
  const int key = 1000000 + w.bs * 16 + w.rpt + (w.ov ? 100000 : 0);
  auto it = lu2_resident_.find(key);
  if (it == lu2_resident_.end())
    it = lu2_resident_.emplace(key, w.ov ? hipk::lu2_mr_resident_per_cu_ov() : hipk::lu2_mr_resident_per_cu(w.bs, w.rpt)).first;
  if (sharing > 1 ? (int64_t)sharing * ((((w.grid + 7) / 8) + 3) / 4) > (int64_t)se_cus * it->second
                  : (int64_t)it->second * ncus_ < (int64_t)w.grid)
    return no("the leaf grids (" + std::to_string(w.grid) + " workgroups per rank, " + std::to_string(sharing) +
              " ranks on this device) would not all be resident");
  w.rank = comm->rank; w.nranks = G;
  for (int g = 0; g < G; ++g) w.peer[g] = mr_peer_[g];
  w.info = flags_ + FLAG_LU_INFO;
  if (const char* e = getenv("GSI_LU_POLL_LIMIT")) w.poll_limit = atoi(e);
  mr_work_ = w;
  mr_reason_.clear();
  return true;
}
int64_t HipBackend::lus_mr_signature() {
  return ((((int64_t)mr_work_.bs * 64 + mr_work_.rpt) * 1024 + mr_work_.grid) * 2 + mr_work_.hier) * 2 + mr_work_.ov;
}
// Every kernel of the persistent-leaf factorization once, on private dummies (a 64-row panel, a record buffer of its
// own, its own info word), with the geometry flags of the form that is about to run: what a first launch may cost the
// runtime -- loading the code object, growing the queue's scratch (the overflow-row leaves spill) -- happens here,
// before the ranks' barrier, and not while a peer's leaf spins for this rank's launch.  Once per instantiation.
void HipBackend::lus_mr_warmup() {
  bind();
  const int64_t key = (((int64_t)mr_work_.bs * 64 + mr_work_.rpt) * 2 + mr_work_.hier) * 2 + mr_work_.ov;
  if (mr_warm_.count(key)) return;
  mr_warm_.insert(key);
  const int64_t R = 256, Cc = 128;
  const size_t rec_doubles = hipk::lu2_mr_record_granules(1, 4);
  Scratch D(this, (size_t)R * Cc + 64), U(this, (size_t)64 * 128), recs(this, rec_doubles);
  hipk::randn_fill(st_, D.p, (size_t)R * Cc, 0x77a12eull);
  HIP_CHECK(hipMemsetAsync(D.p + R * Cc, 0, 64 * sizeof(double), st_));
  HIP_CHECK(hipMemsetAsync(recs.p, 0, rec_doubles * sizeof(double), st_));
  hipk::Lu2MrWork w = mr_work_;
  w.rank = 0; w.nranks = 1; w.grid = 1;
  w.peer[0] = (unsigned long long*)recs.p;
  w.info = (int32_t*)(D.p + R * Cc);
  w.ipiv = (int32_t*)(D.p + R * Cc + 16);
  hipk::lu2_leaf_mr(st_, w, D.p, R, 64, 0, 64, 8, 0, 0, 8, nullptr, 0);
  hipk::lus_swap_peer(st_, w, D.p, R, 64, 0, 64, 8, 0, 8, 0);
  hipk::lus_u12_block(st_, D.p, R, 0, 0, 64, 64, 128, U.p);
  hipk::lus_rankk(st_, D.p, R, R, 0, 0, 64, 64, 64, U.p);
  hipk::lus_u12_block(st_, D.p, R, 0, 0, 32, 32, 64, U.p);
  hipk::lus_rankk(st_, D.p, R, R, 0, 0, 32, 32, 32, U.p);
  hipk::lus_finish(st_, D.p, R, R, 0, 8);
  hipk::lu_flag_export(st_, w.info, U.p);
  hipk::lu_flag_import(st_, w.info, U.p);
  check_launch("lus_mr_warmup");
  HIP_CHECK(hipStreamSynchronize(st_));
}
void HipBackend::lu_flag_export(double* flag) {
  bind();
  hipk::lu_flag_export(st_, flags_ + FLAG_LU_INFO, flag);
}
void HipBackend::lu_flag_import(const double* flag) {
  bind();
  hipk::lu_flag_import(st_, flags_ + FLAG_LU_INFO, flag);
  check_launch("lu_flag_import");
}
void HipBackend::lus_leaf_mr(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t jb, int64_t j0, int w,
                             const double* U12) {
  bind();
  mr_work_.ipiv = lus_ws(mloc, l).ipiv;
  hipk::lu2_leaf_mr(st_, mr_work_, Yloc, ld, mloc, row0, m, l, jb, j0, w, U12, mr_epoch_);
  // the rows this leaf's pivots exchange, in the columns outside the leaf: peer pushes + polls, no collective
  static const bool host_swaps = (getenv("GSI_LU_MR_HOST_SWAPS") != nullptr);      // A/B: pack + all-reduce + apply instead
  mr_peer_swaps_ = !host_swaps;
  if (mr_peer_swaps_) hipk::lus_swap_peer(st_, mr_work_, Yloc, ld, mloc, row0, m, l, j0, w, mr_epoch_);
  mr_epoch_ += (uint32_t)hipk::LU2_LEAF;
  mr_in_flight_ = true;
  check_launch("lu2_leaf_mr");
}
void HipBackend::lus_swap_pack(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                               double* table) {
  bind();
  hipk::lus_swap_pack(st_, Yloc, ld, mloc, row0, l, j0, w, lus_ws(mloc, l).ipiv, table);
  check_launch("lus_swap_pack");
}
void HipBackend::lus_swap_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                                const double* table) {
  bind();
  if (mloc > 0) hipk::lus_swap_apply(st_, Yloc, ld, mloc, row0, l, j0, w, lus_ws(mloc, l).ipiv, table);
  check_launch("lus_swap_apply");
}
void HipBackend::lus_pivots(int32_t* host, int64_t l) {
  bind();
  LusWs w = lus_ws(1, l);
  HIP_CHECK(hipMemcpyAsync(host, w.ipiv, sizeof(int32_t) * l, hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
}
// ---- the first CholeskyQR tier, as qr_thinQ, qr_thinQ_deferred and svd_tall_fused all try it ----
bool HipBackend::cholqr_gate(int64_t m, int64_t l) {
  static const bool no_cholqr = (getenv("GSI_NO_CHOLQR") != nullptr);
  return !no_cholqr && l <= 1024 && m >= 2 * l;
}
// contraction workspace: the Gram matrix (upper tiles, or the dedicated kernel's slab partials), Y R^-1, the l x l inverse
size_t HipBackend::cholqr_ws_doubles(int64_t m, int64_t l) {
  return std::max({hipk::gemm_workspace_doubles(l, l, m), hipk::gemm_syrk_workspace_doubles(l, m), hipk::syrk_upper_workspace_doubles(l, m),
                   hipk::gemm_workspace_doubles(m, l, l), hipk::gemm_workspace_doubles(l, 32, l)});
}
// Both rounds out of place: Y is read only, T = Y R1^-1 (ld ldt) and the small factors are what a true leaves behind.  A
// false sets the caller's hint: the next eight factorizations of this kind do not try this tier.
bool HipBackend::cholqr2_try(const double* Y, int64_t m, int64_t l, int64_t ld, double* T, int64_t ldt, double* small, double* ws, int& skip) {
  HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
  hipk::cholqr2_factor(st_, Y, m, l, ld, T, ldt, small, flags_ + FLAG_CHOLQR, ws);
  check_launch("cholqr2_factor");
  if (read_flag(FLAG_CHOLQR) == 0) return true;
  skip = 8;
  return false;
}
void HipBackend::qr_thinQ(double* Y, int64_t m, int64_t l, int64_t ld, double* R, bool replicated) {
  bind();
  const int64_t nb = hipk::qr_max_blocks(m);
  const int NB = hipk::QR_NB;
  const int64_t npan = (l + NB - 1) / NB;
  Carve c;
  const size_t o_coef = c.take(2 + NB + 2), o_part = c.take((size_t)nb * NB), o_tau = c.take(l),
               o_T = c.take((size_t)npan * NB * NB), o_G = c.take(NB * NB),
               o_Wt = c.take((size_t)l * NB), o_W2 = c.take((size_t)l * NB), o_small = c.take(hipk::cholqr_small_doubles(l)),
               o_Q = c.take((size_t)(m + 1) * l), o_amax = c.take(1 + hipk::QR_AMAX_PARTS);
  grow(ws_qr_, c.total * sizeof(double));
  TrimGuard trim_qr{this, &ws_qr_}, trim_hh{this, &ws_qr_hh_};
  double* base = (double*)ws_qr_.p;
  hipk::QrWork w;
  w.coef = base + o_coef; w.part = base + o_part; w.tau = base + o_tau; w.T = base + o_T; w.G = base + o_G;
  w.Vbuf = nullptr; w.Wt = base + o_Wt; w.W2 = base + o_W2; w.Qo = base + o_Q; w.maxblocks = nb;
  // gemm shapes inside: (t x NB, K = m), (NB x NB, K = m), (m x t, K = NB), (l x l, K = m), (m x 32, K <= l)
  size_t gmax = std::max({hipk::gemm_workspace_doubles(l, NB, m), hipk::gemm_workspace_doubles(NB, NB, m), cholqr_ws_doubles(m, l)});
  for (int64_t t = NB; t <= l; t += NB) gmax = std::max(gmax, hipk::gemm_workspace_doubles(t, NB, m));
  double* ws = gemm_ws(gmax + 64).p;
  // Three tiers, each leaving Y untouched until it is known to have worked (one 4-byte flag read):
  //   CholeskyQR2 (a handful of MFMA passes; needs cond(Y) < ~1e7), shifted CholeskyQR3 (cond up to ~1e13: sketches
  //   of fast-decaying covariance spectra), Householder reflectors (anything, including exact rank deficiency).
  // A panel that needed the second tier makes the next few factorizations OF THE SAME HEIGHT AND KIND start there:
  // consecutive panels of one operator are alike, and a failed first attempt costs ~1.2 ms at C2.  Keyed by
  // (height, replicated) so that, with several ranks, the replicated factorizations (stacked R factors, gathered
  // panels: identical input everywhere) never see a hint left by a rank's own row block -- not even when a row
  // block happens to have G*l rows -- and stay bit-identical across ranks.
  if (cholqr_gate(m, l)) {
    const int64_t ldt = (m + 1) & ~(int64_t)1;   // even: 16-byte loads in the contraction kernel
    int& skip_tier1_ = skip_tier1_by_height_[std::make_pair(m, replicated)];
    if (skip_tier1_ > 0) {
      --skip_tier1_;
    } else if (cholqr2_try(Y, m, l, ld, w.Qo, ldt, base + o_small, ws, skip_tier1_)) {   // Y -> Qo, and only now Qo -> Y
      hipk::cholqr2_apply(st_, Y, m, l, ld, w.Qo, ldt, R, base + o_small, ws);
      check_launch("cholqr2_apply");
      ++n_cholqr_;
      return;
    }
    // second tier: shifted CholeskyQR3 with one more transient panel; Y still untouched
    static const bool no_scholqr3 = (getenv("GSI_NO_SCHOLQR3") != nullptr);
    Scratch S2(this);                            // (stream-ordered pool; memory is no reason to fail: the third tier)
    if (!no_scholqr3 && S2.try_alloc((size_t)ldt * l) != nullptr) {
      HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
      hipk::scholqr3_factor(st_, Y, m, l, ld, w.Qo, ldt, S2.p, ldt, base + o_small, flags_ + FLAG_CHOLQR, ws);
      check_launch("scholqr3_factor");
      if (read_flag(FLAG_CHOLQR) == 0) {
        hipk::scholqr3_apply(st_, Y, m, l, ld, S2.p, ldt, R, base + o_small, ws);
        check_launch("scholqr3_apply");
        ++n_scholqr3_;
        return;
      }
    }
    skip_tier1_ = 0;   // neither Cholesky tier applies to this kind of panel: probe from the top next time
  }
  ++n_householder_;
  grow(ws_qr_hh_, (size_t)m * NB * sizeof(double));       // the reflector block: only this tier needs it
  w.Vbuf = (double*)ws_qr_hh_.p;
  // Range guard: the reflectors are formed from plain sums of squares, so a panel whose largest entry
  // lies outside [2^-400, 2^400] is factored as 2^-e Y (same Q, bit for bit) and R is scaled back by 2^e.  One pass over
  // the panel and one 8-byte read; inside the window nothing else runs.
  hipk::qr_absmax(st_, Y, m, l, ld, base + o_amax);
  double amax = 0.0;
  HIP_CHECK(hipMemcpyAsync(&amax, base + o_amax, sizeof(double), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  const int e = hipk::qr_prescale_exponent(amax);
  if (e != 0) hipk::qr_scale(st_, Y, m, l, ld, std::ldexp(1.0, -e));
  hipk::qr_thinQ(st_, Y, m, l, ld, R, w, ws);
  if (e != 0 && R != nullptr) hipk::qr_scale(st_, R, l, l, l, std::ldexp(1.0, e));
  check_launch("qr_thinQ");
}
// CholeskyQR2 stopped one tall product short (Backend::qr_thinQ_deferred): T = Y R1^-1 stays in the QR workspace, X2 = R2^-1
// goes to the caller.  Only the first tier (the guard of qr_thinQ decides: a panel that needs the shifted tier or
// Householder gets its Q the ordinary way), and only while the workspace is one this backend keeps between calls.
bool HipBackend::qr_thinQ_deferred(const double* Y, int64_t m, int64_t l, int64_t ld, const double** Q1, int64_t* ldq1, double* X2) {
  bind();
  static const bool off = (getenv("GSI_NO_QR_DEFER") != nullptr);
  if (off || !cholqr_gate(m, l)) return false;
  const int64_t ldt = (m + 1) & ~(int64_t)1;
  if ((size_t)ldt * l * sizeof(double) > ((size_t)8 << 30)) return false;       // trimmed on return: nothing would be left to hand out
  int& skip_tier1 = skip_tier1_by_height_[std::make_pair(m, false)];
  if (skip_tier1 > 0) return false;
  Carve c;
  const size_t o_small = c.take(hipk::cholqr_small_doubles(l)), o_T = c.take((size_t)ldt * l);
  grow(ws_qr_, c.total * sizeof(double));
  double* base = (double*)ws_qr_.p;
  double* ws = gemm_ws(cholqr_ws_doubles(m, l) + 64).p;
  if (!cholqr2_try(Y, m, l, ld, base + o_T, ldt, base + o_small, ws, skip_tier1)) return false;
  HIP_CHECK(hipMemcpyAsync(X2, hipk::cholqr2_X2(base + o_small, l), sizeof(double) * (size_t)l * l, hipMemcpyDeviceToDevice, st_));
  *Q1 = base + o_T; *ldq1 = ldt;
  ++n_cholqr_;
  return true;
}
// svd(B) for B = W' (RandMatFact.jl:86-88) without forming the thin Q of W: CholeskyQR2's first round leaves
// T = W R1^-1 and R2, R2^-1; R = R2 R1 goes to the Jacobi SVD, and Z = T (R2^-1 (U sqrt(S))) is ONE tall product
// (the generic path runs Y = T R2^-1 and Z = Y (U sqrt(S)): two).  Declines when CholeskyQR2 does not apply.
bool HipBackend::svd_tall_fused(const double* W, int64_t m, int64_t l, int64_t ld, int64_t K_scale, double* V, int64_t ldv,
                                double* S, const double* Xr) {
  bind();
  static const bool off = (getenv("GSI_NO_SVD_FUSION") != nullptr);
  if (off || !cholqr_gate(m, l)) return false;
  int& skip_tier1 = skip_tier1_by_height_[std::make_pair(m, false)];
  if (skip_tier1 > 0) return false;                       // this kind of panel needs the shifted tier: generic path
  const int64_t ldt = (m + 1) & ~(int64_t)1;
  Carve c;
  const size_t o_small = c.take(hipk::cholqr_small_doubles(l)), o_R = c.take((size_t)l * l), o_U = c.take((size_t)l * l),
               o_M = c.take((size_t)l * l), o_T = c.take((size_t)ldt * l);
  grow(ws_svdf_, c.total * sizeof(double));
  TrimGuard trim_svdf{this, &ws_svdf_};
  double* base = (double*)ws_svdf_.p;
  const GemmWs ws = gemm_ws(std::max(cholqr_ws_doubles(m, l), hipk::gemm_workspace_doubles(l, l, l)) + 64);
  phase_begin(PH_QR);
  if (!cholqr2_try(W, m, l, ld, base + o_T, ldt, base + o_small, ws.p, skip_tier1)) {
    phase_end(PH_QR);
    return false;                                         // W is untouched: the caller's generic path takes over
  }
  hipk::cholqr2_R(st_, l, base + o_small, base + o_R);    // R = R2 R1
  if (Xr != nullptr) {                                    // the SVD wanted is that of W Xr = Q (R Xr): one l x l product
    gemm("svd_tall_fused", ws, false, l, l, l, 1.0, base + o_R, l, Xr, l, 0.0, base + o_M, l);
    HIP_CHECK(hipMemcpyAsync(base + o_R, base + o_M, sizeof(double) * (size_t)l * l, hipMemcpyDeviceToDevice, st_));
  }
  phase_end(PH_QR);
  ++n_cholqr_;
  phase_begin(PH_SVD);
  svd_small(base + o_R, l, base + o_U, S);
  if (K_scale >= 0) hipk::scale_cols_sqrt(st_, base + o_U, l, S, K_scale);
  phase_end(PH_SVD);
  phase_begin(PH_SMALL_GEMM);
  gemm("svd_tall_fused", ws, false, l, l, l, 1.0, hipk::cholqr2_X2(base + o_small, l), l, base + o_U, l, 0.0, base + o_M, l);
  // Z = V sqrt(S) has its last p columns ZERO by definition (RandMatFact.jl:87): they are not multiplied out (a fifth of
  // the product at K = 256, p = 64), they are cleared
  const int64_t lz = (K_scale >= 0 && K_scale < l) ? K_scale : l;
  gemm("svd_tall_fused", ws, false, m, lz, l, 1.0, base + o_T, ldt, base + o_M, l, 0.0, V, ldv);
  if (lz < l) HIP_CHECK(hipMemsetAsync(V + (size_t)lz * ldv, 0, sizeof(double) * ((size_t)(l - lz - 1) * ldv + m), st_));
  check_launch("svd_tall_fused");
  phase_end(PH_SMALL_GEMM);
  return true;
}
void HipBackend::svd_small(double* G, int64_t l, double* U, double* S) {
  bind();
  if (l > 5000) throw Error(GSI_ERR_ARG, "sketch width l = K+p > 5000 is not supported by the LDS-resident block Jacobi SVD");
  grow(ws_svd_, sizeof(double) * (l + 8) + 64 + sizeof(int32_t) * hipk::SVD_SCHED_INTS);
  hipk::SvdWork w;
  w.norms = (double*)ws_svd_.p;
  w.pairs = (int32_t*)((char*)ws_svd_.p + sizeof(double) * (l + 8) + 64);
  w.rotcount = flags_ + FLAG_SVD_ROTATIONS;
  const int sw = hipk::svd_small(st_, G, l, U, S, w);
  last_svd_sweeps_ = sw < 0 ? -sw : sw;
  if (sw < 0) ++n_svd_cap_hits_;          // 40 sweeps and rotatable pairs left (factors graded over > 1e10): gsi_ctx_path_info reports it
  check_launch("svd_small");
}
void HipBackend::chol_upper(double* B, int64_t j) {
  bind();
  if (j > 2048) throw Error(GSI_ERR_ARG, "chol_upper: j too large");
  hipk::chol_upper(st_, B, j, flags_ + FLAG_CHOL_INFO);
  check_launch("chol_upper");
}
void HipBackend::trsm_right_upper(double* F, int64_t m, int64_t j, int64_t ldf, const double* C) {
  bind();
  hipk::trsm_right_upper(st_, F, m, j, ldf, C);
  check_launch("trsm_right_upper");
}
void HipBackend::scale_cols_sqrt(double* U, int64_t l, const double* S, int64_t K) {
  bind();
  hipk::scale_cols_sqrt(st_, U, l, S, K);
}

}  // namespace gsi
