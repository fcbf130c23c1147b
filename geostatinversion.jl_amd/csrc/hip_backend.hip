// hip_backend.hip -- the gfx950 implementation of gsi::Backend: one HIP stream per context, every operation enqueued on it (no host
// round trips except where the algorithm needs a scalar), workspaces grown on demand.  The communicators are in hip_comm.hip.
#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <map>
#include <memory>
#include <set>
#include <vector>
#include "hip_backend.hpp"
#include "hip_common.hpp"
#include "host_staging.hpp"
#include "fftrf_points.hpp"

namespace gsi {

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool pooled = false;      // a panel-sized workspace taken from (and returned to) the block cache instead of hipMalloc / hipFree
};

// roctx ranges around the phases of the hot path: bound lazily, so the library has no hard
// dependency on the profiler's marker library; visible with `rocprofv3 --marker-trace`.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
static RoctxApi& roctx() { static RoctxApi api; return api; }
static const char* const kPhaseNames[PH_COUNT] = {"gsi:A*X", "gsi:A'*X", "gsi:lu(Y).L", "gsi:thin QR", "gsi:svd(l x l)",
                                                 "gsi:panel x (l x l)", "gsi:collective", "gsi:other", "gsi:waiting for peers"};

class HipBackend : public HipDevice {
  // A pooled temporary that goes back to the block cache on every exit path (a throwing HIP_CHECK between alloc
  // and release leaked pooled blocks).  release() is ordered on the stream: WHERE a Scratch ends is part of what a function does.
  // try_alloc: null instead of an exception, where memory is no reason to fail.
  struct Scratch {
    HipBackend* be; double* p;
    explicit Scratch(HipBackend* b, size_t doubles = 0) : be(b), p(doubles ? b->alloc(doubles) : nullptr) {}
    ~Scratch() { if (p) be->release(p); }
    double* try_alloc(size_t doubles) { try { return p = be->alloc(doubles); } catch (const Error&) { return p = nullptr; } }
    void adopt(double* q) { p = q; }
    double* give_up() { double* q = p; p = nullptr; return q; }
    Scratch(const Scratch&) = delete; Scratch& operator=(const Scratch&) = delete;
  };
 public:
  explicit HipBackend(int device) : HipDevice(device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
      throw Error(GSI_ERR_HIP, "no HIP device visible (libgsi_hip needs an AMD GPU; there is no CPU fallback)");
    if (device < 0 || device >= count) throw Error(GSI_ERR_ARG, "device id out of range");
    HIP_CHECK(hipSetDevice(device_));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device_));
    arch_ = prop.gcnArchName;
    ncus_ = prop.multiProcessorCount;
    if (arch_.find("gfx950") == std::string::npos)
      throw Error(GSI_ERR_HIP, "libgsi_hip is built for gfx950 (MI355X); device reports " + arch_);
    // non-blocking: nothing of this library uses the NULL stream, and a runtime-internal or foreign NULL-stream operation
    // must never wait for (or be waited for by) a persistent kernel of ours that spins for its peers
    HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    HIP_CHECK(hipMalloc(&flags_, FLAG_COUNT * sizeof(int32_t)));
    HIP_CHECK(hipMemsetAsync(flags_, 0, FLAG_COUNT * sizeof(int32_t), st_));
    HIP_CHECK(hipMalloc(&scal_, (64 + 8 + 256) * sizeof(double)));   // scalars + partial sums of long dot products
  }
  ~HipBackend() override {
    hipSetDevice(device_);
    hipStreamSynchronize(st_);
    drain_side();
    stager_.reset();
    if (ev_stage_) hipEventDestroy(ev_stage_);
    for (DevBuf* b : ws_all_) free_ws(*b);
    collect_garbage();
    for (auto& b : pool_) hipFree(b.p);
    for (auto& ev : ev_pool_) hipEventDestroy(ev);
    for (auto& r : records_) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    hipFree(flags_);
    hipFree(scal_);
    if (pin_power_) hipHostFree(pin_power_);
    if (mr_recs_) hipFree(mr_recs_);
    if (ev_fork_) hipEventDestroy(ev_fork_);
    if (ev_join_) hipEventDestroy(ev_join_);
    if (st2_) hipStreamDestroy(st2_);
    hipStreamDestroy(st_);
  }
  const char* name() const override { return "hip-gfx950"; }

  // ---- memory ----
  // Panel-sized temporaries come and go inside every entry point; everything is ordered on the one
  // stream, so a released block can be handed to the next request without synchronising or going back
  // to hipFree/hipMalloc.  Exact-size free lists (the sizes repeat from call to call), trimmed when the
  // cache exceeds half of what is in use.
  double* alloc(size_t count) override {
    bind();
    if (count == 0) count = 1;
    size_t bytes = count * sizeof(double);
    // Panel-sized requests are rounded up to 256 MiB: the n x l panel, the (n + 1) x l workspace of the out-of-place QR and the
    // even-ld copy of the thin SVD then have the SAME size and hand one cached block to each other instead of going through
    // hipFree / hipMalloc (at 512^3, l = 48 -- 51.5 GB blocks -- that was 4.9 s of an 11.4 s randsvd).
    if (bytes > ((size_t)1 << 30)) bytes = (bytes + (((size_t)256 << 20) - 1)) & ~(((size_t)256 << 20) - 1);
    {
      std::lock_guard<std::mutex> g(mu_);
      for (size_t i = 0; i < pool_.size(); ++i)
        if (pool_[i].bytes == bytes) {
          void* p = pool_[i].p;
          pool_[i] = pool_.back();
          pool_.pop_back();
          pooled_ -= (int64_t)bytes;
          sizes_.push_back({p, bytes});
          in_use_ += (int64_t)bytes;
          return (double*)p;
        }
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {   // give the cache back and retry once
      (void)hipGetLastError();
      trim_pool(0);
      e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      throw Error(GSI_ERR_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> g(mu_);
    sizes_.push_back({p, bytes});
    in_use_ += (int64_t)bytes;
    return (double*)p;
  }
  void release(double* p) override {
    if (!p) return;
    bind();
    size_t bytes = 0;
    {
      std::lock_guard<std::mutex> g(mu_);
      for (size_t i = 0; i < sizes_.size(); ++i)
        if (sizes_[i].p == p) {
          bytes = sizes_[i].bytes;
          in_use_ -= (int64_t)bytes;
          sizes_[i] = sizes_.back();
          sizes_.pop_back();
          break;
        }
      if (bytes != 0) {
        pool_.push_back({p, bytes});
        pooled_ += (int64_t)bytes;
        p = nullptr;
      }
    }
    if (p) {
      hipStreamSynchronize(st_);
      drain_side();
      hipFree(p);
    }
    // Panels of the tall problems are GBs each and come back every pass: keep up to 160 GB of them (of 288 GB; a
    // failed hipMalloc empties the cache and retries, so nothing is ever refused because of it).  A tighter policy
    // cost 0.7 s of hipFree/hipMalloc per randsvd at n = 1.7e7 and 4.9 s at n = 1.3e8.
    // (ranks that share this device -- one-GPU rehearsals -- share the budget: a co-tenant cannot reach into this cache, it
    // would just see an out-of-memory error)
    const int64_t cap = ((int64_t)160 << 30) / std::max(1, ranks_sharing_device_);
    if (pooled_ > cap) trim_pool(cap / 3 * 2);
  }
  void trim_pool(int64_t keep_bytes) {
    hipStreamSynchronize(st_);
    drain_side();
    std::lock_guard<std::mutex> g(mu_);
    while (!pool_.empty() && pooled_ > keep_bytes) {
      hipFree(pool_.back().p);
      pooled_ -= (int64_t)pool_.back().bytes;
      pool_.pop_back();
    }
  }
  void release_cache() override {
    bind();
    for (DevBuf* b : ws_all_)
      if (b->bytes > ((size_t)64 << 20)) free_ws(*b);
    (void)hipStreamSynchronize(st_);
    drain_side();
    collect_garbage();
    trim_pool(0);
  }
  int64_t bytes_in_use() const override {
    int64_t ws = 0;
    for (const DevBuf* b : ws_all_)                     // (ws_lus_ has never been part of this figure: it stays out of it)
      if (b != &ws_lus_ && !b->pooled) ws += (int64_t)b->bytes;          // pooled workspaces are counted by alloc()
    return in_use_ + pooled_ + ws + (int64_t)garbage_bytes_;
  }
  // ---- the host boundary (host_staging.hpp): caller memory is pageable; transfers of GSI_STAGE_MIN_MB (default 16) MiB and
  // more go through the pinned staging ring (GSI_STAGE_THREADS workers, default 6 -- four reach the link rate on contiguous
  // sources, the strided row-block reads want the margin --, GSI_STAGE_CHUNK_MB MiB chunks, default 16: 0.98 of this box's
  // pinned-copy rate in both directions, profiles/r05_h2d_rates.log); smaller ones straight from the
  // caller's pages (54 us for C1's 768 KB Omega).  If the ring cannot be allocated the direct path serves everything.
  HostStager* stager() {
    if (stager_ || stager_failed_) return stager_.get();
    static const int threads = getenv("GSI_STAGE_THREADS") ? std::max(1, std::min(32, atoi(getenv("GSI_STAGE_THREADS")))) : 6;
    static const size_t chunk = (size_t)(getenv("GSI_STAGE_CHUNK_MB") ? std::max(1, std::min(1024, atoi(getenv("GSI_STAGE_CHUNK_MB")))) : 16) << 20;
    try {
      stager_.reset(new HostStager(device_, threads, chunk));
      HIP_CHECK(hipEventCreateWithFlags(&ev_stage_, hipEventDisableTiming));
    } catch (const std::exception&) {
      (void)hipGetLastError();
      stager_.reset();
      stager_failed_ = true;
    }
    return stager_.get();
  }
  static size_t stage_min_bytes() {
    const char* e = getenv("GSI_STAGE_MIN_MB");            // read per call (a getenv against a transfer of MiBs; tests switch it)
    return (size_t)(e ? std::max(0ll, atoll(e)) : 16) << 20;
  }
  bool staged(bool h2d, double* dev, int64_t ldd, double* host, int64_t ldh, int64_t rows, int64_t cols) {
    if (sizeof(double) * (size_t)rows * (size_t)cols < std::max<size_t>(stage_min_bytes(), 1)) return false;
    HostStager* s = stager();
    if (!s) return false;
    HIP_CHECK(hipEventRecord(ev_stage_, st_));       // copies start after everything queued so far (pooled destination / source in the making)
    try {
      // mid-size transfers (C1's 32 MB matrix): smaller rectangles, so that every worker has several in flight
      const size_t bytes = sizeof(double) * (size_t)rows * (size_t)cols;
      size_t chunk = std::min(s->chunk_bytes(), std::max<size_t>((size_t)1 << 20, (bytes / (4 * (size_t)s->threads())) & ~(((size_t)1 << 18) - 1)));
      s->begin(h2d, dev, ldd, host, ldh, stage_plan_whole(rows, cols, chunk), 1, ev_stage_);
      s->end();
    } catch (const Error&) {
      throw;
    } catch (const std::exception& e) {
      throw Error(GSI_ERR_HIP, e.what());
    }
    return true;
  }
  void upload2d(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols) override {
    if (rows <= 0 || cols <= 0) return;
    bind();
    if (staged(true, dst, ldd, const_cast<double*>(host), ldh, rows, cols)) return;
    HIP_CHECK(hipMemcpy2DAsync(dst, ldd * sizeof(double), host, ldh * sizeof(double), rows * sizeof(double),
                               cols, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));  // the caller may reuse / free the host buffer on return
  }
  void download2d(double* host, int64_t ldh, const double* src, int64_t lds, int64_t rows, int64_t cols) override {
    if (rows <= 0 || cols <= 0) return;
    bind();
    if (staged(false, const_cast<double*>(src), lds, host, ldh, rows, cols)) return;
    HIP_CHECK(hipMemcpy2DAsync(host, ldh * sizeof(double), src, lds * sizeof(double), rows * sizeof(double),
                               cols, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  // Row-block upload in the background (Backend::upload2d_begin): matrices of 256 MiB and more, in blocks of up to 32768 rows
  // = 256 output tiles, one full round of the contraction (what stays exposed after the upload is the LAST block's product,
  // ~10 ms at C2 whatever the block height, so tall blocks lose nothing) and 256 KB per column segment on the host side:
  // the workers' strided reads of the caller's matrix ran at 0.24 s per 8.6 GB against 0.35 s with 32 KB segments, and
  // with short segments the upload was sometimes bound by them (profiles/r05_boundary_probe.log).  At least two blocks.
  // GSI_STAGE_BLOCK_ROWS overrides (tests: many small blocks).
  int64_t upload_block_rows(int64_t rows, int64_t cols) override {
    const int64_t forced = getenv("GSI_STAGE_BLOCK_ROWS") ? atoll(getenv("GSI_STAGE_BLOCK_ROWS")) : 0;
    if (forced >= 128) return std::min(rows, (forced / 128) * 128);
    if (sizeof(double) * (size_t)rows * (size_t)cols < ((size_t)256 << 20) || rows < 2 * 4096) return rows;
    const int64_t half = (((rows + 1) / 2 + 127) / 128) * 128;
    return std::max<int64_t>(4096, std::min<int64_t>(32768, half));
  }
  void* upload2d_begin(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols,
                       int64_t block_rows) override {
    if (rows <= 0 || cols <= 0) return nullptr;
    bind();
    HostStager* s = (block_rows < rows) ? stager() : nullptr;
    if (!s) { upload2d(dst, ldd, host, ldh, rows, cols); return nullptr; }
    HIP_CHECK(hipEventRecord(ev_stage_, st_));
    int nblocks = 0;
    std::vector<StageRect> plan = stage_plan_rowblocks(rows, cols, block_rows, s->chunk_bytes(), &nblocks);
    try {
      s->begin(true, dst, ldd, const_cast<double*>(host), ldh, std::move(plan), nblocks, ev_stage_);
    } catch (const std::exception& e) {
      throw Error(GSI_ERR_HIP, e.what());
    }
    return s;
  }
  void upload2d_wait_block(void* handle, int64_t b) override {
    if (!handle) return;
    bind();
    try {
      static_cast<HostStager*>(handle)->wait_block((int)b, st_);
    } catch (const std::exception& e) {
      throw Error(GSI_ERR_HIP, e.what());
    }
  }
  void pinned_copy_rate(int64_t bytes, double* h2d_gbs, double* d2h_gbs) override {
    bind();
    if (bytes < (1 << 20)) bytes = 1 << 20;
    void* pin = nullptr;
    HIP_CHECK(hipHostMalloc(&pin, (size_t)bytes, hipHostMallocDefault));
    struct FreePin { void* p; ~FreePin() { hipHostFree(p); } } fp{pin};
    memset(pin, 1, (size_t)bytes);
    Scratch dev(this, (size_t)bytes / sizeof(double) + 1);
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    struct FreeEv { hipEvent_t a, b; ~FreeEv() { hipEventDestroy(a); hipEventDestroy(b); } } fe{e0, e1};
    double best[2] = {0.0, 0.0};
    for (int dir = 0; dir < 2; ++dir)
      for (int rep = 0; rep < 3; ++rep) {
        HIP_CHECK(hipEventRecord(e0, st_));
        if (dir == 0) HIP_CHECK(hipMemcpyAsync(dev.p, pin, (size_t)bytes, hipMemcpyHostToDevice, st_));
        else HIP_CHECK(hipMemcpyAsync(pin, dev.p, (size_t)bytes, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipEventRecord(e1, st_));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (ms > 0.f) best[dir] = std::max(best[dir], (double)bytes / (ms * 1e-3) / 1e9);
      }
    *h2d_gbs = best[0];
    *d2h_gbs = best[1];
  }
  void upload2d_end(void* handle) override {
    if (!handle) return;
    try {
      static_cast<HostStager*>(handle)->end();
    } catch (const std::exception& e) {
      throw Error(GSI_ERR_HIP, e.what());
    }
  }
  void copy2d(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols) override {
    if (rows <= 0 || cols <= 0) return;
    bind();
    HIP_CHECK(hipMemcpy2DAsync(dst, ldd * sizeof(double), src, lds * sizeof(double), rows * sizeof(double),
                               cols, hipMemcpyDeviceToDevice, st_));
  }
  void fill_zero(double* p, size_t count) override {
    bind();
    HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(double), st_));
  }
  void sync() override {
    bind();
    HIP_CHECK(hipStreamSynchronize(st_));
    if (st2_) HIP_CHECK(hipStreamSynchronize(st2_));
  }

  // ---- products ----
  void gemm_nn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
               int64_t ldb, double beta, double* C, int64_t ldc) override {
    bind();
    double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
    hipk::gemm_f64(st_, false, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc, ws);
    check_launch("gemm_nn");
  }
  void gemm_nn_rowblock(int64_t m_full, int64_t r0, int64_t mb, int64_t l, int64_t k, const double* A, int64_t lda,
                        const double* B, int64_t ldb, double* C, int64_t ldc) override {
    bind();
    double* ws = gemm_ws(hipk::gemm_rowblock_workspace_doubles(m_full, mb, l, k));
    hipk::gemm_f64_nn_rowblock(st_, m_full, r0, mb, l, k, A, lda, B, ldb, C, ldc, ws);
    check_launch("gemm_nn_rowblock");
  }
  void gemm_tn(int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda, const double* B,
               int64_t ldb, double beta, double* C, int64_t ldc) override {
    bind();
    double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
    hipk::gemm_f64(st_, true, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc, ws);
    check_launch("gemm_tn");
  }
  void gemm_view(int form, bool trans, int64_t m, int64_t l, int64_t k, double alpha, const double* A, int64_t lda,
                 const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int64_t m_full, int64_t r0,
                 int64_t* plan8) override {
    bind();
    hipk::GemmPlan p = {0, 0, 0, 0, 0, 0, 0, 0};
    if (form == 0) {
      double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
      hipk::gemm_f64(st_, trans, m, l, k, alpha, A, lda, B, ldb, beta, C, ldc, ws, &p);
    } else if (form == 1) {
      double* ws = gemm_ws(hipk::gemm_syrk_workspace_doubles(l, k));
      hipk::gemm_f64_syrk_upper(st_, l, k, A, lda, C, ldc, ws, &p);
    } else if (form == 2) {
      double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
      hipk::gemm_f64_trmm_upper(st_, m, l, k, A, lda, B, ldb, C, ldc, ws, &p);
    } else {
      double* ws = gemm_ws(hipk::gemm_rowblock_workspace_doubles(m_full, m, l, k));
      hipk::gemm_f64_nn_rowblock(st_, m_full, r0, m, l, k, A, lda, B, ldb, C, ldc, ws, &p);
    }
    check_launch("gemm_view");
    const int64_t out[8] = {p.nt, p.nchunks, p.xmode, p.wide, p.nsplit, p.persistent, p.grid_x, p.active};
    for (int i = 0; i < 8; ++i) plan8[i] = out[i];
  }
  void fill_bytes(double* p, int byte, size_t count) override {
    bind();
    HIP_CHECK(hipMemsetAsync(p, byte, count * sizeof(double), st_));
  }
  void gemm_nn_gridcov(int64_t m, int64_t l, int64_t k, const double* tab, int64_t nx, int64_t ny, int64_t roff,
                       int64_t koff, const double* B, int64_t ldb, double* C, int64_t ldc) override {
    bind();
    double* ws = gemm_ws(hipk::gemm_workspace_doubles(m, l, k));
    hipk::gemm_f64_gridcov(st_, m, l, k, tab, nx, ny, roff, koff, B, ldb, C, ldc, ws);
    check_launch("gemm_nn_gridcov");
  }

  // Scattered-point covariance, row-streamed: the entries are generated inside the contraction's tile loader (gemm_f64.hip
  // GEN 2: 128 x 160 tiles; pointcov_gemm.hip: 96 x 320) -- nothing of A ever exists in HBM.  (Round 3's form, row panels of A
  // generated into HBM on a second stream, is kept as tools/rejected_kernels/pointcov_round3_panels.hip.txt: 39 TFLOP/s
  // against 59.)
  void gemm_nn_pointcov(int64_t m, int64_t l, int64_t k, const double* pts, int d, int kind, double ell, double sigma2,
                        double nugget, int64_t roff, int64_t koff, const double* B, int64_t ldb, double* C,
                        int64_t ldc) override {
    bind();
    if (m <= 0 || l <= 0 || k <= 0) return;
    const int64_t npts = std::max(roff + m, koff + k);
    Scratch p4(this, (size_t)4 * npts);                  // the points as 32-byte records (x, y, z, 0): one scalar load each
    hipk::pointcov_pad_points(st_, pts, d, npts, hipk::pointcov_point_scale(kind, 1.0 / ell), p4.p);
    double* ws = gemm_ws(hipk::gemm_pointcov_workspace_doubles(m, l, k));
    // the wide kernel streams a tile-ordered copy of the sketch panel (k x l doubles); memory is never a reason to fail: without
    // the copy the product runs on the 128 x 160 kernel, which reads X where it lies
    Scratch xpack(this);
    const size_t xdoubles = hipk::gemm_pointcov_pack_doubles(m, l, k);          // 0: not the wide kernel's product
    if (xdoubles > 0) xpack.try_alloc(xdoubles);
    hipk::gemm_f64_pointcov(st_, m, l, k, p4.p, npts, d, kind, sigma2, nugget, roff, koff, B, ldb, C, ldc, ws, xpack.p);
    check_launch("gemm_nn_pointcov (in-loader generator)");
  }

  // ---- matrix-free FFT covariance ----
  struct FftCov {                         // (W goes back before lam, on every way out)
    int64_t N[3], M[3]; Scratch lam, W; int nb_max;
    explicit FftCov(HipBackend* be) : lam(be), W(be) {}
  };
  // the grid squeezed of its singleton axes, its embedding, the limits, and the plan's two arrays (spectrum, work array);
  // *reembed: FFTRF's exact 2 N embedding is not a power of two on some axis
  std::unique_ptr<FftCov> fftcov_new_plan(const int64_t N[3], int fftrf, bool* reembed, int* dims) {
    std::unique_ptr<FftCov> p(new FftCov(this));
    int64_t Mtot = 1;
    int d = 0;
    for (int a = 0; a < 3; ++a) { p->N[a] = 1; p->M[a] = 1; }
    *reembed = false;
    for (int a = 0; a < 3; ++a) {        // squeeze singleton axes: vec() of a 1 x 50 field is a 50-point line
      if (N[a] < 1) throw Error(GSI_ERR_ARG, "fft covariance: grid dimensions must be >= 1");
      if (N[a] == 1) continue;
      p->N[d] = N[a]; p->M[d] = hipk::fft_embed_size(N[a]);
      if (fftrf && p->M[d] != 2 * N[a]) *reembed = true;
      if (p->M[d] > 8192) throw Error(GSI_ERR_ARG, "fft covariance: at most 4096 grid points per axis (a line must fit LDS)");
      Mtot *= p->M[d];
      ++d;
    }
    // element offsets inside one column pair's array are 32-bit in the pass kernels (fft_cov.hip): refuse such grids HERE, before
    // the spectrum and the work array (tens of GB) are allocated, not at the first product
    if (Mtot >= ((int64_t)1 << 31))
      throw Error(GSI_ERR_ARG, "fft covariance: the embedding grid must have fewer than 2^31 points (e.g. 1024 x 512 x 512 embeds to 2^31)");
    // work array: as many column pairs at once as fit ~2 GB, at most 64.  (GSI_FFT_W_MB: the experiment of VERDICT r4 item 7 --
    // few enough pairs per batch that the array between the passes stays in the 256 MB Infinity Cache: DESIGN.md 4.6,
    // profiles/r05_fft_pair_major.log)
    // 2-D grids whose pair array is <= 128 MB run 256 MB batches: +4 % at 1000^2 (6.57 -> 6.31 ms per 256 columns), the only
    // place the experiment moved anything; 128 MB and less lose to the shorter launches.
    static const int64_t w_env = getenv("GSI_FFT_W_MB") ? std::max<int64_t>(1, atoll(getenv("GSI_FFT_W_MB"))) : 0;
    const int64_t w_mb = w_env > 0 ? w_env : ((d == 2 && 16 * Mtot <= ((int64_t)128 << 20)) ? 256 : 2048);
    int64_t nb = (w_mb << 20) / (16 * Mtot);
    p->nb_max = (int)std::max<int64_t>(1, std::min<int64_t>(nb, 64));
    p->lam.adopt(alloc(hipk::fft_plan_doubles(p->M)));
    p->W.adopt(alloc((size_t)2 * Mtot * p->nb_max));
    *dims = d;
    return p;
  }
  // One per-axis factor of the re-embedding, applied to the FASTEST axis of the array in bufh (dimensions cur, tot elements,
  // d real axes) as cur' = cur^T B (the contraction kernel's A'B form: the array as a k x rest matrix), which also rotates
  // that axis to the back: d applications restore the natural order.
  enum FftFactor { FFT_F_COS = 0, FFT_F_COS_WEIGHTED = 1, FFT_F_SIN_WEIGHTED = 2 };
  void fft_rotate_apply(Scratch& buf, int64_t cur[3], int64_t& tot, int d, int64_t rows_out, int64_t period, FftFactor f) {
    // cur = (k, rest) column-major; B = k x rows_out; result (rest x rows_out) = the array with axis 0 replaced and last
    const int64_t k = cur[0], rest = (tot / k);
    Scratch B(this, (size_t)k * rows_out);
    // B[kk + t k] : weighted (the D and S factors) is indexed [t = row of the INPUT, k' = output]; unweighted [k, t]
    if (f == FFT_F_COS) hipk::fft_cos_matrix(st_, B.p, k, rows_out, period, false);              // C_a^T: B[k, t]
    else if (f == FFT_F_COS_WEIGHTED) hipk::fft_cos_matrix(st_, B.p, k, rows_out, period, true);  // D_a^T: B[t, k'] = w_t cos(.)
    else hipk::fft_sin_matrix(st_, B.p, k, rows_out, period);                                   // S_a^T: B[t, k'] = w_t sin(.)
    Scratch out(this, (size_t)rest * rows_out);
    double* ws = gemm_ws(hipk::gemm_workspace_doubles(rest, rows_out, k));
    hipk::gemm_f64(st_, true, rest, rows_out, k, 1.0, buf.p, k, B.p, k, 0.0, out.p, rest, ws);
    check_launch("fft re-embedding product");
    release(buf.give_up());
    buf.adopt(out.give_up());
    tot = rest * rows_out;
    // rotate the dimension list: (k, c1, c2) -> (c1, c2, rows_out) over the d real axes
    int64_t nd[3] = {1, 1, 1};
    for (int a = 0; a + 1 < d; ++a) nd[a] = cur[a + 1];
    nd[d - 1] = rows_out;
    for (int a = 0; a < 3; ++a) cur[a] = nd[a];
  }
  // The second half of the re-embedding, shared by the power-law and the covariance-function plans: the lags of a kernel over
  // the box (bufh: N[0] x N[1] x N[2], natural order) -> (x_a D_a) c on the power-of-two embedding M, natural order; with
  // sine = true (x_a S_a) c, the odd-odd part of a centrally symmetric 2-D kernel.
  void fftcov_lags_to_spectrum(Scratch& bufh, int64_t cur[3], int64_t& tot, const FftCov* p, int d, bool sine) {
    for (int a = 0; a < d; ++a) fft_rotate_apply(bufh, cur, tot, d, p->M[a], p->M[a], sine ? FFT_F_SIN_WEIGHTED : FFT_F_COS_WEIGHTED);
  }
  void* fftcov_create(const int64_t N[3], double beta, int fftrf) override {
    bind();
    bool reembed = false;
    int d = 0;
    std::unique_ptr<FftCov> p = fftcov_new_plan(N, fftrf, &reembed, &d);
    const int64_t Mtot = p->M[0] * p->M[1] * p->M[2];
    if (!reembed) {
      hipk::fft_spectrum(st_, p->lam.p, p->lam.p + Mtot, p->M, beta, fftrf);
      check_launch("fft_spectrum");
      return p.release();
    }
    // FFTRF's convention on an arbitrary grid (FFTRF.jl:83-90 embeds on exactly 2 N points for ANY N): the same matrix
    // through the power-of-two passes with a re-embedded spectrum (fft_cov.hip, "FFTRF's convention on a grid ...").
    //   c  = (x_a C_a) lambda_{2N}    C_a[t, k]  = cos(2 pi t k / 2 N_a),            t < N_a, k < 2 N_a     (lags 0 .. N_a - 1)
    //   l' = (x_a D_a) c              D_a[k', t] = w_t cos(2 pi t k' / M'_a), w_0 = 1, w_t = 2              (c' even, 0 beyond)
    int64_t cur[3] = {1, 1, 1};
    for (int a = 0; a < d; ++a) cur[a] = 2 * p->N[a];
    int64_t tot = cur[0] * cur[1] * cur[2];
    Scratch bufh(this, (size_t)tot);
    hipk::fft_spectrum_natural(st_, bufh.p, cur, beta, 1);
    for (int a = 0; a < d; ++a) fft_rotate_apply(bufh, cur, tot, d, p->N[a], 2 * p->N[a], FFT_F_COS);   // lags 0 .. N_a - 1 of c
    fftcov_lags_to_spectrum(bufh, cur, tot, p.get(), d, false);              // the spectrum of the re-embedded kernel
    hipk::fft_lines_layout(st_, bufh.p, p->lam.p, p->M);
    hipk::fft_finish_plan(st_, p->lam.p, p->lam.p + Mtot, p->M);
    check_launch("fft re-embedded spectrum");
    return p.release();
  }
  // The same operator type for a covariance FUNCTION of the grid lags (gsi_op_fft_gridcov[_table]):
  //   lambda' = (x_a D_a) c                              kernels even along every axis
  //   lambda' = (D_0 x D_1) c_ee - (S_0 x S_1) c_oo      centrally symmetric 2-D kernels (cos(a + b) = cos a cos b - sin a sin b;
  //                                                      c_ee, c_oo = half the sum / difference of the lags (t0, t1), (t0, -t1))
  // stored as (lambda' + nugget) / Mtot: no unit diagonal, and nugget * I on the box exactly.
  void* fftcov_create_lags(const int64_t N[3], int kind, const double ell[3], double theta, double sigma2, double nugget,
                           const double* table, const double* table_mirror) override {
    bind();
    bool reembed = false;
    int d = 0;
    std::unique_ptr<FftCov> p = fftcov_new_plan(N, 0, &reembed, &d);
    int64_t cur[3] = {p->N[0], p->N[1], p->N[2]};      // singleton axes do not move an element of the lag table
    int64_t tot = cur[0] * cur[1] * cur[2];
    // a second quadrant only where it differs from the first: both axes of a 2-D grid longer than one point
    const bool mirrored = (table ? table_mirror != nullptr : theta != 0.0) && d == 2 && N[2] == 1;
    Scratch cp(this, (size_t)tot), cm(this, mirrored ? (size_t)tot : 0);
    if (table) {
      upload2d(cp.p, tot, table, tot, tot, 1);
      if (mirrored) upload2d(cm.p, tot, table_mirror, tot, tot, 1);
    } else {
      const double inv_ell[3] = {1.0 / ell[0], 1.0 / ell[1], 1.0 / ell[2]};
      hipk::fft_lag_table(st_, cp.p, cm.p, N, kind, inv_ell, std::cos(theta), std::sin(theta), sigma2);
      check_launch("fft_lag_table");
    }
    if (mirrored) {
      hipk::fft_even_odd_split(st_, cp.p, cm.p, tot);
      int64_t cur_s[3] = {cur[0], cur[1], cur[2]};
      int64_t tot_s = tot;
      fftcov_lags_to_spectrum(cm, cur_s, tot_s, p.get(), d, true);
    }
    fftcov_lags_to_spectrum(cp, cur, tot, p.get(), d, false);
    if (mirrored) hipk::fft_subtract(st_, cp.p, cm.p, tot);
    hipk::fft_lines_layout(st_, cp.p, p->lam.p, p->M);
    hipk::fft_finish_plan_lags(st_, p->lam.p, p->M, nugget);
    check_launch("fft covariance-function spectrum");
    return p.release();
  }
  void fftcov_destroy(void* plan) override {
    delete static_cast<FftCov*>(plan);
  }
  void fftcov_apply(void* plan, int64_t l, const double* X, int64_t ldx, double* Y, int64_t ldy) override {
    bind();
    FftCov* p = static_cast<FftCov*>(plan);
    hipk::fft_cov_apply(st_, p->N, p->M, p->lam.p, reinterpret_cast<double2*>(p->W.p), p->nb_max, l, X, ldx, Y, ldy);
    check_launch("fft_cov_apply");
  }

  // ---- panels ----
  void lu_L(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host) override {
    lu_L_impl(Y, m, l, ld, ipiv_host, nullptr);
  }
  // every form below leaves its interchanges in ws_lu_ (untouched until the next factorization): no form declines
  bool lu_L_keep(double* Y, int64_t m, int64_t l, int64_t ld, int32_t** ipiv_dev) override {
    if (ipiv_dev == nullptr) return false;
    lu_L_impl(Y, m, l, ld, nullptr, ipiv_dev);
    return true;
  }
  void lu_L_impl(double* Y, int64_t m, int64_t l, int64_t ld, int32_t* ipiv_host, int32_t** ipiv_dev_out) {
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
      static const int nb_env = getenv("GSI_LU_NB") ? atoi(getenv("GSI_LU_NB")) : 0;
      w2.nb = (nb_env == 32 || nb_env == 64) ? nb_env : hipk::LU2_NB;
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
  // ---- row-sharded LU primitives ----
  int lus_block() const override { return hipk::LU2_NB; }
  struct LusWs { double* pval; int64_t* pidx; int32_t* ipiv; };
  LusWs lus_ws(int64_t, int64_t l) {
    // fixed layout: pivots (l <= 8188), then the per-workgroup partial arg-maxes (<= 1024 workgroups)
    if (l > 8188) throw Error(GSI_ERR_ARG, "sharded lu: sketch width too large");
    grow(ws_lus_, 32768 + 2 * 8 * 1024 + 64);
    char* base = (char*)ws_lus_.p;
    LusWs w;
    w.ipiv = (int32_t*)base;
    w.pval = (double*)(base + 32768);
    w.pidx = (int64_t*)(base + 32768 + 8 * 1024);
    return w;
  }
  void lus_u12_leaf(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w, double* U12) override {
    bind();
    hipk::lus_u12_leaf(st_, Yloc, ld, row0, jb, j0, w, U12);
    check_launch("lus_u12_leaf");
  }
  void lus_pending(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int64_t j0, int w,
                   const double* U12) override {
    bind();
    if (mloc > 0) hipk::lus_pending(st_, Yloc, ld, mloc, row0, jb, j0, w, U12);
    check_launch("lus_pending");
  }
  void lus_candidate(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j, double* rec) override {
    bind();
    LusWs w = lus_ws(mloc, l);
    // the previous pivot step's apply kernel may already have left this column's per-workgroup partials (same panel, same rows)
    const bool ready = (lus_part_col_ == j && lus_part_Y_ == Yloc && lus_part_mloc_ == mloc);
    lus_part_col_ = -1;
    hipk::lus_candidate(st_, Yloc, ld, mloc, row0, l, j, rec, w.pval, w.pidx, ready);
    check_launch("lus_candidate");
  }
  void lus_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t j0, int s, int w,
                 const double* recs, int nranks) override {
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
  void lus_u12_block(const double* Yloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t c1,
                     double* U12) override {
    bind();
    hipk::lus_u12_block(st_, Yloc, ld, row0, jb, b, c0, c1, U12);
    check_launch("lus_u12_block");
  }
  void lus_rankk(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t jb, int b, int64_t c0, int64_t t,
                 const double* U12) override {
    bind();
    hipk::lus_rankk(st_, Yloc, ld, mloc, row0, jb, b, c0, t, U12);
    check_launch("lus_rankk");
  }
  void lus_finish(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l) override {
    bind();
    hipk::lus_finish(st_, Yloc, ld, mloc, row0, l);
  }
  bool lus_mr_begin(Comm* comm, int64_t m, int64_t l) override {
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
  int64_t lus_mr_signature() override {
    return ((((int64_t)mr_work_.bs * 64 + mr_work_.rpt) * 1024 + mr_work_.grid) * 2 + mr_work_.hier) * 2 + mr_work_.ov;
  }
  const char* lus_mr_reason() override { return mr_reason_.c_str(); }
  int64_t lus_mr_generation() override { return mr_gen_; }
  // Every kernel of the persistent-leaf factorization once, on private dummies (a 64-row panel, a record buffer of its
  // own, its own info word), with the geometry flags of the form that is about to run: what a first launch may cost the
  // runtime -- loading the code object, growing the queue's scratch (the overflow-row leaves spill) -- happens here,
  // before the ranks' barrier, and not while a peer's leaf spins for this rank's launch.  Once per instantiation.
  void lus_mr_warmup() override {
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
  void lu_flag_export(double* flag) override {
    bind();
    hipk::lu_flag_export(st_, flags_ + FLAG_LU_INFO, flag);
  }
  void lu_flag_import(const double* flag) override {
    bind();
    hipk::lu_flag_import(st_, flags_ + FLAG_LU_INFO, flag);
    check_launch("lu_flag_import");
  }
  void lus_leaf_mr(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t m, int64_t l, int64_t jb, int64_t j0, int w,
                   const double* U12) override {
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
  bool lus_mr_swaps_done() override { return mr_peer_swaps_; }
  int lus_mr_mode() override { return mr_work_.ov ? 2 : (mr_work_.hier ? 1 : 0); }
  void lus_mr_force(int mode) override { mr_force_ = mode; }
  void lus_swap_pack(const double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                     double* table) override {
    bind();
    hipk::lus_swap_pack(st_, Yloc, ld, mloc, row0, l, j0, w, lus_ws(mloc, l).ipiv, table);
    check_launch("lus_swap_pack");
  }
  void lus_swap_apply(double* Yloc, int64_t mloc, int64_t ld, int64_t row0, int64_t l, int64_t j0, int w,
                      const double* table) override {
    bind();
    if (mloc > 0) hipk::lus_swap_apply(st_, Yloc, ld, mloc, row0, l, j0, w, lus_ws(mloc, l).ipiv, table);
    check_launch("lus_swap_apply");
  }
  void lus_pivots(int32_t* host, int64_t l) override {
    bind();
    LusWs w = lus_ws(1, l);
    HIP_CHECK(hipMemcpyAsync(host, w.ipiv, sizeof(int32_t) * l, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  // ---- the first CholeskyQR tier, as qr_thinQ, qr_thinQ_deferred and svd_tall_fused all try it ----
  bool cholqr_gate(int64_t m, int64_t l) {
    static const bool no_cholqr = (getenv("GSI_NO_CHOLQR") != nullptr);
    return !no_cholqr && l <= 1024 && m >= 2 * l;
  }
  // contraction workspace: the Gram matrix (upper tiles, or the dedicated kernel's slab partials), Y R^-1, the l x l inverse
  static size_t cholqr_ws_doubles(int64_t m, int64_t l) {
    return std::max({hipk::gemm_workspace_doubles(l, l, m), hipk::gemm_syrk_workspace_doubles(l, m), hipk::syrk_upper_workspace_doubles(l, m),
                     hipk::gemm_workspace_doubles(m, l, l), hipk::gemm_workspace_doubles(l, 32, l)});
  }
  int32_t read_flag(int slot) {                             // one 4-byte read-back: the stream is idle afterwards
    int32_t f = 0;
    HIP_CHECK(hipMemcpyAsync(&f, flags_ + slot, sizeof(int32_t), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    return f;
  }
  // Both rounds out of place: Y is read only, T = Y R1^-1 (ld ldt) and the small factors are what a true leaves behind.  A
  // false sets the caller's hint: the next eight factorizations of this kind do not try this tier.
  bool cholqr2_try(const double* Y, int64_t m, int64_t l, int64_t ld, double* T, int64_t ldt, double* small, double* ws, int& skip) {
    HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
    hipk::cholqr2_factor(st_, Y, m, l, ld, T, ldt, small, flags_ + FLAG_CHOLQR, ws);
    check_launch("cholqr2_factor");
    if (read_flag(FLAG_CHOLQR) == 0) return true;
    skip = 8;
    return false;
  }
  void qr_thinQ(double* Y, int64_t m, int64_t l, int64_t ld, double* R, bool replicated) override {
    bind();
    const int64_t nb = hipk::qr_max_blocks(m);
    const int NB = hipk::QR_NB;
    const int64_t npan = (l + NB - 1) / NB;
    size_t cnt = 0;
    auto take = [&](size_t c) { size_t o = cnt; cnt += (c + 7) & ~(size_t)7; return o; };
    const size_t o_coef = take(2 + NB + 2), o_part = take((size_t)nb * NB), o_tau = take(l),
                 o_T = take((size_t)npan * NB * NB), o_G = take(NB * NB),
                 o_Wt = take((size_t)l * NB), o_W2 = take((size_t)l * NB), o_small = take(hipk::cholqr_small_doubles(l)),
                 o_Q = take((size_t)(m + 1) * l);
    grow(ws_qr_, cnt * sizeof(double));
    TrimGuard trim_qr{this, &ws_qr_}, trim_hh{this, &ws_qr_hh_};
    double* base = (double*)ws_qr_.p;
    hipk::QrWork w;
    w.coef = base + o_coef; w.part = base + o_part; w.tau = base + o_tau; w.T = base + o_T; w.G = base + o_G;
    w.Vbuf = nullptr; w.Wt = base + o_Wt; w.W2 = base + o_W2; w.Qo = base + o_Q; w.maxblocks = nb;
    // gemm shapes inside: (t x NB, K = m), (NB x NB, K = m), (m x t, K = NB), (l x l, K = m), (m x 32, K <= l)
    size_t gmax = std::max({hipk::gemm_workspace_doubles(l, NB, m), hipk::gemm_workspace_doubles(NB, NB, m), cholqr_ws_doubles(m, l)});
    for (int64_t t = NB; t <= l; t += NB) gmax = std::max(gmax, hipk::gemm_workspace_doubles(t, NB, m));
    double* ws = gemm_ws(gmax + 64);
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
    hipk::qr_thinQ(st_, Y, m, l, ld, R, w, ws);
    check_launch("qr_thinQ");
  }
  // CholeskyQR2 stopped one tall product short (Backend::qr_thinQ_deferred): T = Y R1^-1 stays in the QR workspace, X2 = R2^-1
  // goes to the caller.  Only the first tier (the guard of qr_thinQ decides: a panel that needs the shifted tier or
  // Householder gets its Q the ordinary way), and only while the workspace is one this backend keeps between calls.
  bool qr_thinQ_deferred(const double* Y, int64_t m, int64_t l, int64_t ld, const double** Q1, int64_t* ldq1, double* X2) override {
    bind();
    static const bool off = (getenv("GSI_NO_QR_DEFER") != nullptr);
    if (off || !cholqr_gate(m, l)) return false;
    const int64_t ldt = (m + 1) & ~(int64_t)1;
    if ((size_t)ldt * l * sizeof(double) > ((size_t)8 << 30)) return false;       // trimmed on return: nothing would be left to hand out
    int& skip_tier1 = skip_tier1_by_height_[std::make_pair(m, false)];
    if (skip_tier1 > 0) return false;
    size_t cnt = 0;
    auto take = [&](size_t c) { size_t o = cnt; cnt += (c + 7) & ~(size_t)7; return o; };
    const size_t o_small = take(hipk::cholqr_small_doubles(l)), o_T = take((size_t)ldt * l);
    grow(ws_qr_, cnt * sizeof(double));
    double* base = (double*)ws_qr_.p;
    double* ws = gemm_ws(cholqr_ws_doubles(m, l) + 64);
    if (!cholqr2_try(Y, m, l, ld, base + o_T, ldt, base + o_small, ws, skip_tier1)) return false;
    HIP_CHECK(hipMemcpyAsync(X2, hipk::cholqr2_X2(base + o_small, l), sizeof(double) * (size_t)l * l, hipMemcpyDeviceToDevice, st_));
    *Q1 = base + o_T; *ldq1 = ldt;
    ++n_cholqr_;
    return true;
  }
  // svd(B) for B = W' (RandMatFact.jl:86-88) without forming the thin Q of W: CholeskyQR2's first round leaves
  // T = W R1^-1 and R2, R2^-1; R = R2 R1 goes to the Jacobi SVD, and Z = T (R2^-1 (U sqrt(S))) is ONE tall product
  // (the generic path runs Y = T R2^-1 and Z = Y (U sqrt(S)): two).  Declines when CholeskyQR2 does not apply.
  bool svd_tall_fused(const double* W, int64_t m, int64_t l, int64_t ld, int64_t K_scale, double* V, int64_t ldv,
                      double* S, const double* Xr) override {
    bind();
    static const bool off = (getenv("GSI_NO_SVD_FUSION") != nullptr);
    if (off || !cholqr_gate(m, l)) return false;
    int& skip_tier1 = skip_tier1_by_height_[std::make_pair(m, false)];
    if (skip_tier1 > 0) return false;                       // this kind of panel needs the shifted tier: generic path
    const int64_t ldt = (m + 1) & ~(int64_t)1;
    size_t cnt = 0;
    auto take = [&](size_t c) { size_t o = cnt; cnt += (c + 7) & ~(size_t)7; return o; };
    const size_t o_small = take(hipk::cholqr_small_doubles(l)), o_R = take((size_t)l * l), o_U = take((size_t)l * l),
                 o_M = take((size_t)l * l), o_T = take((size_t)ldt * l);
    grow(ws_svdf_, cnt * sizeof(double));
    TrimGuard trim_svdf{this, &ws_svdf_};
    double* base = (double*)ws_svdf_.p;
    double* ws = gemm_ws(std::max(cholqr_ws_doubles(m, l), hipk::gemm_workspace_doubles(l, l, l)) + 64);
    phase_begin(PH_QR);
    if (!cholqr2_try(W, m, l, ld, base + o_T, ldt, base + o_small, ws, skip_tier1)) {
      phase_end(PH_QR);
      return false;                                         // W is untouched: the caller's generic path takes over
    }
    hipk::cholqr2_R(st_, l, base + o_small, base + o_R);    // R = R2 R1
    if (Xr != nullptr) {                                    // the SVD wanted is that of W Xr = Q (R Xr): one l x l product
      hipk::gemm_f64(st_, false, l, l, l, 1.0, base + o_R, l, Xr, l, 0.0, base + o_M, l, ws);
      HIP_CHECK(hipMemcpyAsync(base + o_R, base + o_M, sizeof(double) * (size_t)l * l, hipMemcpyDeviceToDevice, st_));
    }
    phase_end(PH_QR);
    ++n_cholqr_;
    phase_begin(PH_SVD);
    svd_small(base + o_R, l, base + o_U, S);
    if (K_scale >= 0) hipk::scale_cols_sqrt(st_, base + o_U, l, S, K_scale);
    phase_end(PH_SVD);
    phase_begin(PH_SMALL_GEMM);
    hipk::gemm_f64(st_, false, l, l, l, 1.0, hipk::cholqr2_X2(base + o_small, l), l, base + o_U, l, 0.0, base + o_M, l, ws);
    // Z = V sqrt(S) has its last p columns ZERO by definition (RandMatFact.jl:87): they are not multiplied out (a fifth of
    // the product at K = 256, p = 64), they are cleared
    const int64_t lz = (K_scale >= 0 && K_scale < l) ? K_scale : l;
    hipk::gemm_f64(st_, false, m, lz, l, 1.0, base + o_T, ldt, base + o_M, l, 0.0, V, ldv, ws);
    if (lz < l) HIP_CHECK(hipMemsetAsync(V + (size_t)lz * ldv, 0, sizeof(double) * ((size_t)(l - lz - 1) * ldv + m), st_));
    check_launch("svd_tall_fused");
    phase_end(PH_SMALL_GEMM);
    return true;
  }
  // G = S'S of a LowRankCovMatrix's samples: the upper tiles of the general contraction (fixed K split: the same bits on
  // every call), mirrored.  2 n N^2 flop less the skipped lower tiles, once per operator (pipeline.cpp caches it).
  bool sample_gram(const double* S, int64_t ld, int64_t n, int64_t N, double* G) override {
    bind();
    if (n < 1 || N < 1) return false;
    double* ws = gemm_ws(hipk::gemm_syrk_workspace_doubles(N, n) + 64);
    hipk::gemm_f64_syrk_upper(st_, N, n, S, ld, G, N, ws);
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
  // The overlap.  Between the last Gram round and M = (XW2 U sqrt(S))[:, 0:K] lies a chain of small dependent launches (the
  // Cholesky, the Jacobi sweeps) on a few workgroups, and behind it the one tall product.  C = B1 M, and B1 is known before the
  // chain: Y_f = S[0:n_f] B1 (n_f x l) is formed on the side stream while the chain runs, on all but TAIL_RESERVE_CUS CUs
  // (hipk::gemm_f64_nn_capped), and those rows of Z then cost a reduction of length l instead of N: Z[0:n_f] = Y_f M.  The rows
  // from n_f on are the row block of today's product (the same tiles in the same order: the same bits).  n_f is a multiple of
  // the contraction's row tile fixed by (n, the fraction), so repeated calls give the same bits.  Y_f goes into `scratch` (the
  // caller's dead panel) or a pooled temporary.  On by default where the capped product runs persistent;
  // GSI_LOWRANK_TAIL_OVERLAP=0 switches it off, =<fraction in (0, 1)> forces that row fraction on any shape the capped
  // launch takes.
  // Both constants were measured at the headline: with 8 or 16 CUs left free the first kernel behind the
  // fork waited for the whole side product; 0.40 n rows at 224 CUs end just before M is ready (0.34 and 0.46 were slower).
  static constexpr double TAIL_OVERLAP_FRACTION = 0.40;
  static constexpr int TAIL_RESERVE_CUS = 32;
  bool lowrank_tail(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T, int64_t l,
                    int64_t K, double c, double* Z, int64_t ldz, double* Sv, double* scratch, size_t scratch_doubles) override {
    bind();
    if (!cholqr_gate(n, l) || l < 1 || l > 384 || l > N - 1 || K < 1 || K > l || N > 4096) return false;
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
    const size_t Nl = ((size_t)N * l + 7) & ~(size_t)7, ll = ((size_t)l * l + 7) & ~(size_t)7;
    Scratch buf(this, 3 * Nl + 12 * ll);
    const int cap = std::max(8, ((ncus_ - reserve) / 8) * 8);
    int64_t nf = 0;
    if (ov_env != 0.0) {
      nf = (int64_t)((ov_env > 0.0 ? ov_env : TAIL_OVERLAP_FRACTION) * (double)n) / 128 * 128;
      if (nf >= n) nf = (n - 1) / 128 * 128;
    }
    double* A0 = buf.p;                 // c T; then B0; then C
    double* A1 = A0 + Nl;               // A0 X1; then B1
    double* P = A1 + Nl;                // G times the current coefficients
    double* Gr[4];                      // the four Gram matrices, each R in place afterwards
    for (int i = 0; i < 4; ++i) Gr[i] = P + Nl + (size_t)i * ll;
    double* X[4];                       // X1, X2, XW1, XW2
    for (int i = 0; i < 4; ++i) X[i] = P + Nl + (size_t)(4 + i) * ll;
    double* R = P + Nl + 8 * ll;
    double* Rf = R + ll;
    double* U = Rf + ll;
    double* Mm = U + ll;
    size_t gmax = hipk::gemm_workspace_doubles(N, l, N);
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(l, l, N));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, l));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(l, l, l));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, K, l));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(n, K, N));
    if (nf >= 128) {
      // (the capped launch reads its operands' alignment: A1 is where B1 will be)
      hipk::GemmPlan plan = {0, 0, 0, 0, 0, 0, 0, 0};
      const bool takes = hipk::gemm_f64_nn_capped(st_, nf, l, N, Sm, lds, A1, N, A1, nf, cap, true, &plan);
      if (!takes || (ov_env < 0.0 && plan.persistent == 0)) nf = 0;
    } else {
      nf = 0;
    }
    Scratch own(this, (nf > 0 && (scratch == nullptr || scratch_doubles < (size_t)nf * (size_t)l)) ? (size_t)nf * (size_t)l : 0);
    double* Yf = (nf > 0) ? (own.p != nullptr ? own.p : scratch) : nullptr;      // nf x l, ld nf
    if (nf > 0) gmax = std::max(gmax, hipk::gemm_workspace_doubles(nf, K, l));
    double* ws = gemm_ws(gmax + 64);
    SideJoin side(this);                                    // (after every buffer the side stream touches: joined before they go)
    // one round on the panel S M: P = G M, Gram = M'P, R = chol(Gram) in place, X = R^-1
    auto round = [&](const double* M, int i, bool check) {
      hipk::gemm_f64(st_, false, N, l, N, 1.0, G, N, M, N, 0.0, P, N, ws);
      hipk::gemm_f64(st_, true, l, l, N, 1.0, M, N, P, N, 0.0, Gr[i], l, ws);
      (void)hipk::cq_gram_round(st_, Gr[i], l, X[i], check, flags_ + FLAG_CHOLQR);
    };
    phase_begin(PH_QR);
    HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOLQR, 0, sizeof(int32_t), st_));
    hipk::scal_copy(st_, (int64_t)N * l, c, T, A0);                                          // Y = S A0
    round(A0, 0, false);
    hipk::gemm_f64(st_, false, N, l, l, 1.0, A0, N, X[0], l, 0.0, A1, N, ws);               // Q1 = Y R1^-1 = S A1
    round(A1, 1, true);                                                                       // X2 = R2^-1: Q = Q1 X2
    hipk::scal_copy(st_, (int64_t)N * l, c, P, A0);                                          // W = A'Q1 = S (c G A1) = S B0
    round(A0, 2, false);
    hipk::gemm_f64(st_, false, N, l, l, 1.0, A0, N, X[2], l, 0.0, A1, N, ws);               // W RW1^-1 = S B1
    round(A1, 3, true);
    check_launch("lowrank_tail");
    if (nf > 0) {
      side.fork();
      (void)hipk::gemm_f64_nn_capped(st2_, nf, l, N, Sm, lds, A1, N, Yf, nf, cap);        // Y_f = S[0:n_f] B1
      check_launch("lowrank_tail (side product)");
    }
    if (read_flag(FLAG_CHOLQR) != 0) {
      side.join();
      phase_end(PH_QR);
      return false;                                         // nothing of Z or Sv written: the caller's path takes over
    }
    hipk::tri_product(st_, Gr[3], Gr[2], l, R);                                               // R_W = RW2 RW1
    hipk::gemm_f64(st_, false, l, l, l, 1.0, R, l, X[1], l, 0.0, Rf, l, ws);                // svd(W X2) = svd(R_W X2)
    phase_end(PH_QR);
    n_cholqr_ += 2;
    phase_begin(PH_SVD);
    svd_small(Rf, l, U, Sv);
    hipk::scale_cols_sqrt(st_, U, l, Sv, K);
    phase_end(PH_SVD);
    phase_begin(PH_SMALL_GEMM);
    hipk::gemm_f64(st_, false, l, K, l, 1.0, X[3], l, U, l, 0.0, Mm, l, ws);                // XW2 U sqrt(S), first K columns
    hipk::gemm_f64(st_, false, N, K, l, 1.0, A1, N, Mm, l, 0.0, A0, N, ws);                 // C = B1 (XW2 U sqrt(S))
    if (nf > 0) {
      side.join();
      hipk::gemm_f64(st_, false, nf, K, l, 1.0, Yf, nf, Mm, l, 0.0, Z, ldz, ws);            // Z[0:n_f] = Y_f M
      hipk::gemm_f64_nn_rowblock(st_, n, nf, n - nf, K, N, Sm, lds, A0, N, Z, ldz, ws);     // Z[n_f:n] = S[n_f:n] C
      ++n_tail_overlaps_;
    } else {
      hipk::gemm_f64(st_, false, n, K, N, 1.0, Sm, lds, A0, N, 0.0, Z, ldz, ws);            // Z = S C
    }
    // the last l - K columns of Z are zero by definition (RandMatFact.jl:87)
    if (K < l) HIP_CHECK(hipMemsetAsync(Z + (size_t)K * ldz, 0, sizeof(double) * ((size_t)(l - K - 1) * ldz + n), st_));
    check_launch("lowrank_tail");
    phase_end(PH_SMALL_GEMM);
    return true;
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
  bool lowrank_power_step(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* G, const double* T,
                          const int32_t* ipiv, const double* L, int64_t ldl, int64_t l, double c, double* Tn) override {
    bind();
    static const bool trace = (getenv("GSI_LOWRANK_POWER_TRACE") != nullptr);
    constexpr int64_t NSAMPLE = 256;        // rows below the pivot block that the check also reads
    constexpr int NPARTS = 128;             // workgroups of the check (partial maxima)
    constexpr double CHECK_MAX = 1e-8;      // |(P S) C - L|max above this: the coefficients no longer reproduce L (declined)
    if (l < 1 || l > 384 || N < 1 || N > 4096 || n < 2 * l || n >= ((int64_t)1 << 31)) return false;
    const int64_t ns = std::min<int64_t>(NSAMPLE, n - l), nchk = l + ns;
    auto up8 = [](int64_t x) { return (x + 7) & ~(int64_t)7; };
    // gathered rows (ld ldr, every block starting on an even row): [0, 2l) D = S[perm(mv)] - S[mv]; [o_chk, o_chk + nchk)
    // (P S) of the check rows; [o_sm, o_sm + 2l) S[mv].  Rows past the nmv moved ones, and padding rows, are S[0] - S[0] = 0.
    const int64_t o_chk = up8(2 * l), o_sm = o_chk + up8(nchk), nr = o_sm + 2 * l, ldr = up8(nr);
    const size_t nidx = (size_t)(2 * ldr + nchk);
    const size_t ll = (size_t)up8(l * l), Nl = (size_t)up8(N * l);
    Scratch buf(this, 2 * ll + Nl + (size_t)ldr * (size_t)N + (size_t)ldr * (size_t)l + nidx + NPARTS + 2);
    double* Mp = buf.p;                     // S[perm(0:l)] T
    double* Ut = Mp + ll;                   // U' = (c L11^-1 Mp)', on and below its diagonal
    double* C = Ut + ll;                    // c T U^-1
    double* R = C + Nl;                     // the gathered rows
    double* E = R + (size_t)ldr * N;        // rows [0, o_chk + nchk) of R times C
    int64_t* idx_dev = reinterpret_cast<int64_t*>(E + (size_t)ldr * l);   // src, sub (ldr each), chk
    double* part = reinterpret_cast<double*>(idx_dev + nidx);
    int32_t* verdict = reinterpret_cast<int32_t*>(part + NPARTS);         // LU info, invalid pivot, nmv, 0
    const int64_t me = o_chk + nchk;
    size_t gmax = hipk::gemm_workspace_doubles(l, l, N);
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(me, l, N));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, N));
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l, 2 * l));
    double* ws = gemm_ws(gmax + 64);
    struct Verdict { double parts[NPARTS]; int32_t v[4]; };
    if (pin_power_ == nullptr) HIP_CHECK(hipHostMalloc(&pin_power_, sizeof(Verdict), hipHostMallocDefault));
    hipk::lr_compose(st_, ipiv, flags_ + FLAG_LU_INFO, n, l, nchk, o_chk, o_sm, ldr, idx_dev, idx_dev + ldr, idx_dev + 2 * ldr, verdict);
    hipk::lr_gather_rows(st_, Sm, lds, N, idx_dev, idx_dev + ldr, nr, R, ldr);
    hipk::gemm_f64(st_, false, l, l, N, 1.0, R + o_chk, ldr, T, N, 0.0, Mp, l, ws);          // S[perm(0:l)] T
    hipk::lr_solve_u(st_, L, ldl, Mp, l, c, Ut);                                               // U = c L11^-1 Mp
    hipk::lr_solve_c(st_, Ut, l, T, N, c, C);                                                  // C U = c T
    hipk::gemm_f64(st_, false, me, l, N, 1.0, R, ldr, C, N, 0.0, E, ldr, ws);                // [D; (P S)_chk] C
    hipk::lr_check_rows(st_, E + o_chk, ldr, L, ldl, idx_dev + 2 * ldr, nchk, l, part, NPARTS);
    hipk::gemm_f64(st_, false, N, l, N, 1.0, G, N, C, N, 0.0, Tn, N, ws);                    // G C
    hipk::gemm_f64(st_, true, N, l, 2 * l, 1.0, R + o_sm, ldr, E, ldr, 1.0, Tn, N, ws);      // + S[mv]' (D C)
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
  static constexpr int64_t SPLIT_MAX_L1 = 192;
  struct SplitWs { int32_t* piv; int32_t* verdict1; int32_t* verdict2; int64_t* idx1; int64_t o_chk, o_sm, ldr; };
  static int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }
  SplitWs split_ws(int64_t l1) {
    // lr_compose's lists for the first half: the moved rows at 0, its l1 pivot rows at o_chk (no sampled rows), S[mv] at o_sm
    SplitWs w;
    w.o_chk = up8(2 * l1); w.o_sm = w.o_chk + up8(l1); w.ldr = up8(w.o_sm + 2 * l1);
    grow(ws_split_, 2048 + sizeof(int64_t) * (size_t)(2 * up8(5 * SPLIT_MAX_L1 + 16) + SPLIT_MAX_L1));
    char* base = (char*)ws_split_.p;
    w.piv = (int32_t*)base;                               // [2 SPLIT_MAX_L1]
    w.verdict1 = (int32_t*)(base + 1536 + 64);
    w.verdict2 = w.verdict1 + 4;
    w.idx1 = (int64_t*)(base + 2048);                      // src, sub (ldr each), chk (l1)
    return w;
  }
  // Ranks that SHARE this device (the RCCL-free communicators, one-GPU rehearsals of a multi-GPU job) each factor their
  // replicated panel with a whole-chip grid of their own: the grids cannot all be resident, so the persistent kernels are
  // not candidates at all (seen: 2 rank processes on one GPU, gathered 10^6 x 320 panel: a poll time-out on some runs).
  bool lu2_resident_ok() const {
    static const bool tall_first = (getenv("GSI_LU_TALL") != nullptr && getenv("GSI_LU_TALL")[0] == '1');
    return !tall_first && !lu2_lost_ && ranks_sharing_device_ <= 1;
  }
  bool lu2_takes(int64_t m, hipk::Lu2Work* w) {           // lu_L_impl's first choice: the leaves held in registers (geometry in *w)
    return lu2_resident_ok() && hipk::lu2_config(m, ncus_, &w->bs, &w->rpt, &w->grid) && lu2_fits(w->bs, w->rpt, w->grid);
  }
  bool lowrank_split_ok(int64_t n, int64_t N, int64_t l, int64_t l1) override {
    bind();
    if (l1 < 1 || l1 > SPLIT_MAX_L1 || l <= l1 || l > 2 * l1 || l - l1 < 8 || l > 384 || N < 1 || N > 4096 || n < 2 * l ||
        n >= ((int64_t)1 << 31))
      return false;
    hipk::Lu2Work w;
    return lu2_takes(n, &w) && lu2_takes(n - l1, &w);
  }
  void lowrank_split_schur(const double* Sm, int64_t lds, int64_t n, int64_t N, const double* T, const int32_t* ipiv1,
                           const double* P, int64_t ldp, int64_t l, int64_t l1, double c, double* Tt) override {
    bind();
    const int64_t l2 = l - l1;
    const SplitWs w = split_ws(l1);
    const size_t l1l = (size_t)up8(l1 * l), Nl1 = (size_t)up8(N * l1);
    Scratch buf(this, (size_t)up8(l1) * (size_t)N + 2 * l1l + 8 + Nl1);
    double* R = buf.p;                      // S[perm(0:l1)] (l1 x N, ld up8(l1))
    double* Mp = R + (size_t)up8(l1) * N;   // R T (l1 x l)
    double* Ut11 = Mp + l1l;                // U11' (l1 x l1), then U12 (l1 x l2)
    double* U12 = Ut11 + (size_t)up8(l1 * l1);
    double* C1 = Mp + 2 * l1l + 8;          // c T1 U11^-1 (N x l1)
    size_t gmax = hipk::gemm_workspace_doubles(l1, l, N);
    gmax = std::max(gmax, hipk::gemm_workspace_doubles(N, l2, l1));
    double* ws = gemm_ws(gmax + 64);
    int64_t* src = w.idx1, * sub = w.idx1 + w.ldr, * chk = w.idx1 + 2 * w.ldr;
    hipk::lr_compose(st_, ipiv1, flags_ + FLAG_LU_INFO, n, l1, l1, w.o_chk, w.o_sm, w.ldr, src, sub, chk, w.verdict1);
    hipk::lr_pivots(st_, ipiv1, l1, 0, w.piv);                                                  // (the next LU reuses ws_lu_)
    hipk::lr_gather_rows(st_, Sm, lds, N, src + w.o_chk, sub + w.o_chk, l1, R, up8(l1));
    hipk::gemm_f64(st_, false, l1, l, N, 1.0, R, up8(l1), T, N, 0.0, Mp, l1, ws);             // S[perm(0:l1)] T
    hipk::lr_solve_u12(st_, P, ldp, Mp, l1, l, c, Ut11, U12);                                   // [U11 | U12] = c L11^-1 Mp
    hipk::lr_solve_c(st_, Ut11, l1, T, N, c, C1);                                               // C1 U11 = c T1
    hipk::scal_copy(st_, N * l2, c, T + (size_t)N * l1, Tt);
    hipk::gemm_f64(st_, false, N, l2, l1, -1.0, C1, N, U12, l1, 1.0, Tt, N, ws);              // c T2 - C1 U12
    check_launch("lowrank_split_schur");
  }
  void lowrank_split_rows(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1) override {
    bind();
    (void)n;
    const int64_t l2 = l - l1;
    const SplitWs w = split_ws(l1);
    Scratch tmp(this, (size_t)(2 * l1) * (size_t)l2);
    hipk::lr_move_rows(st_, P + (size_t)l1 * ldp, ldp, l2, w.idx1, w.idx1 + w.ldr, w.verdict1, 2 * l1, tmp.p, 2 * l1, l1);
    check_launch("lowrank_split_rows");
  }
  void lowrank_split_join(double* P, int64_t ldp, int64_t n, int64_t l, int64_t l1, const int32_t* ipiv2,
                          int32_t** ipiv) override {
    bind();
    const int64_t l2 = l - l1;
    const SplitWs w = split_ws(l1);
    const int64_t ldr = up8(4 * l2);        // the moved rows at 0 and S[mv] at 2 l2; no check rows
    Scratch buf(this, (size_t)(2 * ldr + 8) + (size_t)(2 * l2) * (size_t)l1);
    int64_t* src = reinterpret_cast<int64_t*>(buf.p), * sub = src + ldr, * chk = sub + ldr;
    double* tmp = buf.p + 2 * ldr + 8;
    hipk::lr_compose(st_, ipiv2, flags_ + FLAG_LU_INFO, n - l1, l2, 0, 2 * l2, 2 * l2, ldr, src, sub, chk, w.verdict2);
    hipk::lr_pivots(st_, ipiv2, l2, l1, w.piv + l1);
    hipk::lr_move_rows(st_, P + l1, ldp, l1, src, sub, w.verdict2, 2 * l2, tmp, 2 * l2, 0);
    check_launch("lowrank_split_join");
    *ipiv = w.piv;
  }
  void lowrank_split_undo() override {
    bind();
    hipk::lr_forget_zero_pivot(st_, flags_ + FLAG_LU_INFO);
    check_launch("lowrank_split_undo");
  }
  void svd_small(double* G, int64_t l, double* U, double* S) override {
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
  void chol_upper(double* B, int64_t j) override {
    bind();
    if (j > 2048) throw Error(GSI_ERR_ARG, "chol_upper: j too large");
    hipk::chol_upper(st_, B, j, flags_ + FLAG_CHOL_INFO);
    check_launch("chol_upper");
  }
  void trsm_right_upper(double* F, int64_t m, int64_t j, int64_t ldf, const double* C) override {
    bind();
    hipk::trsm_right_upper(st_, F, m, j, ldf, C);
    check_launch("trsm_right_upper");
  }
  void scale_cols_sqrt(double* U, int64_t l, const double* S, int64_t K) override {
    bind();
    hipk::scale_cols_sqrt(st_, U, l, S, K);
  }
  void center_rows(double* S, int64_t n, int64_t N, int64_t ld) override {
    bind();
    hipk::center_rows(st_, S, n, N, ld);
  }
  void randn(double* p, size_t count, uint64_t seed) override {
    bind();
    hipk::randn_fill(st_, p, count, seed);
  }
  void fill_gridcov(double* A, int64_t lda, int64_t nx, int64_t ny, double ell, int kind, int64_t row0,
                    int64_t mloc) override {
    bind();
    hipk::fill_gridcov(st_, A, lda, nx, ny, ell, kind, row0, mloc);
    check_launch("fill_gridcov");
  }
  void fill_lowrank_samples(double* S, int64_t ld, int64_t nloc, int64_t N, int64_t row0, uint64_t seed,
                            double decay) override {
    bind();
    hipk::fill_lowrank_samples(st_, S, ld, nloc, N, row0, seed, decay);
    check_launch("fill_lowrank_samples");
  }
  // Batches of fields: phi and the intermediate array of a batch stay within 2 GiB of workspace (GSI_FFTRF_BATCH=<b>, read
  // at every call, overrides the batch size).  Nothing a field computes depends on the batch it rides in.
  void fftrf_fields(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                    double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0) override {
    fftrf_batches(dst, ldd, row0, nloc, nf, ndims, N, k0, dk, beta, phi, ldphi, seed, field0, nullptr);
  }
  // The same batches, each field interpolated at the plan's points (fftrf_interp.hip) instead of copied out: the
  // normalising write goes to the field's own workspace (over its phi, dead after the first pass) and the gather reads it
  // there.  dst is plan.m_local x nf.
  void fftrf_fields_at(double* dst, int64_t ldd, int64_t nf, int ndims, const int64_t* N, double k0, double dk, double beta,
                       const double* phi, int64_t ldphi, uint64_t seed, int64_t field0, const FftrfPointsPlan& plan) override {
    fftrf_batches(dst, ldd, 0, 0, nf, ndims, N, k0, dk, beta, phi, ldphi, seed, field0, &plan);
  }
  void fftrf_interpolate(double* dst, int64_t ldd, int64_t nf, const double* grid, int64_t ldg,
                         const FftrfPointsPlan& plan) override {
    bind();
    if (nf <= 0 || plan.m_local <= 0) return;
    Scratch dplan(this, points_plan_doubles(plan));
    upload_points_plan(plan, dplan.p);
    for (int64_t f0 = 0; f0 < nf; f0 += 4096) {
      const int b = (int)((nf - f0 < 4096) ? (nf - f0) : 4096);
      interp_batch(plan, dplan.p, grid + f0 * ldg, ldg, b, dst + f0 * ldd, ldd);
    }
  }
 private:
  // the plan on the device: frac (ndims x m_local doubles), then base (m_local int32)
  static size_t points_plan_doubles(const FftrfPointsPlan& plan) {
    return (size_t)plan.m_local * plan.ndims + (size_t)(plan.m_local + 1) / 2;
  }
  void upload_points_plan(const FftrfPointsPlan& plan, double* d) {
    const int64_t m = plan.m_local, nfr = m * plan.ndims;
    upload2d(d, nfr, plan.frac.data(), nfr, nfr, 1);
    std::vector<double> packed((size_t)(m + 1) / 2, 0.0);
    std::memcpy(packed.data(), plan.base.data(), sizeof(int32_t) * (size_t)m);
    upload2d(d + nfr, (int64_t)packed.size(), packed.data(), (int64_t)packed.size(), (int64_t)packed.size(), 1);
  }
  void interp_batch(const FftrfPointsPlan& plan, const double* dplan, const double* V, int64_t v_fs, int nb, double* dst,
                    int64_t ldd) {
    const int64_t m = plan.m_local;
    hipk::fftrf_interp(st_, plan.ndims, reinterpret_cast<const int32_t*>(dplan + m * plan.ndims), dplan, m, plan.N[0],
                       plan.N[0] * plan.N[1], V, v_fs, nb, dst, ldd);
    check_launch("fftrf_interp");
  }
  void fftrf_batches(double* dst, int64_t ldd, int64_t row0, int64_t nloc, int64_t nf, int ndims, const int64_t* N, double k0,
                     double dk, double beta, const double* phi, int64_t ldphi, uint64_t seed, int64_t field0,
                     const FftrfPointsPlan* at) {
    bind();
    if (nf <= 0 || (at && at->m_local <= 0)) return;
    hipk::FftrfGeom g;
    hipk::fftrf_geometry(ndims, N, &g);
    int64_t fs = (int64_t)hipk::fftrf_field_doubles(g);
    fs += fs & 1;                                     // the complex array of every field 16-byte aligned
    int64_t nb = (((int64_t)2 << 30) / (int64_t)sizeof(double)) / fs;
    if (const char* e = getenv("GSI_FFTRF_BATCH")) { if (atoll(e) >= 1) nb = atoll(e); }
    if (nb > 4096) nb = 4096;
    if (nb > nf) nb = nf;
    if (nb < 1) nb = 1;
    Scratch plan(this, hipk::fftrf_plan_doubles(g)), ws(this, (size_t)(fs * nb));
    Scratch dplan(this, at ? points_plan_doubles(*at) : 0);
    if (at) upload_points_plan(*at, dplan.p);
    hipk::fftrf_plan(st_, g, plan.p);
    for (int64_t f0 = 0; f0 < nf; f0 += nb) {
      const int b = (int)((nf - f0 < nb) ? (nf - f0) : nb);
      if (phi) {
        if (f0 > 0) HIP_CHECK(hipStreamSynchronize(st_));      // the previous batch still reads the workspace
        upload2d(ws.p, fs, phi + f0 * ldphi, ldphi, g.Mtot, b);
      } else {
        for (int i = 0; i < b; ++i) hipk::randn_fill(st_, ws.p + (int64_t)i * fs, (size_t)g.Mtot, seed + (uint64_t)(field0 + f0 + i));
      }
      if (!at) {
        hipk::fftrf_sample(st_, g, plan.p, ws.p, fs, b, k0, dk, beta, dst + f0 * ldd, ldd, row0, nloc);
        check_launch("fftrf_sample");
      } else {
        hipk::fftrf_sample(st_, g, plan.p, ws.p, fs, b, k0, dk, beta, ws.p, fs, 0, g.n);   // field i: ws + i fs, n values
        check_launch("fftrf_sample");
        interp_batch(*at, dplan.p, ws.p, fs, b, dst + f0 * ldd, ldd);
      }
    }
  }
 public:
  void colnorms(const double* Y, int64_t m, int64_t c, int64_t ld, double* host_out) override {
    bind();
    if (c > 64) throw Error(GSI_ERR_ARG, "colnorms: at most 64 columns at a time");
    hipk::colnorms_sq(st_, Y, m, c, ld, scal_);
    HIP_CHECK(hipMemcpyAsync(host_out, scal_, sizeof(double) * c, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (int64_t i = 0; i < c; ++i) host_out[i] = std::sqrt(host_out[i]);
  }
  void axpy(int64_t n, double a, const double* x, double* y) override { bind(); hipk::axpy(st_, n, a, x, y); }
  double dot(int64_t n, const double* x, const double* y) override {
    bind();
    hipk::dot_dev(st_, n, x, y, scal_);
    double v = 0.0;
    HIP_CHECK(hipMemcpyAsync(&v, scal_, sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    return v;
  }
  double nrm2(int64_t n, const double* x) override { return std::sqrt(dot(n, x, x)); }
  void scal_copy(int64_t n, double a, const double* x, double* y) override {
    bind();
    hipk::scal_copy(st_, n, a, x, y);
  }
  void pcga_params(const double* Z, int64_t n, int64_t K, const double* s, const double* X, double delta,
                   double* out) override {
    bind();
    hipk::pcga_params(st_, Z, n, K, s, X, delta, out);
    check_launch("pcga_params");
  }
  void gemv_n(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double beta,
              double* y) override {
    bind();
    hipk::gemv_n(st_, m, k, alpha, A, lda, x, beta, y);
    check_launch("gemv_n");
  }
  void gemv_t(int64_t m, int64_t k, double alpha, const double* A, int64_t lda, const double* x, double* y) override {
    bind();
    grow(ws_blas2_, sizeof(double) * hipk::gemv_t_workspace_doubles(k));
    hipk::gemv_t(st_, m, k, alpha, A, lda, x, y, (double*)ws_blas2_.p);
    check_launch("gemv_t");
  }
  void project_out(int64_t m, int64_t ncols, const double* q, double* Y, int64_t ld) override {
    bind();
    if (ncols > 64) throw Error(GSI_ERR_ARG, "project_out: at most 64 columns at a time");
    grow(ws_blas2_, sizeof(double) * hipk::gemv_t_workspace_doubles(ncols));
    hipk::project_out(st_, m, ncols, q, Y, ld, (double*)ws_blas2_.p);
    check_launch("project_out");
  }
  void scal(int64_t n, double a, double* x) override { bind(); hipk::scal(st_, n, a, x); }
  void diag_mul_add(int64_t n, const double* d, const double* x, double* y) override {
    bind();
    hipk::diag_mul_add(st_, n, d, x, y);
  }
  size_t lsqr_work_doubles() override { return hipk::lsqr_work_doubles(); }
  void lsqr_begin(int64_t n, const double* w, double* work) override {
    bind();
    hipk::lsqr_begin(st_, n, w, work);
    check_launch("lsqr_begin");
  }
  void lsqr_step_u(int64_t m, const double* t, double* u, double* work) override {
    bind();
    hipk::lsqr_step_u(st_, m, t, u, work);
    check_launch("lsqr_step_u");
  }
  void lsqr_step_v(int64_t n, const double* t, double* v, double* w, double* x, double* work) override {
    bind();
    hipk::lsqr_step_v(st_, n, t, v, w, x, work);
    check_launch("lsqr_step_v");
  }
  void f64_to_f32(const double* src, void* dst32, size_t count) override {
    bind();
    hipk::f64_to_f32(st_, src, (float*)dst32, count);
    check_launch("f64_to_f32");
  }
  void pcga_params_f32(const void* Z32, int64_t n, int64_t K, const double* s, const double* X, double delta,
                       double* out) override {
    bind();
    hipk::pcga_params_f32(st_, (const float*)Z32, n, K, s, X, delta, out);
    check_launch("pcga_params_f32");
  }
  void basis_gemv_f32(const void* Z32, int64_t n, int64_t K, const double* w, double beta, const double* X,
                      double* y) override {
    bind();
    if (K > 8000) throw Error(GSI_ERR_ARG, "basis_gemv_f32: K too large for the LDS-resident weights");
    hipk::basis_gemv_f32(st_, (const float*)Z32, n, K, w, beta, X, y);
    check_launch("basis_gemv_f32");
  }
  // The sparse forward model (pcga_forward.hip).  The form follows the mean segment length: FWD_WAVE_MIN nonzeros and more
  // go one wave per segment, shorter ones one lane per output (the crossover of the sweep in profiles/pcga_forward.json:
  // 4096 rays of 16 cells run 0.65 ms in the wave form against 0.83 ms, rays of 4 cells 0.66 against 0.62;
  // DESIGN.md section 4.7b).  GSI_FWD_FORM=lane|wave, read at every call, overrides.
  static constexpr int64_t FWD_WAVE_MIN = 16;
  int fwd_products(const FwdProduct& a) override {
    bind();
    int form = (a.nseg > 0 && a.nnz / a.nseg >= FWD_WAVE_MIN) ? 2 : 1;
    if (const char* e = getenv("GSI_FWD_FORM")) {
      const std::string f(e);
      if (f == "lane") form = 1;
      else if (f == "wave") form = 2;
      else if (!f.empty()) throw Error(GSI_ERR_ARG, "GSI_FWD_FORM must be lane or wave, not '" + f + "'");
    }
    if (form == 1) hipk::fwd_lane(st_, a);
    else hipk::fwd_wave(st_, a);
    check_launch(form == 1 ? "fwd_lane" : "fwd_wave");
    if (a.rowseg) {
      hipk::fwd_reduce(st_, a);
      check_launch("fwd_reduce");
    }
    return form;
  }

  // The blocked Cholesky and the saddle-point solve (chol_saddle.hip).  The pivot flag has a slot
  // of its own behind the error words: the caller gets the column as a return value, not through take_error.
  int64_t chol_lower(double* A, int64_t m, int64_t n, int64_t ld) override {
    bind();
    if (n < 1 || m < n || ld < m || n >= ((int64_t)1 << 31)) throw Error(GSI_ERR_ARG, "chol_lower: need 1 <= n <= m <= ld, n < 2^31");
    HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOL_LOWER, 0, sizeof(int32_t), st_));
    hipk::cs_chol_lower(st_, A, m, n, ld, flags_ + FLAG_CHOL_LOWER);
    check_launch("chol_lower");
    return read_flag(FLAG_CHOL_LOWER);
  }
  int64_t saddle_solve(const double* E, int64_t nobs, int64_t K, const double* HX, const double* R, bool r_diag, const double* b,
                       double* x, bool* singular) override {
    bind();
    const int64_t ld = nobs + 2;
    Scratch W(this, (size_t)ld * nobs);
    HIP_CHECK(hipMemsetAsync(flags_ + FLAG_CHOL_LOWER, 0, sizeof(int32_t), st_));
    phase_begin(PH_SMALL_GEMM);                              // (profiling: the formation counts as a small product ...
    hipk::cs_syrk_lower(st_, W.p, ld, nobs, nobs, E, nobs, K, 1.0, 0.0, R, nobs, r_diag ? 2 : 1, flags_ + FLAG_CHOL_LOWER);
    hipk::cs_set_rows(st_, W.p, ld, nobs, HX, b);
    phase_end(PH_SMALL_GEMM);
    phase_begin(PH_OTHER);                                   // ... the factorization as "other": tools/pcga_direct_bench.py)
    hipk::cs_chol_lower(st_, W.p, nobs + 2, nobs, ld, flags_ + FLAG_CHOL_LOWER);
    phase_end(PH_OTHER);
    check_launch("saddle_solve: factorization");
    const int64_t col = read_flag(FLAG_CHOL_LOWER);
    *singular = false;
    if (col != 0) return col;
    hipk::cs_schur(st_, W.p, ld, nobs, b, x, scal_);
    grow(ws_blas2_, sizeof(double) * hipk::cs_backsolve_workspace_doubles());
    hipk::cs_backsolve(st_, W.p, nobs, ld, x, (double*)ws_blas2_.p);
    check_launch("saddle_solve: substitution");
    double out3[3] = {0.0, 0.0, 0.0};
    HIP_CHECK(hipMemcpyAsync(out3, scal_, sizeof(out3), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    *singular = (out3[2] == 0.0);
    return 0;
  }

  // The row pass of the posterior variance (posterior_var.hip).
  int basis_quadform(const void* Z, int zbits, int64_t n, int64_t ldz, int64_t K, const double* W, int64_t ldw, int64_t ncols,
                     bool upper, const double* u, double* a, double* q, double* t) override {
    bind();
    if (n < 1 || K < 1 || ncols < 1 || ldz < n || ldw < K || (zbits != 64 && zbits != 32) || (u == nullptr) != (t == nullptr))
      throw Error(GSI_ERR_ARG, "basis_quadform: need n, K, ncols >= 1, ldz >= n, ldw >= K, 32 or 64 bits, u and t together");
    hipk::pv_quadform(st_, Z, zbits, n, ldz, K, W, ldw, ncols, upper, u, a, q, t);
    check_launch("basis_quadform");
    return 1;
  }
  int scale_rows(int64_t m, int64_t c, const double* d, const double* src, int64_t lds, double* dst, int64_t ldd) override {
    bind();
    hipk::pv_scale_rows(st_, m, c, d, src, lds, dst, ldd);
    check_launch("scale_rows");
    return 1;
  }

  // The persistent leaf kernel spins on records of ALL its workgroups: the grid must fit the chip at this kernel's
  // occupancy (registers, LDS, waves).  Queried once per instantiation; a panel that does not fit takes the streamed leaves.
  bool lu2_fits(int bs, int rpt, int grid) {
    const int key = bs * 16 + rpt;
    auto it = lu2_resident_.find(key);
    if (it == lu2_resident_.end()) it = lu2_resident_.emplace(key, hipk::lu2_resident_per_cu(bs, rpt)).first;
    return (int64_t)it->second * ncus_ >= grid;
  }
  void forgive_lost_coresidency() override {
    bind();
    (void)hipMemsetAsync(flags_, 0, FLAG_ERROR_WORDS * sizeof(int32_t), st_);
    lu2_lost_ = false;
    lu2_retry_ = false;          // (mr_disabled_ stays as the self-test left it)
  }
  bool retryable_failure() override {
    const bool r = lu2_retry_;
    lu2_retry_ = false;
    return r;
  }

  int take_error(std::string* msg) override {
    bind();
    int32_t h[FLAG_COUNT];
    HIP_CHECK(hipMemcpyAsync(h, flags_, sizeof(h), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    if (st2_) HIP_CHECK(hipStreamSynchronize(st2_));   // (idle unless a call ended in an exception between fork and join)
    HIP_CHECK(hipGetLastError());
    if (!garbage_.empty()) collect_garbage();
    const int32_t lu = h[FLAG_LU_INFO], chol = h[FLAG_CHOL_INFO];
    if (lu >= 0) mr_in_flight_ = false;
    if (lu != 0 || chol != 0) {
      HIP_CHECK(hipMemsetAsync(flags_, 0, FLAG_ERROR_WORDS * sizeof(int32_t), st_));
      if (lu < 0) {
        // co-residency of the persistent leaf kernel was lost (a workgroup never got a CU: the GPU is shared with
        // another queue).  The panel of that factorization is destroyed; this context factors with
        // streamed leaves (no spin-waits between workgroups) from now on, and the entry point may be re-run on its inputs.
        lu2_lost_ = true;
        lu2_retry_ = true;
        ++n_lu_timeouts_;
        if (mr_in_flight_) {
          // a multi-rank factorization: the flag was made global on the stream (pipeline.cpp: lu_flag_export / _import), so
          // EVERY rank is here in the same call, switches the in-kernel exchange off and voids the ranks' agreements
          mr_disabled_ = true;
          mr_why_disabled_ = "a pivot exchange between the ranks' kernels timed out";
          ++mr_gen_;
        }
        mr_in_flight_ = false;
        if (msg) *msg = "lu(): the pivot exchange between workgroups timed out (GPU shared with another job?); "
                        "this context now streams its leaves (no spin-waits) [waited for: phase " + std::to_string(h[FLAG_WAIT_PHASE]) +
                        ", slot " + std::to_string(h[FLAG_WAIT_SLOT]) + ", epoch " + std::to_string(h[FLAG_WAIT_EPOCH]) +
                        ", by rank*1024+workgroup " + std::to_string(h[FLAG_WAIT_WHO]) + "]";
        return GSI_ERR_INTERNAL;
      }
      if (lu != 0) {
        if (msg) *msg = "SingularException(" + std::to_string(lu) + "): exactly zero pivot in lu()";
        return GSI_ERR_SINGULAR;
      }
      if (msg) *msg = "PosDefException: matrix is not positive definite; Cholesky failed at " + std::to_string(chol);
      return GSI_ERR_NOT_POSDEF;
    }
    return 0;
  }

  // ---- profiling ----
  void profile(bool on) override { prof_ = on; }
  void phase_begin(Phase p) override {
    if (!prof_) return;
    bind();
    if (roctx().push) roctx().push(kPhaseNames[p]);
    cur_.phase = p;
    cur_.a = get_event();
    cur_.b = get_event();
    hipEventRecord(cur_.a, st_);
  }
  void phase_end(Phase) override { phase_end_counted(true); }
  void phase_end_more(Phase) override { phase_end_counted(false); }
  void phase_end_counted(bool counted) {
    if (!prof_) return;
    if (roctx().pop) roctx().pop();
    hipEventRecord(cur_.b, st_);
    cur_.counted = counted;
    records_.push_back(cur_);
  }
  void phase_reset() override {
    bind();
    hipStreamSynchronize(st_);
    for (auto& r : records_) { ev_pool_.push_back(r.a); ev_pool_.push_back(r.b); }
    records_.clear();
    for (int i = 0; i < PH_COUNT; ++i) { acc_ms_[i] = 0.0; acc_n_[i] = 0; }
  }
  void phase_times(double* ms, int64_t* counts) override {
    bind();
    hipStreamSynchronize(st_);
    for (auto& r : records_) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { acc_ms_[r.phase] += t; acc_n_[r.phase] += r.counted ? 1 : 0; }
      ev_pool_.push_back(r.a);
      ev_pool_.push_back(r.b);
    }
    records_.clear();
    for (int i = 0; i < PH_COUNT; ++i) { ms[i] = acc_ms_[i]; counts[i] = acc_n_[i]; }
  }

  void counters(int64_t* out4) override {
    out4[0] = n_cholqr_; out4[1] = n_householder_; out4[2] = last_svd_sweeps_; out4[3] = n_scholqr3_;
  }
  int64_t lu_timeouts() override { return n_lu_timeouts_; }
  int64_t svd_cap_hits() override { return n_svd_cap_hits_; }
  int64_t lowrank_tail_overlaps() override { return n_tail_overlaps_; }
  void set_ranks_sharing_device(int n) override { ranks_sharing_device_ = n; }

 private:
  struct Rec { Phase phase; hipEvent_t a, b; bool counted; };
  hipEvent_t get_event() {
    if (!ev_pool_.empty()) { hipEvent_t e = ev_pool_.back(); ev_pool_.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
  }
  void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw Error(GSI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  // Cached workspaces make repeated factorizations allocation-free; one of panel size at 512^3 (tens of GB) would
  // instead starve the next phase, so anything above 8 GiB is given back when the call that grew it returns.
  // A workspace that is outgrown is not freed on the spot: hipFree waits for the whole DEVICE, and with the ranks of a
  // communicator as threads of one process (GSI_LOCAL_COMM) another rank's persistent LU kernel may at that moment be
  // spinning for a record of the very kernel this thread is about to launch -- a dead-lock that ends in the kernel's poll
  // time-out (seen once in five runs of test_multirank_pipeline_on_one_gpu[3]: rank B grew ws_lu_ inside the sharded LU
  // while rank A's first leaf was already waiting for it).  The block waits in garbage_ until this context's call has
  // finished its own device work (take_error: whatever still spins for us has all it needs by then).
  void free_ws(DevBuf& b) {
    if (!b.p) return;
    if (b.pooled) release((double*)b.p);       // back to the block cache (stream-ordered: no synchronisation)
    else { std::lock_guard<std::mutex> g(mu_); garbage_.push_back(b.p); garbage_bytes_ += b.bytes; }
    b.p = nullptr; b.bytes = 0; b.pooled = false;
  }
  void collect_garbage() {                     // caller: this context's stream is idle
    std::vector<void*> g;
    { std::lock_guard<std::mutex> lk(mu_); g.swap(garbage_); garbage_bytes_ = 0; }
    for (void* p : g) (void)hipFree(p);
  }
  void trim(DevBuf& b) {
    if (b.bytes <= ((size_t)8 << 30) || !b.p) return;
    free_ws(b);
  }
  struct TrimGuard { HipBackend* be; DevBuf* b; ~TrimGuard() { be->trim(*b); } };
  void grow(DevBuf& b, size_t bytes) {
    if (bytes <= b.bytes) return;
    if (bytes > ((size_t)1 << 30)) {             // panel-sized: from the block cache, where a just-released panel usually waits
      free_ws(b);
      b.p = alloc((bytes + 7) / 8);
      b.bytes = bytes;
      b.pooled = true;
      return;
    }
    free_ws(b);
    bytes = (bytes + 4095) & ~(size_t)4095;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {   // give the cache of released panels back and retry once (the other phases' workspaces may be
      (void)hipGetLastError();   // in use by the caller: they stay)
      (void)hipStreamSynchronize(st_);
      drain_side();
      collect_garbage();
      trim_pool(0);
      e = hipMalloc(&b.p, bytes);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      b.p = nullptr;
      throw Error(GSI_ERR_OOM, "workspace hipMalloc of " + std::to_string(bytes) + " bytes failed");
    }
    b.bytes = bytes;
  }
  void drain_side() { if (st2_) (void)hipStreamSynchronize(st2_); }
  hipStream_t side_stream() {
    if (st2_ != nullptr) return st2_;
    int least = 0, greatest = 0;                  // (numerically larger = lower priority; st_ has the default, 0)
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least));
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) {
      if (a) hipEventDestroy(a);
      hipStreamDestroy(s);
      throw Error(GSI_ERR_HIP, "lowrank_tail: the side stream's events could not be created");
    }
    st2_ = s; ev_fork_ = a; ev_join_ = b;
    return st2_;
  }
  // Joins the side stream into st_ on every way out of the scope that forked it.  join(): the ordinary way (st_ waits for what
  // the side stream was given; the host does not).  Left to the destructor -- an exception is in flight -- the host waits too.
  struct SideJoin {
    HipBackend* be; bool open = false;
    explicit SideJoin(HipBackend* b) : be(b) {}
    void fork() {
      hipStream_t s2 = be->side_stream();
      HIP_CHECK(hipEventRecord(be->ev_fork_, be->st_));
      HIP_CHECK(hipStreamWaitEvent(s2, be->ev_fork_, 0));
      open = true;
    }
    void join() {
      if (!open) return;
      open = false;
      HIP_CHECK(hipEventRecord(be->ev_join_, be->st2_));
      HIP_CHECK(hipStreamWaitEvent(be->st_, be->ev_join_, 0));
    }
    ~SideJoin() {
      if (!open) return;
      if (hipEventRecord(be->ev_join_, be->st2_) == hipSuccess) (void)hipStreamWaitEvent(be->st_, be->ev_join_, 0);
      (void)hipStreamSynchronize(be->st2_);
    }
    SideJoin(const SideJoin&) = delete;
    SideJoin& operator=(const SideJoin&) = delete;
  };
  double* gemm_ws(size_t doubles) {
    if (doubles == 0) return (double*)ws_gemm_.p;
    grow(ws_gemm_, doubles * sizeof(double));
    return (double*)ws_gemm_.p;
  }

  int ncus_ = 0;
  std::string arch_;
  // the side stream of lowrank_tail's overlap (created at its first use, lower priority than st_) and the two events that
  // order it against st_: work is put on it only between a fork and a join inside one call, so whatever drains st_ after
  // that call has drained it too; the places that drain or tear down st_ drain it all the same (drain_side)
  hipStream_t st2_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
  int64_t n_tail_overlaps_ = 0;
  std::unique_ptr<HostStager> stager_;        // the pinned staging ring of the host boundary (created at the first large transfer)
  bool stager_failed_ = false;
  hipEvent_t ev_stage_ = nullptr;
  enum FlagSlot {                // the slots of flags_; the first FLAG_ERROR_WORDS are what take_error reads and clears
    FLAG_LU_INFO = 0,            // lu: 0, the column of an exactly zero pivot, or < 0 when the pivot exchange timed out
    FLAG_CHOL_INFO = 1,          // chol_upper: 0 or the column at which the matrix stopped being positive definite
    FLAG_WAIT_PHASE = 2, FLAG_WAIT_SLOT = 3, FLAG_WAIT_EPOCH = 4, FLAG_WAIT_WHO = 5,   // what a timed-out LU workgroup waited for
    FLAG_ERROR_WORDS = 8, FLAG_SVD_ROTATIONS = 8,     // (behind the error words:) the Jacobi SVD's rotation counter
    FLAG_CHOLQR = 9,             // the verdict of a CholeskyQR attempt: non-zero = this tier does not apply (read_flag)
    FLAG_CHOL_LOWER = 10,        // chol_lower / saddle_solve: 0 or the 1-based column of the first bad pivot (read_flag)
    FLAG_COUNT = 16
  };
  int32_t* flags_ = nullptr;
  double* scal_ = nullptr;
  void* pin_power_ = nullptr; // pinned: the verdict of a power step (lowrank_power_step)
  DevBuf ws_gemm_, ws_lu_, ws_split_, ws_qr_, ws_svd_, ws_blas2_, ws_lus_, ws_svdf_, ws_qr_hh_;
  DevBuf* const ws_all_[9] = {&ws_gemm_, &ws_lu_, &ws_split_, &ws_qr_, &ws_svd_, &ws_blas2_, &ws_lus_, &ws_svdf_, &ws_qr_hh_};
  std::mutex mu_;
  std::vector<DevBuf> sizes_;
  std::vector<DevBuf> pool_;
  std::vector<void*> garbage_;                 // outgrown workspaces, freed when this context's call has finished (free_ws)
  size_t garbage_bytes_ = 0;
  int64_t in_use_ = 0, pooled_ = 0;
  bool prof_ = false;
  Rec cur_{};
  std::vector<Rec> records_;
  std::vector<hipEvent_t> ev_pool_;
  double acc_ms_[PH_COUNT] = {0};
  int64_t acc_n_[PH_COUNT] = {0};
  int last_svd_sweeps_ = 0;
  int64_t n_svd_cap_hits_ = 0;
  int64_t n_cholqr_ = 0, n_householder_ = 0, n_scholqr3_ = 0;
  std::map<std::pair<int64_t, bool>, int> skip_tier1_by_height_;
  std::map<int, int> lu2_resident_;   // (bs, rpt) -> resident workgroups per CU of that leaf instantiation
  bool lu2_lost_ = false, lu2_retry_ = false;
  int lu2_ov_resident_ = -1;
  int mr_force_ = 0;
  // multi-rank persistent leaves: this rank's record buffer, the peers' (as this rank addresses them), the running epoch
  unsigned long long* mr_recs_ = nullptr;
  unsigned long long* mr_peer_[hipk::LU2_MAX_RANKS] = {nullptr};
  Comm* mr_comm_ = nullptr;
  uint32_t mr_epoch_ = 0;
  bool mr_disabled_ = false, mr_peer_swaps_ = true;
  bool mr_share_tried_ = false, mr_in_flight_ = false;
  int ranks_sharing_device_ = 1;
  int64_t mr_gen_ = 0, n_lu_timeouts_ = 0;
  std::string mr_reason_, mr_why_disabled_;
  std::set<int64_t> mr_warm_;
  hipk::Lu2MrWork mr_work_{};
  int64_t lus_part_col_ = -1, lus_part_mloc_ = 0;     // sharded LU: column whose arg-max partials the last apply kernel left
  const double* lus_part_Y_ = nullptr;
};

}  // namespace

Backend* make_backend(int device_id) { return new HipBackend(device_id); }
const char* backend_name() { return "hip-gfx950"; }

}  // namespace gsi
