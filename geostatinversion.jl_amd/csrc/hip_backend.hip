// hip_backend.hip -- the gfx950 implementation of gsi::Backend: one HIP stream per context, every operation enqueued on it (no host
// round trips except where the algorithm needs a scalar), workspaces grown on demand.  This file: construction, memory, the host
// boundary, streams, errors and profiling; the other subsystems are listed in hip_backend_impl.hpp.  The communicators are in
// hip_comm.hip.
#include <dlfcn.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "hip_backend_impl.hpp"

namespace gsi {

namespace {

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

}  // namespace

HipBackend::HipBackend(int device) : HipDevice(device) {
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
HipBackend::~HipBackend() {
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

// ---- memory ----
// Panel-sized temporaries come and go inside every entry point; everything is ordered on the one
// stream, so a released block can be handed to the next request without synchronising or going back
// to hipFree/hipMalloc.  Exact-size free lists (the sizes repeat from call to call), trimmed when the
// cache exceeds half of what is in use.
double* HipBackend::alloc(size_t count) {
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
void HipBackend::release(double* p) {
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
void HipBackend::trim_pool(int64_t keep_bytes) {
  hipStreamSynchronize(st_);
  drain_side();
  std::lock_guard<std::mutex> g(mu_);
  while (!pool_.empty() && pooled_ > keep_bytes) {
    hipFree(pool_.back().p);
    pooled_ -= (int64_t)pool_.back().bytes;
    pool_.pop_back();
  }
}
void HipBackend::release_cache() {
  bind();
  for (DevBuf* b : ws_all_)
    if (b->bytes > ((size_t)64 << 20)) free_ws(*b);
  (void)hipStreamSynchronize(st_);
  drain_side();
  collect_garbage();
  trim_pool(0);
}
int64_t HipBackend::bytes_in_use() const {
  int64_t ws = 0;
  for (const DevBuf* b : ws_all_)                     // (ws_lus_ has never been part of this figure: it stays out of it)
    if (b != &ws_lus_ && !b->pooled) ws += (int64_t)b->bytes;          // pooled workspaces are counted by alloc()
  return in_use_ + pooled_ + ws + (int64_t)garbage_bytes_;
}
// Cached workspaces make repeated factorizations allocation-free; one of panel size at 512^3 (tens of GB) would
// instead starve the next phase, so anything above 8 GiB is given back when the call that grew it returns.
// A workspace that is outgrown is not freed on the spot: hipFree waits for the whole DEVICE, and with the ranks of a
// communicator as threads of one process (GSI_LOCAL_COMM) another rank's persistent LU kernel may at that moment be
// spinning for a record of the very kernel this thread is about to launch -- a dead-lock that ends in the kernel's poll
// time-out (seen once in five runs of test_multirank_pipeline_on_one_gpu[3]: rank B grew ws_lu_ inside the sharded LU
// while rank A's first leaf was already waiting for it).  The block waits in garbage_ until this context's call has
// finished its own device work (take_error: whatever still spins for us has all it needs by then).
void HipBackend::free_ws(DevBuf& b) {
  if (!b.p) return;
  if (b.pooled) release((double*)b.p);       // back to the block cache (stream-ordered: no synchronisation)
  else { std::lock_guard<std::mutex> g(mu_); garbage_.push_back(b.p); garbage_bytes_ += b.bytes; }
  b.p = nullptr; b.bytes = 0; b.pooled = false;
}
void HipBackend::collect_garbage() {
  std::vector<void*> g;
  { std::lock_guard<std::mutex> lk(mu_); g.swap(garbage_); garbage_bytes_ = 0; }
  for (void* p : g) (void)hipFree(p);
}
void HipBackend::trim(DevBuf& b) {
  if (b.bytes <= ((size_t)8 << 30) || !b.p) return;
  free_ws(b);
}
void HipBackend::grow(DevBuf& b, size_t bytes) {
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
// The contractions' split-K workspace, grown to `doubles` (0: as it is), with what it holds now: the launchers behind
// HipBackend::gemm and its kin (hip_backend_products.hip) check their own need against that.
HipBackend::GemmWs HipBackend::gemm_ws(size_t doubles) {
  if (doubles != 0) grow(ws_gemm_, doubles * sizeof(double));
  return {(double*)ws_gemm_.p, ws_gemm_.bytes / sizeof(double)};
}

// ---- the host boundary (host_staging.hpp): caller memory is pageable; transfers of GSI_STAGE_MIN_MB (default 16) MiB and
// more go through the pinned staging ring (GSI_STAGE_THREADS workers, default 6 -- four reach the link rate on contiguous
// sources, the strided row-block reads want the margin --, GSI_STAGE_CHUNK_MB MiB chunks, default 16: 0.98 of this box's
// pinned-copy rate in both directions, profiles/r05_h2d_rates.log); smaller ones straight from the
// caller's pages (54 us for C1's 768 KB Omega).  If the ring cannot be allocated the direct path serves everything.
HostStager* HipBackend::stager() {
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
size_t HipBackend::stage_min_bytes() {
  const char* e = getenv("GSI_STAGE_MIN_MB");            // read per call (a getenv against a transfer of MiBs; tests switch it)
  return (size_t)(e ? std::max(0ll, atoll(e)) : 16) << 20;
}
bool HipBackend::staged(bool h2d, double* dev, int64_t ldd, double* host, int64_t ldh, int64_t rows, int64_t cols) {
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
void HipBackend::upload2d(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return;
  bind();
  if (staged(true, dst, ldd, const_cast<double*>(host), ldh, rows, cols)) return;
  HIP_CHECK(hipMemcpy2DAsync(dst, ldd * sizeof(double), host, ldh * sizeof(double), rows * sizeof(double),
                             cols, hipMemcpyHostToDevice, st_));
  HIP_CHECK(hipStreamSynchronize(st_));  // the caller may reuse / free the host buffer on return
}
void HipBackend::download2d(double* host, int64_t ldh, const double* src, int64_t lds, int64_t rows, int64_t cols) {
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
int64_t HipBackend::upload_block_rows(int64_t rows, int64_t cols) {
  const int64_t forced = getenv("GSI_STAGE_BLOCK_ROWS") ? atoll(getenv("GSI_STAGE_BLOCK_ROWS")) : 0;
  if (forced >= 128) return std::min(rows, (forced / 128) * 128);
  if (sizeof(double) * (size_t)rows * (size_t)cols < ((size_t)256 << 20) || rows < 2 * 4096) return rows;
  const int64_t half = (((rows + 1) / 2 + 127) / 128) * 128;
  return std::max<int64_t>(4096, std::min<int64_t>(32768, half));
}
void* HipBackend::upload2d_begin(double* dst, int64_t ldd, const double* host, int64_t ldh, int64_t rows, int64_t cols,
                                 int64_t block_rows) {
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
void HipBackend::upload2d_wait_block(void* handle, int64_t b) {
  if (!handle) return;
  bind();
  try {
    static_cast<HostStager*>(handle)->wait_block((int)b, st_);
  } catch (const std::exception& e) {
    throw Error(GSI_ERR_HIP, e.what());
  }
}
void HipBackend::pinned_copy_rate(int64_t bytes, double* h2d_gbs, double* d2h_gbs) {
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
void HipBackend::upload2d_end(void* handle) {
  if (!handle) return;
  try {
    static_cast<HostStager*>(handle)->end();
  } catch (const std::exception& e) {
    throw Error(GSI_ERR_HIP, e.what());
  }
}
void HipBackend::copy2d(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return;
  bind();
  HIP_CHECK(hipMemcpy2DAsync(dst, ldd * sizeof(double), src, lds * sizeof(double), rows * sizeof(double),
                             cols, hipMemcpyDeviceToDevice, st_));
}
void HipBackend::fill_zero(double* p, size_t count) {
  bind();
  HIP_CHECK(hipMemsetAsync(p, 0, count * sizeof(double), st_));
}
void HipBackend::fill_bytes(double* p, int byte, size_t count) {
  bind();
  HIP_CHECK(hipMemsetAsync(p, byte, count * sizeof(double), st_));
}
void HipBackend::sync() {
  bind();
  HIP_CHECK(hipStreamSynchronize(st_));
  if (st2_) HIP_CHECK(hipStreamSynchronize(st2_));
}

// ---- the side stream ----
hipStream_t HipBackend::side_stream() {
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

// ---- what kernels report: flags and errors ----
int32_t HipBackend::read_flag(int slot) {
  int32_t f = 0;
  HIP_CHECK(hipMemcpyAsync(&f, flags_ + slot, sizeof(int32_t), hipMemcpyDeviceToHost, st_));
  HIP_CHECK(hipStreamSynchronize(st_));
  return f;
}
void HipBackend::check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error(GSI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
void HipBackend::forgive_lost_coresidency() {
  bind();
  (void)hipMemsetAsync(flags_, 0, FLAG_ERROR_WORDS * sizeof(int32_t), st_);
  lu2_lost_ = false;
  lu2_retry_ = false;          // (mr_disabled_ stays as the self-test left it)
}
bool HipBackend::retryable_failure() {
  const bool r = lu2_retry_;
  lu2_retry_ = false;
  return r;
}

int HipBackend::take_error(std::string* msg) {
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
void HipBackend::phase_begin(Phase p) {
  if (!prof_) return;
  bind();
  if (roctx().push) roctx().push(kPhaseNames[p]);
  cur_.phase = p;
  cur_.a = get_event();
  cur_.b = get_event();
  hipEventRecord(cur_.a, st_);
}
void HipBackend::phase_end_counted(bool counted) {
  if (!prof_) return;
  if (roctx().pop) roctx().pop();
  hipEventRecord(cur_.b, st_);
  cur_.counted = counted;
  records_.push_back(cur_);
}
void HipBackend::phase_reset() {
  bind();
  hipStreamSynchronize(st_);
  for (auto& r : records_) { ev_pool_.push_back(r.a); ev_pool_.push_back(r.b); }
  records_.clear();
  for (int i = 0; i < PH_COUNT; ++i) { acc_ms_[i] = 0.0; acc_n_[i] = 0; }
}
void HipBackend::phase_times(double* ms, int64_t* counts) {
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
hipEvent_t HipBackend::get_event() {
  if (!ev_pool_.empty()) { hipEvent_t e = ev_pool_.back(); ev_pool_.pop_back(); return e; }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

void HipBackend::counters(int64_t* out4) {
  out4[0] = n_cholqr_; out4[1] = n_householder_; out4[2] = last_svd_sweeps_; out4[3] = n_scholqr3_;
}

Backend* make_backend(int device_id) { return new HipBackend(device_id); }
const char* backend_name() { return "hip-gfx950"; }

}  // namespace gsi
