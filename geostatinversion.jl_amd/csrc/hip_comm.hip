// hip_comm.hip -- the gfx950 implementations of gsi::Comm: RCCL (one process per GPU) and the two RCCL-free communicators that
// make the multi-rank code runnable on one GPU.  Of the backend they use its device and stream (hip_backend.hpp), alloc, release.
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <time.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "hip_backend.hpp"
#include "hip_common.hpp"

namespace gsi {
namespace {

// ---- RCCL, bound lazily so a single-GPU user never needs librccl to resolve -----------------
struct RcclApi {
  void* h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
};
RcclApi& rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    api.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!api.h) api.h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!api.h) return;
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.h, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.h, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.h, "ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))dlsym(api.h, "ncclAllReduce");
    api.AllGather = (decltype(api.AllGather))dlsym(api.h, "ncclAllGather");
    api.ReduceScatter = (decltype(api.ReduceScatter))dlsym(api.h, "ncclReduceScatter");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.h, "ncclGetErrorString");
    api.Send = (decltype(api.Send))dlsym(api.h, "ncclSend");
    api.Recv = (decltype(api.Recv))dlsym(api.h, "ncclRecv");
    api.GroupStart = (decltype(api.GroupStart))dlsym(api.h, "ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.h, "ncclGroupEnd");
  });
  if (!api.h || !api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.AllGather || !api.ReduceScatter)
    throw Error(GSI_ERR_RCCL, "librccl.so could not be loaded: multi-GPU needs RCCL");
  return api;
}
#define RCCL_CHECK(expr)                                                                       \
  do {                                                                                         \
    ncclResult_t _r = (expr);                                                                  \
    if (_r != ncclSuccess)                                                                     \
      throw Error(GSI_ERR_RCCL, std::string(#expr) + ": " +                                     \
                                    (rccl().GetErrorString ? rccl().GetErrorString(_r) : "rccl error")); \
  } while (0)

// all[g] = rank g's buffer as this process addresses it: its own pointer, an IPC mapping of everybody else's
static bool ipc_open_all(int nranks, int rank, void* mine, const hipIpcMemHandle_t* hs, void** all, std::vector<void*>* opened) {
  bool ok = true;
  for (int g = 0; g < nranks && ok; ++g) {
    if (g == rank) { all[g] = mine; continue; }
    void* p = nullptr;
    if (hipIpcOpenMemHandle(&p, hs[g], hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); ok = false; p = nullptr; }
    all[g] = p;
    if (p && opened) opened->push_back(p);
  }
  return ok;
}

class RcclComm : public Comm {
 public:
  RcclComm(HipDevice* be, int n, int r, const void* id) : be_(be) {
    nranks = n;
    rank = r;
    static_assert(sizeof(ncclUniqueId) <= GSI_UNIQUE_ID_BYTES, "unique id does not fit the ABI slot");
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    be_->bind();
    RCCL_CHECK(rccl().CommInitRank(&comm_, n, uid, r));
  }
  ~RcclComm() override {
    if (comm_) {
      be_->bind();
      hipStreamSynchronize(be_->stream());
      rccl().CommDestroy(comm_);
    }
  }
  void do_allreduce_sum(double* buf, size_t count) override {
    be_->bind();
    RCCL_CHECK(rccl().AllReduce(buf, buf, count, ncclDouble, ncclSum, comm_, be_->stream()));
  }
  void do_allgather(const double* send, double* recv, size_t count) override {
    be_->bind();
    RCCL_CHECK(rccl().AllGather(send, recv, count, ncclDouble, comm_, be_->stream()));
  }
  void do_reduce_scatter_sum(const double* send, double* recv, size_t count) override {
    be_->bind();
    RCCL_CHECK(rccl().ReduceScatter(send, recv, count, ncclDouble, ncclSum, comm_, be_->stream()));
  }
  // point-to-point xGMI: every pair of GPUs has a direct link, so the grouped sends / receives use all 7 links at once
  void do_alltoall(const double* send, double* recv, size_t count) override {
    be_->bind();
    RcclApi& r = rccl();
    if (!r.Send || !r.Recv || !r.GroupStart || !r.GroupEnd) throw Error(GSI_ERR_RCCL, "librccl has no ncclSend / ncclRecv");
    RCCL_CHECK(r.GroupStart());
    for (int g = 0; g < nranks; ++g) {
      RCCL_CHECK(r.Send(send + (size_t)g * count, count, ncclDouble, g, comm_, be_->stream()));
      RCCL_CHECK(r.Recv(recv + (size_t)g * count, count, ncclDouble, g, comm_, be_->stream()));
    }
    RCCL_CHECK(r.GroupEnd());
  }
  // one process per GPU: IPC handles travel through an all-gather, every rank maps its peers' buffers.  The mapping of
  // OTHER processes' buffers cannot be exercised on the one-GPU build box (RCCL refuses two ranks on one device), which is
  // why pipeline.cpp:lus_mr_selftest makes the path prove itself on the machine it runs on before it is used.
  bool share_pointers(void* mine, size_t bytes, void** all) override {
    (void)bytes;
    static const bool on = !(getenv("GSI_LU_PEER") != nullptr && getenv("GSI_LU_PEER")[0] == '0');   // GSI_LU_PEER=0: never
    if (!on) return false;
    be_->bind();
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof(h));
    bool ok = (hipIpcGetMemHandle(&h, mine) == hipSuccess);     // a failure here must not skip the collective below
    if (!ok) (void)hipGetLastError();
    double* send = be_->alloc(8);
    double* recv = be_->alloc((size_t)8 * nranks);
    HIP_CHECK(hipMemcpyAsync(send, &h, 64, hipMemcpyHostToDevice, be_->stream()));
    allgather(send, recv, 8);
    std::vector<hipIpcMemHandle_t> hs((size_t)nranks);
    HIP_CHECK(hipMemcpyAsync(hs.data(), recv, (size_t)64 * nranks, hipMemcpyDeviceToHost, be_->stream()));
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    be_->release(send);
    be_->release(recv);
    if (ok) ok = ipc_open_all(nranks, rank, mine, hs.data(), all, nullptr);
    return ok;      // false on this rank alone is fine: the ranks all-reduce their answers before anyone relies on the buffers
  }

 private:
  HipDevice* be_;
  ncclComm_t comm_ = nullptr;
};

// ---- ranks as THREADS of one process (GSI_LOCAL_COMM=1): one context per thread, on different GPUs with peer access or --
//      what makes the whole multi-rank pipeline runnable on a one-GPU box -- on the SAME GPU.  RCCL refuses two ranks on one
//      device; this communicator needs nothing but HIP: every rank's device pointers are valid in every thread of the
//      process, so a collective is "synchronise my stream, meet at a host barrier, read the peers' buffers with kernels /
//      copies on my own stream, synchronise, meet again".  Rank-ordered sums (deterministic).  Not a performance path.
struct LocalGroup {
  int nranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t generation = 0;
  std::vector<const double*> src;
  std::vector<int> device;               // device of every rank's context
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t gen = generation;
    if (++arrived == nranks) { arrived = 0; ++generation; cv.notify_all(); return; }
    // a rank thread that died (an exception on its way out, a caller that returned) must not hang the others for ever
    static const int timeout_s = getenv("GSI_SHM_TIMEOUT_S") ? std::max(1, atoi(getenv("GSI_SHM_TIMEOUT_S"))) : 300;
    if (!cv.wait_for(lk, std::chrono::seconds(timeout_s), [&] { return generation != gen; })) {
      --arrived;
      throw Error(GSI_ERR_RCCL, "local communicator: a rank did not reach the barrier (GSI_SHM_TIMEOUT_S)");
    }
  }
};
static std::mutex g_local_mu;
static std::map<std::string, std::shared_ptr<LocalGroup>> g_local_groups;

class LocalComm : public Comm {
 public:
  LocalComm(HipDevice* be, int n, int r, const void* id) : be_(be) {
    nranks = n;
    rank = r;
    const std::string key((const char*)id, 32);
    std::unique_lock<std::mutex> lk(g_local_mu);
    auto& grp = g_local_groups[key];
    if (!grp) { grp = std::make_shared<LocalGroup>(); grp->nranks = n; grp->src.assign((size_t)n, nullptr); grp->device.assign((size_t)n, -1); }
    if (grp->nranks != n) throw Error(GSI_ERR_ARG, "local communicator: ranks disagree on nranks");
    grp->device[(size_t)r] = be_->device();
    grp_ = grp;
    lk.unlock();
    grp_->barrier();                      // like ncclCommInitRank: returns when every rank has joined (and registered its device)
    for (int d = 0, cnt = 0; hipGetDeviceCount(&cnt) == hipSuccess && d < cnt; ++d)      // best effort: peers on other GPUs
      if (d != be_->device()) { (void)hipDeviceEnablePeerAccess(d, 0); (void)hipGetLastError(); }
  }
  // publish my buffer, wait until every rank has published and its producing work is complete
  void publish(const double* p) {
    be_->bind();
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    { std::lock_guard<std::mutex> g(grp_->mu); grp_->src[(size_t)rank] = p; }
    grp_->barrier();
  }
  void finish() {                       // my reads of the peers' buffers are done; nobody may reuse a buffer before all are
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    grp_->barrier();
  }
  void do_allreduce_sum(double* buf, size_t count) override {
    publish(buf);
    double* tmp = be_->alloc(count);
    hipStream_t st = be_->stream();
    HIP_CHECK(hipMemcpyAsync(tmp, grp_->src[0], count * sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int g = 1; g < nranks; ++g) hipk::axpy(st, (int64_t)count, 1.0, grp_->src[(size_t)g], tmp);
    finish();                           // every rank has summed the ORIGINAL buffers
    HIP_CHECK(hipMemcpyAsync(buf, tmp, count * sizeof(double), hipMemcpyDeviceToDevice, st));
    be_->release(tmp);
  }
  void do_allgather(const double* send, double* recv, size_t count) override {
    publish(send);
    for (int g = 0; g < nranks; ++g)
      HIP_CHECK(hipMemcpyAsync(recv + (size_t)g * count, grp_->src[(size_t)g], count * sizeof(double), hipMemcpyDeviceToDevice,
                               be_->stream()));
    finish();
  }
  void do_reduce_scatter_sum(const double* send, double* recv, size_t count) override {
    publish(send);
    hipStream_t st = be_->stream();
    HIP_CHECK(hipMemcpyAsync(recv, grp_->src[0] + (size_t)rank * count, count * sizeof(double), hipMemcpyDeviceToDevice, st));
    for (int g = 1; g < nranks; ++g) hipk::axpy(st, (int64_t)count, 1.0, grp_->src[(size_t)g] + (size_t)rank * count, recv);
    finish();
  }
  void do_alltoall(const double* send, double* recv, size_t count) override {
    publish(send);
    for (int g = 0; g < nranks; ++g)
      HIP_CHECK(hipMemcpyAsync(recv + (size_t)g * count, grp_->src[(size_t)g] + (size_t)rank * count, count * sizeof(double),
                               hipMemcpyDeviceToDevice, be_->stream()));
    finish();
  }
  bool share_pointers(void* mine, size_t, void** all) override {       // one process: the pointers themselves
    publish((const double*)mine);
    for (int g = 0; g < nranks; ++g) all[g] = const_cast<double*>(grp_->src[(size_t)g]);
    finish();
    return true;
  }
  void host_barrier() override { grp_->barrier(); }
  int ranks_on_my_device() override {
    std::lock_guard<std::mutex> g(grp_->mu);
    int c = 0;
    for (int q = 0; q < nranks; ++q) c += (grp_->device[(size_t)q] == be_->device()) ? 1 : 0;
    return std::max(c, 1);
  }

 private:
  HipDevice* be_;
  std::shared_ptr<LocalGroup> grp_;
};
static bool local_comm_requested() { return getenv("GSI_LOCAL_COMM") != nullptr; }

// ---- ranks as PROCESSES of one node without RCCL (GSI_SHM_COMM=1): host barriers and IPC handles in a POSIX shared-memory
//      block, payloads through one staging buffer per rank that every peer maps with hipIpcOpenMemHandle.  Two uses: the
//      cross-PROCESS half of the multi-rank code (IPC mapping of the pivot-exchange buffer, persistent kernels of different
//      processes polling each other's memory) runs on a one-GPU box, where RCCL refuses two ranks on one device; and a node
//      without librccl still has a communicator.  Rank-ordered sums (deterministic, identical on every rank).  A collective
//      is: copy into my staging buffer, synchronise, barrier, read the peers' staging buffers, synchronise, barrier -- not
//      a performance path.
struct ShmBlock {
  std::atomic<uint32_t> arrived;
  std::atomic<uint32_t> generation;
  uint32_t ok[16];
  char busid[16][32];                    // PCI bus id of every rank's device
  hipIpcMemHandle_t stage[16];
  hipIpcMemHandle_t shared[16];
};
static_assert(std::atomic<uint32_t>::is_always_lock_free, "process-shared atomics");

class ShmComm : public Comm {
 public:
  ShmComm(HipDevice* be, int n, int r, const void* id) : be_(be) {
    nranks = n;
    rank = r;
    if (n < 1 || n > 16) throw Error(GSI_ERR_ARG, "shared-memory communicator: 1..16 ranks");
    char name[96];
    std::memcpy(name, (const char*)id + 16, 95);
    name[95] = 0;
    if (std::memcmp(id, "gsi-shm-comm", 12) != 0 || name[0] != '/')
      throw Error(GSI_ERR_ARG, "shared-memory communicator: the id does not come from gsi_comm_unique_id() under GSI_SHM_COMM");
    if (const char* e = getenv("GSI_SHM_TIMEOUT_S")) timeout_s_ = std::max(1, atoi(e));
    const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);      // whoever comes first creates it: zero-filled = initial state
    if (fd < 0) throw Error(GSI_ERR_RCCL, std::string("shm_open(") + name + ") failed");
    if (ftruncate(fd, sizeof(ShmBlock)) != 0) { close(fd); throw Error(GSI_ERR_RCCL, "shared-memory communicator: ftruncate failed"); }
    void* m = mmap(nullptr, sizeof(ShmBlock), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) throw Error(GSI_ERR_RCCL, "shared-memory communicator: mmap failed");
    blk_ = (ShmBlock*)m;
    be_->bind();
    size_t mb = 64;
    if (const char* e = getenv("GSI_SHM_STAGE_MB")) mb = (size_t)std::max(1, atoi(e));
    cap_ = mb * 1024 * 1024 / sizeof(double);
    bool ok = (hipMalloc((void**)&stage_, cap_ * sizeof(double)) == hipSuccess);
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof(h));
    if (ok) ok = (hipIpcGetMemHandle(&h, stage_) == hipSuccess);
    if (!ok) (void)hipGetLastError();
    blk_->stage[rank] = h;
    blk_->ok[rank] = ok ? 1u : 0u;
    std::memset(blk_->busid[rank], 0, sizeof(blk_->busid[rank]));
    if (hipDeviceGetPCIBusId(blk_->busid[rank], (int)sizeof(blk_->busid[rank]) - 1, be_->device()) != hipSuccess) {
      (void)hipGetLastError();
      snprintf(blk_->busid[rank], sizeof(blk_->busid[rank]), "device-%d", be_->device());
    }
    barrier();
    if (rank == 0) shm_unlink(name);                            // every rank has it mapped: nothing is left behind in /dev/shm
    for (int g = 0; g < nranks; ++g) ok = ok && blk_->ok[g] != 0;
    std::vector<hipIpcMemHandle_t> hs(blk_->stage, blk_->stage + nranks);
    void* all[16] = {nullptr};
    if (ok) ok = ipc_open_all(nranks, rank, stage_, hs.data(), all, &opened_);
    blk_->ok[rank] = ok ? 1u : 0u;
    barrier();
    for (int g = 0; g < nranks; ++g) ok = ok && blk_->ok[g] != 0;
    barrier();                                                  // ok[] is reused by share_pointers
    if (!ok) { cleanup(); throw Error(GSI_ERR_RCCL, "shared-memory communicator: the ranks' staging buffers could not be mapped (hipIpc)"); }
    for (int g = 0; g < nranks; ++g) peer_[g] = (const double*)all[g];
    for (int g = 0; g < nranks; ++g) same_device_ += (std::strncmp(blk_->busid[g], blk_->busid[rank], sizeof(blk_->busid[g])) == 0) ? 1 : 0;
  }
  int ranks_on_my_device() override { return std::max(same_device_, 1); }
  ~ShmComm() override {
    be_->bind();
    (void)hipStreamSynchronize(be_->stream());
    cleanup();
  }
  void do_allreduce_sum(double* buf, size_t count) override {
    hipStream_t st = be_->stream();
    for (size_t off = 0; off < count || off == 0; off += cap_) {
      const size_t c = std::min(cap_, count - off);
      stage_in(buf + off, c);
      if (c) HIP_CHECK(hipMemcpyAsync(buf + off, peer_[0], c * sizeof(double), hipMemcpyDeviceToDevice, st));
      for (int g = 1; g < nranks && c; ++g) hipk::axpy(st, (int64_t)c, 1.0, peer_[g], buf + off);
      done_reading();
      if (count == 0) break;
    }
  }
  void do_allgather(const double* send, double* recv, size_t count) override {
    for (size_t off = 0; off < count || off == 0; off += cap_) {
      const size_t c = std::min(cap_, count - off);
      stage_in(send + off, c);
      for (int g = 0; g < nranks && c; ++g)
        HIP_CHECK(hipMemcpyAsync(recv + (size_t)g * count + off, peer_[g], c * sizeof(double), hipMemcpyDeviceToDevice, be_->stream()));
      done_reading();
      if (count == 0) break;
    }
  }
  // blocks of `count` doubles per destination: the staging buffer holds nranks segments of one chunk
  void do_reduce_scatter_sum(const double* send, double* recv, size_t count) override {
    hipStream_t st = be_->stream();
    const size_t cc = std::max<size_t>(cap_ / (size_t)nranks, 1);
    for (size_t off = 0; off < count || off == 0; off += cc) {
      const size_t c = std::min(cc, count - off);
      stage_blocks(send, count, off, c, cc);
      if (c) HIP_CHECK(hipMemcpyAsync(recv + off, peer_[0] + (size_t)rank * cc, c * sizeof(double), hipMemcpyDeviceToDevice, st));
      for (int g = 1; g < nranks && c; ++g) hipk::axpy(st, (int64_t)c, 1.0, peer_[g] + (size_t)rank * cc, recv + off);
      done_reading();
      if (count == 0) break;
    }
  }
  void do_alltoall(const double* send, double* recv, size_t count) override {
    const size_t cc = std::max<size_t>(cap_ / (size_t)nranks, 1);
    for (size_t off = 0; off < count || off == 0; off += cc) {
      const size_t c = std::min(cc, count - off);
      stage_blocks(send, count, off, c, cc);
      for (int g = 0; g < nranks && c; ++g)
        HIP_CHECK(hipMemcpyAsync(recv + (size_t)g * count + off, peer_[g] + (size_t)rank * cc, c * sizeof(double), hipMemcpyDeviceToDevice,
                                 be_->stream()));
      done_reading();
      if (count == 0) break;
    }
  }
  // the buffers are mapped exactly as RcclComm maps them (the handles travel through the shared block instead of an all-gather)
  bool share_pointers(void* mine, size_t, void** all) override {
    static const bool on = !(getenv("GSI_LU_PEER") != nullptr && getenv("GSI_LU_PEER")[0] == '0');
    if (!on) return false;
    be_->bind();
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof(h));
    bool ok = (hipIpcGetMemHandle(&h, mine) == hipSuccess);
    if (!ok) (void)hipGetLastError();
    blk_->shared[rank] = h;
    blk_->ok[rank] = ok ? 1u : 0u;
    barrier();
    for (int g = 0; g < nranks; ++g) ok = ok && blk_->ok[g] != 0;
    std::vector<hipIpcMemHandle_t> hs(blk_->shared, blk_->shared + nranks);
    barrier();                                                  // everybody has read the slots
    if (ok) ok = ipc_open_all(nranks, rank, mine, hs.data(), all, &opened_);
    return ok;      // as with RCCL: the caller all-reduces the ranks' answers before anyone relies on the buffers
  }

 private:
  void barrier() {
    const uint32_t gen = blk_->generation.load(std::memory_order_acquire);
    if (blk_->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)nranks) {
      blk_->arrived.store(0, std::memory_order_relaxed);
      blk_->generation.fetch_add(1, std::memory_order_release);
      return;
    }
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t it = 0; blk_->generation.load(std::memory_order_acquire) == gen; ++it) {
      if (it < 4096) continue;
      sched_yield();
      if ((it & 1023) == 0) {
        timespec t1;
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (t1.tv_sec - t0.tv_sec > timeout_s_)
          throw Error(GSI_ERR_RCCL, "shared-memory communicator: a rank did not reach the barrier (GSI_SHM_TIMEOUT_S)");
      }
    }
  }
  void stage_in(const double* src, size_t c) {                 // my chunk -> my staging buffer, visible to every rank
    be_->bind();
    if (c) HIP_CHECK(hipMemcpyAsync(stage_, src, c * sizeof(double), hipMemcpyDeviceToDevice, be_->stream()));
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    barrier();
  }
  void stage_blocks(const double* send, size_t count, size_t off, size_t c, size_t cc) {
    be_->bind();
    for (int g = 0; g < nranks && c; ++g)
      HIP_CHECK(hipMemcpyAsync(stage_ + (size_t)g * cc, send + (size_t)g * count + off, c * sizeof(double), hipMemcpyDeviceToDevice,
                               be_->stream()));
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    barrier();
  }
  void done_reading() {                                        // nobody overwrites a staging buffer a peer still reads
    HIP_CHECK(hipStreamSynchronize(be_->stream()));
    barrier();
  }
  void cleanup() {
    for (void* p : opened_) (void)hipIpcCloseMemHandle(p);
    opened_.clear();
    (void)hipGetLastError();
    if (blk_) {
      try { if (!std::uncaught_exceptions()) { const int t = timeout_s_; timeout_s_ = std::min(t, 10); barrier(); timeout_s_ = t; } } catch (...) {}
      munmap(blk_, sizeof(ShmBlock));
      blk_ = nullptr;
    }
    if (stage_) { (void)hipFree(stage_); stage_ = nullptr; }
  }

  HipDevice* be_;
  ShmBlock* blk_ = nullptr;
  double* stage_ = nullptr;
  size_t cap_ = 0;
  const double* peer_[16] = {nullptr};
  std::vector<void*> opened_;
  int same_device_ = 0;
  int timeout_s_ = 300;
};
static bool shm_comm_requested() { return getenv("GSI_SHM_COMM") != nullptr; }

}  // namespace

Comm* make_comm(Backend* be, int nranks, int rank, const void* unique_id) {
  if (local_comm_requested()) return new LocalComm(static_cast<HipDevice*>(be), nranks, rank, unique_id);
  if (shm_comm_requested()) return new ShmComm(static_cast<HipDevice*>(be), nranks, rank, unique_id);
  return new RcclComm(static_cast<HipDevice*>(be), nranks, rank, unique_id);
}
void comm_unique_id(void* id_out) {
  std::memset(id_out, 0, GSI_UNIQUE_ID_BYTES);
  if (local_comm_requested()) {         // ranks are threads of this process: any id that is unique within it
    static std::atomic<uint64_t> counter{1};
    const uint64_t c = counter.fetch_add(1);
    std::memcpy(id_out, "gsi-local-comm", 14);
    std::memcpy((char*)id_out + 16, &c, sizeof(c));
    return;
  }
  if (shm_comm_requested()) {           // ranks are processes of this node: the name of a shared-memory block nobody has used
    static std::atomic<uint64_t> counter{1};
    timespec t;
    clock_gettime(CLOCK_REALTIME, &t);
    std::memcpy(id_out, "gsi-shm-comm", 12);
    snprintf((char*)id_out + 16, 96, "/gsi-shm-%ld-%llu-%lld%09ld", (long)getpid(), (unsigned long long)counter.fetch_add(1),
             (long long)t.tv_sec, (long)t.tv_nsec);
    return;
  }
  ncclUniqueId uid;
  RCCL_CHECK(rccl().GetUniqueId(&uid));
  std::memcpy(id_out, &uid, sizeof(uid));
}

}  // namespace gsi
