// hip_backend.hpp -- what the communicators (hip_comm.hip) need of the gfx950 backend (hip_backend.hip): the error check and
// the device and stream of a context.  Memory comes through Backend::alloc / release.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/gsi_hip.h"
#include "backend.hpp"

namespace gsi {

#define HIP_CHECK(expr)                                                                            \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      throw Error(_e == hipErrorOutOfMemory ? GSI_ERR_OOM : GSI_ERR_HIP,                            \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                               \
  } while (0)

class __attribute__((visibility("hidden"))) HipDevice : public Backend {     // (the library exports nothing of it)
 public:
  hipStream_t stream() const { return st_; }
  void bind() { hipSetDevice(device_); }
  int device() const { return device_; }
 protected:
  explicit HipDevice(int device) : device_(device) {}
  int device_;
  hipStream_t st_ = nullptr;
};

}  // namespace gsi
