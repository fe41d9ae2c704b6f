// csrc/host_launch.h — what the host sides of the translation units share: the failure of an entry point and the two checks in front of it, the
// alignment predicates of the argument checks, the check behind a launch, and the launch of a kernel with more than 64 KiB of dynamic LDS.
// Failures go to the calling thread's message (tmjx_hip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/tmjx.h"

extern "C" int tmjx_internal_fail(int code, const char *msg);       // tmjx_hip.hip: records the calling thread's error message
static inline int fail(int code, const std::string &msg) { return tmjx_internal_fail(code, msg.c_str()); }
// an argument check returns its message, empty where the arguments are good
#define TM_TRY(expr) do { const std::string e_ = (expr); if (!e_.empty()) return fail(TMJX_EINVAL, e_); } while (0)
#define TM_HIP(what, expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(TMJX_EHIP, std::string(what) + ": " + hipGetErrorString(e_)); } while (0)
static inline bool al4(const void *p) { return !((uintptr_t)p & 3); }
static inline bool al16(const void *p) { return !((uintptr_t)p & 15); }
static inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TMJX_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  return TMJX_OK;
}
// More than 64 KiB of dynamic LDS needs the attribute, set to `lds_max`: the largest size the entry point accepts.  The attribute belongs to the
// device, so it is set once per kernel (the mask is one per instantiation) and device, not once per process; devices past 63 set it before
// every launch.  Then the launch with the `lds` bytes this call needs, and its check.
template <auto Kernel, class... Args>
static int launch_lds(const char *what, dim3 grid, dim3 block, size_t lds_max, size_t lds, hipStream_t s, Args... args) {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  TM_HIP("hipGetDevice", hipGetDevice(&dev));
  const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t)1 << dev : 0;
  if (!bit || !(done.load(std::memory_order_acquire) & bit)) {
    TM_HIP(std::string("hipFuncSetAttribute(") + what + ")", hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    done.fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return check_launch(what);
}
// a kernel whose every launch takes the same size
template <auto Kernel, class... Args>
static int launch_lds(const char *what, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  return launch_lds<Kernel>(what, grid, block, lds, lds, s, args...);
}
