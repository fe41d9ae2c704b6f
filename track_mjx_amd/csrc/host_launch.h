// csrc/host_launch.h — what the host sides of the translation units share: the alignment predicates of the argument checks, the check behind a
// launch, and the launch of a kernel with more than 64 KiB of dynamic LDS.  Failures go to the calling thread's message (tmjx_hip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"

extern "C" int tmjx_internal_fail(int code, const char *msg);       // tmjx_hip.hip: records the calling thread's error message
static inline bool al4(const void *p) { return !((uintptr_t)p & 3); }
static inline bool al16(const void *p) { return !((uintptr_t)p & 15); }
static inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return tmjx_internal_fail(TMJX_EHIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return TMJX_OK;
}
// > 64 KiB of dynamic LDS needs the attribute once per kernel (the flag is one per instantiation, i.e. per kernel), then the launch and its check
template <auto Kernel, class... Args>
static int launch_lds(const char *what, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return tmjx_internal_fail(TMJX_EHIP, (std::string("hipFuncSetAttribute(") + what + "): " + hipGetErrorString(e)).c_str());
    attr_set = true;
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return check_launch(what);
}
