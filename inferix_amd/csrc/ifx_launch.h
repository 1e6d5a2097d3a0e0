// Launch mechanics every kernel with more than the default dynamic LDS shares.  Host only.  The rule: what is looked up or requested
// once is looked up or requested once PER DEVICE (one process drives several) and, for the opt-in, per kernel instantiation; the
// result of the request is checked; and any number of host threads may launch at once.  The caches are atomics indexed by the
// device index: two threads may both do the work the first time (it is idempotent), none goes on before its own has succeeded.
// A launcher that needs the device twice (CU count, then the launch) asks for it once and hands the index on.
#pragma once
#include <atomic>
#include <utility>

#include "ifx_common.h"

namespace ifx {

constexpr int kLaunchDevices = 64;      // device indices the two caches cover; a device past them is asked every time

// Index of the calling thread's current device, -1 when it cannot be read.  A process that sees ONE device is not asked: the launch
// path of the single-device pipelines then makes no runtime call that the launch itself does not make.
inline int current_device() {
  static const int visible = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  int dev = 0;
  return visible == 1 || hipGetDevice(&dev) == hipSuccess ? dev : -1;
}

// CUs of device `dev`: a persistent grid must not exceed them (a split-K consumer spins on a producer that has to be resident).
// 256 when the device or the attribute cannot be read; such an answer is not kept.
inline int device_cu_count(int dev = current_device()) {
  static std::atomic<int> cus[kLaunchDevices];
  int v = 0;
  if (dev < 0) return 256;
  if (dev < kLaunchDevices && (v = cus[dev].load(std::memory_order_relaxed)) > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
  if (dev < kLaunchDevices) cus[dev].store(v, std::memory_order_relaxed);
  return v;
}

// Lets `Kernel` be launched with up to `bytes` of dynamic LDS on the current device `dev`; `what` names the entry point in the error text.
template <auto Kernel>
int allow_dynamic_lds(int bytes, const char* what, int dev = current_device()) {
  static std::atomic<uint64_t> allowed{0};      // bit d: device d has granted it
  const uint64_t bit = dev >= 0 && dev < kLaunchDevices ? uint64_t(1) << dev : 0;
  if (allowed.load(std::memory_order_acquire) & bit) return IFX_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();      // reported here, not by the next launch's check_launch
    set_error("%s: %d bytes of dynamic LDS refused: %s", what, bytes, hipGetErrorString(e));
    return IFX_ELAUNCH;
  }
  allowed.fetch_or(bit, std::memory_order_release);
  return IFX_OK;
}

// The opt-in on the current device `dev`, then the launch (whose own result the caller reads with check_launch, as after any launch).
// no_sanitize: a launch through a template argument goes through the kernel's handle, a variable, and UBSan's function-type check
// (tools/*_check.cpp are built with it) would read the bytes in front of that variable as a function's signature.
template <auto Kernel, class... Args>
__attribute__((no_sanitize("function"))) int launch_lds_on(int dev, dim3 grid, dim3 block, int lds, hipStream_t s, const char* what, Args&&... args) {
  if (const int rc = allow_dynamic_lds<Kernel>(lds, what, dev)) return rc;
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, std::forward<Args>(args)...);
  return IFX_OK;
}
template <auto Kernel, class... Args>
int launch_lds(dim3 grid, dim3 block, int lds, hipStream_t s, const char* what, Args&&... args) {
  return launch_lds_on<Kernel>(current_device(), grid, block, lds, s, what, std::forward<Args>(args)...);
}

}  // namespace ifx
