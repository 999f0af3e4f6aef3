// rdyn_launch_util.h -- host-side pieces every launch function needs: the switch from a run-time joint count to the kernel instantiated
// for it, and the opt-in for more than 64 KB of dynamic LDS.
#ifndef RDYN_LAUNCH_UTIL_H
#define RDYN_LAUNCH_UTIL_H
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

// `return CALL(nj)` with nj as a compile-time constant; hipErrorInvalidValue for a count the kernel is not instantiated for.  CALL is a
// function-like macro of the call site.  1 .. 10 joints (RDYN_MAX_SWEPT_JOINTS) for the one-lane-per-sample kernels; the LDS-staged Gram
// / QR kernels start at 2 and, where the factor must fit the LDS beside the tiles, end at 7 (a case that is not listed is not instantiated).
#define RDYN_NJ_CASES_2_7(CALL) \
  case 2: return CALL(2);       \
  case 3: return CALL(3);       \
  case 4: return CALL(4);       \
  case 5: return CALL(5);       \
  case 6: return CALL(6);       \
  case 7: return CALL(7);
#define RDYN_NJ_CASES_8_10(CALL) \
  case 8: return CALL(8);        \
  case 9: return CALL(9);        \
  case 10: return CALL(10);
#define RDYN_DISPATCH_NJ(nj, CALL)      \
  switch (nj)                           \
  {                                     \
  case 1: return CALL(1);               \
  RDYN_NJ_CASES_2_7(CALL)               \
  RDYN_NJ_CASES_8_10(CALL)              \
  default: return hipErrorInvalidValue; \
  }
#define RDYN_DISPATCH_JOINTS_2_7(nj, CALL) \
  switch (nj)                              \
  {                                        \
  RDYN_NJ_CASES_2_7(CALL)                  \
  default: return hipErrorInvalidValue;    \
  }

namespace
{
// More than 64 KB of dynamic LDS needs the attribute, once per kernel and device (one bit per device ordinal).  A call site that mostly
// launches with less tests its size before it calls.
template <auto Kernel>
hipError_t opt_in_lds_once(int max_bytes = 160 * 1024)
{
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_acquire) & bit))
  {
    e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
    if (e != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_release);
  }
  return hipSuccess;
}
}  // namespace
#endif
