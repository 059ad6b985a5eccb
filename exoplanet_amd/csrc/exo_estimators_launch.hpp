// exo_estimators_launch.hpp -- what the six translation units of the estimators (exo_estimators.hip, exo_detrend.hip,
// exo_trend.hip, exo_timing.hip, exo_keplerian.hip, exo_astrometric.hip) share on the host side of a launch: the status of
// the launches just enqueued, the widest-window kernel of the two plans, and the permission a kernel needs for more than
// 64 KiB of dynamic LDS.  Everything sits in an unnamed namespace: no device code crosses translation units, so each unit
// that includes this gets a copy of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"

namespace {

inline int launch_status() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

constexpr int kWidestThreads = 1024;

// the widest window, max(hi - lo + 1) (one workgroup of kWorkgroup, launched with kWidestThreads; a fixed order, no atomics).
// A template, so that a unit that does not launch it does not carry it.
template <int kWorkgroup>
__global__ __launch_bounds__(kWorkgroup) void widest_window_kernel(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                        int64_t n, int32_t* __restrict__ widest) {
  __shared__ int32_t part[kWorkgroup];
  int32_t w = 0;
  for (int64_t i = threadIdx.x; i < n; i += kWorkgroup) {
    const int32_t wi = hi[i] - lo[i] + 1;
    w = wi > w ? wi : w;
  }
  part[threadIdx.x] = w;
  __syncthreads();
  for (int o = kWorkgroup / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] = part[threadIdx.x + o] > part[threadIdx.x] ? part[threadIdx.x + o] : part[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) *widest = part[0];
}

// Dynamic LDS above the 64 KiB a launch may ask for by default: a property of the function, not a stream operation.
// false: the runtime refused.
template <class Kernel>
inline bool allow_dynamic_lds(Kernel* kernel, size_t bytes) {
  return bytes <= 64 * 1024 ||
         hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

}  // namespace
