// exo_detrend.hip -- the running location filters before the period search (exoplanet_amd/estimators.py: location_plan,
// running_location, flatten, sde): time windows on a sorted axis, and the running median, MAD and biweight location of a
// batch of series over them.  A translation unit of its own: none of the other kernels changes.  The arithmetic of one
// window lives in exo_detrend_core.hpp (tested on the host); definition, layout, resources and timings: DESIGN.md section 19.
//
// The filter: a workgroup of kTile threads owns kTile consecutive cadences of one series and stages, once, every value that
// any of their windows holds -- from the first cadence's window start to the last cadence's window end, at most
// kTile + 2 max_window - 2 values -- in LDS, an excluded cadence as a NaN.  A thread owns one cadence; the lanes of a wave own
// consecutive cadences, whose windows start at (all but) consecutive LDS addresses, so that every pass of the selection
// reads consecutive 8-byte words across the wave.  No atomics, no scratch, nothing but kernels enqueued.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_detrend_core.hpp"
#include "exo_estimators_launch.hpp"

namespace {

using namespace detrend;

constexpr int kTile = 256;         // cadences (threads) per workgroup of the filter
constexpr int kPlanThreads = 1024; // the segments kernel: one workgroup
constexpr int kWinThreads = 256;
constexpr int kMaxWindow = EXO_LOCATION_MAX_WINDOW;
// the staged span of the widest call: 133 104 bytes of the 160 KiB a workgroup may have
static_assert((kTile + 2 * kMaxWindow - 2) * 8 <= 160 * 1024, "EXO_LOCATION_MAX_WINDOW does not fit the LDS");
static_assert(EXO_LOCATION_MEDIAN == kMethodMedian && EXO_LOCATION_BIWEIGHT == kMethodBiweight, "method constants");

// A window as the core header reads it: a pointer into the LDS address space, so that every read is a ds_read, and
// volatile, so that each stays ONE 8-byte read (ds_read_b64: 256 B per clock and CU).  Left alone, the compiler pairs a
// lane's neighbouring values into two-address reads (ds_read2_b64), which move half as much per LDS cycle -- and the LDS
// is what bounds these kernels (measured both ways).
using Window = const volatile __attribute__((address_space(3))) double*;

__device__ __forceinline__ bool opens_segment(const double* __restrict__ t, int64_t i, double break_tolerance) {
  return i == 0 || t[i] - t[i - 1] > break_tolerance;
}

// Segments.  One workgroup, thread k owns the cadences [k c, (k + 1) c): lo[i] <- the first cadence of i's segment,
// hi[i] <- its last.  (The outputs of the plan double as its scratch: location_windows_kernel replaces them in place.)
__global__ __launch_bounds__(kPlanThreads) void location_segments_kernel(const double* __restrict__ t, int64_t n,
                                                                          double break_tolerance, int32_t* __restrict__ lo,
                                                                          int32_t* __restrict__ hi) {
  __shared__ int64_t last_open[kPlanThreads], first_open[kPlanThreads];
  const int64_t c = (n + kPlanThreads - 1) / kPlanThreads;
  const int64_t i0 = threadIdx.x * c < n ? threadIdx.x * c : n, i1 = i0 + c < n ? i0 + c : n;
  int64_t last = -1, first = n;
  for (int64_t i = i0; i < i1; ++i)
    if (opens_segment(t, i, break_tolerance)) {
      last = i;
      first = first == n ? i : first;
    }
  last_open[threadIdx.x] = last;
  first_open[threadIdx.x] = first;
  __syncthreads();
  int64_t start = 0, next = n;  // the segment open at i0, and the first one opened at or after i1
  for (int k = 0; k < (int)threadIdx.x; ++k) start = last_open[k] > start ? last_open[k] : start;
  for (int k = kPlanThreads - 1; k > (int)threadIdx.x; --k) next = first_open[k] < next ? first_open[k] : next;
  for (int64_t i = i0; i < i1; ++i) {
    if (opens_segment(t, i, break_tolerance)) start = i;
    lo[i] = (int32_t)start;
  }
  for (int64_t i = i1 - 1; i >= i0; --i) {
    hi[i] = (int32_t)(next - 1);
    if (opens_segment(t, i, break_tolerance)) next = i;
  }
}

// Windows: cadence i's [lo, hi] inside its segment [lo[i], hi[i]] (read, then replaced), and its edge flag
__global__ __launch_bounds__(kWinThreads) void location_windows_kernel(const double* __restrict__ t, int64_t n, double half_window,
                                                                        double edge_cutoff, int32_t* __restrict__ lo,
                                                                        int32_t* __restrict__ hi, uint8_t* __restrict__ edge) {
  const int64_t i = (int64_t)blockIdx.x * kWinThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t s = lo[i], e = hi[i];
  const double ti = t[i];
  const double below = ti - half_window, above = ti + half_window;  // one fp64 operation each: DESIGN.md 19.1
  edge[i] = (ti - t[s] < edge_cutoff || t[e] - ti < edge_cutoff) ? 1 : 0;
  lo[i] = (int32_t)window_lo(t, s, i, below);
  hi[i] = (int32_t)window_hi(t, i, e, above);
}

// The filter.  grid: (tiles of kTile cadences, series); dynamic LDS: `capacity` doubles.  Every index is checked against
// [0, n) and against the staged span before it is used: a cadence whose window is wider than max_window, does not hold
// the cadence's tile-mates' order (lo, hi not from the plan) or does not fit the span gets NaN.
__global__ __launch_bounds__(kTile) void running_location_kernel(const double* __restrict__ y, const uint8_t* __restrict__ exclude,
                                                                  int64_t exclude_stride, int64_t n, const int32_t* __restrict__ lo,
                                                                  const int32_t* __restrict__ hi, const uint8_t* __restrict__ edge,
                                                                  int32_t max_window, int32_t capacity, int32_t method, double cval,
                                                                  int32_t n_iter, double* __restrict__ trend,
                                                                  double* __restrict__ scale) {
  extern __shared__ __align__(16) double span[];
  const int64_t b = blockIdx.y;
  const int64_t first = (int64_t)blockIdx.x * kTile;
  const int64_t last = first + kTile <= n ? first + kTile - 1 : n - 1;
  int64_t base = lo[first], end = hi[last];
  base = base < 0 ? 0 : (base > first ? first : base);
  end = end > n - 1 ? n - 1 : (end < last ? last : end);
  const int64_t staged = end - base + 1 < capacity ? end - base + 1 : capacity;
  const double* yb = y + b * n;
  const uint8_t* xb = exclude ? exclude + b * exclude_stride : nullptr;
  for (int64_t k = threadIdx.x; k < staged; k += kTile) {
    double v = yb[base + k];
    if (xb && xb[base + k]) v = bits_double(kExcludedBits);
    span[k] = v;
  }
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  if (i >= n) return;
  const int64_t l = lo[i], h = hi[i];
  double loc = NAN, sc = NAN;
  const bool inside = l >= base && h >= l && h - l + 1 <= max_window && h - base < staged;
  if (inside && !(edge && edge[i])) loc = window_location((Window)(span + (l - base)),(int)(h - l + 1), method, cval, n_iter, scale != nullptr, &sc);
  trend[b * n + i] = loc;
  if (scale) scale[b * n + i] = sc;
}

}  // namespace

extern "C" {

int exo_location_windows_f64(const double* t, int64_t n, double half_window, double break_tolerance, double edge_cutoff,
                             int32_t* lo, int32_t* hi, uint8_t* edge, int32_t* widest, void* stream) {
  if (!t || !lo || !hi || !edge || !widest || n < 1 || n > INT32_MAX || !(half_window >= 0.0) || !(break_tolerance > 0.0) ||
      !(edge_cutoff >= 0.0))
    return EXO_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(location_segments_kernel, dim3(1), dim3(kPlanThreads), 0, s, t, n, break_tolerance, lo, hi);
  hipLaunchKernelGGL(location_windows_kernel, dim3((unsigned)((n + kWinThreads - 1) / kWinThreads)), dim3(kWinThreads), 0, s, t, n,
                     half_window, edge_cutoff, lo, hi, edge);
  hipLaunchKernelGGL(widest_window_kernel<kWidestThreads>, dim3(1), dim3(kWidestThreads), 0, s, (const int32_t*)lo, (const int32_t*)hi, n, widest);
  return launch_status();
}

int exo_running_location_f64(const double* y, const uint8_t* exclude, int64_t n_exclude, int64_t n, int64_t n_series,
                             const int32_t* lo, const int32_t* hi, const uint8_t* edge, int32_t max_window, int32_t method,
                             double cval, int32_t n_iter, double* trend, double* scale, void* stream) {
  if (!y || !lo || !hi || !trend || n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535 || !(cval > 0.0) || n_iter < 0 ||
      (method != EXO_LOCATION_MEDIAN && method != EXO_LOCATION_BIWEIGHT) || max_window < 1 || max_window > kMaxWindow ||
      (n_exclude != 0 && n_exclude != 1 && n_exclude != n_series) || (n_exclude > 0 && !exclude))
    return EXO_ERR_INVALID_ARGUMENT;
  const int32_t capacity = kTile + 2 * max_window - 2;
  const size_t lds = (size_t)capacity * 8;
  if (!allow_dynamic_lds(running_location_kernel, lds)) return EXO_ERR_LAUNCH;
  hipLaunchKernelGGL(running_location_kernel, dim3((unsigned)((n + kTile - 1) / kTile), (unsigned)n_series), dim3(kTile), lds,
                     (hipStream_t)stream, y, n_exclude > 0 ? exclude : nullptr, n_exclude > 1 ? n : (int64_t)0, n, lo, hi, edge,
                     max_window, capacity, method, cval, n_iter, trend, scale);
  return launch_status();
}

}  // extern "C"
