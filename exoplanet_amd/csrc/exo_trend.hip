// exo_trend.hip -- the robust local-polynomial trend of exoplanet_amd/estimators.py (running_location / flatten with
// order = 1 or 2): Tukey-biweight M-estimation of a polynomial of degree 1 or 2 in the time of each cadence's window,
// evaluated at the cadence's own time.  The windows are those of exo_detrend.hip (exo_location_windows_f64); the arithmetic
// of one window lives in exo_detrend_core.hpp (window_trend, tested on the host); definition, layout, resources and
// timings: DESIGN.md section 21.  A translation unit of its own, built without contraction into fused multiply-adds
// (__graft_entry__.py), so that the kernel does the IEEE operations of the host build, in the same order.
//
// The kernel is running_location_kernel with a second staged array: a workgroup of kTile threads owns kTile consecutive
// cadences of one series and stages, once, the span of y (an excluded cadence as a NaN) AND of t that their windows hold, at
// most kTile + 2 max_window - 2 cadences each.  A thread owns one cadence and makes every pass over the two arrays at the same
// offsets, each read one 8-byte LDS read.  No atomics, no scratch, no workspace, nothing but the kernel enqueued.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_detrend_core.hpp"
#include "exo_estimators_launch.hpp"

namespace {

using namespace detrend;

constexpr int kTile = 256;  // cadences (threads) per workgroup
constexpr int kMaxWindow = EXO_TREND_MAX_WINDOW;
// the two staged spans of the widest call: 135 136 bytes of the 160 KiB a workgroup may have
static_assert(2 * (kTile + 2 * kMaxWindow - 2) * 8 <= 160 * 1024, "EXO_TREND_MAX_WINDOW does not fit the LDS");
static_assert(kMaxWindow >= 4096 && kMaxWindow <= EXO_LOCATION_MAX_WINDOW, "EXO_TREND_MAX_WINDOW");

// as in exo_detrend.hip: an LDS-address-space volatile pointer keeps every read ONE ds_read_b64
using Window = const volatile __attribute__((address_space(3))) double*;

// grid: (tiles of kTile cadences, series); dynamic LDS: 2 * `capacity` doubles, the values then the times.  Every index is
// checked against [0, n) and against the staged span before it is used: a cadence whose window is wider than max_window,
// does not hold the cadence itself, does not follow its tile-mates' order (lo, hi not from the plan) or does not fit the span
// gets NaN.
template <int ORDER>
__global__ __launch_bounds__(kTile) void running_trend_kernel(const double* __restrict__ t, const double* __restrict__ y,
                                                               const uint8_t* __restrict__ exclude, int64_t exclude_stride, int64_t n,
                                                               const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                               const uint8_t* __restrict__ edge, int32_t max_window, int32_t capacity,
                                                               double cval, int32_t n_iter, int32_t rescale, double* __restrict__ trend,
                                                               double* __restrict__ scale) {
  extern __shared__ __align__(16) double span[];
  double* const values = span;
  double* const times = span + capacity;
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
    values[k] = v;
    times[k] = t[base + k];
  }
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  if (i >= n) return;
  const int64_t l = lo[i], h = hi[i];
  double loc = NAN, sc = NAN;
  const bool inside = l >= base && l <= i && h >= i && h - l + 1 <= max_window && h - base < staged;
  if (inside && !(edge && edge[i])) {
    const double t0 = ((Window)times)[i - base];
    loc = window_trend<ORDER>((Window)(values + (l - base)), (Window)(times + (l - base)), (int)(h - l + 1), t0, cval, n_iter, rescale, &sc);
  }
  trend[b * n + i] = loc;
  if (scale) scale[b * n + i] = sc;
}

template <int ORDER>
int launch(const double* t, const double* y, const uint8_t* exclude, int64_t exclude_stride, int64_t n, int64_t n_series,
           const int32_t* lo, const int32_t* hi, const uint8_t* edge, int32_t max_window, double cval, int32_t n_iter, int32_t rescale,
           double* trend, double* scale, hipStream_t stream) {
  const int32_t capacity = kTile + 2 * max_window - 2;
  const size_t lds = (size_t)capacity * 16;
  if (!allow_dynamic_lds(running_trend_kernel<ORDER>, lds)) return EXO_ERR_LAUNCH;
  hipLaunchKernelGGL(running_trend_kernel<ORDER>, dim3((unsigned)((n + kTile - 1) / kTile), (unsigned)n_series), dim3(kTile), lds, stream,
                     t, y, exclude, exclude_stride, n, lo, hi, edge, max_window, capacity, cval, n_iter, rescale, trend, scale);
  return launch_status();
}

}  // namespace

extern "C" {

int exo_running_trend_f64(const double* t, const double* y, const uint8_t* exclude, int64_t n_exclude, int64_t n, int64_t n_series,
                          const int32_t* lo, const int32_t* hi, const uint8_t* edge, int32_t max_window, int32_t order, double cval,
                          int32_t n_iter, int32_t rescale, double* trend, double* scale, void* stream) {
  if (!t || !y || !lo || !hi || !trend || n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535 || !(cval > 0.0) || n_iter < 0 ||
      rescale < 0 || (order != 1 && order != 2) || max_window < 1 || max_window > kMaxWindow ||
      (n_exclude != 0 && n_exclude != 1 && n_exclude != n_series) || (n_exclude > 0 && !exclude))
    return EXO_ERR_INVALID_ARGUMENT;
  const uint8_t* ex = n_exclude > 0 ? exclude : nullptr;
  const int64_t stride = n_exclude > 1 ? n : (int64_t)0;
  return order == 1 ? launch<1>(t, y, ex, stride, n, n_series, lo, hi, edge, max_window, cval, n_iter, rescale, trend, scale, (hipStream_t)stream)
                    : launch<2>(t, y, ex, stride, n, n_series, lo, hi, edge, max_window, cval, n_iter, rescale, trend, scale, (hipStream_t)stream);
}

}  // extern "C"
