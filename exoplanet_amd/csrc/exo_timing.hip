// exo_timing.hip -- per-transit times and depths (exoplanet_amd/estimators.py: timing_plan, transit_times, ttv_estimator):
// the windows of the transits of a linear ephemeris on a sorted time axis, and in each of them the search over the
// mid-time's shift with a limb-darkened template.  A translation unit of its own: none of the other kernels changes.  The
// arithmetic lives in exo_timing_core.hpp (tested on the host); definition, layout, resources and timings: DESIGN.md
// section 20.  Compiled with -ffp-contract=off, as the host build of the core is.
//
// The fit: a workgroup of EXO_TIMING_THREADS lanes owns one (transit, series).  It stages t - T_k, y and w of the window in
// LDS once, reduces W, sum w y and the count of w > 0 in a fixed shape, subtracts ybar, and then lane l takes the trial shifts
// l, l + 256, ...: for each it bisects the run of cadences inside the template and sums over that run in the window's order.
// The curve L lives in LDS; a lane remembers the best of its own shifts, a fixed-shape reduction finds the best of all
// (ties: the lowest j), and the lane that owns it writes the record.  No atomics, no scratch, nothing but kernels enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_timing_core.hpp"

namespace {

using namespace timing;

constexpr int kThreads = EXO_TIMING_THREADS;
constexpr int kWinThreads = 256;

__global__ __launch_bounds__(kWinThreads) void timing_windows_kernel(const double* __restrict__ t, int64_t n,
                                                                      const int64_t* __restrict__ epochs, int64_t n_transit,
                                                                      double period, double t0, double half_window,
                                                                      double* __restrict__ linear_time, int32_t* __restrict__ lo,
                                                                      int32_t* __restrict__ hi) {
  const int64_t k = (int64_t)blockIdx.x * kWinThreads + threadIdx.x;
  if (k >= n_transit) return;
  const double T = t0 + period * (double)epochs[k];
  linear_time[k] = T;
  transit_window(t, n, T, half_window, lo + k, hi + k);
}

// The fit.  grid: (transits, series); dynamic LDS: lds_bytes(max_window, m, n_shift).  lo and hi are clamped to [0, n) and the
// window's length to max_window before anything is read: a window that does not fit gives an invalid transit.
__global__ __launch_bounds__(kThreads) void transit_timing_kernel(
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ ivar, int64_t ivar_stride, int64_t n,
    const double* __restrict__ linear_time, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int64_t n_transit,
    int32_t max_window, double half_duration, double max_shift, int32_t n_shift, const double* __restrict__ tmpl, int32_t m,
    const double* __restrict__ depth, int64_t depth_stride, int32_t min_in_transit, double* __restrict__ out,
    int32_t* __restrict__ iout, double* __restrict__ curve) {
  extern __shared__ __align__(16) double lds[];
  double* tp = lds;
  double* yp = tp + max_window;
  double* w = yp + max_window;
  double* g = w + max_window;
  double* L = g + m;
  double* red_a = L + n_shift;
  double* red_b = red_a + kThreads;
  int32_t* red_i = (int32_t*)(red_b + kThreads);

  const int64_t k = blockIdx.x, b = blockIdx.y, n_series = gridDim.y;
  const int lane = threadIdx.x;
  int64_t first = lo[k], last = hi[k];
  const int32_t n_window = (int32_t)(last - first + 1 > 0 ? last - first + 1 : 0);
  first = first < 0 ? 0 : first;
  last = last > n - 1 ? n - 1 : last;
  int len = (int)(last - first + 1 > 0 ? last - first + 1 : 0);
  if (len != n_window || len > max_window) len = 0;  // (not a window of this axis, or wider than promised: no fit)
  const double T = linear_time[k];
  const double* yb = y + b * n;
  const double* wb = ivar ? ivar + b * ivar_stride : nullptr;

  // stage the window and the template; lane partials of W, sum w y and #{w > 0} over the cadences i = lane, lane + 256, ...
  double sw = 0.0, swy = 0.0;
  int n_pos = 0;
  for (int i = lane; i < len; i += kThreads) {
    const double yi = yb[first + i];
    const double wi = wb ? wb[first + i] : 1.0;
    tp[i] = t[first + i] - T;
    yp[i] = yi;
    w[i] = wi;
    sw += wi;
    swy += wi * yi;
    n_pos += wi > 0.0 ? 1 : 0;
  }
  for (int q = lane; q < m; q += kThreads) g[q] = tmpl[q];
  red_a[lane] = sw;
  red_b[lane] = swy;
  red_i[lane] = n_pos;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (lane < o) {
      red_a[lane] += red_a[lane + o];
      red_b[lane] += red_b[lane + o];
      red_i[lane] += red_i[lane + o];
    }
    __syncthreads();
  }
  const double W = red_a[0];
  const double ybar = red_b[0] / W;
  n_pos = red_i[0];
  __syncthreads();  // (the reduction's arrays are used again below)
  for (int i = lane; i < len; i += kThreads) yp[i] -= ybar;
  __syncthreads();

  // the shifts of this lane, ascending: a strict > keeps the lowest j of equal maxima
  const bool held = depth != nullptr;
  const double d_held = held ? depth[b * depth_stride] : 0.0;
  const double h = shift_step(max_shift, n_shift);
  double best_L = -INFINITY, best_d = NAN, best_e = NAN;
  int best_j = INT_MAX, best_in = 0;
  double* curve_row = curve ? curve + (b * n_transit + k) * (int64_t)n_shift : nullptr;
  for (int j = lane; j < n_shift; j += kThreads) {
    ShiftFit f = {-INFINITY, NAN, NAN};
    int n_in = 0;
    if (n_pos > 0) {
      const ShiftSums s = shift_sums((const double*)tp, (const double*)yp, (const double*)w, len, (const double*)g, m,
                                     shift_value(max_shift, h, j), half_duration);
      f = solve_shift(s, W, n_pos, min_in_transit, held, d_held);
      n_in = s.n_in;
    }
    L[j] = f.L;
    if (curve_row) curve_row[j] = f.L;
    if (f.L > best_L) {
      best_L = f.L;
      best_d = f.depth;
      best_e = f.depth_err;
      best_j = j;
      best_in = n_in;
    }
  }
  red_a[lane] = best_L;
  red_i[lane] = best_j;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (lane < o) {
      const double la = red_a[lane], lb = red_a[lane + o];
      const int ja = red_i[lane], jb = red_i[lane + o];
      if (lb > la || (lb == la && jb < ja)) {
        red_a[lane] = lb;
        red_i[lane] = jb;
      }
    }
    __syncthreads();
  }
  const int j_star = red_i[0];
  const bool valid = j_star != INT_MAX;
  if (lane != (valid ? j_star % kThreads : 0)) return;

  const int64_t slot = b * n_transit + k, plane = n_series * n_transit;
  double rec[7] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN};
  int at_edge = 0;
  if (valid) {
    const double delta = shift_value(max_shift, h, j_star);
    const Vertex v = parabola_vertex(j_star > 0 ? L[j_star - 1] : -INFINITY, best_L, j_star < n_shift - 1 ? L[j_star + 1] : -INFINITY,
                                     j_star, n_shift, delta, h);
    rec[0] = T + v.shift;
    rec[1] = v.shift;
    rec[2] = v.time_err;
    rec[3] = best_d;
    rec[4] = best_e;
    rec[5] = best_L;
    rec[6] = best_d / best_e;
    at_edge = v.at_edge;
  }
  for (int f = 0; f < 7; ++f) out[f * plane + slot] = rec[f];
  iout[0 * plane + slot] = n_window;
  iout[1 * plane + slot] = valid ? best_in : 0;
  iout[2 * plane + slot] = valid ? 1 : 0;
  iout[3 * plane + slot] = at_edge;
}

}  // namespace

extern "C" {

int exo_timing_windows_f64(const double* t, int64_t n, const int64_t* epochs, int64_t n_transit, double period, double t0,
                           double window, double* linear_time, int32_t* lo, int32_t* hi, int32_t* widest, void* stream) {
  if (!t || !epochs || !linear_time || !lo || !hi || !widest || n < 1 || n > INT32_MAX || n_transit < 1 || n_transit > INT32_MAX ||
      !(period > 0.0) || !(window > 0.0) || !(fabs(t0) < INFINITY))
    return EXO_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(timing_windows_kernel, dim3((unsigned)((n_transit + kWinThreads - 1) / kWinThreads)), dim3(kWinThreads), 0, s, t,
                     n, epochs, n_transit, period, t0, 0.5 * window, linear_time, lo, hi);
  hipLaunchKernelGGL(widest_window_kernel<kWidestThreads>, dim3(1), dim3(kWidestThreads), 0, s, (const int32_t*)lo, (const int32_t*)hi, n_transit,
                     widest);
  return launch_status();
}

int exo_transit_timing_f64(const double* t, const double* y, const double* ivar, int64_t n_ivar, int64_t n, int64_t n_series,
                           const double* linear_time, const int32_t* lo, const int32_t* hi, int64_t n_transit,
                           int32_t max_window, double duration, double max_shift, int32_t n_shift, double window,
                           const double* tmpl, int32_t n_template, const double* depth, int64_t n_depth,
                           int32_t min_in_transit, double* out, int32_t* iout, double* curve, void* stream) {
  if (!t || !y || !linear_time || !lo || !hi || !tmpl || !out || !iout || n < 1 || n > INT32_MAX || n_series < 1 ||
      n_series > 65535 || n_transit < 1 || n_transit > INT32_MAX || n_shift < 3 || n_shift % 2 == 0 || n_shift > EXO_TIMING_MAX_SHIFTS ||
      !(duration > 0.0) || !(window > 0.0) || !(max_shift >= 0.0) || !(window >= duration + 2.0 * max_shift) || max_window < 1 ||
      max_window > EXO_TIMING_MAX_WINDOW || n_template < 1 || n_template > EXO_TIMING_MAX_TEMPLATE || min_in_transit < 1 ||
      (n_ivar != 0 && n_ivar != 1 && n_ivar != n_series) || (n_ivar > 0 && !ivar) ||
      (n_depth != 0 && n_depth != 1 && n_depth != n_series) || (n_depth > 0 && !depth))
    return EXO_ERR_INVALID_ARGUMENT;
  const size_t lds = (size_t)lds_bytes(max_window, n_template, n_shift);
  if (!allow_dynamic_lds(transit_timing_kernel, lds)) return EXO_ERR_LAUNCH;
  hipLaunchKernelGGL(transit_timing_kernel, dim3((unsigned)n_transit, (unsigned)n_series), dim3(kThreads), lds, (hipStream_t)stream,
                     t, y, n_ivar > 0 ? ivar : nullptr, n_ivar > 1 ? n : (int64_t)0, n, linear_time, lo, hi, n_transit, max_window,
                     0.5 * duration, max_shift, n_shift, tmpl, n_template, n_depth > 0 ? depth : nullptr,
                     n_depth > 1 ? (int64_t)1 : (int64_t)0, min_in_transit, out, iout, curve);
  return launch_status();
}

}  // extern "C"
