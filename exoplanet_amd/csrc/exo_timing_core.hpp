// exo_timing_core.hpp -- the arithmetic of the per-transit fit (exoplanet_amd/estimators.py: timing_plan, transit_times,
// ttv_estimator): the template as a continuous function, the sums of one trial shift over a window and their solution, the
// vertex of the parabola through the likelihood's three samples around its maximum, and the window search.  Definitions:
// DESIGN.md section 20.  Compiles for the device (exo_timing.hip) and, with EXO_HOST_BUILD, for the host
// (tests/timing_harness.cpp checks it against the numpy statement tests/timing_oracle.py without a GPU).  Both builds use
// -ffp-contract=off: every expression below is the IEEE operations it spells, in the order it spells them.
//
// A window is `len` consecutive cadences: tp[i] = t_i - T_k (non-decreasing), yp[i] = y_i - ybar, w[i] >= 0.  Nothing here
// stores: on the device the window stays where the workgroup staged it (LDS) and a lane needs a handful of registers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_TIM_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_TIM_HD __device__ __forceinline__
#endif

#include "../../include/exoplanet_amd.h"  // the caps EXO_TIMING_MAX_WINDOW, _MAX_TEMPLATE, _MAX_SHIFTS

#define EXO_TIMING_THREADS 256  // lanes of the workgroup of one (transit, series)

namespace timing {

// bytes of LDS of a workgroup: the window (tp, yp, w), the template, the curve L, and the reduction's two doubles and one
// int per lane
constexpr int64_t lds_bytes(int64_t max_window, int64_t n_template, int64_t n_shift) {
  return 8 * (3 * max_window + n_template + n_shift + 2 * EXO_TIMING_THREADS) + 4 * EXO_TIMING_THREADS;
}
static_assert(lds_bytes(EXO_TIMING_MAX_WINDOW, EXO_TIMING_MAX_TEMPLATE, EXO_TIMING_MAX_SHIFTS) <= 160 * 1024,
              "the caps of the timing kernel do not fit the LDS");

// trial shift j of M: exactly this expression, never an accumulated sum
EXO_TIM_HD double shift_step(double max_shift, int n_shift) { return 2.0 * max_shift / (double)(n_shift - 1); }
EXO_TIM_HD double shift_value(double max_shift, double h, int j) { return -max_shift + (double)j * h; }

// The template g[0 .. m - 1], samples at the bin centres x_q = (2 q + 1) / m - 1, as a continuous function of x: linear
// between neighbouring centres, linear to 0 at x = -1 and x = +1 beyond the outermost ones, 0 for |x| >= 1 (and for a NaN).
// u = (x + 1) (m / 2) - 1/2 is the position in units of bins, centre q at u = q.
template <class P>
EXO_TIM_HD double template_value(P g, int m, double x) {
  if (!(fabs(x) < 1.0)) return 0.0;
  const double u = (x + 1.0) * (0.5 * (double)m) - 0.5;
  if (u <= 0.0) return g[0] * (2.0 * u + 1.0);
  const double last = (double)(m - 1);
  if (u >= last) return g[m - 1] * (2.0 * (last - u) + 1.0);
  const int q = (int)u;  // 0 <= q <= m - 2: floor, u being positive
  const double f = u - (double)q;
  const double a = g[q];
  return a + f * (g[q + 1] - a);
}

EXO_TIM_HD double template_argument(double tp, double delta, double half_duration) { return (tp - delta) / half_duration; }

struct ShiftSums {
  double G, GG, GY;
  int n_in;  // cadences with w > 0 and |x| < 1
};

// The sums of one trial shift over the window, in the window's order.  x is non-decreasing along the window (each of its
// two operations is monotone), so the cadences inside the template, |x| < 1, are one run [a, b): both ends are bisected on
// the very x the sum uses, and the cadences outside -- whose terms are exact zeros -- are not visited.
template <class P, class Q>
EXO_TIM_HD ShiftSums shift_sums(P tp, P yp, P w, int len, Q g, int m, double delta, double half_duration) {
  int a = 0, e = len;  // first cadence with x > -1
  while (a < e) {
    const int mid = a + (e - a) / 2;
    if (template_argument(tp[mid], delta, half_duration) > -1.0) e = mid; else a = mid + 1;
  }
  int b = a;           // first cadence at or after a with x >= 1
  e = len;
  while (b < e) {
    const int mid = b + (e - b) / 2;
    if (template_argument(tp[mid], delta, half_duration) < 1.0) b = mid + 1; else e = mid;
  }
  ShiftSums s = {0.0, 0.0, 0.0, 0};
  for (int i = a; i < b; ++i) {
    const double wi = w[i];
    const double gi = template_value(g, m, template_argument(tp[i], delta, half_duration));
    const double wg = wi * gi;
    s.G += wg;
    s.GG += wg * gi;
    s.GY += wg * yp[i];
    s.n_in += wi > 0.0 ? 1 : 0;
  }
  return s;
}

struct ShiftFit {
  double L, depth, depth_err;  // L = -inf: not admissible (depth and depth_err then NaN)
};

// The model c - d g with the level c always fitted.  W = sum w and n_pos = #{w > 0} of the window.  Free depth:
// d = -GY / D, depth_err = 1 / sqrt(D), L = GY^2 / (2 D); held depth: d as given, L = -d GY - d d D / 2, depth_err NaN.
EXO_TIM_HD ShiftFit solve_shift(const ShiftSums& s, double W, int n_pos, int min_in_transit, bool held, double depth) {
  ShiftFit f = {-INFINITY, NAN, NAN};
  const double D = s.GG - s.G * s.G / W;
  if (s.n_in < min_in_transit || n_pos - s.n_in < 1 || !(D > 0.0)) return f;
  if (held) {
    f.depth = depth;
    f.L = -depth * s.GY - depth * depth * D / 2.0;
  } else {
    f.depth = -s.GY / D;
    f.depth_err = 1.0 / sqrt(D);
    f.L = s.GY * s.GY / (2.0 * D);
  }
  if (!(f.L > -INFINITY)) f = ShiftFit{-INFINITY, NAN, NAN};  // (a NaN in the series: no fit)
  return f;
}

struct Vertex {
  double shift, time_err;
  int at_edge;
};

// The maximum at shift j of M with the curve's values lm, l0, lp at j - 1, j, j + 1 (lm / lp are not read at the grid's ends):
// S = (lm - 2 l0) + lp; an end of the grid, a neighbour without a fit or S >= 0: at_edge, the grid's shift, time_err NaN.
EXO_TIM_HD Vertex parabola_vertex(double lm, double l0, double lp, int j, int n_shift, double delta, double h) {
  Vertex v = {delta, NAN, 1};
  if (j <= 0 || j >= n_shift - 1 || !(lm > -INFINITY) || !(lp > -INFINITY)) return v;
  const double S = (lm - 2.0 * l0) + lp;
  if (!(S < 0.0)) return v;
  v.shift = delta - 0.5 * h * (lp - lm) / S;
  v.time_err = h / sqrt(-S);
  v.at_edge = 0;
  return v;
}

// ---- the windows ---------------------------------------------------------------------------------------------------------

// The window of the transit at T: the cadences with -half_window <= t_i - T <= half_window, the difference ONE fp64 operation
// (monotone in t_i, so both ends are bisected).  *lo = the first such cadence, *hi = the last; none: *hi = *lo - 1.
EXO_TIM_HD void transit_window(const double* t, int64_t n, double T, double half_window, int32_t* lo, int32_t* hi) {
  int64_t a = 0, e = n;  // first i with t_i - T >= -half_window
  while (a < e) {
    const int64_t mid = a + (e - a) / 2;
    if (t[mid] - T >= -half_window) e = mid; else a = mid + 1;
  }
  int64_t b = a;         // first i at or after a with t_i - T > half_window
  e = n;
  while (b < e) {
    const int64_t mid = b + (e - b) / 2;
    if (t[mid] - T <= half_window) b = mid + 1; else e = mid;
  }
  *lo = (int32_t)a;
  *hi = (int32_t)(b - 1);
}

}  // namespace timing
