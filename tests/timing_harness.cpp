// Host build of exoplanet_amd/csrc/exo_timing_core.hpp for tests/test_timing_host.py: the template as a function, the window
// search, the vertex of the parabola, and one whole transit the way the kernel strings them together (stage, mean, every shift
// in ascending order, the lowest index of the maximum, the record).  g++ -O2 -std=c++17 -ffp-contract=off; no GPU.
#define EXO_HOST_BUILD 1
#include "../exoplanet_amd/csrc/exo_timing_core.hpp"

#include <chrono>
#include <vector>

using namespace timing;

extern "C" {

int harness_cap(int which) {
  return which == 0 ? EXO_TIMING_MAX_WINDOW : which == 1 ? EXO_TIMING_MAX_TEMPLATE : which == 2 ? EXO_TIMING_MAX_SHIFTS : EXO_TIMING_THREADS;
}

int64_t harness_lds_bytes(int64_t max_window, int64_t n_template, int64_t n_shift) { return lds_bytes(max_window, n_template, n_shift); }

double harness_template_value(const double* g, int m, double x) { return template_value(g, m, x); }

double harness_shift_value(double max_shift, int n_shift, int j) { return shift_value(max_shift, shift_step(max_shift, n_shift), j); }

void harness_windows(const double* t, int64_t n, const int64_t* epochs, int64_t n_transit, double period, double t0, double window,
                     double* linear_time, int32_t* lo, int32_t* hi) {
  for (int64_t k = 0; k < n_transit; ++k) {
    linear_time[k] = t0 + period * (double)epochs[k];
    transit_window(t, n, linear_time[k], 0.5 * window, lo + k, hi + k);
  }
}

// -> at_edge; out: shift, time_err
int harness_vertex(double lm, double l0, double lp, int j, int n_shift, double delta, double h, double* out) {
  const Vertex v = parabola_vertex(lm, l0, lp, j, n_shift, delta, h);
  out[0] = v.shift;
  out[1] = v.time_err;
  return v.at_edge;
}

// One transit of one series.  ivar, depth: null or one value per cadence / one value.  rec[7]: transit_time, shift, time_err,
// depth, depth_err, log_likelihood, depth_snr; irec[4]: n_window, n_in, valid, at_edge; curve[n_shift].
void harness_transit(const double* t, const double* y, const double* ivar, double T, int32_t lo, int32_t hi, double duration,
                     double max_shift, int n_shift, const double* g, int m, const double* depth, int min_in_transit, double* rec,
                     int32_t* irec, double* curve) {
  const int len = hi - lo + 1 > 0 ? hi - lo + 1 : 0;
  std::vector<double> tp(len), yp(len), w(len);
  double W = 0.0, WY = 0.0;
  int n_pos = 0;
  for (int i = 0; i < len; ++i) {
    tp[i] = t[lo + i] - T;
    w[i] = ivar ? ivar[lo + i] : 1.0;
    yp[i] = y[lo + i];
    W += w[i];
    WY += w[i] * yp[i];
    n_pos += w[i] > 0.0 ? 1 : 0;
  }
  const double ybar = WY / W;
  for (int i = 0; i < len; ++i) yp[i] -= ybar;
  const double h = shift_step(max_shift, n_shift);
  double best_L = -INFINITY, best_d = NAN, best_e = NAN;
  int best_j = -1, best_in = 0;
  for (int j = 0; j < n_shift; ++j) {
    ShiftFit f = {-INFINITY, NAN, NAN};
    int n_in = 0;
    if (n_pos > 0) {
      const ShiftSums s = shift_sums((const double*)tp.data(), (const double*)yp.data(), (const double*)w.data(), len, g, m,
                                     shift_value(max_shift, h, j), 0.5 * duration);
      f = solve_shift(s, W, n_pos, min_in_transit, depth != nullptr, depth ? *depth : 0.0);
      n_in = s.n_in;
    }
    curve[j] = f.L;
    if (f.L > best_L) {
      best_L = f.L;
      best_d = f.depth;
      best_e = f.depth_err;
      best_j = j;
      best_in = n_in;
    }
  }
  for (int f = 0; f < 7; ++f) rec[f] = NAN;
  irec[0] = len;
  irec[1] = irec[2] = irec[3] = 0;
  if (best_j < 0) return;
  const Vertex v = parabola_vertex(best_j > 0 ? curve[best_j - 1] : -INFINITY, best_L, best_j < n_shift - 1 ? curve[best_j + 1] : -INFINITY,
                                   best_j, n_shift, shift_value(max_shift, h, best_j), h);
  rec[0] = T + v.shift;
  rec[1] = v.shift;
  rec[2] = v.time_err;
  rec[3] = best_d;
  rec[4] = best_e;
  rec[5] = best_L;
  rec[6] = best_d / best_e;
  irec[1] = best_in;
  irec[2] = 1;
  irec[3] = v.at_edge;
}

// every transit of n_series series (the shape of exo_transit_timing_f64's outputs, without the curve) -> seconds on this core
double harness_all(const double* t, const double* y, const double* ivar, int64_t n, int64_t n_series, const double* linear_time,
                   const int32_t* lo, const int32_t* hi, int64_t n_transit, double duration, double max_shift, int n_shift,
                   const double* g, int m, int min_in_transit, double* out, int32_t* iout) {
  const auto start = std::chrono::steady_clock::now();
  std::vector<double> curve(n_shift);
  const int64_t plane = n_series * n_transit;
  for (int64_t b = 0; b < n_series; ++b)
    for (int64_t k = 0; k < n_transit; ++k) {
      double rec[7];
      int32_t irec[4];
      harness_transit(t, y + b * n, ivar, linear_time[k], lo[k], hi[k], duration, max_shift, n_shift, g, m, nullptr, min_in_transit, rec,
                      irec, curve.data());
      for (int f = 0; f < 7; ++f) out[f * plane + b * n_transit + k] = rec[f];
      for (int f = 0; f < 4; ++f) iout[f * plane + b * n_transit + k] = irec[f];
    }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
}

}  // extern "C"
