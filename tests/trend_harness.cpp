// Host build of the local-polynomial trend of exoplanet_amd/csrc/exo_detrend_core.hpp (window_trend) for
// tests/test_trend_host.py and tools/flatten_timing.py (g++, no GPU), exactly as the kernel of exo_trend.hip calls it.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_detrend_core.hpp"

#include <vector>

using namespace detrend;

extern "C" {

// an excluded cadence of a window, as the kernel stages it
double trend_harness_excluded(void) { return bits_double(kExcludedBits); }

// one window: `len` values (excluded: the NaN above) and their times, the cadence's own time t0
double trend_harness_window(const double* v, const double* t, int len, double t0, int order, double cval, int n_iter, int rescale,
                            double* scale) {
  return order == 1 ? window_trend<1>(v, t, len, t0, cval, n_iter, rescale, scale)
                    : window_trend<2>(v, t, len, t0, cval, n_iter, rescale, scale);
}

// the filter over the cadences [i0, i1) of one series, one window at a time (the CPU time beside the kernel's)
void trend_harness_running(const double* t, const double* y, const uint8_t* exclude, const int32_t* lo, const int32_t* hi, int64_t i0,
                           int64_t i1, int order, double cval, int n_iter, int rescale, double* trend, double* scale) {
  std::vector<double> span;
  for (int64_t i = i0; i < i1; ++i) {
    const double* v = y + lo[i];
    const int len = hi[i] - lo[i] + 1;
    if (exclude) {
      span.assign(v, v + len);
      for (int j = 0; j < len; ++j)
        if (exclude[lo[i] + j]) span[j] = bits_double(kExcludedBits);
      v = span.data();
    }
    double sc = NAN;
    trend[i] = trend_harness_window(v, t + lo[i], len, t[i], order, cval, n_iter, rescale, &sc);
    if (scale) scale[i] = sc;
  }
}

}  // extern "C"
