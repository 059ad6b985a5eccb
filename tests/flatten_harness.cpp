// Host build of exoplanet_amd/csrc/exo_detrend_core.hpp for tests/test_flatten_host.py and tools/flatten_timing.py (g++, no
// GPU): the key map, selection, median, MAD, biweight and the window search, exactly as the kernels call them.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_detrend_core.hpp"

#include <vector>

using namespace detrend;

extern "C" {

uint64_t harness_key(double x) { return double_key(x); }
double harness_unkey(uint64_t k) { return key_double(k); }

// an excluded cadence of a window, as the kernel stages it
double harness_excluded(void) { return bits_double(kExcludedBits); }

int harness_count_valid(const double* v, int len) { return count_valid(v, len); }
double harness_select(const double* v, int len, int k) { return select_kth(v, len, k, Identity{}); }
double harness_median(const double* v, int len) { return median(v, len, count_valid(v, len)); }
double harness_mad(const double* v, int len, double centre) { return mad(v, len, count_valid(v, len), centre); }
double harness_biweight(const double* v, int len, double med, double mad_, double cval, int n_iter) {
  return biweight(v, len, med, mad_, cval, n_iter);
}

// the windows of the cadences [i0, i1) of one segment [s, e]
void harness_windows(const double* t, int64_t s, int64_t e, double half_window, int64_t i0, int64_t i1, int32_t* lo, int32_t* hi) {
  for (int64_t i = i0; i < i1; ++i) {
    lo[i] = (int32_t)window_lo(t, s, i, t[i] - half_window);
    hi[i] = (int32_t)window_hi(t, i, e, t[i] + half_window);
  }
}

// the filter over the cadences [i0, i1) of one series, one window at a time (the CPU time beside the kernel's)
void harness_running_location(const double* y, const uint8_t* exclude, const int32_t* lo, const int32_t* hi, int64_t i0, int64_t i1,
                              int method, double cval, int n_iter, double* trend, double* scale) {
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
    trend[i] = window_location(v, len, method, cval, n_iter, scale != nullptr, &sc);
    if (scale) scale[i] = sc;
  }
}

}  // extern "C"
