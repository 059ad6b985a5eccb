// exo_detrend_core.hpp -- the per-window arithmetic of the running location filters (exoplanet_amd/estimators.py,
// running_location / flatten / sde): the order-preserving map from a double to a 64-bit key, selection of the k-th smallest
// value of a window by bisection on those keys, the median, the median absolute deviation and Tukey's biweight location.
// Definitions: DESIGN.md section 19.  Compiles for the device (exo_detrend.hip) and, with EXO_HOST_BUILD, for the host
// (tests/flatten_harness.cpp checks it against the numpy restatement tests/flatten_oracle.py without a GPU).  Below them, for
// order = 1 and 2 of the same functions, the biweight-weighted local polynomial in the window's time (DESIGN.md section 21;
// exo_trend.hip, tests/trend_harness.cpp, tests/trend_oracle.py).
//
// A window is `len` consecutive doubles v[0 .. len - 1]; a cadence that takes no part (the caller's `exclude`) holds
// kExcludedBits, a quiet NaN, and drops out of every comparison below by itself (a NaN compares false).  Nothing here sorts
// or stores: every function is a number of read-only passes over the window, so that on the device the window stays where
// the workgroup staged it (LDS) and a lane needs a handful of registers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_DET_HD inline
#define EXO_DET_UNROLL
#else
#include <hip/hip_runtime.h>
#define EXO_DET_HD __device__ __forceinline__
#define EXO_DET_UNROLL _Pragma("unroll 8")
#endif

namespace detrend {

constexpr uint64_t kSignBit = 0x8000000000000000ull;
constexpr uint64_t kExcludedBits = 0x7ff8000000000000ull;  // what an excluded cadence holds: +NaN (quiet)
constexpr uint64_t kKeyNegInf = 0x000fffffffffffffull;     // double_key(-inf): keys below it are NaNs with the sign bit
constexpr uint64_t kKeyPosInf = 0xfff0000000000000ull;     // double_key(+inf): keys above it are NaNs without

EXO_DET_HD uint64_t double_bits(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  return b;
}

EXO_DET_HD double bits_double(uint64_t b) {
  double x;
  __builtin_memcpy(&x, &b, 8);
  return x;
}

// The order-preserving map: a < b as doubles  =>  double_key(a) < double_key(b) as unsigned integers, for every pair of
// non-NaN doubles; -0 comes immediately before +0, -inf first, +inf last (NaNs beyond either end, by their sign).
EXO_DET_HD uint64_t double_key(double x) {
  const uint64_t b = double_bits(x);
  return (b & kSignBit) ? ~b : (b | kSignBit);
}

EXO_DET_HD double key_double(uint64_t k) { return bits_double((k & kSignBit) ? (k & ~kSignBit) : ~k); }

// what is selected from: the values themselves, or their absolute deviations from a centre (one correctly rounded
// subtraction each; never stored)
struct Identity {
  EXO_DET_HD double operator()(double v) const { return v; }
};

struct AbsDeviation {
  double centre;
  EXO_DET_HD double operator()(double v) const { return fabs(v - centre); }
};

// The window functions below take the window as any pointer P to double: a plain one on the host, the kernel's LDS pointer
// on the device (exo_detrend.hip, Window).  Every pass reads each value ONCE, in order.

// the number of cadences of the window that take part
template <class P>
EXO_DET_HD int count_valid(P v, int len) {
  int m = 0;
  EXO_DET_UNROLL
  for (int j = 0; j < len; ++j) {
    const double x = v[j];
    m += (x == x) ? 1 : 0;
  }
  return m;
}

// The k-th smallest (k = 0 .. m - 1) of the m participating values f(v[j]), as a number: the largest key x with
// #{f(v) < x} <= k is the key of that value, and it is built from the top bit down, one counting pass per bit.  The pass
// compares doubles, not keys (one comparison per value): the two orders agree except that -0 = +0 as doubles, so a zero
// comes back as +0 whatever its sign was -- the same NUMBER.  A trial key in the NaN ranges needs no pass: beyond +inf it
// is above every value (count = m > k), before -inf below every value (count = 0).  first_bit = 62 for values known to
// be non-negative (the top bit of their keys is set).
template <class P, class F>
EXO_DET_HD double select_kth(P v, int len, int k, F f, int first_bit = 63) {
  uint64_t r = first_bit < 63 ? kSignBit : 0;
  for (int bit = first_bit; bit >= 0; --bit) {
    const uint64_t trial = r | (1ull << bit);
    if (trial > kKeyPosInf) continue;
    if (trial >= kKeyNegInf) {
      const double x = key_double(trial);
      int c = 0;
      EXO_DET_UNROLL
      for (int j = 0; j < len; ++j) c += (f(v[j]) < x) ? 1 : 0;
      if (c > k) continue;
    }
    r = trial;
  }
  return key_double(r) + 0.0;  // (-0 -> +0: see above)
}

// the value after `a` in the sorted order, a being the k-th smallest: a itself where it is tied, else the smallest value above
template <class P, class F>
EXO_DET_HD double select_next(P v, int len, int k, double a, F f) {
  int c = 0;
  double up = INFINITY;
  EXO_DET_UNROLL
  for (int j = 0; j < len; ++j) {
    const double d = f(v[j]);
    c += (d <= a) ? 1 : 0;
    up = (d > a && d < up) ? d : up;
  }
  return c >= k + 2 ? a : up;
}

// median of the m >= 1 participating values: v[(m-1)/2] of the sorted values for odd m, 0.5 * (v[m/2-1] + v[m/2]) for even m
template <class P, class F>
EXO_DET_HD double median_of(P v, int len, int m, F f, int first_bit = 63) {
  const int k = (m - 1) / 2;
  const double a = select_kth(v, len, k, f, first_bit);
  if (m & 1) return a;
  return 0.5 * (a + select_next(v, len, k, a, f));
}

template <class P>
EXO_DET_HD double median(P v, int len, int m) { return median_of(v, len, m, Identity{}); }

// the median of |v - centre|, unscaled
template <class P>
EXO_DET_HD double mad(P v, int len, int m, double centre) { return median_of(v, len, m, AbsDeviation{centre}, 62); }

// Tukey's biweight location from the median and the MAD: exactly n_iter steps x += sum(d w) / sum(w), d = v - x,
// u = d / (cval mad), w = (1 - u^2)^2 inside |u| < 1; sums in the window's order.  mad == 0: the median.
template <class P>
EXO_DET_HD double biweight(P v, int len, double med, double mad_, double cval, int n_iter) {
  double x = med;
  if (mad_ == 0.0) return x;
  const double s = 1.0 / (cval * mad_);
  for (int it = 0; it < n_iter; ++it) {
    double sw = 0.0, sdw = 0.0;
    EXO_DET_UNROLL
    for (int j = 0; j < len; ++j) {
      const double d = v[j] - x;
      const double u = d * s;
      if (fabs(u) < 1.0) {
        const double q = 1.0 - u * u;
        const double w = q * q;
        sw += w;
        sdw += d * w;
      }
    }
    if (sw == 0.0) break;
    x += sdw / sw;
  }
  return x;
}

constexpr int kMethodMedian = 0, kMethodBiweight = 1;  // EXO_LOCATION_MEDIAN, EXO_LOCATION_BIWEIGHT

// location and scale (the MAD) of one window; no participating cadence: NaN and NaN.  want_scale = false and the median:
// the MAD is not computed (*scale untouched).
template <class P>
EXO_DET_HD double window_location(P v, int len, int method, double cval, int n_iter, bool want_scale, double* scale) {
  const int m = count_valid(v, len);
  if (m == 0) {
    if (want_scale) *scale = NAN;
    return NAN;
  }
  const double med = median(v, len, m);
  if (method == kMethodMedian && !want_scale) return med;
  const double s = mad(v, len, m, med);
  if (want_scale) *scale = s;
  return method == kMethodMedian ? med : biweight(v, len, med, s, cval, n_iter);
}

// ---- the local polynomial trend -----------------------------------------------------------------------
//
// Tukey-biweight M-estimation of a polynomial of degree P <= 2 in the time of a window, evaluated at the cadence's own time.
// The window is now two runs of `len` doubles read at the same offsets, the values v (an excluded cadence: NaN, as above) and
// their times t; nothing is stored, and the moments and the factorisation of a fit live in registers.

// a window value beside its time: what the selection functions above see when they select among residuals
struct Sample {
  double v, t;
};

template <class PV, class PT>
struct Samples {
  PV v;
  PT t;
  EXO_DET_HD Sample operator[](int j) const { return Sample{v[j], t[j]}; }
};

// the polynomial of a fit in x = (t - t0) * inv_span, by Horner
template <int P>
struct Poly {
  double c[P + 1];
  double t0, inv_span;
  EXO_DET_HD double abscissa(double t) const { return (t - t0) * inv_span; }
  EXO_DET_HD double at(double x) const {
    double r = c[P];
    for (int k = P - 1; k >= 0; --k) r = r * x + c[k];
    return r;
  }
};

// |v - P_c(x)|: the residuals whose median rescales a fit (an excluded cadence: NaN, which no comparison counts)
template <int P>
struct AbsResidual {
  Poly<P> poly;
  EXO_DET_HD double operator()(Sample s) const { return fabs(s.v - poly.at(poly.abscissa(s.t))); }
};

constexpr double kPivotFloor = 1e-10;  // a pivot <= kPivotFloor * M_0 stops a stage

// the number of distinct times among the participating cadences of a window on a non-decreasing axis: an exact count
template <class PV, class PT>
EXO_DET_HD int count_distinct_times(PV v, PT t, int len) {
  int n = 0;
  double prev = NAN;
  EXO_DET_UNROLL
  for (int j = 0; j < len; ++j) {
    const double vj = v[j], tj = t[j];
    const bool in = vj == vj;
    n += (in && tj != prev) ? 1 : 0;
    prev = in ? tj : prev;
  }
  return n;
}

// One stage: exactly n_iter steps c += M^-1 b from the coefficients in `poly`, with M_k = sum w x^k, b_k = sum w x^k d,
// d = v - P_c(x), u = d / (cval scale), w = (1 - u^2)^2 inside |u| < 1; sums in the window's order.  M, the Hankel matrix
// M_{a+b}, is factored as L D L^T (the Cholesky factorisation without its square roots) in the order written below.  false:
// the stage stopped -- M_0 == 0 or a pivot <= kPivotFloor * M_0 -- and c is what the last completed step left.
template <int P, class PV, class PT>
EXO_DET_HD bool trend_stage(PV v, PT t, int len, Poly<P>& poly, double scale, double cval, int n_iter) {
  const double r = 1.0 / (cval * scale);
  for (int it = 0; it < n_iter; ++it) {
    double M[2 * P + 1], b[P + 1];
    for (int k = 0; k <= 2 * P; ++k) M[k] = 0.0;
    for (int k = 0; k <= P; ++k) b[k] = 0.0;
    EXO_DET_UNROLL
    for (int j = 0; j < len; ++j) {
      const double vj = v[j], tj = t[j];
      const double x = poly.abscissa(tj);
      const double d = vj - poly.at(x);
      const double u = d * r;
      if (fabs(u) < 1.0) {
        const double q = 1.0 - u * u;
        double wk = q * q;
        for (int k = 0; k <= 2 * P; ++k) {
          M[k] += wk;
          if (k <= P) b[k] += d * wk;
          wk = wk * x;
        }
      }
    }
    if (M[0] == 0.0) return false;
    const double floor_ = kPivotFloor * M[0];
    if constexpr (P == 0) {
      poly.c[0] += b[0] / M[0];
    } else if constexpr (P == 1) {
      const double l10 = M[1] / M[0];
      const double d1 = M[2] - l10 * M[1];
      if (d1 <= floor_) return false;
      const double a1 = (b[1] - l10 * b[0]) / d1;
      poly.c[0] += b[0] / M[0] - l10 * a1;
      poly.c[1] += a1;
    } else {
      const double l10 = M[1] / M[0], l20 = M[2] / M[0];
      const double d1 = M[2] - l10 * M[1];
      if (d1 <= floor_) return false;
      const double e = M[3] - l20 * M[1];
      const double l21 = e / d1;
      const double d2 = (M[4] - l20 * M[2]) - l21 * e;
      if (d2 <= floor_) return false;
      const double z1 = b[1] - l10 * b[0];
      const double z2 = (b[2] - l20 * b[0]) - l21 * z1;
      const double a2 = z2 / d2;
      const double a1 = z1 / d1 - l21 * a2;
      poly.c[0] += (b[0] / M[0] - l10 * a1) - l20 * a2;
      poly.c[1] += a1;
      poly.c[2] += a2;
    }
  }
  return true;
}

// the fit of effective order P from the median and the MAD (> 0): the stage, then `rescale` times the median of the
// absolute residuals as the new scale and another stage.  *scale: the scale of the last stage run.
template <int P, class PV, class PT>
EXO_DET_HD double trend_fit(PV v, PT t, int len, int m, double med, double t0, double inv_span, double cval, int n_iter, int rescale,
                            double* scale) {
  Poly<P> poly;
  poly.c[0] = med;
  for (int k = 1; k <= P; ++k) poly.c[k] = 0.0;
  poly.t0 = t0;
  poly.inv_span = inv_span;
  bool ran = trend_stage<P>(v, t, len, poly, *scale, cval, n_iter);
  for (int pass = 0; pass < rescale && ran; ++pass) {
    const double s = median_of(Samples<PV, PT>{v, t}, len, m, AbsResidual<P>{poly}, 62);
    if (s == 0.0) break;
    *scale = s;
    ran = trend_stage<P>(v, t, len, poly, s, cval, n_iter);
  }
  return poly.c[0];
}

// The trend of one window at the time t0 of its cadence, t[0] <= t0 <= t[len - 1], and the last scale used; no participating
// cadence: NaN and NaN.  ORDER = 1 or 2; the effective order is min(ORDER, number of distinct times - 1).
template <int ORDER, class PV, class PT>
EXO_DET_HD double window_trend(PV v, PT t, int len, double t0, double cval, int n_iter, int rescale, double* scale) {
  const int m = count_valid(v, len);
  if (m == 0) {
    *scale = NAN;
    return NAN;
  }
  const double med = median(v, len, m);
  *scale = mad(v, len, m, med);
  if (*scale == 0.0) return med;
  const double first = t[0], last = t[len - 1];
  const double span = fmax(last - t0, t0 - first);
  if (span == 0.0) return med;
  const double inv_span = 1.0 / span;
  const int distinct = count_distinct_times(v, t, len);
  const int p = distinct - 1 < ORDER ? distinct - 1 : ORDER;
  if constexpr (ORDER >= 2)
    if (p == 2) return trend_fit<2>(v, t, len, m, med, t0, inv_span, cval, n_iter, rescale, scale);
  if (p >= 1) return trend_fit<1>(v, t, len, m, med, t0, inv_span, cval, n_iter, rescale, scale);
  return trend_fit<0>(v, t, len, m, med, t0, inv_span, cval, n_iter, rescale, scale);
}

// ---- the windows -----------------------------------------------------------------------------------------------------------

// first j in [s, i] with t[j] >= bound (t non-decreasing there, t[i] >= bound)
EXO_DET_HD int64_t window_lo(const double* t, int64_t s, int64_t i, double bound) {
  int64_t a = s, b = i;  // the answer lies in [a, b]
  while (a < b) {
    const int64_t mid = a + (b - a) / 2;
    if (t[mid] >= bound) b = mid; else a = mid + 1;
  }
  return a;
}

// last j in [i, e] with t[j] <= bound (t[i] <= bound)
EXO_DET_HD int64_t window_hi(const double* t, int64_t i, int64_t e, double bound) {
  int64_t a = i, b = e;
  while (a < b) {
    const int64_t mid = a + (b - a + 1) / 2;
    if (t[mid] <= bound) a = mid; else b = mid - 1;
  }
  return a;
}

}  // namespace detrend
