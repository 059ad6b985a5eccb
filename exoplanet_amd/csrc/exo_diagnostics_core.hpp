// exo_diagnostics_core.hpp -- the arithmetic of the rank-normalised split diagnostics of Vehtari, Gelman, Simpson, Carpenter &
// Buerkner (2021) (exoplanet_amd/diagnostics.py -- the torch statement there is the definition): the
// normal score of an average rank, the quantiles of a sorted array, the autocorrelation of a lag from its sum, Geyer's
// truncation as a state that is advanced one block of lags at a time, the monotone sequence and the effective sample size.
// Compiled for the device (exo_diagnostics.hip) and for the host (tests/diagnostics_harness.cpp, with EXO_HOST_BUILD),
// templated on the scalar type: the host build runs in double and in long double.
//
// Both builds compile with contraction off and form every sum in the same order -- a half-chain's sums over its draws in
// turn, the sums over half-chains in the order of `wave_order_sum` -- so the double build on the host and the kernels do
// the same IEEE operations; they differ by the library functions behind `z_of_rank` and the square roots only.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_DIAG_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_DIAG_HD __device__ __forceinline__
#endif

namespace diag {

constexpr int kLagBlock = 16;   // lags per pass of the autocovariance kernel (EXO_DIAG_LAG_BLOCK): even, a pair never straddles
constexpr int kSets = 5;        // series sets of a parameter
enum Set : int { kZ = 0, kZFold = 1, kLow = 2, kHigh = 3, kRaw = 4 };
constexpr int kWave = 64;
// per-set state carried between lag blocks (doubles)
enum State : int { sW = 0, sVarPlus = 1, sRhat = 2, sRe = 3, sRo = 4, sT = 5, sEss = 6, sMaxT = 7, kState = 8 };
// per-parameter moments written by the preparation (doubles)
enum Moment : int { mMean = 0, mSd = 1, mQ05 = 2, mQ50 = 3, mQ95 = 4, mBad = 5, mConst = 6, mPivot = 7, kMoments = 8 };
// per-parameter results (doubles; the max_t as whole numbers)
enum Out : int { oMean = 0, oSd, oQ05, oQ50, oQ95, oMcse, oEssBulk, oEssTail, oEssMean, oRhat, oMaxTBulk, oMaxTLow, oMaxTHigh,
                 oMaxTMean, oRhatZ, oRhatFold, kOut };

EXO_DIAG_HD double erfc_of(double v) { return erfc(v); }
EXO_DIAG_HD double exp_of(double v) { return exp(v); }
EXO_DIAG_HD double log_of(double v) { return log(v); }
EXO_DIAG_HD double sqrt_of(double v) { return sqrt(v); }
EXO_DIAG_HD double log10_of(double v) { return log10(v); }
#ifdef EXO_HOST_BUILD
inline long double erfc_of(long double v) { return erfcl(v); }
inline long double exp_of(long double v) { return expl(v); }
inline long double log_of(long double v) { return logl(v); }
inline long double sqrt_of(long double v) { return sqrtl(v); }
inline long double log10_of(long double v) { return log10l(v); }
#endif

template <typename T>
EXO_DIAG_HD bool finite(T v) { return v - v == T(0); }          // (inf - inf and NaN - NaN are NaN)

// Phi^-1(p) for 0 < p <= 1/2 (a value <= 0): Wichura's AS 241 (PPND16), then Halley steps against erfc -- Phi(z) =
// erfc(-z / sqrt 2) / 2 has full relative accuracy in the lower tail, which is why the upper half goes through 1 - p
template <typename T>
EXO_DIAG_HD T ndtri_lower(T p) {
  const T q = p - T(0.5);
  T z;
  if (q >= T(-0.425)) {
    const T r = T(0.180625) - q * q;
    z = q * (((((((T(2.5090809287301226727e3) * r + T(3.3430575583588128105e4)) * r + T(6.7265770927008700853e4)) * r +
                 T(4.5921953931549871457e4)) * r + T(1.3731693765509461125e4)) * r + T(1.9715909503065514427e3)) * r +
               T(1.3314166789178437745e2)) * r + T(3.3871328727963666080)) /
        (((((((T(5.2264952788528545610e3) * r + T(2.8729085735721942674e4)) * r + T(3.9307895800092710610e4)) * r +
             T(2.1213794301586595867e4)) * r + T(5.3941960214247511077e3)) * r + T(6.8718700749205790830e2)) * r +
          T(4.2313330701600911252e1)) * r + T(1));
  } else {
    T r = sqrt_of(-log_of(p));
    if (r <= T(5)) {
      r -= T(1.6);
      z = (((((((T(7.74545014278341407640e-4) * r + T(2.27238449892691845833e-2)) * r + T(2.41780725177450611770e-1)) * r +
              T(1.27045825245236838258)) * r + T(3.64784832476320460504)) * r + T(5.76949722146069140550)) * r +
            T(4.63033784615654529590)) * r + T(1.42343711074968357734)) /
          (((((((T(1.05075007164441684324e-9) * r + T(5.47593808499534494600e-4)) * r + T(1.51986665636164571966e-2)) * r +
               T(1.48103976427480074590e-1)) * r + T(6.89767334985100004550e-1)) * r + T(1.67638483018380384940)) * r +
            T(2.05319162663775882187)) * r + T(1));
    } else {
      r -= T(5);
      z = (((((((T(2.01033439929228813265e-7) * r + T(2.71155556874348757815e-5)) * r + T(1.24266094738807843860e-3)) * r +
              T(2.65321895265761230930e-2)) * r + T(2.96560571828504891230e-1)) * r + T(1.78482653991729133580)) * r +
            T(5.46378491116411436990)) * r + T(6.65790464350110377720)) /
          (((((((T(2.04426310338993978564e-15) * r + T(1.42151175831644588870e-7)) * r + T(1.84631831751005468180e-5)) * r +
               T(7.86869131145613259100e-4)) * r + T(1.48753612908506148525e-2)) * r + T(1.36929880922735805310e-1)) * r +
            T(5.99832206555887937690e-1)) * r + T(1));
    }
    z = -z;
  }
  const T kInvSqrt2 = T(0.70710678118654752440084436210484903928L), kSqrt2Pi = T(2.50662827463100050241576528481104525L);
  const int steps = sizeof(T) > 8 ? 2 : 1;
  for (int k = 0; k < steps; ++k) {
    const T e = T(0.5) * erfc_of(-z * kInvSqrt2) - p;
    const T u = e * kSqrt2Pi * exp_of(T(0.5) * z * z);
    z = z - u / (T(1) + T(0.5) * z * u);
  }
  return z;
}

// the normal score of an average rank among S values; `rank2` is twice the rank (ties: a whole number all the same):
// p = (r - 3/8) / (S + 1/4) = (4 rank2 - 3) / (8 S + 2), formed from whole numbers on the side of its tail
template <typename T>
EXO_DIAG_HD T z_of_rank(int64_t rank2, int64_t S) {
  const int64_t num = 4 * rank2 - 3, den = 8 * S + 2;
  if (2 * num <= den) return ndtri_lower(T(num) / T(den));
  return -ndtri_lower(T(den - num) / T(den));
}

// twice the average rank (1-based) of sorted[i] among sorted[0 .. S): the ends of its run of equal values by bisection
EXO_DIAG_HD int64_t rank2_of(const double* sorted, int64_t S, int64_t i) {
  const double v = sorted[i];
  int64_t lo = 0, hi = i;                       // first index of the run: in [0, i]
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (sorted[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  const int64_t first = lo;
  lo = i;
  hi = S - 1;                                   // last index of the run: in [i, S - 1]
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (sorted[mid] > v) hi = mid - 1;
    else lo = mid;
  }
  return first + lo + 2;
}

// the `percent` / 100 quantile of sorted[0 .. n) by linear interpolation between order statistics (numpy.quantile's default)
template <typename T>
EXO_DIAG_HD T quantile_sorted(const double* sorted, int64_t n, int percent) {
  const int64_t num = (n - 1) * percent, lo = num / 100;
  const T frac = T(num % 100) / T(100), a = T(sorted[lo]);
  if (lo + 1 >= n || num % 100 == 0) return a;
  return a + frac * (T(sorted[lo + 1]) - a);
}

// |v - median| of sorted[0 .. n), written through the two middle order statistics a <= b as |(v - a) + (v - b)| / 2: for an
// even n, a and b themselves are tied at (b - a) / 2 in exact arithmetic, and in this form they are tied in every precision
// (a rounded median would break the tie one way or the other)
template <typename T>
EXO_DIAG_HD T folded_of(T v, const double* sorted, int64_t n) {
  const T f = ((v - T(sorted[(n - 1) / 2])) + (v - T(sorted[n / 2]))) / T(2);
  return f < T(0) ? -f : f;
}

#ifdef EXO_HOST_BUILD
// sum of v[0 .. n) in the order of the kernels: groups of 64 by the halving tree of a wave reduction, the groups in turn
template <typename T>
inline T wave_order_sum(const T* v, int64_t n) {
  T total = T(0);
  for (int64_t g = 0; g < n; g += kWave) {
    T a[kWave];
    for (int i = 0; i < kWave; ++i) a[i] = g + i < n ? v[g + i] : T(0);
    for (int off = kWave / 2; off > 0; off >>= 1)
      for (int i = 0; i < off; ++i) a[i] = a[i] + a[i + off];
    total = g == 0 ? a[0] : total + a[0];
  }
  return total;
}
#endif

// what a set's first block fixes.  sum0: sum over half-chains of sum_n d^2; means [M]: the half-chains' means
template <typename T>
EXO_DIAG_HD void begin_set(T sum0, const T* means, int64_t M, int64_t L, T* st) {
  const T a0 = sum0 / T(L) / T(M);
  const T W = a0 * T(L) / T(L - 1);
  T mm = T(0);
  for (int64_t m = 0; m < M; ++m) mm = mm + means[m];
  mm = mm / T(M);
  T vb = T(0);
  for (int64_t m = 0; m < M; ++m) vb = vb + (means[m] - mm) * (means[m] - mm);
  vb = M > 1 ? vb / T(M - 1) : T(0);
  const T var_plus = W * T(L - 1) / T(L) + vb;
  st[sW] = W;
  st[sVarPlus] = var_plus;
  st[sRhat] = sqrt_of(var_plus / W);            // ((L - 1) / L W + B / L) / W, with B / L the variance of the means
  st[sRe] = T(1);
  st[sRo] = T(0);
  st[sT] = T(1);
  st[sEss] = T(0);
  st[sMaxT] = T(-1);
}

template <typename T>
EXO_DIAG_HD T rho_of(T lag_sum, int64_t M, int64_t L, const T* st) {
  const T abar = lag_sum / T(L) / T(M);
  return T(1) - (st[sW] - abar) / st[sVarPlus];
}

// the initial monotone sequence on rho[0 .. max_t], tau with its floor, the effective sample size
template <typename T>
EXO_DIAG_HD T finish_set(T* rho, int64_t max_t, T re, int64_t M, int64_t L) {
  for (int64_t t = 1; t <= max_t - 2; t += 2)
    if (rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]) {
      rho[t + 1] = (rho[t - 1] + rho[t]) / T(2);
      rho[t + 2] = rho[t + 1];
    }
  T sum = T(0);
  for (int64_t t = 0; t <= max_t; ++t) sum = sum + rho[t];
  T tau = T(-1) + T(2) * sum + (re > T(0) ? re : T(0));
  const T S = T(M * L), floor_tau = T(1) / log10_of(S);
  if (!(tau >= floor_tau)) tau = tau == tau ? floor_tau : tau;
  return S / tau;
}

// Geyer's initial positive sequence, advanced over the lags below `n_lag` (a whole number of blocks; rho[0 .. n_lag) are in
// place, rho[0] = 1): pairs (rho[t + 1], rho[t + 2]) are taken while their sum is positive and t < L - 3.  Returns true when
// the set is finished (st[sEss], st[sMaxT] written), false when it needs the next block.
template <typename T>
EXO_DIAG_HD bool advance_set(T* rho, int64_t n_lag, int64_t M, int64_t L, T* st) {
  int64_t t = (int64_t)st[sT];
  T re = st[sRe], ro = st[sRo];
  for (;;) {
    if (!(t < L - 3 && re + ro > T(0))) {
      const int64_t max_t = t - 2;
      st[sMaxT] = T(max_t);
      // (no variance at all -- an indicator that is the same everywhere: every draw counts, as for a constant series)
      st[sEss] = st[sVarPlus] == T(0) ? T(M * L) : finish_set(rho, max_t, re, M, L);
      return true;
    }
    if (t + 2 >= n_lag) break;
    re = rho[t + 1];
    ro = rho[t + 2];
    t += 2;
  }
  st[sT] = T(t);
  st[sRe] = re;
  st[sRo] = ro;
  return false;
}

// one parameter's results from its sets' states and its moments
template <typename T>
EXO_DIAG_HD void assemble(const T* st /* [kSets][kState] */, const T* mom, int64_t M, int64_t L, T* out) {
  const T nan = T(NAN);
  const bool bad = mom[mBad] != T(0), constant = mom[mConst] != T(0);
  for (int k = 0; k < kOut; ++k) out[k] = nan;
  out[oMaxTBulk] = out[oMaxTLow] = out[oMaxTHigh] = out[oMaxTMean] = T(-1);
  if (bad) return;
  out[oMean] = mom[mMean]; out[oSd] = mom[mSd]; out[oQ05] = mom[mQ05]; out[oQ50] = mom[mQ50]; out[oQ95] = mom[mQ95];
  if (constant) {                               // no autocorrelation to speak of: every draw counts, R-hat has no scale
    out[oEssBulk] = out[oEssTail] = out[oEssMean] = T(M * L);
    out[oMcse] = mom[mSd] / sqrt_of(T(M * L));
    return;
  }
  const T lo = st[kLow * kState + sEss], hi = st[kHigh * kState + sEss];
  out[oEssBulk] = st[kZ * kState + sEss];
  out[oEssTail] = lo == lo && hi == hi ? (lo < hi ? lo : hi) : nan;
  out[oEssMean] = st[kRaw * kState + sEss];
  out[oMcse] = mom[mSd] / sqrt_of(out[oEssMean]);
  const T rz = st[kZ * kState + sRhat], rf = st[kZFold * kState + sRhat];
  out[oRhatZ] = rz; out[oRhatFold] = rf;
  out[oRhat] = rz == rz && rf == rf ? (rz > rf ? rz : rf) : nan;
  out[oMaxTBulk] = st[kZ * kState + sMaxT]; out[oMaxTLow] = st[kLow * kState + sMaxT];
  out[oMaxTHigh] = st[kHigh * kState + sMaxT]; out[oMaxTMean] = st[kRaw * kState + sMaxT];
}

}  // namespace diag
