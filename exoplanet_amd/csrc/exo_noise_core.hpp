// exo_noise_core.hpp -- the data side of the white-noise likelihood with a sampled mean and a jitter added in
// quadrature (exo_white_noise_terms_f64; definitions: DESIGN.md section 11).  For draw d and cadence n, with
// v_n = yerr_n^2, s2_d = jitter_d^2, w = 1 / (v_n + s2_d), r = y_n - mean_d:
//     Q = sum w r^2,   Lam = sum log(v_n + s2_d),   G = sum w r,   H = sum w^2 r^2,   A = sum w
// over ALL cadences.  Two forms: (a) from per-series sums, O(1) per draw, when the weight separates into a per-cadence
// and a per-draw factor (one variance for the whole series, or no jitter); (b) element by element otherwise.  Compiles for
// the device (exo_noise.hip) and, with EXO_HOST_BUILD, for the host (tests/noise_harness.cpp holds it to a long-double
// evaluation of the definitions without a GPU).
#pragma once
#include <math.h>
#include <stdint.h>

#include "exo_math.hpp"

#ifdef EXO_HOST_BUILD
#define EXO_NZ_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_NZ_HD __device__ __forceinline__
#endif

namespace nz {

constexpr int kQ = 0, kLam = 1, kG = 2, kH = 3, kA = 4, kTerms = 5;
// a running product of mantissas is brought back to [0.5, 1) at least this often: every factor is >= 0.5, so the product
// stays above 2^-512, far from the subnormals
constexpr int kRenorm = 512;

// 1 / x: hardware seed (2^-24) and two Newton steps, as exo::fast_rcp; the host takes the division
EXO_NZ_HD double rcp(double x) {
#ifdef EXO_HOST_BUILD
  return 1.0 / x;
#else
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
#endif
}

// ---- (a) per-series sums --------------------------------------------------------------------------------------------------
// With u_n = 1 (one variance) or 1 / v_n (per-cadence variances, no jitter) and y' = y - ybar, ybar the u-weighted mean:
//     S0 = sum u, S1 = sum u y', S2 = sum u y'^2, T0 = sum u^2, T1 = sum u^2 y', T2 = sum u^2 y'^2, SL = sum log v_n
// Centring makes S1 vanish up to rounding, so Q = S2 - 2 delta S1 + S0 delta^2 (delta = mean - ybar) is a sum of two
// non-negative terms and a correction of rounding size; on the raw series (y ~ 1, residuals ~ 1e-4) the same expansion
// cancels eight digits.
constexpr int kSeries = 8;   // ybar, S0, S1, S2, T0, T1, T2, SL
struct Series {
  double ybar, S0, S1, S2, T0, T1, T2, SL;
};

struct Pass1 {   // sum u, sum u y
  double u, uy;
};
EXO_NZ_HD void pass1_add(Pass1& a, double y, double u) {
  a.u += u;
  a.uy = fma(u, y, a.uy);
}
struct Pass2 {
  double S1, S2, T0, T1, T2;
};
EXO_NZ_HD void pass2_add(Pass2& a, double y, double u, double ybar) {
  const double yc = y - ybar, uy = u * yc, uu = u * u;
  a.S1 += uy;
  a.S2 = fma(uy, yc, a.S2);
  a.T0 += uu;
  a.T1 = fma(uu, yc, a.T1);
  a.T2 = fma(uu * yc, yc, a.T2);
}

// the five terms of one draw from the series sums.  one_var: the series has ONE variance v0 (then u = 1 and the draw's
// weight is 1 / (v0 + s2)); otherwise per-cadence variances without jitter (u = 1 / v_n, s2 = 0)
EXO_NZ_HD void from_series(const Series& s, bool one_var, double v0, double n_cad, double mean, double s2, double* out) {
  const double delta = mean - s.ybar;
  const double q = fma(s.S0 * delta, delta, fma(-2.0 * delta, s.S1, s.S2));   // sum u r^2
  const double g = fma(-s.S0, delta, s.S1);                                    // sum u r
  if (one_var) {
    const double x = v0 + s2, w = rcp(x);
    out[kQ] = w * q;
    out[kLam] = n_cad * log(x);
    out[kG] = w * g;
    out[kH] = w * w * q;
    out[kA] = w * s.S0;
  } else {
    out[kQ] = q;
    out[kLam] = s.SL;
    out[kG] = g;
    out[kH] = fma(s.T0 * delta, delta, fma(-2.0 * delta, s.T1, s.T2));
    out[kA] = s.S0;
  }
}

// ---- sum of logarithms as the logarithm of a product ---------------------------------------------------------------------
// x = m 2^e with m in [0.5, 1): the mantissas are multiplied, the exponents added, and ONE logarithm is taken at the end.
// Each factor costs one rounding of the product (1.1e-16 of log scale), where a separate logarithm costs |log x| x 1.1e-16:
// for variances of 1e-8 (|log| = 18) the product is the more accurate form as well as the cheaper one (measured on the host:
// DESIGN.md 11.3).  The caller renormalises every kRenorm factors at the latest.
struct LogProd {
  double m;
  int e;
};
EXO_NZ_HD LogProd logprod_one() { return LogProd{1.0, 0}; }
EXO_NZ_HD void logprod_mul(LogProd& p, double x) {
  int e;
  p.m *= frexp(x, &e);
  p.e += e;
}
EXO_NZ_HD void logprod_renorm(LogProd& p) {
  int e;
  p.m = frexp(p.m, &e);
  p.e += e;
}
EXO_NZ_HD double logprod_value(const LogProd& p) { return fma((double)p.e, exo::kLn2, log(p.m)); }

// ---- (b) element by element -----------------------------------------------------------------------------------------------
struct Acc {
  double Q, G, H, A;
  LogProd lam;
};
EXO_NZ_HD Acc acc_zero() { return Acc{0.0, 0.0, 0.0, 0.0, logprod_one()}; }
// one (draw, cadence) element: a reciprocal, a mantissa split and six multiply-adds
EXO_NZ_HD void acc_add(Acc& a, double y, double v, double mean, double s2) {
  const double x = v + s2, w = rcp(x), r = y - mean, wr = w * r;
  a.Q = fma(wr, r, a.Q);
  a.G += wr;
  a.H = fma(wr, wr, a.H);
  a.A += w;
  logprod_mul(a.lam, x);
}

}  // namespace nz
