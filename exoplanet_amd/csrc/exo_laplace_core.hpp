// exo_laplace_core.hpp -- the arithmetic of the Laplace approximation at a posterior mode (exoplanet_amd/laplace.py;
// exo_laplace_points_f64, exo_laplace_factor_f64): the points of a central-difference stencil around a chain's position, and
// from the gradients there the Hessian of f = -logp, its scaled Cholesky factor, the covariance H^-1 and the Laplace
// log-evidence.  Definition: DESIGN.md section 28 and tests/laplace_oracle.py.  Compiles for the device (exo_laplace.hip)
// and, with EXO_HOST_BUILD, for the host (tests/laplace_harness.cpp checks it against the long-double numpy statement without a
// GPU).
//
// Every sum has ONE order, stated at the function, and no product is contracted into a fused multiply-add (both builds are
// compiled with -ffp-contract=off), so the kernels and the host build give the same bits.  The only library functions are
// sqrt, fabs, frexp and isfinite, which are exact or correctly rounded on both sides; the logarithm of the determinant is
// written out here (log_fixed), because a library's log is neither.
#pragma once
#include <math.h>
#include <stdint.h>

#include "exo_metric_core.hpp"

namespace laplace {

using metric::cholesky_entry;
using metric::kMaxN;
using metric::Packed;
using metric::packed_size;

constexpr int kOk = 0, kNotFinite = 1, kNotPositive = 2;   // EXO_LAPLACE_STATUS_*
constexpr double kEps = 2.220446049250313e-16;             // DBL_EPSILON
constexpr double kCbrtEps = 6.0554544523933395e-06;        // DBL_EPSILON^(1/3): the pilot step of a central difference
constexpr double kLog2Pi = 1.8378770664093453;             // log(2 pi)
constexpr double kLn2Hi = 6.93147180369123816490e-01;      // log(2) in two parts, the first with 21 trailing zero bits:
constexpr double kLn2Lo = 1.90821492927058770002e-10;      // e * kLn2Hi is exact for every binary exponent e

// ---- the stencil ---------------------------------------------------------------------------------------------------------------
// the step of one free coordinate: the pilot step eps^(1/3) * scale (scale: the caller's, or max(|x|, 1) where it gives none);
// with the previous pass's H_kk finite and positive, delta / sqrt(H_kk) where that is finite and positive
EXO_MET_HD double step(double x, bool has_scale, double scale, bool has_hess, double hkk, double delta) {
  const double pilot = kCbrtEps * (has_scale ? scale : (fabs(x) > 1.0 ? fabs(x) : 1.0));
  if (!has_hess || !isfinite(hkk) || !(hkk > 0.0)) return pilot;
  const double h = delta / sqrt(hkk);
  return isfinite(h) && h > 0.0 ? h : pilot;
}

// the intended offset of stencil set s: +h, -h, +2h, -2h
EXO_MET_HD double offset(int s, double h) { return s == 0 ? h : s == 1 ? -h : s == 2 ? 2.0 * h : -2.0 * h; }

// ---- the Hessian ---------------------------------------------------------------------------------------------------------------
// one raw entry: the difference of dlogp / dx_i between the + and the - point of coordinate k over the REALISED distance
EXO_MET_HD double raw_entry(double g_plus, double g_minus, double dx_plus, double dx_minus) {
  return -(g_plus - g_minus) / (dx_plus - dx_minus);
}

// Richardson's combination of the h and the 2h difference
EXO_MET_HD double richardson(double a1, double a2) { return (4.0 * a1 - a2) / 3.0; }

EXO_MET_HD double symmetrise(double a_ik, double a_ki) { return 0.5 * (a_ik + a_ki); }

// |v| in units of the entry's scale sqrt(|H_ii H_kk|)
EXO_MET_HD double scaled_abs(double v, double hii, double hkk) { return fabs(v) / sqrt(fabs(hii * hkk)); }

// a running maximum that a NaN does not enter
EXO_MET_HD double max_of(double acc, double v) { return v > acc ? v : acc; }

// ---- the factor and the covariance ---------------------------------------------------------------------------------------------
EXO_MET_HD double inv_sqrt(double h) { return 1.0 / sqrt(h); }

// C_ik = (s_i H_ik) s_k off the diagonal; the diagonal is exactly 1
EXO_MET_HD double scaled_entry(double si, double h, double sk, bool diagonal) { return diagonal ? 1.0 : si * h * sk; }

// a pivot of the unit-diagonal C at or below m eps is the rounding of its m subtractions of products bounded by 1
EXO_MET_HD bool pivot_ok(double pivot, int m) { return pivot > (double)m * kEps; }

// entry (i, k), k <= i, of T = R^-1 from the entries above it in column k: 1 / R_kk on the diagonal, below it
// (((-R_ik T_kk) - R_i,k+1 T_k+1,k) - ...) / R_ii, j ascending
template <class TR, class TT>
EXO_MET_HD double inverse_entry(const TR& R, const TT& T, int i, int k) {
  if (i == k) return 1.0 / R(k, k);
  double acc = -(R(i, k) * T(k, k));
  for (int j = k + 1; j < i; ++j) acc -= R(i, j) * T(j, k);
  return acc / R(i, i);
}

// (C^-1)_ik = T_ii T_ik + T_i+1,i T_i+1,k + ..., l ascending from i (k <= i)
template <class TT>
EXO_MET_HD double gram_entry(const TT& T, int m, int i, int k) {
  double acc = T(i, i) * T(i, k);
  for (int l = i + 1; l < m; ++l) acc += T(l, i) * T(l, k);
  return acc;
}

EXO_MET_HD double cov_entry(double si, double sk, double cinv) { return si * sk * cinv; }

// ---- the logarithm, written out ------------------------------------------------------------------------------------------------
// log(x) of a finite x > 0 from IEEE operations alone: x = 2^e f, f in [sqrt(1/2), sqrt(2)); with s = (f - 1) / (f + 1) (f - 1
// is exact), log f = 2 s (1 + s^2 / 3 + s^4 / 5 + ... + s^24 / 25) by Horner's rule -- s^2 <= 0.0295, the first term left out is
// below 1e-20 --; log x = e ln2_hi + (log f + e ln2_lo).  Two or three roundings of log f, one of the sum.
EXO_MET_HD double log_fixed(double x) {
  int e;
  double f = frexp(x, &e);                               // f in [0.5, 1)
  if (f < 0.70710678118654752) {
    f = 2.0 * f;
    e -= 1;
  }
  const double s = (f - 1.0) / (f + 1.0), z = s * s;
  double p = 1.0 / 25.0;
  for (int k = 23; k >= 3; k -= 2) p = p * z + 1.0 / (double)k;
  const double logf = 2.0 * s * (p * z + 1.0);
  return (double)e * kLn2Hi + (logf + (double)e * kLn2Lo);
}

// log det H = (log H_00 + log H_11 + ...) + 2 (log R_00 + log R_11 + ...), each sum i ascending
template <class TR>
EXO_MET_HD double log_det(const double* hdiag, const TR& R, int m) {
  double a = log_fixed(hdiag[0]), b = log_fixed(R(0, 0));
  for (int i = 1; i < m; ++i) {
    a += log_fixed(hdiag[i]);
    b += log_fixed(R(i, i));
  }
  return a + 2.0 * b;
}

// the Laplace log-evidence: (logp + (m / 2) log(2 pi)) - logdet / 2
EXO_MET_HD double log_evidence(double logp, int m, double logdet) { return (logp + 0.5 * (double)m * kLog2Pi) - 0.5 * logdet; }

}  // namespace laplace
