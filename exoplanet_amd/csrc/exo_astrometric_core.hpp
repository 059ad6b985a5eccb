// exo_astrometric_core.hpp -- the per-candidate arithmetic of the astrometric orbit search on the Thiele-Innes constants
// (exoplanet_amd/estimators.py: astrometric_power, astrometric_estimator): one epoch's orbital-plane coordinates (xi, eta),
// its contribution to the thirteen sums of a candidate's normal equations, the scaled Cholesky solve of the 4 x 4 system with
// its pivot floor, and the conversion of the four constants to a_angular, incl, omega, Omega.  Definition: DESIGN.md section
// 23.  Compiles for the device (exo_astrometric.hip) and, with EXO_HOST_BUILD, for the host (tests/astrometric_harness.cpp
// checks it against the numpy statement without a GPU).  Every product that is meant to be fused is written as an fma: both
// builds are compiled with -ffp-contract=off.  The candidates, their numbering and the arg-max: exo_orbit_search.hpp.
#pragma once
#include <math.h>

#include "exo_estimators_core.hpp"
#include "exo_math.hpp"
#include "exo_orbit_search.hpp"

namespace ast {

// a candidate whose scaled normal matrix has a squared Cholesky pivot below this is none at that frequency: a cap on the
// condition number, and part of the definition
constexpr double kPivotFloor = 1e-12;
constexpr double kPi = 3.141592653589793;

// xi = cos E - e and eta = sqrt(1 - e^2) sin E of one epoch: the position in the orbital plane in units of the semi-major
// axis.  `turns` = ls_phase_turns(f, t - t_min); the phase of periastron comes off in turns, and only then the factor 2 pi.
// Both are the half-angle forms of exo_math.hpp: no reciprocal, no rounded cos E.  se = sqrt(1 - e), pe = sqrt(1 + e).
EXO_EST_HD void orbit_plane(double turns, double phi, double e, double se, double pe, double* xi, double* eta) {
  const exo::KeplerHalf kh = exo::kepler_half(orb::kTwoPi * (turns - phi), e, se, pe);
  *xi = fma(kh.X, kh.X, -(kh.Y * kh.Y));
  *eta = 2.0 * kh.X * kh.Y;
}

// The thirteen sums of a candidate over the epochs.  With the precision matrix P = [[pxx, pxy], [pxy, pyy]] of an epoch and
// q = P (x, y):  sum xi^2 P, sum xi eta P, sum eta^2 P (three numbers each: xx, xy, yy) and sum xi q, sum eta q (two each).
struct Sums {
  double xx0, xx1, xx2, xe0, xe1, xe2, ee0, ee1, ee2, bx0, bx1, be0, be1;
};
EXO_EST_HD Sums sums_init() { return Sums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// one epoch into the sums
EXO_EST_HD void accumulate(Sums& a, double xi, double eta, double pxx, double pxy, double pyy, double qx, double qy) {
  const double xx = xi * xi, xe = xi * eta, ee = eta * eta;
  a.xx0 = fma(xx, pxx, a.xx0);
  a.xx1 = fma(xx, pxy, a.xx1);
  a.xx2 = fma(xx, pyy, a.xx2);
  a.xe0 = fma(xe, pxx, a.xe0);
  a.xe1 = fma(xe, pxy, a.xe1);
  a.xe2 = fma(xe, pyy, a.xe2);
  a.ee0 = fma(ee, pxx, a.ee0);
  a.ee1 = fma(ee, pxy, a.ee1);
  a.ee2 = fma(ee, pyy, a.ee2);
  a.bx0 = fma(xi, qx, a.bx0);
  a.bx1 = fma(xi, qy, a.bx1);
  a.be0 = fma(eta, qx, a.be0);
  a.be1 = fma(eta, qy, a.be1);
}

// The fit of  X = TA xi + TF eta,  Y = TB xi + TG eta:  N beta = b with beta = (TA, TB, TF, TG),
//   N = [[Sxx, Sxe], [Sxe, See]] (each block 2 x 2),  b = (bx, be).
// N is scaled by d = sqrt(diag N) to a unit diagonal and factored by an unpivoted Cholesky; `pivot` is the smallest squared
// pivot (the first is 1).  ok: every diag N > 0 and pivot >= kPivotFloor -- otherwise this is no candidate and power and beta
// mean nothing.  power = |L^-1 (b / d)|^2 / 2 = (chi2_0 - chi2_min) / 2.  Written out: no array, nothing indexed.
struct Fit {
  double power, ta, tb, tf, tg, pivot;
  bool ok;
};
EXO_EST_HD Fit fit(const Sums& a) {
  Fit r;
  const bool pos = a.xx0 > 0.0 && a.xx2 > 0.0 && a.ee0 > 0.0 && a.ee2 > 0.0;
  const double d0 = sqrt(pos ? a.xx0 : 1.0), d1 = sqrt(pos ? a.xx2 : 1.0), d2 = sqrt(pos ? a.ee0 : 1.0), d3 = sqrt(pos ? a.ee2 : 1.0);
  const double m01 = a.xx1 / (d0 * d1), m02 = a.xe0 / (d0 * d2), m03 = a.xe1 / (d0 * d3);
  const double m12 = a.xe1 / (d1 * d2), m13 = a.xe2 / (d1 * d3), m23 = a.ee1 / (d2 * d3);
  const double c0 = a.bx0 / d0, c1 = a.bx1 / d1, c2 = a.be0 / d2, c3 = a.be1 / d3;
  // column 0: the pivot is 1
  const double l10 = m01, l20 = m02, l30 = m03;
  const double p1 = fma(-l10, l10, 1.0);
  const double l11 = sqrt(p1);
  const double l21 = fma(-l20, l10, m12) / l11, l31 = fma(-l30, l10, m13) / l11;
  const double p2 = fma(-l21, l21, fma(-l20, l20, 1.0));
  const double l22 = sqrt(p2);
  const double l32 = fma(-l31, l21, fma(-l30, l20, m23)) / l22;
  const double p3 = fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, 1.0)));
  const double l33 = sqrt(p3);
  r.pivot = fmin(p1, fmin(p2, p3));
  // (a NaN pivot compares false: no candidate)
  r.ok = pos && p1 >= kPivotFloor && p2 >= kPivotFloor && p3 >= kPivotFloor;
  const double z0 = c0;
  const double z1 = fma(-l10, z0, c1) / l11;
  const double z2 = fma(-l21, z1, fma(-l20, z0, c2)) / l22;
  const double z3 = fma(-l32, z2, fma(-l31, z1, fma(-l30, z0, c3))) / l33;
  r.power = 0.5 * fma(z3, z3, fma(z2, z2, fma(z1, z1, z0 * z0)));
  const double u3 = z3 / l33;
  const double u2 = fma(-l32, u3, z2) / l22;
  const double u1 = fma(-l31, u3, fma(-l21, u2, z1)) / l11;
  const double u0 = fma(-l30, u3, fma(-l20, u2, fma(-l10, u1, z0)));
  r.ta = u0 / d0;
  r.tb = u1 / d1;
  r.tf = u2 / d2;
  r.tg = u3 / d3;
  return r;
}

// The Campbell elements of the four constants, in the package's convention: KeplerianOrbit rotates the orbital plane with
// the amplitude -a_angular (get_relative_position), so beta is MINUS the textbook Thiele-Innes constants at the package's
// omega.  Omega is brought into [0, pi) -- astrometry alone cannot tell (omega, Omega) from (omega + pi, Omega + pi) -- and
// omega, which moves by the same multiple of pi, into (-pi, pi].
struct Elements {
  double a_angular, incl, omega, Omega;
};
EXO_EST_HD Elements campbell(double ta, double tb, double tf, double tg) {
  Elements r;
  const double k = 0.5 * fma(tg, tg, fma(tf, tf, fma(tb, tb, ta * ta)));
  const double m = fma(ta, tg, -(tb * tf));
  const double j = sqrt(fmax(fma(k, k, -(m * m)), 0.0));
  const double a2 = j + k;
  r.a_angular = sqrt(a2);
  r.incl = acos(fmax(-1.0, fmin(1.0, m / a2)));
  const double p = atan2(tb - tf, ta + tg), q = atan2(-tb - tf, ta - tg);
  double Om = 0.5 * (p - q), om = 0.5 * (p + q);
  if (Om < 0.0) {
    Om += kPi;
    om += kPi;
  } else if (Om >= kPi) {
    Om -= kPi;
    om -= kPi;
  }
  om -= kPi;
  if (om <= -kPi) om += 2.0 * kPi;
  if (om <= -kPi) om += 2.0 * kPi;
  if (om > kPi) om -= 2.0 * kPi;
  r.Omega = Om;
  r.omega = om;
  return r;
}

}  // namespace ast
