// exo_rv_core.hpp -- the per-sample arithmetic of the radial-velocity and orbit-vector kernels (exo_rv.hip): one sample of
// the value, and one sample's contribution to the cotangent of its record.  Compiled for gfx950 by exo_rv.hip and for the
// host by tests/host_harness.cpp (EXO_HOST_BUILD), so that the same lines are held to the multiprecision fixture
// (tests/golden/orbit_mp.npz) on a machine without a GPU.
//
// Three things here are written the way they are because of e -> 1 and of times far from t_periastron:
//   * 1 - e^2 is formed as (1 - e)(1 + e): 1 - e * e loses the digits of 1 - e (relative error 1.3e-8 at e = 1 - 1e-8);
//   * 1 + e cos f and cos f + e come from the half-angle pair (X, Y) = (sqrt(1-e) cos E/2, sqrt(1+e) sin E/2) of the solver,
//         1 + e cos f = (1 - e)(1 + e) / (X^2 + Y^2),      cos f + e = ((1 + e) X^2 - (1 - e) Y^2) / (X^2 + Y^2),
//     and the position is (cos E - e, sqrt(1-e^2) sin E) = (X^2 - Y^2, 2 X Y): formed from a rounded cos f they cancel at
//     apoapsis (cos f -> -1), which is where an eccentric orbit spends its time;
//   * the mean anomaly (t - tp) n is carried as a sum of two doubles until it has been reduced to [-pi, pi]: with BJD-sized t
//     and tp = O(1) the two roundings of the plain product are 2.3e-16 |M| ~ 3e-9 rad at |M| = 3e7, which the derivative
//     df/dM ~ (1 - e)^-3/2 at periastron multiplies.  The reduced value is good to ~2e-16 (1 + |M| 1e-16) instead.
#pragma once
#include "../../include/exoplanet_amd.h"
#include "exo_math.hpp"

namespace exo {

// (mean_anomaly_reduced: exo_math.hpp, shared with the light-curve kernels)

struct RvSample {
  double g;      // cw (cos f + e) - sw sin f
  double sinf, cosf;
  double q;      // 1 + e cos f
  double cpe;    // cos f + e
};

// e outside [0, 1): NaN (the docstring's contract for the Kepler op, keplerian.py:58)
EXO_HD RvSample rv_sample(double t, const double* __restrict__ p) {
  const double e = p[EXO_RV_ECC];
  const bool ok = (e >= 0.0) && (e < 1.0);
  const double es = ok ? e : 0.5;
  const KeplerHalf kh = kepler_half(mean_anomaly_reduced(t, p[EXO_RV_TP], p[EXO_RV_N]), es, sqrt(1.0 - es), sqrt(1.0 + es));
  const double X2 = kh.X * kh.X, Y2 = kh.Y * kh.Y;
  const double iden = 1.0 / (X2 + Y2);
  const double nan = __builtin_nan("");
  RvSample s;
  s.sinf = ok ? 2.0 * kh.X * kh.Y * iden : nan;
  s.cosf = ok ? (X2 - Y2) * iden : nan;
  s.q = ok ? (1.0 - e) * (1.0 + e) * iden : nan;
  s.cpe = ok ? ((1.0 + e) * X2 - (1.0 - e) * Y2) * iden : nan;
  s.g = p[EXO_RV_COSW] * s.cpe - p[EXO_RV_SINW] * s.sinf;
  return s;
}

// one epoch's contribution to the cotangent of its record: acc[EXO_RV_NPAR] += gb * d rv / d rec
EXO_HD void rv_vjp_term(double tn, const double* __restrict__ rec, double gb, double* acc) {
  const double nn = rec[EXO_RV_N], tp = rec[EXO_RV_TP], e = rec[EXO_RV_ECC], cw = rec[EXO_RV_COSW], sw = rec[EXO_RV_SINW],
               amp = rec[EXO_RV_AMP];
  const double ome2 = (1.0 - e) * (1.0 + e);
  const double iome2 = 1.0 / ome2, iome32 = iome2 / sqrt(ome2);
  const RvSample s = rv_sample(tn, rec);
  // d f / d M = (1 + e cos f)^2 / (1 - e^2)^(3/2),  d f / d e = (2 + e cos f) sin f / (1 - e^2)
  const double q = s.q;
  const double dfdM = q * q * iome32, dfde = (1.0 + q) * s.sinf * iome2;
  const double dgdf = -(cw * s.sinf + sw * s.cosf);
  const double a = gb * amp;
  acc[EXO_RV_N] += a * dgdf * dfdM * (tn - tp);
  acc[EXO_RV_TP] -= a * dgdf * dfdM * nn;
  acc[EXO_RV_ECC] += a * (dgdf * dfde + cw);
  acc[EXO_RV_COSW] += a * s.cpe;
  acc[EXO_RV_SINW] -= a * s.sinf;
  acc[EXO_RV_AMP] += gb * s.g;
}

// ---------------------------------------------------------------------------------------------
// Position / velocity / acceleration vectors in the observer frame from the same solve (keplerian.py:380-409 _get_position,
// :572-578 _get_velocity, :679-706, :283-322 _rotate_vector).  In the orbital plane
//     position:  (u, v) = (1 - e^2) / (1 + e cos f) (cos f, sin f)        velocity:  (u, v) = (-sin f, cos f + e)
//     acceleration:  (u, v) = -(1 + e cos f)^2 / (1 - e^2) (cos f, sin f)
// times an amplitude, then the three rotations
//     x1 = cw u - sw v,  y1 = sw u + cw v;   x2 = x1,  y2 = ci y1,  Z = -si y1;   X = cO x2 - sO y2,  Y = sO x2 + cO y2.
// ---------------------------------------------------------------------------------------------
struct OvSample {
  double sinf, cosf;
  double q;             // 1 + e cos f
  double cpe;           // cos f + e
  double u, v;          // in-plane vector for unit amplitude
  double x2, y1, y2;    // after the omega and inclination rotations
  double X, Y, Z;       // unit amplitude
};

template <int MODE>
EXO_HD OvSample ov_sample(double t, const double* __restrict__ p) {
  const double e = p[EXO_OV_ECC];
  const bool ok = (e >= 0.0) && (e < 1.0);
  const double es = ok ? e : 0.5;
  const KeplerHalf kh = kepler_half(mean_anomaly_reduced(t, p[EXO_OV_TP], p[EXO_OV_N]), es, sqrt(1.0 - es), sqrt(1.0 + es));
  const double X2 = kh.X * kh.X, Y2 = kh.Y * kh.Y;
  const double iden = 1.0 / (X2 + Y2);
  const double nan = __builtin_nan("");
  const double ome2 = (1.0 - e) * (1.0 + e);
  OvSample s;
  s.sinf = ok ? 2.0 * kh.X * kh.Y * iden : nan;
  s.cosf = ok ? (X2 - Y2) * iden : nan;
  s.q = ok ? ome2 * iden : nan;
  s.cpe = ok ? ((1.0 + e) * X2 - (1.0 - e) * Y2) * iden : nan;
  if (MODE == 1) {
    s.u = -s.sinf; s.v = s.cpe;
  } else if (MODE == 2) {
    const double g = s.q * s.q / ome2;
    s.u = -g * s.cosf; s.v = -g * s.sinf;
  } else {
    s.u = ok ? X2 - Y2 : nan; s.v = ok ? 2.0 * kh.X * kh.Y : nan;     // = rho (cos f, sin f), without the quotient
  }
  const double x1 = p[EXO_OV_COSW] * s.u - p[EXO_OV_SINW] * s.v;
  s.y1 = p[EXO_OV_SINW] * s.u + p[EXO_OV_COSW] * s.v;
  s.x2 = x1;
  s.y2 = p[EXO_OV_COSI] * s.y1;
  s.Z = -p[EXO_OV_SINI] * s.y1;
  s.X = p[EXO_OV_COSO] * s.x2 - p[EXO_OV_SINO] * s.y2;
  s.Y = p[EXO_OV_SINO] * s.x2 + p[EXO_OV_COSO] * s.y2;
  return s;
}

// one epoch's contribution to the cotangent of its record: acc[EXO_OV_NPAR] += (gX0, gY0, gZ0) . d out / d rec
template <int MODE>
EXO_HD void ov_vjp_term(double tn, const double* __restrict__ rec, double gX0, double gY0, double gZ0, double* acc) {
  const double nn = rec[EXO_OV_N], tp = rec[EXO_OV_TP], e = rec[EXO_OV_ECC], cw = rec[EXO_OV_COSW], sw = rec[EXO_OV_SINW],
               ci = rec[EXO_OV_COSI], si = rec[EXO_OV_SINI], amp = rec[EXO_OV_AMP], cO = rec[EXO_OV_COSO],
               sO = rec[EXO_OV_SINO];
  const double ome2 = (1.0 - e) * (1.0 + e);
  const double iome2 = 1.0 / ome2, iome32 = iome2 / sqrt(ome2);
  const OvSample s = ov_sample<MODE>(tn, rec);
  acc[EXO_OV_AMP] += gX0 * s.X + gY0 * s.Y + gZ0 * s.Z;
  const double gX = amp * gX0, gY = amp * gY0, gZ = amp * gZ0;
  acc[EXO_OV_COSO] += gX * s.x2 + gY * s.y2;
  acc[EXO_OV_SINO] += gY * s.x2 - gX * s.y2;
  const double gx2 = gX * cO + gY * sO, gy2 = gY * cO - gX * sO;
  acc[EXO_OV_COSI] += gy2 * s.y1;
  acc[EXO_OV_SINI] -= gZ * s.y1;
  const double gy1 = gy2 * ci - gZ * si, gx1 = gx2;
  acc[EXO_OV_COSW] += gx1 * s.u + gy1 * s.v;
  acc[EXO_OV_SINW] += gy1 * s.u - gx1 * s.v;
  const double gu = gx1 * cw + gy1 * sw, gv = gy1 * cw - gx1 * sw;
  // (u, v) as functions of (f, e), f = f(M, e):  d f / d M = (1 + e cos f)^2 / (1 - e^2)^(3/2),
  // d f / d e = (2 + e cos f) sin f / (1 - e^2)
  const double q = s.q;
  double gf, ge;
  if (MODE == 1) {
    gf = -gu * s.cosf - gv * s.sinf;
    ge = gv;
  } else if (MODE == 2) {
    const double g = q * q * iome2;
    const double g_f = -2.0 * q * e * s.sinf * iome2;                                 // d g / d f
    const double g_e = 2.0 * q * (s.cosf * ome2 + e * q) * iome2 * iome2;             // d g / d e at fixed f
    gf = -gu * (g_f * s.cosf - g * s.sinf) - gv * (g_f * s.sinf + g * s.cosf);
    ge = -(gu * s.cosf + gv * s.sinf) * g_e;
  } else {
    const double iq = 1.0 / q, rho = ome2 * iq;
    const double rho_f = rho * e * s.sinf * iq;                                // d rho / d f
    // d rho / d e at fixed f = -(2 e + cos f (1 + e^2)) / q^2, its numerator as e q + (cos f + e): -(1 - e)^2 at apoapsis
    const double rho_e = -(e * q + s.cpe) * iq * iq;
    gf = gu * (rho_f * s.cosf - rho * s.sinf) + gv * (rho_f * s.sinf + rho * s.cosf);
    ge = (gu * s.cosf + gv * s.sinf) * rho_e;
  }
  const double dfdM = q * q * iome32, dfde = (1.0 + q) * s.sinf * iome2;
  const double gM = gf * dfdM;
  acc[EXO_OV_N] += gM * (tn - tp);
  acc[EXO_OV_TP] -= gM * nn;
  acc[EXO_OV_ECC] += ge + gf * dfde;
}

}  // namespace exo
