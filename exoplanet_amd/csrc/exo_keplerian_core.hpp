// exo_keplerian_core.hpp -- the per-candidate arithmetic of the Keplerian periodogram of a radial-velocity series
// (exoplanet_amd/estimators.py: keplerian_power, keplerian_estimator): one epoch's true anomaly and its contribution to a
// candidate's sums, the fold of one instrument's segment, and the power and the coefficients from the centred sums.  The
// candidates, their numbering and the arg-max: exo_orbit_search.hpp.  Definition: DESIGN.md section 22.  Compiles for the
// device (exo_keplerian.hip) and, with EXO_HOST_BUILD, for the host (tests/keplerian_harness.cpp checks it against the numpy
// statement without a GPU).  Every product that is meant to be fused is written as an fma: both builds are compiled with
// -ffp-contract=off.
#pragma once
#include <math.h>

#include "exo_estimators_core.hpp"
#include "exo_math.hpp"
#include "exo_orbit_search.hpp"

namespace kep {

// The five sums of a candidate over the epochs, raw while a segment is open and centred once it is folded:
// sum w y sin nu, w y cos nu, w sin^2 nu, w cos^2 nu, w cos nu sin nu ...
struct Sums {
  double ys, yc, ss, cc, cs;
};
// ... and the two sums of the open segment, sum w sin nu and sum w cos nu.  Every sum is formed of sin nu - s0 and cos nu - c0,
// (s0, c0) being the values at the segment's first epoch: the instrument's free constant makes the fit blind to such a shift,
// and at frequencies where nu hardly moves over the baseline the centred sums are then no longer the small difference of two
// large ones -- the reason ls_accumulate takes kappa off its cosine.
struct Segment {
  double s, c, s0, c0;
};

// cos nu and sin nu of one epoch.  `turns` = ls_phase_turns(f, t - t_min), the reduced product; the phase of periastron comes
// off in turns, and only then the factor 2 pi.  The half-angle pair (X, Y) of the solver gives den = X^2 + Y^2 = 1 - e cos E,
// den cos nu = X^2 - Y^2, den sin nu = 2 X Y (exo_rv_core.hpp): no rounded cos E anywhere.  se = sqrt(1 - e), pe = sqrt(1 + e).
EXO_EST_HD void true_anomaly(double turns, double phi, double e, double se, double pe, double* sn, double* cs) {
  const exo::KeplerHalf kh = exo::kepler_half(orb::kTwoPi * (turns - phi), e, se, pe);
  const double X2 = kh.X * kh.X, Y2 = kh.Y * kh.Y;
  const double iden = exo::fast_rcp(X2 + Y2);  // (1 - e <= X^2 + Y^2 <= 1 + e: well scaled)
  *cs = (X2 - Y2) * iden;
  *sn = 2.0 * kh.X * kh.Y * iden;
}

// one epoch into the sums; `first`: it opens its segment
EXO_EST_HD void accumulate(Sums& a, Segment& g, bool first, double w, double wy, double sn_nu, double cs_nu) {
  if (first) {
    g.s0 = sn_nu;
    g.c0 = cs_nu;
  }
  const double sn = sn_nu - g.s0, cs = cs_nu - g.c0;
  const double ws = w * sn, wc = w * cs;
  a.ys = fma(wy, sn, a.ys);
  a.yc = fma(wy, cs, a.yc);
  a.ss = fma(ws, sn, a.ss);
  a.cc = fma(wc, cs, a.cc);
  a.cs = fma(wc, sn, a.cs);
  g.s += ws;
  g.c += wc;
}

// The end of an instrument's segment with the totals W_k = sum w, Y_k = sum w y: its weighted means come off y, sin nu and
// cos nu, which is what the instrument's free constant does to the normal equations.  The segment's sums start again.
EXO_EST_HD void fold(Sums& a, Segment& g, double Wk, double Yk) {
  const double ybar = Yk / Wk;
  a.ys = a.ys - ybar * g.s;
  a.yc = a.yc - ybar * g.c;
  a.ss = a.ss - g.s * g.s / Wk;
  a.cc = a.cc - g.c * g.c / Wk;
  a.cs = a.cs - g.c * g.s / Wk;
  g.s = 0.0;
  g.c = 0.0;
}

// power = (chi2_0 - chi2) / 2 and the coefficients of  v = c_k + A cos nu + B sin nu  from the centred sums: the 2 x 2 system
// [[SS, CS], [CS, CC]] (B, A) = (YS, YC), solved as ls_power solves its own.  W: the sum of all weights (it scales the
// threshold under which a direction counts as having no variance).
struct Fit {
  double power, A, B;
};
EXO_EST_HD Fit fit(const Sums& a, double W) {
  const est::LsFit r = est::ls_fit_centred(est::LsCentred{a.ys, a.yc, a.ss, a.cc, a.cs}, W);
  return Fit{r.power, r.b, r.a};
}

// the constant of an instrument, given the segment's own sums as they were when it was folded: the weighted mean of
// y - A cos nu - B sin nu
EXO_EST_HD double constant(double Wk, double Yk, const Segment& g, double A, double B) {
  return (Yk - A * g.c - B * g.s) / Wk - (A * g.c0 + B * g.s0);
}

}  // namespace kep
