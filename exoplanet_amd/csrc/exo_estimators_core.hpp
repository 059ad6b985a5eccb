// exo_estimators_core.hpp -- the per-period arithmetic of the period-search estimators (exoplanet_amd/estimators.py):
// the box-least-squares bin index and objective, the template search on the same bins (transit least squares), and the
// closed-form floating-mean Lomb-Scargle power from its weighted sums.  Definitions and derivations: DESIGN.md sections 9
// and 18.  Compiles for the device (exo_estimators.hip) and, with EXO_HOST_BUILD, for the host (tests/estimators_harness.cpp
// and tests/tls_harness.cpp check it against the numpy restatements without a GPU).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_EST_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_EST_HD __device__ __forceinline__
#endif

namespace est {

// ---- box least squares ------------------------------------------------------------------------------------------------------

// n_bins = ceil(p / delta) + oversample.  One correctly rounded fp64 division (the same on the host and on the device).
EXO_EST_HD int64_t bls_n_bins(double p, double delta, int oversample) { return (int64_t)ceil(p / delta) + oversample; }

// floor(x / y) of the EXACT quotient for x >= 0, y > 0, and the exact remainder x - q y, from a reciprocal and one
// correction step: q0 = floor(x * (1 / y)) is off by at most one (x / y < 2^50), fma(-q, y, x) is exact when q is the true
// quotient (the remainder of two doubles is a double) and has the right sign when it is not.
EXO_EST_HD double floor_div(double x, double y, double inv_y, double* rem) {
  double q = floor(x * inv_y);
  double r = fma(-q, y, x);
  if (r < 0.0) {
    q -= 1.0;
    r = fma(-q, y, x);
  } else if (r >= y) {
    q += 1.0;
    r = fma(-q, y, x);
  }
  *rem = r;
  return q;
}

// bin of a cadence at tt = t - t_min >= 0: 1 + floor(fmod(tt, p) / delta).  fmod comes out exact (floor_div's remainder);
// the floor is that of the exact quotient, which differs from the floor of the ROUNDED quotient only where the quotient
// lies within one rounding of an integer -- inside the 1e-9 band in which the bin is not well defined.
// The result is clamped to [1, n_bins] (a NaN time lands in bin 1): the index is used as an address.
EXO_EST_HD int64_t bls_bin_index(double tt, double p, double inv_p, double delta, double inv_delta, int64_t n_bins) {
  double x, e;
  floor_div(tt, p, inv_p, &x);
  const double b = 1.0 + floor_div(x, delta, inv_delta, &e);
  if (!(b >= 1.0)) return 1;
  return b >= (double)n_bins ? n_bins : (int64_t)b;
}

struct BlsBox {
  double depth, depth_err, depth_snr, log_likelihood;
  bool ok;  // w_in > 0 and w_out > 0
};

// one box: the sums inside it (differences of the prefix sums) against the totals
EXO_EST_HD BlsBox bls_box(double y_in, double w_in, double Y, double W) {
  BlsBox r;
  const double y_out = Y - y_in, w_out = W - w_in;
  r.ok = w_in > 0.0 && w_out > 0.0;
  r.depth = y_out / w_out - y_in / w_in;
  r.depth_err = sqrt(1.0 / w_in + 1.0 / w_out);
  r.depth_snr = r.depth / r.depth_err;
  r.log_likelihood = 0.5 * w_in * r.depth * r.depth;
  return r;
}

// objective 0: log likelihood, 1: depth signal to noise
EXO_EST_HD double bls_objective(const BlsBox& b, int objective) { return objective ? b.depth_snr : b.log_likelihood; }

// running arg-max in (k, s) order: `key` = k * key_stride + s; a larger objective wins, an equal one only with a smaller key
// (so the first maximiser survives whatever the order of the comparisons); NaN never wins
struct BlsBest {
  double obj;
  int64_t key;
};
EXO_EST_HD BlsBest bls_best_init() { return BlsBest{-INFINITY, INT64_MAX}; }
EXO_EST_HD void bls_best_take(BlsBest& a, double obj, int64_t key) {
  if (obj > a.obj || (obj == a.obj && key < a.key)) {
    a.obj = obj;
    a.key = key;
  }
}

// the search of one period over prefix sums cy, cw[0 .. n_bins] for the lanes `lane`, lane + n_lane, ... of every duration
template <class Ptr>
EXO_EST_HD BlsBest bls_search(Ptr cy, Ptr cw, int64_t n_bins, const int32_t* m, int n_dur, double Y, double W, int objective,
                              int64_t lane, int64_t n_lane) {
  BlsBest best = bls_best_init();
  for (int k = 0; k < n_dur; ++k) {
    const int64_t mk = m[k];
    if (mk < 1) continue;
    for (int64_t s = lane; s + mk <= n_bins; s += n_lane) {
      const BlsBox b = bls_box(cy[s + mk] - cy[s], cw[s + mk] - cw[s], Y, W);
      if (b.ok) bls_best_take(best, bls_objective(b, objective), (int64_t)k * (n_bins + 1) + s);
    }
  }
  return best;
}

// The seven outputs of one period, for both searches (out[i * stride]: power, depth, depth_err, depth_snr, log_likelihood,
// duration, transit_time): the fit at the maximiser, the objective's value there, and the maximiser itself -- mk bins wide
// from bin s.  Not `found` (no admissible box or window): power = -inf, the rest NaN, and nothing else is read.
EXO_EST_HD void search_outputs(bool found, double depth, double depth_err, double depth_snr, double log_likelihood, double power,
                               int64_t mk, int64_t s, double p, double delta, double t_min, double* out, int64_t stride) {
  if (!found) {
    out[0] = -INFINITY;
    for (int i = 1; i < 7; ++i) out[i * stride] = NAN;
    return;
  }
  out[0] = power;
  out[1 * stride] = depth;
  out[2 * stride] = depth_err;
  out[3 * stride] = depth_snr;
  out[4 * stride] = log_likelihood;
  out[5 * stride] = (double)mk * delta;
  out[6 * stride] = fmod((double)s * delta + 0.5 * (double)mk * delta + t_min, p);
}

// the box search's outputs: its box at the maximiser is taken from the prefix sums again
template <class Ptr>
EXO_EST_HD void bls_outputs(Ptr cy, Ptr cw, int64_t n_bins, const int32_t* m, double Y, double W, int objective, BlsBest best,
                            double p, double delta, double t_min, double* out, int64_t stride) {
  const bool found = best.key != INT64_MAX;
  const int64_t k = best.key / (n_bins + 1), s = best.key % (n_bins + 1), mk = found ? m[k] : 0;
  const BlsBox b = found ? bls_box(cy[s + mk] - cy[s], cw[s + mk] - cw[s], Y, W) : BlsBox{};
  search_outputs(found, b.depth, b.depth_err, b.depth_snr, b.log_likelihood, bls_objective(b, objective), mk, s, p, delta, t_min,
                 out, stride);
}

// ---- transit least squares: a template in place of the box -----------------------------------------------

struct TlsWindow {
  double A, B, C, w_in;  // sum g hw, sum g^2 hw, sum g hy, sum hw over the window
  double D, depth, depth_err, depth_snr, log_likelihood;
  bool ok;  // w_in > 0, W - w_in > 0 and D > 0
};

// one window of the histogram hy, hw (NOT prefix sums): bins s + 1 .. s + mk against the template g[0 .. mk - 1], ascending j.
// The model c - depth g inside, c outside, both fitted: D = B - A^2 / W, depth = (A Y / W - C) / D.  Every product that could
// be contracted into a fused multiply-add is written as one, so that the search and the recomputation at the maximiser, and
// the host and the device build, do the same operations.
template <class Ptr, class GPtr>
EXO_EST_HD TlsWindow tls_window(Ptr hy, Ptr hw, GPtr g, int64_t s, int64_t mk, double Y, double W) {
  TlsWindow r;
  double A = 0.0, B = 0.0, C = 0.0, w_in = 0.0;
#ifndef EXO_HOST_BUILD
#pragma unroll 4  // (four bins' loads in flight before the first fma waits for them; each sum keeps its ascending order)
#endif
  for (int64_t j = 0; j < mk; ++j) {
    const double gj = g[j], wj = hw[s + 1 + j], yj = hy[s + 1 + j];
    A = fma(gj, wj, A);
    B = fma(gj * gj, wj, B);
    C = fma(gj, yj, C);
    w_in += wj;
  }
  r.A = A, r.B = B, r.C = C, r.w_in = w_in;
  r.D = fma(-A, A / W, B);
  r.ok = w_in > 0.0 && W - w_in > 0.0 && r.D > 0.0;
  const double root = sqrt(r.D);
  r.depth = fma(A, Y / W, -C) / r.D;
  r.depth_err = 1.0 / root;
  r.depth_snr = r.depth * root;
  r.log_likelihood = 0.5 * r.depth * r.depth * r.D;
  return r;
}

EXO_EST_HD double tls_objective(const TlsWindow& w, int objective) { return objective ? w.depth_snr : w.log_likelihood; }

// the search of one period over the histogram hy, hw[0 .. n_bins] for the lanes `lane`, lane + n_lane, ... of every duration;
// template k is g[off[k] .. off[k] + m[k] - 1].  Keys and ties as in bls_search.
template <class Ptr, class GPtr>
EXO_EST_HD BlsBest tls_search(Ptr hy, Ptr hw, int64_t n_bins, const int32_t* m, const int32_t* off, int n_dur, GPtr g, double Y,
                              double W, int objective, int64_t lane, int64_t n_lane) {
  BlsBest best = bls_best_init();
  for (int k = 0; k < n_dur; ++k) {
    const int64_t mk = m[k];
    if (mk < 1) continue;
    for (int64_t s = lane; s + mk <= n_bins; s += n_lane) {
      const TlsWindow w = tls_window(hy, hw, g + off[k], s, mk, Y, W);
      if (w.ok) bls_best_take(best, tls_objective(w, objective), (int64_t)k * (n_bins + 1) + s);
    }
  }
  return best;
}

// the seven outputs at the maximiser, laid out as bls_outputs'; its window is summed again in the order of the search
template <class Ptr, class GPtr>
EXO_EST_HD void tls_outputs(Ptr hy, Ptr hw, int64_t n_bins, const int32_t* m, const int32_t* off, GPtr g, double Y, double W,
                            int objective, BlsBest best, double p, double delta, double t_min, double* out, int64_t stride) {
  const bool found = best.key != INT64_MAX;
  const int64_t k = best.key / (n_bins + 1), s = best.key % (n_bins + 1), mk = found ? m[k] : 0;
  const TlsWindow w = found ? tls_window(hy, hw, g + off[k], s, mk, Y, W) : TlsWindow{};
  search_outputs(found, w.depth, w.depth_err, w.depth_snr, w.log_likelihood, tls_objective(w, objective), mk, s, p, delta, t_min,
                 out, stride);
}

// ---- Lomb-Scargle -----------------------------------------------------------------------------------------------------------

// the phase of a cadence in turns, reduced to [-1/2, 1/2] BEFORE the multiplication by 2 pi: the product f t exactly as
// hi + lo (one fma), the integer part taken off hi (exact), lo added back.  Large f t keeps its digits.
EXO_EST_HD double ls_phase_turns(double f, double t) {
  const double hi = f * t, lo = fma(f, t, -hi);
  return (hi - rint(hi)) + lo;
}

// The sums of one frequency over the cadences, x = 2 pi f t, c = cos x - kappa.  kappa is any constant (the power does not
// depend on it: the model has a free constant); the kernel takes the mean of cos x over an evenly filled baseline,
// sinc(f T), so that at low frequencies, where cos x hardly moves, the variance of c is not the small difference of two large
// sums.  For the same reason sin^2 and c^2 are summed themselves and not recovered from the double angle.
struct LsSums {
  double ys, yc, s, c, ss, cc, sc;  // sum w y sin x, w y c, w sin x, w c, w sin^2 x, w c^2, w c sin x
};

EXO_EST_HD double ls_kappa(double f, double T) {
  const double u = fabs(f * T);
  if (!(u > 1e-8)) return 1.0;
#ifdef EXO_HOST_BUILD
  return sin(M_PI * u) / (M_PI * u);
#else
  return sinpi(u) / (M_PI * u);
#endif
}

// one cadence: sin and cos once
EXO_EST_HD void ls_accumulate(LsSums& a, double w, double wy, double sn, double cs, double kappa) {
  const double c = cs - kappa, ws = w * sn, wc = w * c;
  a.ys = fma(wy, sn, a.ys);
  a.yc = fma(wy, c, a.yc);
  a.s += ws;
  a.c += wc;
  a.ss = fma(ws, sn, a.ss);
  a.cc = fma(wc, c, a.cc);
  a.sc = fma(ws, c, a.sc);
}

// power = (chi2_0 - chi2(f)) / 2 of the floating-mean model a sin x + b cos x + const under weights w, from the seven sums and
// the totals W = sum w, Y = sum w y.  Removing the weighted mean of y and of both basis functions leaves the
// 2 x 2 normal equations  [[SS, CS], [CS, CC]] (a, b) = (YS, YC); the rotation by tau, tan 2 tau = 2 CS / (CC - SS),
// diagonalises them, and the power is the sum of the two projections.  A direction with no variance contributes nothing.
//
// In two steps, because the Keplerian periodogram (exo_keplerian_core.hpp) centres its sums instrument by instrument and then
// solves the same 2 x 2 system: ls_fit_centred takes the centred sums and also gives the coefficients (a of the sine column,
// b of the cosine column; a direction with no variance gets the coefficient 0), ls_power centres and takes the power.
struct LsCentred {
  double YS, YC, SS, CC, CS;
};
struct LsFit {
  double power, a, b;
};

EXO_EST_HD LsFit ls_fit_centred(const LsCentred& m, double W) {
  const double YS = m.YS, YC = m.YC, SS = m.SS, CC = m.CC, CS = m.CS;
  const double d = CC - SS, h = hypot(d, 2.0 * CS);
  double c2t = 1.0, s2t = 0.0;
  if (h > 0.0) {
    c2t = d / h;
    s2t = 2.0 * CS / h;
  }
  // cos tau >= 0; sin tau carries the sign of sin 2 tau.  The half-angle that does not cancel is taken first.
  double ct, st;
  if (c2t >= 0.0) {
    ct = sqrt(0.5 * (1.0 + c2t));
    st = 0.5 * s2t / ct;
  } else {
    st = (s2t >= 0.0 ? 1.0 : -1.0) * sqrt(0.5 * (1.0 - c2t));
    ct = 0.5 * s2t / st;
  }
  const double yc = YC * ct + YS * st, ys = YS * ct - YC * st;
  const double cc = CC * ct * ct + 2.0 * CS * ct * st + SS * st * st;  // the larger eigenvalue: (CC + SS + h) / 2
  const double ss = SS * ct * ct - 2.0 * CS * ct * st + CC * st * st;  // the smaller one
  const double tiny = 1e-14 * W;
  double pw = 0.0, ac = 0.0, as = 0.0;  // ac, as: the coefficients of the rotated columns c ct + s st and s ct - c st
  if (cc > tiny) {
    pw += yc * yc / cc;
    ac = yc / cc;
  }
  if (ss > tiny) {
    pw += ys * ys / ss;
    as = ys / ss;
  }
  return LsFit{0.5 * pw, ac * st + as * ct, ac * ct - as * st};
}

EXO_EST_HD double ls_power(const LsSums& a, double W, double Y) {
  const double ybar = Y / W;
  const double YS = a.ys - ybar * a.s, YC = a.yc - ybar * a.c;
  const double CC = a.cc - a.c * a.c / W, SS = a.ss - a.s * a.s / W, CS = a.sc - a.c * a.s / W;
  return ls_fit_centred(LsCentred{YS, YC, SS, CC, CS}, W).power;
}

}  // namespace est
