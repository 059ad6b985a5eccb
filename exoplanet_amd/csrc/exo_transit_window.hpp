// exo_transit_window.hpp -- where in mean anomaly a planet can overlap the disk at all: the conjunction windows of one record
// on eight lanes (window_lanes), the kernel that writes them for every (draw, planet) and checks that the times ascend
// (transit_window_kernel), and the phase test every consumer of a window applies (frac_rev, near_conjunction).
#pragma once
#include "exo_transit_sample.hpp"

namespace {

// Where can the planet overlap the disk at all?  Sky-plane separation (units of R*) is
//   rho sqrt(cos^2(w+f) + cos^2 i sin^2(w+f)) >= (a/R)(1-e) |cos(w+f)|,
// so b < 1 + r needs |cos(w+f)| < q = (1+r) / ((a/R)(1-e)) and, for the planet to be in
// front, sin(w+f) sin i > 0: f within asin(q) of the conjunction f_c = +-pi/2 - w -- a first bound,
// then tightened side by side to the contacts with the inclination and the distance actually reached
// (below: never inside them).  Mapped
// through E(f), M(E) (closed forms in this direction) that is a window of mean anomaly; the
// occultation window is the same about f_c + pi.  One thread per (draw, planet), run ahead of
// the scan kernel (libm's fp64 trigonometry would cost the scan kernel half its occupancy);
// the scan kernel's per-cadence test is then a phase wrap and a compare, and only cadences
// inside a window go on to the position-based classifier.
//   out[kWin] = { nrev = n / 2pi, c0 = -(tp nrev + mid_transit), mid_transit - mid_occultation,
//                 half_transit, half_occultation, inner_transit, inner_occultation }
// in revolutions of mean anomaly: the phase of cadence t is fma(t, nrev, c0), wrapped to +-1/2.
// q >= 1 or anything non-finite: halves = inf, every cadence goes on.  inner_*: an ESTIMATE of the
// half-width of the part of the window in which the small disk is wholly inside the large one
// (b + r < 1; 0 if never): the run-enumeration path sorts a window's cadences into "inside" and
// "limb" with it, so that a wave's vote on entering the arc geometry of the solution vector is
// nearly always unanimous.  A wrong estimate costs time, never a result.
//
// With EXO_FLAG_WINDOW the caller's contact-point windows (record slots T0, PERIOD, TS, TE[, TS2,
// TE2]; keplerian.py:729-731,765-769) are put in the same form instead -- revolutions of the
// orbit, centre t0 + (ts + te)/2, half-width (te - ts)/2 -- and they alone decide what is
// evaluated.
// (Blocks past the records' -- the run-enumeration path launches n_sorted more -- check that t is
// non-decreasing: one flag per kSortBlock cadences, the pair straddling the block's end included.)
#ifndef EXO_WINDOW_REFINE
#define EXO_WINDOW_REFINE 1   // (0: the first bound only -- A/B builds)
#endif
constexpr int kSortBlock = 4096;
constexpr int kWinLanes = 8;   // threads per record: (event, side of the conjunction, contact | inner point)
// Light delay: the body is seen where it was up to |z|max / (c - |vz|max) earlier or later, so the retarded time differs
// from t by at most that: a window's half-width grows by it (and 5 %), in the window's own unit -- `per_day` of them to
// a day: 1 / period for the caller's contact windows, |nrev| for revolutions of mean anomaly.  NaN or v >= c: no window.
__device__ __forceinline__ double light_delay_widening(const double* __restrict__ p, double e, double per_day) {
  const double vmax = fabs(p[EXO_P_N] * p[EXO_P_AOR]) * (1.0 + e) / sqrt(1.0 - e * e);
  const double dmax = fabs(p[EXO_P_AOR]) * (1.0 + e) / (fabs(p[EXO_P_CLIGHT]) - vmax);
  return (dmax >= 0.0 ? dmax : __builtin_inf()) * per_day * 1.05;
}
// The window of one record on EIGHT lanes (sub = 0 .. 7: (point, event, side); all eight must call it together: shuffles).
// On return: with EXO_FLAG_WINDOW every lane holds all seven numbers; otherwise lane sub = 0 holds w[0..3] and w[5] (the
// transit's), lane sub = 2 holds w[4] and w[6] (the occultation's).
__device__ __forceinline__ void window_lanes(const double* __restrict__ p, uint32_t flags, int sub, double* w) {
  const int which = sub >> 2, k = (sub >> 1) & 1, sd = sub & 1;   // point, event (0 transit, 1 occultation), side
  const double e = p[EXO_P_ECC], cw = p[EXO_P_COSW], sw = p[EXO_P_SINW];
  if (flags & EXO_FLAG_WINDOW) {   // (every lane: a dozen operations, and then every lane holds all seven)
    const double ip = 1.0 / p[EXO_P_PERIOD];
    const double ts = p[EXO_P_TS], te = p[EXO_P_TE], ts2 = p[EXO_P_TS2], te2 = p[EXO_P_TE2];
    const bool fin = (fabs(ts) < __builtin_inf()) && (fabs(te) < __builtin_inf());
    const bool fin2 = (fabs(ts2) < __builtin_inf()) && (fabs(te2) < __builtin_inf());
    const double mid = fin ? 0.5 * (ts + te) : 0.0, mid2 = fin2 ? 0.5 * (ts2 + te2) : 0.0;
    w[0] = ip;
    w[1] = -(p[EXO_P_T0] + mid) * ip;
    w[2] = (mid - mid2) * ip;
    // a hair wider than the reference's closed interval: a cadence exactly at a contact has zero flux
    w[3] = fin ? fma(0.5 * (te - ts) * ip, 1.0 + 1e-12, 1e-14) : __builtin_inf();
    w[4] = fin2 ? fma(0.5 * (te2 - ts2) * ip, 1.0 + 1e-12, 1e-14) : __builtin_inf();
    // inner parts: chord ratio sqrt((1-r)^2 - b^2) / sqrt((1+r)^2 - b^2) of the contact window,
    // b = impact parameter at the conjunction
    const double wn_ = sqrt(cw * cw + sw * sw), r_ = fabs(p[EXO_P_ROR]);
    const double sinw_ = wn_ > 0.0 ? sw / wn_ : 0.0;
    for (int q = 0; q < 2; ++q) {
      const double bk = fabs(p[EXO_P_AOR] * p[EXO_P_COSI]) * (1.0 - e * e) / (1.0 + (q ? -e : e) * sinw_);
      const double in2 = (1.0 - r_) * (1.0 - r_) - bk * bk, out2 = (1.0 + r_) * (1.0 + r_) - bk * bk;
      const double h = w[3 + q];
      w[5 + q] = (r_ < 1.0 && in2 > 0.0 && out2 > 0.0 && h < __builtin_inf()) ? 0.95 * h * sqrt(in2 / out2) : 0.0;
    }
    if (flags & EXO_FLAG_LIGHT_DELAY) {
      const double wd = light_delay_widening(p, e, ip);
      w[3] += wd; w[4] += wd;
    }
    return;     // (flag-uniform: every lane of the launch takes this branch or none does)
  }
  // Eight threads per record -- (event, side, contact | inner point) -- each with the short serial chain of its own
  // point.  No forward trigonometry: the conjunction's true anomaly f0 = +-pi/2 - w (+ pi) has cos f0 = +-sin w,
  // sin f0 = +-cos w; every angle of the refinement is carried as its sine (all lie in [0, pi/2)) and composed with f0
  // by the addition formulas; distances enter as 1 / dist = (1 + e cos f) / (a (1 - e^2)).  What is left is one atan2
  // for w, one asin for the angle reached and one atan2 for E(f).  (One thread per record with libm's sin / cos / asin
  // in the loop: 19 us of a 320 us sweep; four threads: 11.6 us; this form: see docs/DESIGN_r1_r4.md 4.)
  const double nrev = p[EXO_P_N] * (0.5 / exo::kPi);
  const double wn = sqrt(cw * cw + sw * sw);
  const double q = (1.0 + fabs(p[EXO_P_ROR])) / (fabs(p[EXO_P_AOR]) * (1.0 - e) * wn);
  const bool bounded = (e >= 0.0 && e < 1.0) && (q < 0.999);   // else NaN everywhere / no bound: every cadence goes on
  const bool want = bounded && (k == 0 || (flags & EXO_FLAG_SECONDARY));
  double m_pt = 0.0;       // this thread's point (contact or inner point of its side), revolutions of mean anomaly
  bool has_in = false;
  if (want) {
    const double se = sqrt(1.0 - e), pe = sqrt(1.0 + e);
    const double s0 = p[EXO_P_SINI] < 0.0 ? -1.0 : 1.0, sk = k ? -1.0 : 1.0;
    const double sinw = sw / wn, cosw = cw / wn;
    const double cf0 = sk * s0 * sinw, sf0 = sk * s0 * cosw;
    const double f0 = 0.5 * s0 * exo::kPi - atan2(sw, cw) + k * exo::kPi;
    const double si2 = p[EXO_P_SINI] * p[EXO_P_SINI], ci2 = p[EXO_P_COSI] * p[EXO_P_COSI];
    const double lim = 1.0 + fabs(p[EXO_P_ROR]), semi = fabs(p[EXO_P_AOR]) * (1.0 - e * e);
    const double sgn = sd ? 1.0 : -1.0;
    double sphi;   // sine of the angle from the conjunction to this thread's point
    if (which == 0) {
      // The bound above is that of an edge-on orbit at its periastron distance.  At phase angle phi from the
      // conjunction the sky-plane separation is dist(f) sqrt(cos^2 i + sin^2 i sin^2 phi): the disks overlap only where
      // phi <= G(phi) = asin sqrt(((1 + r)^2 / dist(f0 +- phi)^2 - cos^2 i) / sin^2 i).  Each side of the conjunction on
      // its own, from the upper bound ub = asin q, never below the contact:
      //   dist falling away from the conjunction (G rising): ub <- G(ub);
      //   dist rising (G falling): lb = G(ub) is a lower bound of the contact, so G(lb) an upper one;
      //   an apsis inside the half-window: G at the smallest distance in it.
      // Three rounds leave the window within ~0.1 % of the contacts (C2: it was 6.8 % wider than them); a planet that
      // never reaches the disk (b > 1 + r) keeps only the safety margin.
      double su = q;
      if (EXO_WINDOW_REFINE && si2 > 1e-12) {
        const double isemi = 1.0 / semi, isi2 = 1.0 / si2, lim2 = lim * lim;
        auto sin_ang = [&](double u) {   // u = 1 / dist
          const double S = (lim2 * u * u - ci2) * isi2;
          return S <= 0.0 ? 0.0 : (S < 1.0 ? sqrt(S) : q);   // (NaN: no information)
        };
        auto u_at = [&](double sa) {     // 1 / dist at f0 + sgn * asin(sa)
          return fma(e, cf0 * sqrt(1.0 - sa * sa) - sgn * sf0 * sa, 1.0) * isemi;
        };
        const double u_c = fma(e, cf0, 1.0) * isemi;
        for (int it = 0; it < 3; ++it) {
          // an apsis (f = m pi) in [f0, f_end] <=> sin f changes sign over it (the interval is shorter than pi / 2);
          // it is the periastron <=> cos f0 > 0
          const double s_end = sf0 * sqrt(1.0 - su * su) + sgn * cf0 * su;
          const bool apsis = sf0 * s_end <= 0.0;
          const double u_end = u_at(su);
          if (!apsis && u_end <= u_c) {
            const double lb = fmin(sin_ang(u_end), su);
            su = fmin(su, sin_ang(u_at(lb)));
          } else {
            su = fmin(su, sin_ang((apsis && cf0 > 0.0) ? (1.0 + e) * isemi : fmax(u_end, u_c)));
          }
        }
      }
      sphi = su;
    } else {
      // inner part: |sky-plane x| < sqrt((1-r)^2 - b^2) at the conjunction's star-planet distance
      const double r = fabs(p[EXO_P_ROR]);
      const double dist = fabs(p[EXO_P_AOR]) * (1.0 - e * e) / (1.0 + (k ? -e : e) * sinw);
      const double bk = dist * fabs(p[EXO_P_COSI]);
      const double in2 = (1.0 - r) * (1.0 - r) - bk * bk;
      has_in = r < 1.0 && in2 > 0.0 && dist > 0.0;
      sphi = has_in ? fmin(0.95 * sqrt(in2) / dist, 1.0) : 0.0;
    }
    // the point's true anomaly f = f0 + sgn (phi (1 + 1e-6) + 1e-6) for a contact, f0 + sgn phi for an inner point:
    // its angle for the revolution count, its sine and cosine by the addition formulas (the margin: a rotation by
    // delta <= 2.6e-6, second order)
    const double phi = asin(sphi), cphi = sqrt(fmax(1.0 - sphi * sphi, 0.0));
    const double delta = which == 0 ? fma(phi, 1e-6, 1e-6) : 0.0;
    const double c1 = cf0 * cphi - sgn * sf0 * sphi, s1 = sf0 * cphi + sgn * cf0 * sphi;
    const double hd = 1.0 - 0.5 * delta * delta;
    const double cf = c1 * hd - sgn * delta * s1, sf = s1 * hd + sgn * delta * c1;
    // E(f) = f - 2 atan(beta sin f / (1 + beta cos f)), beta = e / (1 + sqrt(1 - e^2)): continuous in f, no wrap
    const double rt = se * pe, beta = e / (1.0 + rt);
    const double E = (f0 + sgn * (phi + delta)) - 2.0 * atan2(beta * sf, fma(beta, cf, 1.0));
    m_pt = (E - e * (rt * sf / fma(e, cf, 1.0))) * (0.5 / exo::kPi);
  }
  // the record's other numbers (lanes 8j .. 8j + 7 hold one record: no record straddles a wave)
  const double m_other = __shfl_xor(m_pt, 4, 64);    // (every shuffle outside the branches: all eight lanes take part)
  const int in_other = __shfl_xor((int)has_in, 4, 64);
  const double m_edge = which ? m_other : m_pt, m_in = which ? m_pt : m_other;
  has_in = has_in || in_other != 0;
  const double o_edge = __shfl_xor(m_edge, 1, 64), o_in = __shfl_xor(m_in, 1, 64);
  const double lo = sd ? o_edge : m_edge, hi = sd ? m_edge : o_edge;
  const double mid = 0.5 * (lo + hi);
  const double half = want ? 0.5 * (hi - lo) * (1.0 + 1e-5) + 1e-6 : __builtin_inf();
  // (about the window's centre, which the two contacts set: the smaller of the two sides)
  const double in_lo = sd ? o_in : m_in, in_hi = sd ? m_in : o_in;
  const double inner = (want && has_in) ? fmax(fmin(in_hi - mid, mid - in_lo), 0.0) : 0.0;
  const double mid_other = __shfl_xor(mid, 2, 64);   // the other event's centre
  const double wd = (flags & EXO_FLAG_LIGHT_DELAY) ? light_delay_widening(p, e, fabs(nrev)) : 0.0;
  // (valid on the lanes with sd == 0, which == 0: event 0 -> w[0..3], w[5]; event 1 -> w[4], w[6])
  if (k == 0) {
    w[0] = nrev;
    w[1] = bounded ? -fma(p[EXO_P_TP], nrev, mid) : -p[EXO_P_TP] * nrev;
    w[2] = (bounded && (flags & EXO_FLAG_SECONDARY)) ? mid - mid_other : 0.0;
    w[3] = half + wd;
    w[5] = inner;
  } else {
    w[4] = half + wd;
    w[6] = inner;
  }
}

__global__ __launch_bounds__(kBlock) void transit_window_kernel(const double* __restrict__ params, int64_t n_rec,
    uint32_t flags, double* __restrict__ out, const double* __restrict__ t = nullptr, int64_t n_cad = 0,
    int32_t* __restrict__ sorted = nullptr, int32_t* __restrict__ done = nullptr, int64_t n_done = 0) {
  const int n_rec_blocks = (int)((n_rec * kWinLanes + kBlock - 1) / kBlock);
  // (the per-draw block counters of the sweep that follows: transit_runs_kernel)
  if (done && (int64_t)blockIdx.x * kBlock + threadIdx.x < n_done) done[(int64_t)blockIdx.x * kBlock + threadIdx.x] = 0;
  if ((int)blockIdx.x >= n_rec_blocks) {
    const int sb = blockIdx.x - n_rec_blocks;
    const int64_t b0 = (int64_t)sb * kSortBlock;
    bool ok = true;
    for (int64_t k = b0 + threadIdx.x; k < b0 + kSortBlock && k + 1 < n_cad; k += kBlock) ok = ok && (t[k] <= t[k + 1]);   // NaN: not sorted
    const int all = __syncthreads_and(ok ? 1 : 0);
    if (threadIdx.x == 0) sorted[sb] = all;
    return;
  }
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t i = gid / kWinLanes;
  const int sub = (int)(gid - i * kWinLanes);
  if (i >= n_rec) return;   // (whole groups of eight: the shuffles below stay within a record)
  double w[kWin] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  window_lanes(params + i * EXO_NPAR, flags, sub, w);
  double* o = out + kWin * i;
  if (flags & EXO_FLAG_WINDOW) {
    if (sub == 0)
      for (int q = 0; q < kWin; ++q) o[q] = w[q];
  } else if (sub == 0) {
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[3]; o[5] = w[5];
  } else if (sub == 2) {
    o[4] = w[4]; o[6] = w[6];
  }
}

// first test of the scan kernel: is the wrapped phase within lim of a conjunction?  NaN -> yes.
// x - rint(x) through the 1.5 * 2^52 shift (two full-rate adds; |x| < 2^51 revolutions).
__device__ __forceinline__ double frac_rev(double x) {
  const double kShift = 6755399441055744.0;
  return x - ((x + kShift) - kShift);
}
template <bool SECONDARY>
__device__ __forceinline__ bool near_conjunction(double t, double nrev, double c0, double dmid, double lim0,
                                                 double lim1) {
  const double x = fma(t, nrev, c0);
  bool cand = !(fabs(frac_rev(x)) > lim0);
  if (SECONDARY) cand = cand || !(fabs(frac_rev(x + dmid)) > lim1);
  return cand;
}

}  // namespace
