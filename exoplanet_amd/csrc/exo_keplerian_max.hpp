// exo_keplerian_max.hpp -- the highest peak of the Keplerian periodogram of every series of a batch, without the periodogram
// (exoplanet_amd/estimators.py: keplerian_max_power, false_alarm): what a group of G series on one time axis shares and what
// the arg-max over (frequency, candidate) is.  The true anomaly of an epoch depends on (f, e, phi, t_i) alone, so a candidate
// solves Kepler's equation once per epoch and feeds the sums of all G series; per series the arithmetic is that of
// exo_keplerian_core.hpp, function for function and epoch for epoch, so that a series' power at a (frequency, candidate) is
// bit for bit the one the periodogram's kernel forms.  Definition: DESIGN.md section 26.  Compiles for the device
// (exo_keplerian.hip) and, with EXO_HOST_BUILD, for the host (tests/keplerian_max_harness.cpp); both with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include "exo_keplerian_core.hpp"

namespace kepmax {

using kep::Segment;
using kep::Sums;
using orb::Candidate;

constexpr int kTile = 128;                                // epochs staged at a time (the order of the sums does not depend on it)
constexpr int kTotals = 2 * EXO_KEP_MAX_INSTRUMENTS;      // W_k, Y_k of a series' segments, as the preparation kernel lays them out

// the series behind slot g of the group that starts at series b0: a partly filled last group computes its missing slots on
// the last valid series (and never writes them)
EXO_EST_HD int64_t group_series(int64_t b0, int g, int64_t n_series) { return b0 + g < n_series ? b0 + g : n_series - 1; }

// a candidate's sums for G series; (s0, c0) of the open segment belongs to the candidate, not to a series, and is kept once
template <int G>
struct GroupState {
  Sums a[G];
  double s[G], c[G];
  double s0, c0;
};

// The staged epochs lo .. lo + len - 1 into the candidate's sums of all G series, in the epochs' order: one true anomaly per
// epoch, then kep::accumulate per series and, at a segment's end, kep::fold with that series' totals.  turns[i]: the reduced
// phase of epoch lo + i; pairs[(i * G + g) * 2 + {0, 1}]: w and w y of series g there (one 16-byte read, the same address in
// every lane); totals[g * kTotals + 2 k + {0, 1}]: W_k, Y_k; off[0 .. n_inst]: the segments.
template <int G>
EXO_EST_HD void group_walk(GroupState<G>& st, const Candidate& cd, const double* turns, const double* pairs, const double* totals,
                           const int32_t* off, int n_inst, int64_t lo, int len) {
  for (int k = 0; k < n_inst; ++k) {
    const int64_t begin = off[k], end = off[k + 1];
    const int i0 = (int)((begin > lo ? begin : lo) - lo), i1 = (int)((end < lo + len ? end : lo + len) - lo);
    for (int i = i0; i < i1; ++i) {
      double sn, cs;
      kep::true_anomaly(turns[i], cd.phi, cd.e, cd.se, cd.pe, &sn, &cs);
      const bool first = lo + i == begin;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        Segment sg = {st.s[g], st.c[g], st.s0, st.c0};
        kep::accumulate(st.a[g], sg, first, pairs[(i * G + g) * 2], pairs[(i * G + g) * 2 + 1], sn, cs);
        st.s[g] = sg.s;
        st.c[g] = sg.c;
        if (g == G - 1) {
          st.s0 = sg.s0;
          st.c0 = sg.c0;
        }
      }
    }
    if (end > lo && end <= lo + len) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        Segment sg = {st.s[g], st.c[g], st.s0, st.c0};
        kep::fold(st.a[g], sg, totals[g * kTotals + 2 * k], totals[g * kTotals + 2 * k + 1]);
        st.s[g] = sg.s;
        st.c[g] = sg.c;
      }
    }
  }
}

// the sum of a series' weights, in the order the periodogram's kernel adds them
EXO_EST_HD double total_weight(const double* totals, int n_inst) {
  double W = 0.0;
  for (int k = 0; k < n_inst; ++k) W += totals[2 * k];
  return W;
}

// The arg-max over (frequency, candidate) as one value: a larger power wins, of equal powers the lower frequency index, then
// the lower candidate; NaN never wins, and neither does -inf: a series without a finite power keeps (-inf, -1, -1).  The
// order is total, so partial results combine in any grouping.
struct Best3 {
  double power;
  int32_t frequency, candidate;
};
EXO_EST_HD Best3 best3_init() { return Best3{-INFINITY, -1, -1}; }
EXO_EST_HD void best3_take(Best3& a, double power, int32_t frequency, int32_t candidate) {
  const bool lower = frequency < a.frequency || (frequency == a.frequency && candidate < a.candidate);
  if (power > a.power || (power == a.power && a.frequency >= 0 && lower)) {
    a.power = power;
    a.frequency = frequency;
    a.candidate = candidate;
  }
}

}  // namespace kepmax
