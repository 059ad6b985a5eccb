// Host build of exoplanet_amd/csrc/exo_keplerian_core.hpp for tests/test_keplerian_host.py (g++, no GPU): every candidate's
// sums, power and coefficients, the arg-max and the winner's record, walked exactly as the kernel of exo_keplerian.hip walks
// them; and the Lomb-Scargle path of exo_estimators_core.hpp on the same columns, which ecc = [0] must reproduce.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_keplerian_core.hpp"
#include "orbit_lanes.hpp"

using namespace kep;
using namespace orb;

namespace {

// one candidate over the epochs in order, segment by segment; seg_g (or null) receives the segments as they were folded
Sums walk(const double* turns, const double* w, const double* wy, const int32_t* off, int n_inst, const double* Wk, const double* Yk,
          const Candidate& cd, Segment* seg_g) {
  Sums a = {0.0, 0.0, 0.0, 0.0, 0.0};
  Segment g = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < n_inst; ++k) {
    for (int32_t i = off[k]; i < off[k + 1]; ++i) {
      double sn, cs;
      true_anomaly(turns[i], cd.phi, cd.e, cd.se, cd.pe, &sn, &cs);
      accumulate(a, g, i == off[k], w[i], wy[i], sn, cs);
    }
    if (seg_g) seg_g[k] = g;
    fold(a, g, Wk[k], Yk[k]);
  }
  return a;
}

}  // namespace

extern "C" {

// tt, w, wy: the n epochs sorted by instrument (segments off[0 .. n_inst]).  table[n_ecc * n_phase]: every candidate's power
// (-inf where there is none).  record[4 + n_inst]: power, candidate, A, B and the constants of the winner, found as n_lane
// lanes find it (each its strided share, then the reduction from the LAST lane down, so that the tie rule decides).
void harness_keplerian(const double* tt, const double* w, const double* wy, int32_t n, const int32_t* off, int n_inst, double f,
                       const double* ecc, int n_ecc, int n_phase, int n_lane, double* table, double* record) {
  double* turns = new double[n];
  for (int32_t i = 0; i < n; ++i) turns[i] = est::ls_phase_turns(f, tt[i]);
  double Wk[EXO_KEP_MAX_INSTRUMENTS], Yk[EXO_KEP_MAX_INSTRUMENTS];
  Segment seg_g[EXO_KEP_MAX_INSTRUMENTS];
  double W = 0.0;
  for (int k = 0; k < n_inst; ++k) {
    Wk[k] = Yk[k] = 0.0;
    for (int32_t i = off[k]; i < off[k + 1]; ++i) Wk[k] += w[i], Yk[k] += wy[i];
    W += Wk[k];
  }
  const int n_cand = n_ecc * n_phase;
  for (int c = 0; c < n_cand; ++c) {
    const Candidate cd = candidate_of(c, n_cand, n_phase, ecc);
    table[c] = cd.live ? fit(walk(turns, w, wy, off, n_inst, Wk, Yk, cd, nullptr), W).power : -INFINITY;
  }
  const Best best = lanes_best(
      n_cand, n_lane, [&](int c) { return candidate_of(c, n_cand, n_phase, ecc).live; }, [&](int c) { return table[c]; });
  record[0] = best.power;
  record[1] = best.candidate == INT32_MAX ? -1.0 : (double)best.candidate;
  for (int q = 2; q < 4 + n_inst; ++q) record[q] = NAN;
  if (best.candidate != INT32_MAX) {
    const Fit r = fit(walk(turns, w, wy, off, n_inst, Wk, Yk, candidate_of(best.candidate, n_cand, n_phase, ecc), seg_g), W);
    record[0] = r.power;
    record[2] = r.A;
    record[3] = r.B;
    for (int q = 0; q < n_inst; ++q) record[4 + q] = constant(Wk[q], Yk[q], seg_g[q], r.A, r.B);
  }
  delete[] turns;
}

// the Lomb-Scargle power of the same columns at one frequency, through ls_accumulate and ls_power
double harness_lomb_scargle(const double* tt, const double* w, const double* wy, int32_t n, double f) {
  est::LsSums a{0, 0, 0, 0, 0, 0, 0};
  double W = 0.0, Y = 0.0;
  for (int32_t i = 0; i < n; ++i) {
    const double x = 2.0 * M_PI * est::ls_phase_turns(f, tt[i]);
    est::ls_accumulate(a, w[i], wy[i], sin(x), cos(x), 0.0);
    W += w[i];
    Y += wy[i];
  }
  return est::ls_power(a, W, Y);
}

// the comparison of the arg-max on its own: (power, candidate) pairs taken in the order given -> the survivor's candidate
int32_t harness_best(const double* power, const int32_t* cand, int n) {
  Best best = best_init();
  for (int i = 0; i < n; ++i) best_take(best, power[i], cand[i]);
  return best.candidate;
}

}  // extern "C"
