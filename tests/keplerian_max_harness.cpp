// Host build of exoplanet_amd/csrc/exo_keplerian_max.hpp for tests/test_false_alarm_host.py (g++, no GPU): every candidate's
// power for every series of a batch, walked in groups of G series as keplerian_max_kernel of exo_keplerian.hip walks them (one
// true anomaly per epoch, G accumulations, folds and fits; a partly filled last group on a clamped series), and the three-key
// arg-max on its own.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_keplerian_max.hpp"

using namespace kepmax;

namespace {

// tt[n]; w, wy[n_series][n], the epochs sorted by instrument; table[n_series][n_ecc * n_phase] (-inf where there is no candidate)
template <int G>
void group_table(const double* tt, const double* w, const double* wy, int32_t n, int n_series, const int32_t* off, int n_inst, double f,
                 const double* ecc, int n_ecc, int n_phase, int tile, double* table) {
  double* turns = new double[n];
  double* pairs = new double[(size_t)n * G * 2];
  for (int32_t i = 0; i < n; ++i) turns[i] = est::ls_phase_turns(f, tt[i]);
  const int n_cand = n_ecc * n_phase;
  for (int b0 = 0; b0 < n_series; b0 += G) {
    double totals[G * kTotals] = {}, W[G];
    for (int g = 0; g < G; ++g) {
      const int64_t b = group_series(b0, g, n_series);
      for (int32_t i = 0; i < n; ++i) {
        pairs[((size_t)i * G + g) * 2] = w[b * n + i];
        pairs[((size_t)i * G + g) * 2 + 1] = wy[b * n + i];
      }
      for (int k = 0; k < n_inst; ++k)
        for (int32_t i = off[k]; i < off[k + 1]; ++i) {
          totals[g * kTotals + 2 * k] += w[b * n + i];
          totals[g * kTotals + 2 * k + 1] += wy[b * n + i];
        }
      W[g] = total_weight(totals + g * kTotals, n_inst);
    }
    for (int c = 0; c < n_cand; ++c) {
      const Candidate cd = orb::candidate_of(c, n_cand, n_phase, ecc);
      GroupState<G> st = {};
      // (tile by tile, as the kernel stages them: the sums do not depend on the tile's length)
      if (cd.live)
        for (int32_t lo = 0; lo < n; lo += tile)
          group_walk<G>(st, cd, turns + lo, pairs + (size_t)lo * G * 2, totals, off, n_inst, lo, n - lo < tile ? n - lo : tile);
      for (int g = 0; g < G && b0 + g < n_series; ++g)
        table[(size_t)(b0 + g) * n_cand + c] = cd.live ? kep::fit(st.a[g], W[g]).power : -INFINITY;
    }
  }
  delete[] turns;
  delete[] pairs;
}

}  // namespace

extern "C" {

// -> 0, or -1 for a width that is not instantiated
int harness_group_table(int G, const double* tt, const double* w, const double* wy, int32_t n, int n_series, const int32_t* off,
                        int n_inst, double f, const double* ecc, int n_ecc, int n_phase, int tile, double* table) {
  switch (G) {
    case 4: group_table<4>(tt, w, wy, n, n_series, off, n_inst, f, ecc, n_ecc, n_phase, tile, table); return 0;
    case 8: group_table<8>(tt, w, wy, n, n_series, off, n_inst, f, ecc, n_ecc, n_phase, tile, table); return 0;
    case 16: group_table<16>(tt, w, wy, n, n_series, off, n_inst, f, ecc, n_ecc, n_phase, tile, table); return 0;
  }
  return -1;
}

int harness_tile() { return kTile; }

// the comparison of the arg-max on its own: (power, frequency, candidate) triples taken in the order given -> the survivor
void harness_best3(const double* power, const int32_t* frequency, const int32_t* candidate, int n, double* best_power, int32_t* best) {
  Best3 m = best3_init();
  for (int i = 0; i < n; ++i) best3_take(m, power[i], frequency[i], candidate[i]);
  *best_power = m.power;
  best[0] = m.frequency;
  best[1] = m.candidate;
}

}  // extern "C"
