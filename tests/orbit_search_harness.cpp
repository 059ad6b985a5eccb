// Host build of exoplanet_amd/csrc/exo_orbit_search.hpp for tests/test_orbit_search_host.py (g++, no GPU): the parts of the
// orbit searches that are neither search's own -- the candidate grid, the arg-max over lanes, and what an entry point checks and
// chooses on the host.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_orbit_search.hpp"
#include "orbit_lanes.hpp"

using namespace orb;

extern "C" {

int harness_threads_for(int64_t n_cand) { return threads_for(n_cand); }

// out[4] = e, se, pe, phi of candidate c; -> whether it is live
int harness_candidate_of(int c, int n_cand, int n_phase, const double* ecc, double* out) {
  const Candidate cd = candidate_of(c, n_cand, n_phase, ecc);
  out[0] = cd.e;
  out[1] = cd.se;
  out[2] = cd.pe;
  out[3] = cd.phi;
  return cd.live;
}

// -> whether the grid is accepted; copy[n_ecc] = what travels to the kernel of an accepted one
int harness_ecc_grid(const double* ecc, int n_ecc, double* copy) {
  EccGrid grid = {};
  if (!ecc_grid(ecc, n_ecc, &grid)) return 0;
  for (int j = 0; j < grid.n; ++j) copy[j] = grid.e[j];
  return 1;
}

int harness_sizes_ok(int64_t n, int64_t n_series, int64_t n_frequency, int32_t n_ecc, int32_t n_phase) {
  return sizes_ok(n, n_series, n_frequency, n_ecc, n_phase);
}

// the winner of a table of powers (counts[c] != 0: c is a candidate) as n_lane lanes find it; INT32_MAX: none
int32_t harness_lanes_best(const double* power, const int32_t* counts, int n_cand, int n_lane) {
  return lanes_best(
             n_cand, n_lane, [&](int c) { return counts[c] != 0; }, [&](int c) { return power[c]; })
      .candidate;
}

}  // extern "C"
