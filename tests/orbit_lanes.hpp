// The arg-max of an orbit search as n_lane lanes of a kernel find it (exoplanet_amd/csrc/exo_orbit_search.hpp: lane_search, then
// block_best), restated for the host harnesses: each lane its strided share of the candidates, ascending, then the reduction
// from the LAST lane down, so that the tie rule decides.  counts(c): c is a candidate with a power; power(c): that power.
#pragma once
#include "../exoplanet_amd/csrc/exo_orbit_search.hpp"

template <class Counts, class Power>
inline orb::Best lanes_best(int n_cand, int n_lane, Counts counts, Power power) {
  orb::Best best = orb::best_init();
  for (int lane = n_lane - 1; lane >= 0; --lane) {
    orb::Best mine = orb::best_init();
    for (int c = lane; c < n_cand; c += n_lane)
      if (counts(c)) orb::best_take(mine, power(c), c);
    orb::best_take(best, mine.power, mine.candidate);
  }
  return best;
}
