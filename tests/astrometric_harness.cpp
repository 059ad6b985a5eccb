// Host build of exoplanet_amd/csrc/exo_astrometric_core.hpp for tests/test_astrometric_host.py (g++, no GPU): every
// candidate's thirteen sums, its scaled Cholesky solve and power, the arg-max and the winner's record, walked exactly as the
// kernel of exo_astrometric.hip walks them; and the Campbell conversion on its own.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_astrometric_core.hpp"
#include "orbit_lanes.hpp"

using namespace ast;
using namespace orb;

extern "C" {

// tt and the five columns pxx, pxy, pyy, qx, qy of the n epochs.  table[n_ecc * n_phase]: every candidate's power (-inf where
// there is none); pivot[n_ecc * n_phase]: its smallest squared pivot (NaN where the grid has none).  record[10]: power,
// candidate, TA, TB, TF, TG, a_angular, incl, omega, Omega of the winner (power 0, candidate -1, the rest NaN without one),
// found as n_lane lanes find it (each its strided share, then the reduction from the LAST lane down, so that the tie rule
// decides).
void harness_astrometric(const double* tt, const double* pxx, const double* pxy, const double* pyy, const double* qx, const double* qy,
                         int32_t n, double f, const double* ecc, int n_ecc, int n_phase, int n_lane, double* table, double* pivot,
                         double* record) {
  double* turns = new double[n];
  for (int32_t i = 0; i < n; ++i) turns[i] = est::ls_phase_turns(f, tt[i]);
  const int n_cand = n_ecc * n_phase;
  Fit* fits = new Fit[n_cand];
  for (int c = 0; c < n_cand; ++c) {
    const Candidate cd = candidate_of(c, n_cand, n_phase, ecc);
    table[c] = -INFINITY;
    pivot[c] = NAN;
    fits[c].ok = false;
    if (!cd.live) continue;
    Sums a = sums_init();
    for (int32_t i = 0; i < n; ++i) {
      double xi, eta;
      orbit_plane(turns[i], cd.phi, cd.e, cd.se, cd.pe, &xi, &eta);
      accumulate(a, xi, eta, pxx[i], pxy[i], pyy[i], qx[i], qy[i]);
    }
    fits[c] = fit(a);
    pivot[c] = fits[c].pivot;
    if (fits[c].ok) table[c] = fits[c].power;
  }
  const Best best = lanes_best(
      n_cand, n_lane, [&](int c) { return fits[c].ok; }, [&](int c) { return table[c]; });
  record[0] = 0.0;
  record[1] = -1.0;
  for (int q = 2; q < 10; ++q) record[q] = NAN;
  if (best.candidate != INT32_MAX) {
    const Fit& r = fits[best.candidate];
    const Elements el = campbell(r.ta, r.tb, r.tf, r.tg);
    record[0] = r.power;
    record[1] = (double)best.candidate;
    record[2] = r.ta;
    record[3] = r.tb;
    record[4] = r.tf;
    record[5] = r.tg;
    record[6] = el.a_angular;
    record[7] = el.incl;
    record[8] = el.omega;
    record[9] = el.Omega;
  }
  delete[] fits;
  delete[] turns;
}

// beta[n][4] -> out[n][4] = a_angular, incl, omega, Omega
void harness_campbell(const double* beta, int n, double* out) {
  for (int i = 0; i < n; ++i) {
    const Elements el = campbell(beta[4 * i], beta[4 * i + 1], beta[4 * i + 2], beta[4 * i + 3]);
    out[4 * i] = el.a_angular;
    out[4 * i + 1] = el.incl;
    out[4 * i + 2] = el.omega;
    out[4 * i + 3] = el.Omega;
  }
}

}  // extern "C"
