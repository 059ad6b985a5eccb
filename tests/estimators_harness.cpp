// Host build of exoplanet_amd/csrc/exo_estimators_core.hpp for tests/test_estimators_host.py (g++, no GPU): the bin index, the
// search over prefix sums with its arg-max, and the closed-form Lomb-Scargle power, exactly as the kernels call them.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_estimators_core.hpp"

using namespace est;

extern "C" {

int64_t harness_n_bins(double p, double delta, int oversample) { return bls_n_bins(p, delta, oversample); }

void harness_bin_index(const double* tt, int64_t n, double p, double delta, int64_t n_bins, int64_t* out) {
  const double inv_p = 1.0 / p, inv_delta = 1.0 / delta;
  for (int64_t i = 0; i < n; ++i) out[i] = bls_bin_index(tt[i], p, inv_p, delta, inv_delta, n_bins);
}

// the search as n_lane lanes run it (each its strided share, then the reduction, here from the LAST lane down so that the
// tie rule, not the order of the comparisons, decides), and the seven outputs
void harness_bls_search(const double* cy, const double* cw, int64_t n_bins, const int32_t* m, int n_dur, double Y, double W,
                        int objective, double p, double delta, double t_min, int64_t n_lane, double* out) {
  BlsBest best = bls_best_init();
  for (int64_t lane = n_lane - 1; lane >= 0; --lane) {
    const BlsBest b = bls_search(cy, cw, n_bins, m, n_dur, Y, W, objective, lane, n_lane);
    bls_best_take(best, b.obj, b.key);
  }
  bls_outputs(cy, cw, n_bins, m, Y, W, objective, best, p, delta, t_min, out, 1);
}

void harness_ls_sums(const double* t, const double* w, const double* wy, int64_t n, double f, double kappa, double* sums) {
  LsSums a{0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const double x = 2.0 * M_PI * ls_phase_turns(f, t[i]);
    ls_accumulate(a, w[i], wy[i], sin(x), cos(x), kappa);
  }
  sums[0] = a.ys, sums[1] = a.yc, sums[2] = a.s, sums[3] = a.c, sums[4] = a.ss, sums[5] = a.cc, sums[6] = a.sc;
}

double harness_ls_power(const double* s, double W, double Y) { return ls_power(LsSums{s[0], s[1], s[2], s[3], s[4], s[5], s[6]}, W, Y); }

double harness_ls_kappa(double f, double T) { return ls_kappa(f, T); }

}  // extern "C"
