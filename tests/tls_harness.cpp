// Host build of the template search of exoplanet_amd/csrc/exo_estimators_core.hpp for tests/test_tls_host.py (g++, no GPU):
// one window, and the search over a histogram with its arg-max and outputs, exactly as the kernels call them.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_estimators_core.hpp"

using namespace est;

extern "C" {

// out: A, B, C, w_in, D, depth, depth_err, depth_snr, log_likelihood, ok
void harness_tls_window(const double* hy, const double* hw, const double* g, int64_t s, int64_t mk, double Y, double W,
                        double* out) {
  const TlsWindow w = tls_window(hy, hw, g, s, mk, Y, W);
  out[0] = w.A, out[1] = w.B, out[2] = w.C, out[3] = w.w_in, out[4] = w.D, out[5] = w.depth, out[6] = w.depth_err;
  out[7] = w.depth_snr, out[8] = w.log_likelihood, out[9] = w.ok ? 1.0 : 0.0;
}

// the search as n_lane lanes run it (each its strided share, then the reduction from the LAST lane down, so that the tie rule
// and not the order of the comparisons decides), and the seven outputs
void harness_tls_search(const double* hy, const double* hw, int64_t n_bins, const int32_t* m, const int32_t* off, int n_dur,
                        const double* g, double Y, double W, int objective, double p, double delta, double t_min, int64_t n_lane,
                        double* out) {
  BlsBest best = bls_best_init();
  for (int64_t lane = n_lane - 1; lane >= 0; --lane) {
    const BlsBest b = tls_search(hy, hw, n_bins, m, off, n_dur, g, Y, W, objective, lane, n_lane);
    bls_best_take(best, b.obj, b.key);
  }
  tls_outputs(hy, hw, n_bins, m, off, g, Y, W, objective, best, p, delta, t_min, out, 1);
}

// the box search on the prefix sums of the same histogram (the g = 1 properties)
void harness_box_search(const double* cy, const double* cw, int64_t n_bins, const int32_t* m, int n_dur, double Y, double W,
                        int objective, double p, double delta, double t_min, double* out) {
  const BlsBest best = bls_search(cy, cw, n_bins, m, n_dur, Y, W, objective, 0, 1);
  bls_outputs(cy, cw, n_bins, m, Y, W, objective, best, p, delta, t_min, out, 1);
}

}  // extern "C"
