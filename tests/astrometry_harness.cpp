// Host build of exoplanet_amd/csrc/exo_astrometry_core.hpp for tests/test_astrometry_host.py: one draw of
// exo_astrometry_loglike_vjp_f64 with the kernel's per-epoch arithmetic and the kernel's order of summation
// (astrometry_loglike_kernel of exo_astrometry.hip: lanes striding over the epochs in a single pass, a shuffle tree per wave,
// then the waves in turn), without a GPU.
#define EXO_HOST_BUILD 1
#include "../exoplanet_amd/csrc/exo_astrometry_core.hpp"

#include <stdint.h>

#include <vector>

using namespace exo::ast;

// lane 0 of the tree `for o = 32 .. 1: v += shuffle_down(v, o)`
static double wave_tree(const double* lanes) {
  double v[kWave];
  for (int l = 0; l < kWave; ++l) v[l] = lanes[l];
  for (int o = kWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) v[l] += v[l + o];
  return v[0];
}

extern "C" {

int harness_narrow_cad() { return kNarrowCad; }
int harness_narrow() { return kNarrow; }
int harness_wide() { return kWide; }
int harness_slots() { return kSlots; }
int harness_block_threads(int64_t n_cad) { return block_threads(n_cad); }

// the arrays of ONE draw: rec [10]; jit2_rho / jit2_theta: the draw's value (0.0 for a null pointer)
void harness_draw(const double* t, const double* rho, const double* cos_theta, const double* sin_theta, const double* var_rho,
                  int64_t n_var_rho, const double* var_theta, int64_t n_var_theta, int64_t n_cad, const double* rec,
                  double jit2_rho, double jit2_theta, int with_rec, double* loglike, double* gparams, double* gjit2_rho,
                  double* gjit2_theta) {
  const int block = block_threads(n_cad), n_wave = block / kWave;
  std::vector<Acc> acc(block);
  for (Acc& a : acc) acc_zero(a);
  for (int64_t i = 0; i < n_cad; ++i) {
    const double s2r = var_rho[n_var_rho == 1 ? 0 : i] + jit2_rho, s2t = var_theta[n_var_theta == 1 ? 0 : i] + jit2_theta;
    if (with_rec)
      epoch_add<true>(acc[i % block], t[i], rec, rho[i], cos_theta[i], sin_theta[i], s2r, s2t);
    else
      epoch_add<false>(acc[i % block], t[i], rec, rho[i], cos_theta[i], sin_theta[i], s2r, s2t);
  }
  double sums[kSlots];
  for (int k = 0; k < kSlots; ++k) {
    sums[k] = 0.0;
    for (int w = 0; w < n_wave; ++w) {
      double lanes[kWave];
      for (int l = 0; l < kWave; ++l) lanes[l] = acc[w * kWave + l].v[k];
      sums[k] += wave_tree(lanes);
    }
  }
  *loglike = loglike_from(sums[kChiR], sums[kLogR], sums[kChiT], sums[kLogT], n_cad);
  if (with_rec)
    for (int k = 0; k < EXO_OV_NPAR; ++k) gparams[k] = sums[kRec + k];
  *gjit2_rho = 0.5 * sums[kJitR];
  *gjit2_theta = 0.5 * sums[kJitT];
}

}  // extern "C"
