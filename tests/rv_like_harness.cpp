// Host build of exoplanet_amd/csrc/exo_rv_like_core.hpp for tests/test_rv_like_host.py: one draw of exo_rv_loglike_vjp_f64
// with the kernel's per-epoch arithmetic and the kernel's order of summation (rv_loglike_kernel of exo_rv_like.hip: lanes
// striding over a tile of epochs, the planets in turn, a shuffle tree per wave, the tiles and then the waves in turn),
// without a GPU.
#define EXO_HOST_BUILD 1
#include "../exoplanet_amd/csrc/exo_rv_like_core.hpp"

#include <stdint.h>

#include <vector>

using namespace exo::rvl;

// lane 0 of the tree `for o = 32 .. 1: v += shuffle_down(v, o)`
static double wave_tree(const double* lanes) {
  double v[kWave];
  for (int l = 0; l < kWave; ++l) v[l] = lanes[l];
  for (int o = kWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) v[l] += v[l + o];
  return v[0];
}

extern "C" {

int harness_tile() { return kTile; }
int harness_block_threads(int64_t n_cad) { return block_threads(n_cad); }
int harness_max_trend() { return EXO_RV_MAX_TREND; }
int harness_max_inst() { return EXO_RV_MAX_INST; }

// the arrays of ONE draw: recs [n_planet][6], trend [n_trend], offset / jit2 [n_inst] or null
void harness_draw(const double* t, const double* tau, const int32_t* inst, const double* rv, const double* var, int64_t n_cad,
                  int64_t n_var, const double* recs, int n_planet, const double* trend, int n_trend, const double* offset,
                  const double* jit2, int n_inst, double* loglike, double* gparams, double* gtrend, double* goffset,
                  double* gjit2) {
  const int block = block_threads(n_cad), n_wave = block / kWave, n_gp = n_planet * EXO_RV_NPAR;
  const double nan = __builtin_nan("");
  std::vector<Acc> acc(block);
  for (Acc& a : acc) acc_zero(a);
  std::vector<double> rho(kTile), red_gp((size_t)n_wave * n_gp, 0.0), g((size_t)block * EXO_RV_NPAR);
  for (int64_t t0 = 0; t0 < n_cad; t0 += kTile) {
    const int64_t t1 = t0 + kTile < n_cad ? t0 + kTile : n_cad;
    for (int64_t i = t0; i < t1; ++i) {
      const int ii = inst ? inst[i] : 0;
      const bool ok = (unsigned)ii < (unsigned)n_inst;
      const int ic = ok ? ii : 0;
      const double off = ok ? (offset ? offset[ic] : 0.0) : nan;
      const double s2 = var[n_var == 1 ? 0 : i] + (jit2 ? jit2[ic] : 0.0);
      const double tu = tau ? tau[i] : 0.0;
      const double m = model(t[i], tu, recs, n_planet, trend, n_trend, off);
      rho[i - t0] = epoch_add(acc[(i - t0) % block], rv[i], m, s2, tu, n_trend, ok ? ii : -1);
    }
    for (int p = 0; p < n_planet; ++p) {
      for (double& x : g) x = 0.0;
      for (int64_t i = t0; i < t1; ++i) exo::rv_vjp_term(t[i], recs + p * EXO_RV_NPAR, rho[i - t0], &g[((i - t0) % block) * EXO_RV_NPAR]);
      for (int w = 0; w < n_wave; ++w)
        for (int k = 0; k < EXO_RV_NPAR; ++k) {
          double lanes[kWave];
          for (int l = 0; l < kWave; ++l) lanes[l] = g[(size_t)(w * kWave + l) * EXO_RV_NPAR + k];
          red_gp[(size_t)w * n_gp + p * EXO_RV_NPAR + k] += wave_tree(lanes);
        }
    }
  }
  double sums[kScalars];
  for (int k = 0; k < kScalars; ++k) {
    sums[k] = 0.0;
    for (int w = 0; w < n_wave; ++w) {
      double lanes[kWave];
      for (int l = 0; l < kWave; ++l) lanes[l] = acc[w * kWave + l].v[k];
      sums[k] += wave_tree(lanes);
    }
  }
  *loglike = loglike_from(sums[kChi], sums[kLog], n_cad);
  for (int k = 0; k < n_trend; ++k) gtrend[k] = sums[kTrend + k];
  for (int i = 0; i < n_inst; ++i) {
    goffset[i] = sums[kOff + i];
    gjit2[i] = 0.5 * sums[kJit + i];
  }
  for (int s = 0; s < n_gp; ++s) {
    double v = 0.0;
    for (int w = 0; w < n_wave; ++w) v += red_gp[(size_t)w * n_gp + s];
    gparams[s] = v;
  }
}

}  // extern "C"
