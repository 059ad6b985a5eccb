// exo_rv_like.hip -- Gaussian log-likelihood of an observed radial-velocity series for n_draw parameter sets, value and
// every gradient in one launch (exo_rv_loglike_vjp_f64; definitions: include/exoplanet_amd.h).
//
// The reason of exo_rv.hip carried one level up: a radial-velocity series is tens to a few thousand epochs, so the launches
// are the cost, and on top of the one forward launch the tutorials' model (zero point, trend, jitter, pm.Normal) was a dozen
// launch-bound torch kernels and their reverse.  Here: one workgroup per draw, lanes striding over the epochs, no workspace.
//   pass A (a tile of kTile epochs): m, rho, w; rho stays in LDS; the value and the trend / zero-point / jitter sums go to
//           lane accumulators that persist across the tiles;
//   pass B (the same tile): the planets in turn, six lane accumulators, the Kepler solve done again (rv_vjp_term with
//           cotangent rho); a shuffle tree per wave, whose lane 0 adds the six sums to the wave's slots in LDS -- tile after
//           tile, so those persist across the tiles too.
//   end:    a shuffle tree per wave for the pass-A sums, then one thread per slot adds the waves in turn.
// Every sum has a fixed order and nothing is atomic: the results are bit-reproducible.  The workgroup is one wave up to
// kNarrowCad epochs and four above -- chosen from n_cad alone, so a draw's results do not depend on the batch it is in.
// A lane reads back only the rho it stored itself (same stride in both passes): no barrier between the passes.
// Resources and timings: DESIGN.md section 12.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_rv_like_core.hpp"

namespace {

using namespace exo::rvl;

constexpr int kSlots = kScalars + EXO_MAX_PLANETS * EXO_RV_NPAR;

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void rv_loglike_kernel(
    const double* __restrict__ t, const double* __restrict__ tau, const int32_t* __restrict__ inst, const double* __restrict__ rv,
    const double* __restrict__ var, int64_t n_cad, int one_var, const double* __restrict__ params, int n_planet,
    const double* __restrict__ trend, int n_trend, const double* __restrict__ offset, const double* __restrict__ jit2, int n_inst,
    double* __restrict__ loglike, double* __restrict__ gparams, double* __restrict__ gtrend, double* __restrict__ goffset,
    double* __restrict__ gjit2) {
  constexpr int kWaves = BLOCK / kWave;
  __shared__ double rho_s[kTile];
  __shared__ double red[kWaves][kSlots];
  const int64_t d = blockIdx.x;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const double* __restrict__ recs = params + d * n_planet * EXO_RV_NPAR;
  const double* __restrict__ trend_d = n_trend > 0 ? trend + d * n_trend : nullptr;
  const double* __restrict__ off_d = offset ? offset + d * n_inst : nullptr;
  const double* __restrict__ jit_d = jit2 ? jit2 + d * n_inst : nullptr;
  const int n_gp = n_planet * EXO_RV_NPAR;
  for (int s = lane; s < n_gp; s += kWave) red[wave][kScalars + s] = 0.0;
  __syncthreads();
  const double nan = __builtin_nan("");
  Acc acc;
  acc_zero(acc);
  for (int64_t t0 = 0; t0 < n_cad; t0 += kTile) {
    const int64_t t1 = t0 + kTile < n_cad ? t0 + kTile : n_cad;
    for (int64_t i = t0 + tid; i < t1; i += BLOCK) {
      const int ii = inst ? inst[i] : 0;
      const bool ok = (unsigned)ii < (unsigned)n_inst;      // an index outside the table: NaN, never a read outside it
      const int ic = ok ? ii : 0;
      const double off = ok ? (off_d ? off_d[ic] : 0.0) : nan;
      const double s2 = var[one_var ? 0 : i] + (jit_d ? jit_d[ic] : 0.0);
      const double tu = tau ? tau[i] : 0.0;
      const double m = model(t[i], tu, recs, n_planet, trend_d, n_trend, off);
      rho_s[i - t0] = epoch_add(acc, rv[i], m, s2, tu, n_trend, ok ? ii : -1);
    }
    if (gparams) {
      for (int p = 0; p < n_planet; ++p) {
        const double* __restrict__ rec = recs + p * EXO_RV_NPAR;
        double g[EXO_RV_NPAR];
#pragma unroll
        for (int k = 0; k < EXO_RV_NPAR; ++k) g[k] = 0.0;
        for (int64_t i = t0 + tid; i < t1; i += BLOCK) exo::rv_vjp_term(t[i], rec, rho_s[i - t0], g);
#pragma unroll
        for (int k = 0; k < EXO_RV_NPAR; ++k) {
          const double s = wave_sum(g[k]);
          if (lane == 0) red[wave][kScalars + p * EXO_RV_NPAR + k] += s;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kScalars; ++k) {
    const double s = wave_sum(acc.v[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  for (int s = tid; s < kScalars + n_gp; s += BLOCK) {
    if (s == kLog) continue;      // (taken with kChi)
    double v = 0.0;
    for (int w = 0; w < kWaves; ++w) v += red[w][s];
    if (s == kChi) {
      double lg = 0.0;
      for (int w = 0; w < kWaves; ++w) lg += red[w][kLog];
      loglike[d] = loglike_from(v, lg, n_cad);
    } else if (s < kOff) {
      if (gtrend && s - kTrend < n_trend) gtrend[d * n_trend + (s - kTrend)] = v;
    } else if (s < kJit) {
      if (goffset && s - kOff < n_inst) goffset[d * n_inst + (s - kOff)] = v;
    } else if (s < kScalars) {
      if (gjit2 && s - kJit < n_inst) gjit2[d * n_inst + (s - kJit)] = 0.5 * v;
    } else if (gparams) {
      gparams[d * n_gp + (s - kScalars)] = v;
    }
  }
}

}  // namespace

extern "C" {

int exo_rv_loglike_vjp_f64(const double* t, const double* tau, const int32_t* inst, const double* rv, const double* var,
                           int64_t n_cad, int64_t n_var, const double* params, int64_t n_draw, int32_t n_planet,
                           const double* trend, int32_t n_trend, const double* offset, const double* jit2, int32_t n_inst,
                           double* loglike, double* gparams, double* gtrend, double* goffset, double* gjit2, void* stream) {
  if (n_cad < 0 || n_draw < 0 || n_draw > 0x7fffffff || n_planet < 1 || n_planet > EXO_MAX_PLANETS || n_trend < 0 ||
      n_trend > EXO_RV_MAX_TREND || n_inst < 1 || n_inst > EXO_RV_MAX_INST || (n_var != 1 && n_var != n_cad))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!params || !loglike || (n_trend > 0 && !trend)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_cad > 0 && (!t || !rv || !var || (n_trend > 1 && !tau) || (n_inst > 1 && !inst))) return EXO_ERR_INVALID_ARGUMENT;
  const int one_var = n_var == 1 ? 1 : 0;      // (n_cad == 1: either reading is the same element)
  hipStream_t st = (hipStream_t)stream;
  if (block_threads(n_cad) == kNarrow)
    hipLaunchKernelGGL(rv_loglike_kernel<kNarrow>, dim3((unsigned)n_draw), dim3(kNarrow), 0, st, t, tau, inst, rv, var, n_cad,
                       one_var, params, n_planet, trend, n_trend, offset, jit2, n_inst, loglike, gparams, gtrend, goffset, gjit2);
  else
    hipLaunchKernelGGL(rv_loglike_kernel<kWide>, dim3((unsigned)n_draw), dim3(kWide), 0, st, t, tau, inst, rv, var, n_cad,
                       one_var, params, n_planet, trend, n_trend, offset, jit2, n_inst, loglike, gparams, gtrend, goffset, gjit2);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
