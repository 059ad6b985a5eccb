// exo_astrometry.hip -- Gaussian log-likelihood of an observed astrometric series (separation and position angle of one
// companion) for n_draw parameter sets, value and every gradient in one launch (exo_astrometry_loglike_vjp_f64; definitions:
// include/exoplanet_amd.h).
//
// The reason of exo_rv_like.hip for the third series of the reference's tutorials: tens to hundreds of epochs, so the launches
// are the cost, and on top of the one launch of the position vectors the tutorial's model (sqrt, atan2, the wrap of the angle
// difference through sin / cos / atan2, two Normal log-densities with their jitters) was about twenty launch-bound torch
// kernels and their reverse.  Here: one workgroup per draw, lanes striding over the epochs, no workspace, ONE pass -- with one
// companion the residual of an epoch needs no sum over planets, so the epoch's cotangent is known as soon as its position is,
// and the reverse arithmetic (ov_vjp_term<0>) follows in the same iteration on the same Kepler solve.  16 lane accumulators
// (exo_astrometry_core.hpp), a shuffle tree per wave, then one thread per slot adds the waves in turn.  Every sum has a fixed
// order and nothing is atomic: the results are bit-reproducible.  The workgroup is one wave up to kNarrowCad epochs and four
// above -- chosen from n_cad alone, so a draw's results do not depend on the batch it is in.
// Resources and timings: DESIGN.md section 14.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_astrometry_core.hpp"

namespace {

using namespace exo::ast;

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void astrometry_loglike_kernel(
    const double* __restrict__ t, const double* __restrict__ rho, const double* __restrict__ cos_theta,
    const double* __restrict__ sin_theta, const double* __restrict__ var_rho, int one_var_rho, const double* __restrict__ var_theta,
    int one_var_theta, int64_t n_cad, const double* __restrict__ params, const double* __restrict__ jit2_rho,
    const double* __restrict__ jit2_theta, double* __restrict__ loglike, double* __restrict__ gparams,
    double* __restrict__ gjit2_rho, double* __restrict__ gjit2_theta) {
  constexpr int kWaves = BLOCK / kWave;
  __shared__ double red[kWaves][kSlots];
  const int64_t d = blockIdx.x;
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const double* __restrict__ rec = params + d * EXO_OV_NPAR;
  const double jr = jit2_rho ? jit2_rho[d] : 0.0, jt = jit2_theta ? jit2_theta[d] : 0.0;
  Acc acc;
  acc_zero(acc);
  if (gparams) {
    for (int64_t i = tid; i < n_cad; i += BLOCK)
      epoch_add<true>(acc, t[i], rec, rho[i], cos_theta[i], sin_theta[i], var_rho[one_var_rho ? 0 : i] + jr,
                      var_theta[one_var_theta ? 0 : i] + jt);
  } else {
    for (int64_t i = tid; i < n_cad; i += BLOCK)
      epoch_add<false>(acc, t[i], rec, rho[i], cos_theta[i], sin_theta[i], var_rho[one_var_rho ? 0 : i] + jr,
                       var_theta[one_var_theta ? 0 : i] + jt);
  }
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    const double s = wave_sum(acc.v[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (tid >= kSlots) return;
  if (tid == 0) {
    double v[4];      // kChiR, kLogR, kChiT, kLogT
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.0;
      for (int w = 0; w < kWaves; ++w) v[k] += red[w][k];
    }
    loglike[d] = loglike_from(v[kChiR], v[kLogR], v[kChiT], v[kLogT], n_cad);
    return;
  }
  if (tid < kRec) return;
  double v = 0.0;
  for (int w = 0; w < kWaves; ++w) v += red[w][tid];
  if (tid < kJitR) {
    if (gparams) gparams[d * EXO_OV_NPAR + (tid - kRec)] = v;
  } else if (tid == kJitR) {
    if (gjit2_rho) gjit2_rho[d] = 0.5 * v;
  } else {
    if (gjit2_theta) gjit2_theta[d] = 0.5 * v;
  }
}

}  // namespace

extern "C" {

int exo_astrometry_loglike_vjp_f64(const double* t, const double* rho, const double* cos_theta, const double* sin_theta,
                                   const double* var_rho, int64_t n_var_rho, const double* var_theta, int64_t n_var_theta,
                                   int64_t n_cad, const double* params, int64_t n_draw, const double* jit2_rho,
                                   const double* jit2_theta, double* loglike, double* gparams, double* gjit2_rho,
                                   double* gjit2_theta, void* stream) {
  if (n_cad < 0 || n_draw < 0 || n_draw > 0x7fffffff || (n_var_rho != 1 && n_var_rho != n_cad) ||
      (n_var_theta != 1 && n_var_theta != n_cad))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!params || !loglike) return EXO_ERR_INVALID_ARGUMENT;
  if (n_cad > 0 && (!t || !rho || !cos_theta || !sin_theta || !var_rho || !var_theta)) return EXO_ERR_INVALID_ARGUMENT;
  const int one_r = n_var_rho == 1 ? 1 : 0, one_t = n_var_theta == 1 ? 1 : 0;      // (n_cad == 1: either reading is the same element)
  hipStream_t st = (hipStream_t)stream;
  if (block_threads(n_cad) == kNarrow)
    hipLaunchKernelGGL(astrometry_loglike_kernel<kNarrow>, dim3((unsigned)n_draw), dim3(kNarrow), 0, st, t, rho, cos_theta,
                       sin_theta, var_rho, one_r, var_theta, one_t, n_cad, params, jit2_rho, jit2_theta, loglike, gparams,
                       gjit2_rho, gjit2_theta);
  else
    hipLaunchKernelGGL(astrometry_loglike_kernel<kWide>, dim3((unsigned)n_draw), dim3(kWide), 0, st, t, rho, cos_theta,
                       sin_theta, var_rho, one_r, var_theta, one_t, n_cad, params, jit2_rho, jit2_theta, loglike, gparams,
                       gjit2_rho, gjit2_theta);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
