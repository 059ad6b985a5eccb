// exo_rv.hip -- stellar reflex radial velocity from the same Kepler solve (gfx950).
//
// Reference (all under /root/reference/src/exoplanet/orbits/keplerian.py):
//   :633-677  get_radial_velocity: with K,   K (cos w cos f - sin w sin f + e cos w)   (:660-669)
//                                  circular: K cos f                                    (:658-659)
//             without K:           -conv * z-velocity of the star                       (:671-676)
//   :572-578  _get_velocity, :283-322 _rotate_vector: the z-velocity of the star is
//             -sin(i) K0 m_planet (cos w (cos f + e) - sin w sin f) -- the same function of f with
//             another amplitude, so one kernel serves both forms.
//   :329-334  M = (t - t_periastron) n ; kepler(M, e)
//
// A radial-velocity series is a few hundred to a few thousand epochs: the work is nothing, the
// ~20 launch-bound torch kernels of the composed path (M, Kepler op, rotations, broadcasts, and
// their reverse) were as long as a whole light-curve sweep.  One launch forward, one reverse.
//   rv[d][n][p] = amp[d][p] * (cw (cos f + e) - sw sin f),   f = f(M = (t_n - tp) nn, e)
// Reverse: one block per (draw, planet); lanes stride over the epochs, partial sums in
// registers, one fixed-order LDS reduction (bit-reproducible).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_rv_core.hpp"     // the per-sample arithmetic: rv_sample, ov_sample, rv_vjp_term, ov_vjp_term

namespace {

using exo::OvSample;
using exo::ov_sample;
using exo::rv_sample;

constexpr int kRvBlock = 256;

__global__ __launch_bounds__(kRvBlock) void rv_fwd_kernel(const double* __restrict__ t, int64_t n_cad,
                                                          const double* __restrict__ params, int64_t n_draw,
                                                          int n_planet, double* __restrict__ rv) {
  const int64_t total = n_draw * n_cad * n_planet;
  const int64_t stride = (int64_t)gridDim.x * kRvBlock;
  for (int64_t i = (int64_t)blockIdx.x * kRvBlock + threadIdx.x; i < total; i += stride) {
    const int p = (int)(i % n_planet);
    const int64_t dn = i / n_planet;
    const int64_t n = dn % n_cad, d = dn / n_cad;
    const double* __restrict__ rec = params + (d * n_planet + p) * EXO_RV_NPAR;
    rv[i] = rec[EXO_RV_AMP] * rv_sample(t[n], rec).g;
  }
}

__global__ __launch_bounds__(kRvBlock) void rv_vjp_kernel(const double* __restrict__ t, int64_t n_cad,
                                                          const double* __restrict__ params, int n_planet,
                                                          const double* __restrict__ grv,
                                                          double* __restrict__ gparams) {
  const int64_t rec_i = blockIdx.x;   // draw * n_planet + planet
  const int64_t d = rec_i / n_planet;
  const int p = (int)(rec_i - d * n_planet);
  const double* __restrict__ rec = params + rec_i * EXO_RV_NPAR;
  double acc[EXO_RV_NPAR];
#pragma unroll
  for (int k = 0; k < EXO_RV_NPAR; ++k) acc[k] = 0.0;
  for (int64_t n = threadIdx.x; n < n_cad; n += kRvBlock)
    exo::rv_vjp_term(t[n], rec, grv[(d * n_cad + n) * n_planet + p], acc);
  // fixed-order reduction: thread (slot, c) adds 16 columns, then one thread per slot the 16 partials
  __shared__ double cols[EXO_RV_NPAR][kRvBlock];
  __shared__ double part[EXO_RV_NPAR][16];
#pragma unroll
  for (int k = 0; k < EXO_RV_NPAR; ++k) cols[k][threadIdx.x] = acc[k];
  __syncthreads();
  const int slot = threadIdx.x >> 4, c = threadIdx.x & 15;
  if (slot < EXO_RV_NPAR) {
    double v = 0.0;
    for (int i = 0; i < kRvBlock / 16; ++i) v += cols[slot][c + 16 * i];
    part[slot][c] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < EXO_RV_NPAR) {
    double v = 0.0;
    for (int i = 0; i < 16; ++i) v += part[threadIdx.x][i];
    gparams[rec_i * EXO_RV_NPAR + threadIdx.x] = v;
  }
}

// ---------------------------------------------------------------------------------------------
// Position / velocity vectors in the observer frame from the same solve (keplerian.py:380-409 _get_position,
// :572-578 _get_velocity, :283-322 _rotate_vector): what get_{star,planet,relative}_{position,velocity} and
// get_relative_angles (astrometry, :544-570) are made of.  In the orbital plane
//     position:  (u, v) = (1 - e^2) / (1 + e cos f) (cos f, sin f)        velocity:  (u, v) = (-sin f, cos f + e)
//     acceleration (:679-706):  (u, v) = -(1 + e cos f)^2 / (1 - e^2) (cos f, sin f)
// times an amplitude (a_star, a_planet, -a [x parallax au_per_R_sun]; K0 m; (K0 m)^2 / a), then the three rotations
//     x1 = cw u - sw v,  y1 = sw u + cw v;   x2 = x1,  y2 = ci y1,  Z = -si y1;   X = cO x2 - sO y2,  Y = sO x2 + cO y2.
// An astrometric or imaging series is tens of epochs: as for the radial velocities, the composed path's launch-bound
// torch kernels (solve, radius, three rotations, broadcasts, and their reverse: ~40) are the cost; here one launch
// each way.  out[d][n][p][3]; reverse: one block per (draw, planet), fixed-order reduction.
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(kRvBlock) void ov_fwd_kernel(const double* __restrict__ t, int64_t n_cad,
                                                          const double* __restrict__ params, int64_t n_draw,
                                                          int n_planet, double* __restrict__ out) {
  const int64_t total = n_draw * n_cad * n_planet;
  const int64_t stride = (int64_t)gridDim.x * kRvBlock;
  for (int64_t i = (int64_t)blockIdx.x * kRvBlock + threadIdx.x; i < total; i += stride) {
    const int p = (int)(i % n_planet);
    const int64_t dn = i / n_planet;
    const int64_t n = dn % n_cad, d = dn / n_cad;
    const double* __restrict__ rec = params + (d * n_planet + p) * EXO_OV_NPAR;
    const OvSample s = ov_sample<MODE>(t[n], rec);
    const double a = rec[EXO_OV_AMP];
    out[3 * i] = a * s.X; out[3 * i + 1] = a * s.Y; out[3 * i + 2] = a * s.Z;
  }
}

template <int MODE>
__global__ __launch_bounds__(kRvBlock) void ov_vjp_kernel(const double* __restrict__ t, int64_t n_cad,
                                                          const double* __restrict__ params, int n_planet,
                                                          const double* __restrict__ gout,
                                                          double* __restrict__ gparams) {
  const int64_t rec_i = blockIdx.x;   // draw * n_planet + planet
  const int64_t d = rec_i / n_planet;
  const int p = (int)(rec_i - d * n_planet);
  const double* __restrict__ rec = params + rec_i * EXO_OV_NPAR;
  double acc[EXO_OV_NPAR];
#pragma unroll
  for (int k = 0; k < EXO_OV_NPAR; ++k) acc[k] = 0.0;
  for (int64_t n = threadIdx.x; n < n_cad; n += kRvBlock) {
    const double* __restrict__ g = gout + 3 * ((d * n_cad + n) * n_planet + p);
    exo::ov_vjp_term<MODE>(t[n], rec, g[0], g[1], g[2], acc);
  }
  // fixed-order reduction, as in rv_vjp_kernel
  __shared__ double cols[EXO_OV_NPAR][kRvBlock];
  __shared__ double part[EXO_OV_NPAR][16];
#pragma unroll
  for (int k = 0; k < EXO_OV_NPAR; ++k) cols[k][threadIdx.x] = acc[k];
  __syncthreads();
  const int slot = threadIdx.x >> 4, c = threadIdx.x & 15;
  if (slot < EXO_OV_NPAR) {
    double v = 0.0;
    for (int i = 0; i < kRvBlock / 16; ++i) v += cols[slot][c + 16 * i];
    part[slot][c] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < EXO_OV_NPAR) {
    double v = 0.0;
    for (int i = 0; i < 16; ++i) v += part[threadIdx.x][i];
    gparams[rec_i * EXO_OV_NPAR + threadIdx.x] = v;
  }
}

inline bool rv_args_ok(int64_t n_cad, int64_t n_draw, int32_t n_planet) {
  return n_cad >= 0 && n_draw >= 0 && n_planet >= 1 && n_draw * (int64_t)n_planet <= 0x7fffffff;
}

}  // namespace

extern "C" {

int exo_radial_velocity_fwd_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw,
                                int32_t n_planet, double* rv, void* stream) {
  if (!rv_args_ok(n_cad, n_draw, n_planet)) return EXO_ERR_INVALID_ARGUMENT;
  const int64_t total = n_draw * n_cad * n_planet;
  if (total == 0) return EXO_OK;
  if (!t || !params || !rv) return EXO_ERR_INVALID_ARGUMENT;
  int64_t blocks = (total + kRvBlock - 1) / kRvBlock;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(rv_fwd_kernel, dim3((unsigned)blocks), dim3(kRvBlock), 0, (hipStream_t)stream, t, n_cad, params,
                     n_draw, n_planet, rv);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

int exo_radial_velocity_vjp_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw,
                                int32_t n_planet, const double* grv, double* gparams, void* stream) {
  if (!rv_args_ok(n_cad, n_draw, n_planet)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!params || !gparams || (n_cad > 0 && (!t || !grv))) return EXO_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(rv_vjp_kernel, dim3((unsigned)(n_draw * n_planet)), dim3(kRvBlock), 0, (hipStream_t)stream, t,
                     n_cad, params, n_planet, grv, gparams);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

int exo_orbit_vector_fwd_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, double* out, void* stream) {
  if (!rv_args_ok(n_cad, n_draw, n_planet) || flags > EXO_OV_ACCELERATION) return EXO_ERR_INVALID_ARGUMENT;
  const int64_t total = n_draw * n_cad * n_planet;
  if (total == 0) return EXO_OK;
  if (!t || !params || !out) return EXO_ERR_INVALID_ARGUMENT;
  int64_t blocks = (total + kRvBlock - 1) / kRvBlock;
  if (blocks > 65536) blocks = 65536;
  if (flags == EXO_OV_VELOCITY)
    hipLaunchKernelGGL(ov_fwd_kernel<1>, dim3((unsigned)blocks), dim3(kRvBlock), 0, (hipStream_t)stream, t, n_cad, params,
                       n_draw, n_planet, out);
  else if (flags == EXO_OV_ACCELERATION)
    hipLaunchKernelGGL(ov_fwd_kernel<2>, dim3((unsigned)blocks), dim3(kRvBlock), 0, (hipStream_t)stream, t, n_cad, params,
                       n_draw, n_planet, out);
  else
    hipLaunchKernelGGL(ov_fwd_kernel<0>, dim3((unsigned)blocks), dim3(kRvBlock), 0, (hipStream_t)stream, t, n_cad, params,
                       n_draw, n_planet, out);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

int exo_orbit_vector_vjp_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, const double* gout, double* gparams, void* stream) {
  if (!rv_args_ok(n_cad, n_draw, n_planet) || flags > EXO_OV_ACCELERATION) return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!params || !gparams || (n_cad > 0 && (!t || !gout))) return EXO_ERR_INVALID_ARGUMENT;
  if (flags == EXO_OV_VELOCITY)
    hipLaunchKernelGGL(ov_vjp_kernel<1>, dim3((unsigned)(n_draw * n_planet)), dim3(kRvBlock), 0, (hipStream_t)stream, t,
                       n_cad, params, n_planet, gout, gparams);
  else if (flags == EXO_OV_ACCELERATION)
    hipLaunchKernelGGL(ov_vjp_kernel<2>, dim3((unsigned)(n_draw * n_planet)), dim3(kRvBlock), 0, (hipStream_t)stream, t,
                       n_cad, params, n_planet, gout, gparams);
  else
    hipLaunchKernelGGL(ov_vjp_kernel<0>, dim3((unsigned)(n_draw * n_planet)), dim3(kRvBlock), 0, (hipStream_t)stream, t,
                       n_cad, params, n_planet, gout, gparams);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
