// exo_noise.hip -- the data-side terms of the white-noise likelihood with a per-draw mean and a per-draw jitter
// (exo_white_noise_terms_f64: Q, Lam, G, H, A of exo_noise_core.hpp for every draw).  A translation unit of its own, so that
// none of the light-curve kernels changes.  Three regimes, chosen from n_var / n_mean / n_jit alone:
//   * one variance for the series, or no jitter: per-series sums once (noise_series_kernel; the caller keeps them and says
//     so with series_ready), then O(1) work per draw (noise_series_draws_kernel);
//   * per-cadence variances AND a jitter: one pass over (draw, cadence) without any array of that size
//     (noise_dense_kernel: lanes over cadences, a register tile of kTile draws per lane, the draw's mean and jitter in scalar
//     registers), block partials, summed per draw in block order (noise_dense_finish_kernel).
// Every sum has a fixed order -- lane accumulators, a shuffle tree per wave, the waves and then the blocks in turn: the
// results are bit-reproducible, and a draw's terms do not depend on the batch it is in.
// Definitions, resources and timings: DESIGN.md section 11.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_draw_block.hpp"
#include "exo_noise_core.hpp"

namespace {

using namespace nz;
using exo::draw::kWave;
using exo::draw::wave_sum;

constexpr int kSeriesThreads = 1024;
constexpr int kThreads = 256;
constexpr int kTile = 4;          // draws per lane: 4 x (4 sums + mantissa product + exponent) = 44 registers of accumulators
constexpr int kMaxBlocksX = 64;   // blocks along the cadences

// sum over the workgroup in a fixed order, valid in every thread (scratch: one double per wave + 1)
__device__ __forceinline__ double block_sum_all(double v, double* scratch) {
  v = wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n_wave = blockDim.x / kWave;
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int i = 0; i < n_wave; ++i) r += scratch[i];
    scratch[n_wave] = r;
  }
  __syncthreads();
  return scratch[n_wave];
}

// the per-series sums (one workgroup; two passes: the weighted mean, then the centred sums)
__global__ __launch_bounds__(kSeriesThreads) void noise_series_kernel(const double* __restrict__ y, const double* __restrict__ var,
                                                                     int64_t n, int one_var, double* __restrict__ series) {
  __shared__ double scratch[kSeriesThreads / kWave + 1];
  Pass1 p1{0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n; i += kSeriesThreads) pass1_add(p1, y[i], one_var ? 1.0 : rcp(var[i]));
  const double su = block_sum_all(p1.u, scratch), suy = block_sum_all(p1.uy, scratch);
  const double ybar = suy / su;
  Pass2 p2{0.0, 0.0, 0.0, 0.0, 0.0};
  LogProd lp = logprod_one();
  int cnt = 0;
  for (int64_t i = threadIdx.x; i < n; i += kSeriesThreads) {
    const double v = one_var ? 1.0 : var[i];
    pass2_add(p2, y[i], one_var ? 1.0 : rcp(v), ybar);
    logprod_mul(lp, v);
    if (++cnt == kRenorm) { logprod_renorm(lp); cnt = 0; }
  }
  const double S1 = block_sum_all(p2.S1, scratch), S2 = block_sum_all(p2.S2, scratch), T0 = block_sum_all(p2.T0, scratch);
  const double T1 = block_sum_all(p2.T1, scratch), T2 = block_sum_all(p2.T2, scratch);
  const double SL = block_sum_all(logprod_value(lp), scratch);
  if (threadIdx.x == 0) {
    series[0] = ybar; series[1] = su; series[2] = S1; series[3] = S2;
    series[4] = T0; series[5] = T1; series[6] = T2; series[7] = SL;
  }
}

// terms [kTerms][n_draw] from the series sums: a thread per draw
__global__ __launch_bounds__(kThreads) void noise_series_draws_kernel(const double* __restrict__ series, const double* __restrict__ var,
                                                                     int one_var, int64_t n_cad, const double* __restrict__ mean,
                                                                     int64_t n_mean, const double* __restrict__ jit2, int64_t n_jit,
                                                                     int64_t n_draw, double* __restrict__ terms) {
  const int64_t d = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (d >= n_draw) return;
  const Series s{series[0], series[1], series[2], series[3], series[4], series[5], series[6], series[7]};
  double out[kTerms];
  from_series(s, one_var != 0, one_var ? var[0] : 0.0, (double)n_cad, mean[n_mean == 1 ? 0 : d],
              n_jit == 0 ? 0.0 : jit2[n_jit == 1 ? 0 : d], out);
#pragma unroll
  for (int q = 0; q < kTerms; ++q) terms[q * n_draw + d] = out[q];
}

// per-cadence variances and a jitter: block (bx, tile) takes cadences bx * 256 + lane, stepping by 256 x gridDim.x, for the
// draws [tile * kTile, tile * kTile + kTile); partial[((draw) * gridDim.x + bx) * kTerms + q]
__global__ __launch_bounds__(kThreads) void noise_dense_kernel(const double* __restrict__ y, const double* __restrict__ var,
                                                              int64_t n_cad, const double* __restrict__ mean, int64_t n_mean,
                                                              const double* __restrict__ jit2, int64_t n_jit, int64_t n_draw,
                                                              double* __restrict__ partial) {
  __shared__ double red[kThreads / kWave][kTile * kTerms];
  const int64_t d0 = (int64_t)blockIdx.y * kTile;
  double mu[kTile], s2[kTile];
  Acc acc[kTile];
#pragma unroll
  for (int k = 0; k < kTile; ++k) {
    // (uniform over the block: scalar loads; a tile past the last draw repeats it and is not written)
    const int64_t d = d0 + k < n_draw ? d0 + k : n_draw - 1;
    mu[k] = mean[n_mean == 1 ? 0 : d];
    s2[k] = jit2[n_jit == 1 ? 0 : d];
    acc[k] = acc_zero();
  }
  int cnt = 0;
  const int64_t step = (int64_t)kThreads * gridDim.x;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_cad; i += step) {
    const double yi = y[i], vi = var[i];
#pragma unroll
    for (int k = 0; k < kTile; ++k) acc_add(acc[k], yi, vi, mu[k], s2[k]);
    if (++cnt == kRenorm) {
#pragma unroll
      for (int k = 0; k < kTile; ++k) logprod_renorm(acc[k].lam);
      cnt = 0;
    }
  }
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kTile; ++k) {
    const double v[kTerms] = {acc[k].Q, logprod_value(acc[k].lam), acc[k].G, acc[k].H, acc[k].A};
#pragma unroll
    for (int q = 0; q < kTerms; ++q) {
      const double s = wave_sum(v[q]);
      if (lane == 0) red[wave][k * kTerms + q] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < kTile * kTerms) {
    const int k = threadIdx.x / kTerms, q = threadIdx.x % kTerms;
    double s = 0.0;
    for (int w = 0; w < kThreads / kWave; ++w) s += red[w][threadIdx.x];
    if (d0 + k < n_draw) partial[((d0 + k) * gridDim.x + blockIdx.x) * kTerms + q] = s;
  }
}

__global__ __launch_bounds__(kThreads) void noise_dense_finish_kernel(const double* __restrict__ partial, int nbx, int64_t n_draw,
                                                                     double* __restrict__ terms) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n_draw * kTerms) return;
  const int64_t d = e / kTerms;
  const int q = (int)(e % kTerms);
  double s = 0.0;
  for (int b = 0; b < nbx; ++b) s += partial[(d * nbx + b) * kTerms + q];
  terms[q * n_draw + d] = s;
}

inline int dense_blocks_x(int64_t n_cad) {
  const int64_t b = (n_cad + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b > kMaxBlocksX ? kMaxBlocksX : b));
}

}  // namespace

extern "C" {

int64_t exo_white_noise_workspace_bytes(int64_t n_cad, int64_t n_draw) {
  if (n_cad < 0 || n_draw < 0) return -1;
  return 8 * (int64_t)kTerms * dense_blocks_x(n_cad) * (n_draw < 1 ? 1 : n_draw);
}

int exo_white_noise_terms_f64(const double* y, const double* var, int64_t n_cad, int64_t n_var, const double* mean, int64_t n_mean,
                              const double* jit2, int64_t n_jit, int64_t n_draw, double* series, int32_t series_ready,
                              double* terms, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_cad < 0 || n_draw < 0 || n_draw > 65535 * (int64_t)kTile || (n_var != 1 && n_var != n_cad) ||
      (n_mean != 1 && n_mean != n_draw) || (n_jit != 0 && n_jit != 1 && n_jit != n_draw))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!var || !mean || !terms || (n_cad > 0 && !y) || (n_jit > 0 && !jit2)) return EXO_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const bool separable = n_cad > 0 && (n_jit == 0 || n_var == 1);
  if (separable) {
    if (!series) return EXO_ERR_INVALID_ARGUMENT;
    const int one_var = n_var == 1 ? 1 : 0;
    if (!series_ready) hipLaunchKernelGGL(noise_series_kernel, dim3(1), dim3(kSeriesThreads), 0, st, y, var, n_cad, one_var, series);
    hipLaunchKernelGGL(noise_series_draws_kernel, dim3((unsigned)((n_draw + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, series,
                       var, one_var, n_cad, mean, n_mean, jit2, n_jit, n_draw, terms);
    return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
  }
  // (an empty series comes here as well: no elements, every sum zero)
  if (n_var != n_cad && n_cad > 0) return EXO_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < exo_white_noise_workspace_bytes(n_cad, n_draw)) return EXO_ERR_WORKSPACE;
  const int nbx = dense_blocks_x(n_cad);
  double* partial = (double*)workspace;
  // (no jitter and no cadences: the kernel still reads a jitter -- hand it the mean's address with stride 0, unused)
  const double* j2 = n_jit > 0 ? jit2 : mean;
  hipLaunchKernelGGL(noise_dense_kernel, dim3((unsigned)nbx, (unsigned)((n_draw + kTile - 1) / kTile)), dim3(kThreads), 0, st, y, var,
                     n_cad, mean, n_mean, j2, n_jit > 0 ? n_jit : 1, n_draw, partial);
  hipLaunchKernelGGL(noise_dense_finish_kernel, dim3((unsigned)((n_draw * kTerms + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     partial, nbx, n_draw, terms);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
