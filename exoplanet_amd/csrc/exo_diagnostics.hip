// exo_diagnostics.hip -- rank-normalised split R-hat, effective sample sizes and Monte-Carlo standard errors of a batch of
// chains that stays on the device (exoplanet_amd/diagnostics.py; exo_diag_*_f64).  A call handles P parameters of `chains`
// chains; after splitting, a parameter is M = 2 chains half-chains of L draws, S = M L values.  The caller sorts (plumbing);
// the kernels here do the rest:
//   prepare   per value: |x - median| (to be sorted next), the two tail indicators, the raw copy relative to a pivot; per
//             parameter: mean, sd, quantiles, "not finite" and "constant"
//   rank      per sorted value: ends of its run of equal values by bisection, average rank, Phi^-1, scattered through the
//             permutation into the set's [n][m] array
//   autocov   a lane owns a half-chain and walks its draws (a wave reads 512 contiguous bytes per draw); kLagBlock lags per
//             launch from a window of the last kLagBlock centred values in registers; wave reduction, one partial per wave
//   finish    per series set: sums the partials in turn, rho_t of the block, Geyer's truncation carried from block to block
//             in the workspace, then the monotone sequence, tau, the effective sample size and the set's `done` word
// Every sum has a fixed order and there are no atomics: the same input gives the same bits.  The arithmetic is
// exo_diagnostics_core.hpp, shared with the host harness of the tests.  Definition, layout and resources: DESIGN.md section 16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_diagnostics_core.hpp"

namespace {

using namespace diag;

static_assert(kLagBlock == EXO_DIAG_LAG_BLOCK && kSets == EXO_DIAG_SETS && kOut == EXO_DIAG_OUT && kMoments == EXO_DIAG_MOMENTS,
              "the header's constants are the core's");
constexpr int kBlock = 256;
constexpr int64_t kMaxGridY = 65535;

struct Shape {
  int64_t P, M, L, S, NW, Lp;
};

__host__ __device__ inline Shape shape_of(int64_t P, int64_t M, int64_t L) {
  Shape s;
  s.P = P; s.M = M; s.L = L; s.S = M * L;
  s.NW = (M + kWave - 1) / kWave;
  s.Lp = (L + kLagBlock - 1) / kLagBlock * kLagBlock;
  return s;
}

// the workspace, in doubles: means [P kSets][M], partials [P kSets][NW][kLagBlock], rho [P kSets][Lp], state [P kSets][kState]
struct Workspace {
  double *means, *partial, *rho, *state;
};

__host__ __device__ inline int64_t workspace_doubles(const Shape& s) {
  const int64_t nset = s.P * kSets;
  return nset * (s.M + s.NW * kLagBlock + s.Lp + kState);
}

__host__ __device__ inline Workspace carve(void* base, const Shape& s) {
  const int64_t nset = s.P * kSets;
  Workspace w;
  w.means = (double*)base;
  w.partial = w.means + nset * s.M;
  w.rho = w.partial + nset * s.NW * kLagBlock;
  w.state = w.rho + nset * s.Lp;
  return w;
}

// ---- prepare -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void diag_prepare_kernel(const double* __restrict__ x, const double* __restrict__ sorted,
                                                              const double* __restrict__ sorted_full, int64_t n_full, Shape s,
                                                              double* __restrict__ folded, double* __restrict__ sets) {
  const int64_t p = blockIdx.y, j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= s.S) return;
  const double* sv = sorted + p * s.S;
  const double* sf = sorted_full + p * n_full;
  const double v = x[p * s.S + j];
  const double pivot = sv[s.S / 2];
  const double q05 = quantile_sorted<double>(sf, n_full, 5), q95 = quantile_sorted<double>(sf, n_full, 95);
  folded[p * s.S + j] = folded_of<double>(v, sv, s.S);
  double* base = sets + p * kSets * s.S;
  base[kLow * s.S + j] = v <= q05 ? 1.0 : 0.0;
  base[kHigh * s.S + j] = v <= q95 ? 1.0 : 0.0;
  base[kRaw * s.S + j] = v - pivot;
}

// a block's sum in a fixed order: every thread's strided partial, then the halving tree over the block in shared memory
__device__ __forceinline__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  const double total = sh[0];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kBlock) void diag_moments_kernel(const double* __restrict__ sorted_full, int64_t n_full,
                                                              double* __restrict__ moments) {
  __shared__ double sh[kBlock];
  const int64_t p = blockIdx.x;
  const double* sf = sorted_full + p * n_full;
  const double pivot = sf[n_full / 2];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n_full; i += kBlock) a += sf[i] - pivot;
  const double mean_rel = block_sum(a, sh) / (double)n_full;
  double b = 0.0;
  for (int64_t i = threadIdx.x; i < n_full; i += kBlock) {
    const double d = (sf[i] - pivot) - mean_rel;
    b += d * d;
  }
  const double ss = block_sum(b, sh);
  if (threadIdx.x != 0) return;
  double* m = moments + p * kMoments;
  const double lo = sf[0], hi = sf[n_full - 1];          // (the sort puts NaN last, the infinities at the ends)
  m[mMean] = pivot + mean_rel;
  m[mSd] = n_full > 1 ? sqrt(ss / (double)(n_full - 1)) : NAN;
  m[mQ05] = quantile_sorted<double>(sf, n_full, 5);
  m[mQ50] = quantile_sorted<double>(sf, n_full, 50);
  m[mQ95] = quantile_sorted<double>(sf, n_full, 95);
  m[mBad] = finite(lo) && finite(hi) ? 0.0 : 1.0;
  m[mConst] = lo == hi ? 1.0 : 0.0;
  m[mPivot] = pivot;
}

// ---- rank --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void diag_rank_kernel(const double* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                           Shape s, int set, double* __restrict__ sets) {
  const int64_t p = blockIdx.y, i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= s.S) return;
  const double* sv = sorted + p * s.S;
  const int64_t j = perm[p * s.S + i];
  if (j < 0 || j >= s.S) return;                          // (no permutation: nothing is written outside the set)
  sets[(p * kSets + set) * s.S + j] = z_of_rank<double>(rank2_of(sv, s.S, i), s.S);
}

// ---- autocovariance ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void diag_means_kernel(const double* __restrict__ sets, Shape s, double* __restrict__ means) {
  const int64_t set = blockIdx.y, m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (m >= s.M) return;
  const double* y = sets + set * s.S + m;
  double sum = 0.0;
  for (int64_t n = 0; n < s.L; ++n) sum += y[n * s.M];
  means[set * s.M + m] = sum / (double)s.L;
}

__global__ __launch_bounds__(kBlock) void diag_autocov_kernel(const double* __restrict__ sets, Shape s, int64_t block,
                                                              const int32_t* __restrict__ done, Workspace w) {
  const int64_t set = blockIdx.y, m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (done[set]) return;                                  // (the whole block leaves: nothing below synchronises anyway)
  const bool live = m < s.M;
  const double* y = sets + set * s.S + (live ? m : 0);
  const double mean = live ? w.means[set * s.M + m] : 0.0;
  const int64_t t0 = block * kLagBlock;
  double acc[kLagBlock], win[kLagBlock];
#pragma unroll
  for (int k = 0; k < kLagBlock; ++k) acc[k] = win[k] = 0.0;
  if (live) {
    for (int64_t n = t0; n < s.L; ++n) {
      const double dn = y[n * s.M] - mean, dw = y[(n - t0) * s.M] - mean;
#pragma unroll
      for (int k = kLagBlock - 1; k > 0; --k) win[k] = win[k - 1];
      win[0] = dw;                                        // win[k] = d[n - t0 - k], zero before the series starts
#pragma unroll
      for (int k = 0; k < kLagBlock; ++k) acc[k] += dn * win[k];
    }
  }
  // the halving tree of the wave; lane 0 holds the sum of the wave's 64 half-chains (lanes past M gave zeros)
  const int lane = threadIdx.x % kWave;
  const int64_t wave = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kLagBlock; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if (lane == 0 && wave < s.NW) w.partial[(set * s.NW + wave) * kLagBlock + k] = v;
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void diag_finish_kernel(Shape s, int64_t block, int32_t* __restrict__ done, Workspace w) {
  const int64_t set = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (set >= s.P * kSets || done[set]) return;
  double* st = w.state + set * kState;
  double* rho = w.rho + set * s.Lp;
  double sums[kLagBlock];
  for (int k = 0; k < kLagBlock; ++k) {
    double v = 0.0;
    for (int64_t g = 0; g < s.NW; ++g) {
      const double a = w.partial[(set * s.NW + g) * kLagBlock + k];
      v = g == 0 ? a : v + a;
    }
    sums[k] = v;
  }
  if (block == 0) begin_set<double>(sums[0], w.means + set * s.M, s.M, s.L, st);
  for (int k = 0; k < kLagBlock; ++k) rho[block * kLagBlock + k] = rho_of<double>(sums[k], s.M, s.L, st);
  if (block == 0) {
    rho[0] = 1.0;
    st[sRo] = rho[1];
  }
  // (the folded set is there for its R-hat alone)
  if (set % kSets == kZFold || advance_set<double>(rho, (block + 1) * kLagBlock, s.M, s.L, st)) done[set] = 1;
}

__global__ __launch_bounds__(kWave) void diag_assemble_kernel(Shape s, const double* __restrict__ moments, Workspace w,
                                                              double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (p >= s.P) return;
  assemble<double>(w.state + p * kSets * kState, moments + p * kMoments, s.M, s.L, out + p * kOut);
}

bool sizes_ok(int64_t P, int64_t M, int64_t L) {
  // (L >= 2: a series of fewer than four draws is answered by the caller without a launch)
  return P >= 0 && M >= 0 && L >= 2 && (M % 2 == 0) && P * kSets <= kMaxGridY && (M == 0 || L <= (int64_t(1) << 40) / (M * 8 * kSets));
}

int launched() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

}  // namespace

extern "C" {

int64_t exo_diag_workspace_bytes(int64_t n_param, int64_t n_half, int64_t n_len) {
  if (!sizes_ok(n_param, n_half, n_len)) return -1;
  return workspace_doubles(shape_of(n_param, n_half, n_len)) * (int64_t)sizeof(double);
}

int exo_diag_prepare_f64(const double* x, const double* sorted, const double* sorted_full, int64_t n_full, int64_t n_param,
                         int64_t n_half, int64_t n_len, double* folded, double* sets, double* moments, void* stream) {
  if (!sizes_ok(n_param, n_half, n_len) || n_full < n_half * n_len) return EXO_ERR_INVALID_ARGUMENT;
  if (n_param == 0 || n_half == 0) return EXO_OK;
  if (!x || !sorted || !sorted_full || !folded || !sets || !moments) return EXO_ERR_INVALID_ARGUMENT;
  const Shape s = shape_of(n_param, n_half, n_len);
  hipLaunchKernelGGL(diag_moments_kernel, dim3((unsigned)s.P), dim3(kBlock), 0, (hipStream_t)stream, sorted_full, n_full, moments);
  hipLaunchKernelGGL(diag_prepare_kernel, dim3((unsigned)((s.S + kBlock - 1) / kBlock), (unsigned)s.P), dim3(kBlock), 0,
                     (hipStream_t)stream, x, sorted, sorted_full, n_full, s, folded, sets);
  return launched();
}

int exo_diag_rank_f64(const double* sorted, const int64_t* perm, int64_t n_param, int64_t n_half, int64_t n_len, int32_t set,
                      double* sets, void* stream) {
  if (!sizes_ok(n_param, n_half, n_len) || (set != kZ && set != kZFold)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_param == 0 || n_half == 0) return EXO_OK;
  if (!sorted || !perm || !sets) return EXO_ERR_INVALID_ARGUMENT;
  const Shape s = shape_of(n_param, n_half, n_len);
  hipLaunchKernelGGL(diag_rank_kernel, dim3((unsigned)((s.S + kBlock - 1) / kBlock), (unsigned)s.P), dim3(kBlock), 0,
                     (hipStream_t)stream, sorted, perm, s, (int)set, sets);
  return launched();
}

int exo_diag_autocov_f64(const double* sets, int64_t n_param, int64_t n_half, int64_t n_len, int64_t block, const int32_t* done,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  if (!sizes_ok(n_param, n_half, n_len) || block < 0 || block * kLagBlock >= n_len + kLagBlock) return EXO_ERR_INVALID_ARGUMENT;
  if (n_param == 0 || n_half == 0) return EXO_OK;
  if (!sets || !done || !workspace) return EXO_ERR_INVALID_ARGUMENT;
  const Shape s = shape_of(n_param, n_half, n_len);
  if (workspace_bytes < workspace_doubles(s) * (int64_t)sizeof(double)) return EXO_ERR_WORKSPACE;
  if (block * kLagBlock >= s.Lp) return EXO_ERR_INVALID_ARGUMENT;
  const Workspace w = carve(workspace, s);
  const dim3 grid((unsigned)((s.M + kBlock - 1) / kBlock), (unsigned)(s.P * kSets));
  if (block == 0) hipLaunchKernelGGL(diag_means_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, sets, s, w.means);
  hipLaunchKernelGGL(diag_autocov_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, sets, s, block, done, w);
  return launched();
}

int exo_diag_finish_f64(int64_t n_param, int64_t n_half, int64_t n_len, int64_t block, const double* moments, double* out,
                        int32_t* done, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!sizes_ok(n_param, n_half, n_len) || block < -1) return EXO_ERR_INVALID_ARGUMENT;
  if (n_param == 0 || n_half == 0) return EXO_OK;
  if (!done || !workspace || (block < 0 && (!moments || !out))) return EXO_ERR_INVALID_ARGUMENT;
  const Shape s = shape_of(n_param, n_half, n_len);
  if (workspace_bytes < workspace_doubles(s) * (int64_t)sizeof(double)) return EXO_ERR_WORKSPACE;
  if (block * kLagBlock >= s.Lp) return EXO_ERR_INVALID_ARGUMENT;
  const Workspace w = carve(workspace, s);
  if (block >= 0)
    hipLaunchKernelGGL(diag_finish_kernel, dim3((unsigned)((s.P * kSets + kWave - 1) / kWave)), dim3(kWave), 0, (hipStream_t)stream,
                       s, block, done, w);
  else
    hipLaunchKernelGGL(diag_assemble_kernel, dim3((unsigned)((s.P + kWave - 1) / kWave)), dim3(kWave), 0, (hipStream_t)stream, s,
                       moments, w, out);
  return launched();
}

}  // extern "C"
