// exo_laplace.hip -- the Laplace approximation at the chains' modes (exoplanet_amd/laplace.py): the points of a central-difference
// stencil around every chain's position (exo_laplace_points_f64) and, from the gradients of logp there, per chain the Hessian of
// -logp, its scaled Cholesky factor, the covariance, the log-evidence and two quality numbers (exo_laplace_factor_f64).  The
// arithmetic is exo_laplace_core.hpp's, shared with tests/laplace_harness.cpp; no atomics, no workspace, nothing but kernels
// enqueued: both entries may be captured into a hipGraph.
//
// points: a thread owns one element of the (D, order m, n) array; the thread of the moved coordinate also stores the realised
// offset.  Plain vector stores, coalesced.
// factor: a workgroup is one wave and owns a chain.  The packed triangles of H (then C = S H S in its place), R and T = R^-1 lie
// in LDS (3 x 16.6 KB at m = 64).  H: lane k forms entry (i, k) of row i from the four (eight) gradient entries it needs; the
// factor column by column, lane i the entry (i, j), as metric_update_kernel; T and C^-1 row by row, lane k the entry (i, k) -- a
// column of T depends on nothing but itself and R, so the rows need no barrier between them.  Every entry's own sum is the
// core's, so the numbers are those of the host's loops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_laplace_core.hpp"

namespace {

using namespace laplace;

static_assert(kMaxN == EXO_LAPLACE_MAX_N, "the header's constant is the core's");
static_assert(kOk == EXO_LAPLACE_STATUS_OK && kNotFinite == EXO_LAPLACE_STATUS_NOT_FINITE &&
              kNotPositive == EXO_LAPLACE_STATUS_NOT_POSITIVE, "status words");

constexpr int kWave = 64;
constexpr int kPointThreads = 256;

__global__ __launch_bounds__(kPointThreads) void laplace_points_kernel(const double* __restrict__ x, int64_t D, int n,
                                                                       const int32_t* __restrict__ free_index, int m,
                                                                       const double* __restrict__ scale, int scale_stride,
                                                                       const double* __restrict__ hess, double delta, int order,
                                                                       double* __restrict__ points, double* __restrict__ dx) {
  const int rows = order * m;
  const int64_t e = (int64_t)blockIdx.x * kPointThreads + threadIdx.x;
  if (e >= D * rows * n) return;
  const int j = (int)(e % n);
  const int r = (int)((e / n) % rows);
  const int64_t d = e / ((int64_t)n * rows);
  const int s = r / m, k = r - s * m;
  const double xv = x[d * n + j];
  if (j != free_index[k]) {
    points[e] = xv;
    return;
  }
  const double h = step(xv, scale != nullptr, scale ? scale[d * scale_stride + j] : 0.0, hess != nullptr,
                        hess ? hess[(d * m + k) * m + k] : 0.0, delta);
  const double p = xv + offset(s, h);
  points[e] = p;
  dx[d * rows + r] = p - xv;
}

// a chain that failed: hess, asymmetry and fd_error are written already; everything else is NaN
__device__ __forceinline__ void write_failed(int64_t d, int m, int status_word, double* cov, double* sd, double* logdet,
                                             double* log_evidence, int32_t* status) {
  const int t = threadIdx.x;
  const double nan = __builtin_nan("");
  for (int k = t; k < m * m; k += kWave) cov[d * m * m + k] = nan;
  if (t < m) sd[d * m + t] = nan;
  if (t == 0) {
    logdet[d] = nan;
    log_evidence[d] = nan;
    status[d] = status_word;
  }
}

__global__ __launch_bounds__(kWave) void laplace_factor_kernel(const double* __restrict__ grad, const double* __restrict__ dx,
                                                               const double* __restrict__ logp, int n,
                                                               const int32_t* __restrict__ free_index, int m, int order,
                                                               double* hess, double* cov, double* sd, double* logdet,
                                                               double* log_evidence, double* asymmetry, double* fd_error,
                                                               int32_t* status) {
  __shared__ double Hp[kMaxN * (kMaxN + 1) / 2];       // H, then C = S H S
  __shared__ double Rp[kMaxN * (kMaxN + 1) / 2];       // H1 - H2, then the factor R
  __shared__ double Tp[kMaxN * (kMaxN + 1) / 2];       // A - A^T, then T = R^-1
  __shared__ double hd[kMaxN], sc[kMaxN], part_a[kWave], part_f[kWave];
  __shared__ int F[kMaxN];
  __shared__ int not_finite, not_positive;
  const int t = threadIdx.x;
  const int64_t d = blockIdx.x;
  const int rows = order * m;
  const double* g = grad + d * rows * n;
  const double* h = dx + d * rows;
  if (t == 0) not_finite = not_positive = 0;
  __syncthreads();
  if (t < m) {
    const int j = free_index[t];
    F[t] = j < 0 ? 0 : (j >= n ? n - 1 : j);           // (an index outside the row is never followed)
    if (j != F[t]) not_finite = 1;
  }
  __syncthreads();
  // ---- what must be finite: the offsets, the gradient's free entries, a step that rounding has not swallowed ----
  for (int r = t; r < rows; r += kWave) {
    bool ok = isfinite(h[r]);
    for (int i = 0; i < m; ++i) ok = ok && isfinite(g[r * n + F[i]]);
    if (!ok) not_finite = 1;                           // (several lanes may store the same 1)
  }
  if (t < m) {
    if (h[t] - h[m + t] == 0.0) not_finite = 1;
    if (order == 4 && h[2 * m + t] - h[3 * m + t] == 0.0) not_finite = 1;
  }
  // ---- H, row by row: lane k the entry (i, k) ----
  for (int i = 0; i < m; ++i)
    if (t <= i) {
      const int k = t, p = i * (i + 1) / 2 + k;
      const double a1_ik = raw_entry(g[k * n + F[i]], g[(m + k) * n + F[i]], h[k], h[m + k]);
      const double a1_ki = raw_entry(g[i * n + F[k]], g[(m + i) * n + F[k]], h[i], h[m + i]);
      double a_ik = a1_ik, a_ki = a1_ki, step_diff = __builtin_nan("");
      if (order == 4) {
        const double a2_ik = raw_entry(g[(2 * m + k) * n + F[i]], g[(3 * m + k) * n + F[i]], h[2 * m + k], h[3 * m + k]);
        const double a2_ki = raw_entry(g[(2 * m + i) * n + F[k]], g[(3 * m + i) * n + F[k]], h[2 * m + i], h[3 * m + i]);
        a_ik = richardson(a1_ik, a2_ik);
        a_ki = richardson(a1_ki, a2_ki);
        step_diff = symmetrise(a1_ik, a1_ki) - symmetrise(a2_ik, a2_ki);
      }
      Hp[p] = symmetrise(a_ik, a_ki);
      Tp[p] = a_ik - a_ki;
      Rp[p] = step_diff;
    }
  __syncthreads();
  // ---- the quality numbers, the Hessian out ----
  double asym = 0.0, fd = 0.0;
  for (int i = 0; i < m; ++i)
    if (t <= i) {
      const int p = i * (i + 1) / 2 + t;
      const double hii = Hp[i * (i + 1) / 2 + i], hkk = Hp[t * (t + 1) / 2 + t];
      if (t < i) asym = max_of(asym, scaled_abs(Tp[p], hii, hkk));
      if (order == 4) fd = max_of(fd, scaled_abs(Rp[p], hii, hkk));
      hess[(d * m + i) * m + t] = Hp[p];
      hess[(d * m + t) * m + i] = Hp[p];
    }
  part_a[t] = asym;
  part_f[t] = fd;
  if (t < m) {
    hd[t] = Hp[t * (t + 1) / 2 + t];
    if (!isfinite(hd[t])) not_finite = 1;
    else if (!(hd[t] > 0.0)) not_positive = 1;
  }
  __syncthreads();
  if (t == 0) {
    for (int l = 1; l < kWave; ++l) {
      asym = max_of(asym, part_a[l]);
      fd = max_of(fd, part_f[l]);
    }
    asymmetry[d] = asym;
    fd_error[d] = order == 4 ? fd : __builtin_nan("");
  }
  if (not_finite || not_positive) {                    // (the same for every lane: read after the barrier)
    write_failed(d, m, not_finite ? kNotFinite : kNotPositive, cov, sd, logdet, log_evidence, status);
    return;
  }
  // ---- C = S H S in H's place, its factor column by column ----
  if (t < m) sc[t] = inv_sqrt(hd[t]);
  __syncthreads();
  for (int i = 0; i < m; ++i)
    if (t <= i) {
      const int p = i * (i + 1) / 2 + t;
      Hp[p] = scaled_entry(sc[i], Hp[p], sc[t], i == t);
    }
  __syncthreads();
  bool failed = false;
  for (int j = 0; j < m && !failed; ++j) {
    const int jj = j * (j + 1) / 2 + j;
    if (t == 0) {
      const double pivot = cholesky_entry(Packed{Rp}, Hp[jj], j, j);
      if (!pivot_ok(pivot, m)) not_positive = 1;
      Rp[jj] = sqrt(pivot);
    }
    __syncthreads();
    failed = not_positive != 0;
    if (!failed && t > j && t < m) Rp[t * (t + 1) / 2 + j] = cholesky_entry(Packed{Rp}, Hp[t * (t + 1) / 2 + j], t, j);
    __syncthreads();
  }
  if (failed) {
    write_failed(d, m, kNotPositive, cov, sd, logdet, log_evidence, status);
    return;
  }
  // ---- T = R^-1 and cov = S T^T T S, row by row ----
  for (int i = 0; i < m; ++i)
    if (t <= i) Tp[i * (i + 1) / 2 + t] = inverse_entry(Packed{Rp}, Packed{Tp}, i, t);
  __syncthreads();
  for (int i = 0; i < m; ++i)
    if (t <= i) {
      const double v = cov_entry(sc[i], sc[t], gram_entry(Packed{Tp}, m, i, t));
      cov[(d * m + i) * m + t] = v;
      cov[(d * m + t) * m + i] = v;
      if (t == i) sd[d * m + i] = sqrt(v);
    }
  if (t == 0) {
    const double ld = log_det(hd, Packed{Rp}, m);
    logdet[d] = ld;
    log_evidence[d] = laplace::log_evidence(logp[d], m, ld);
    status[d] = kOk;
  }
}

inline bool sizes_ok(int64_t D, int32_t n, int32_t m, int32_t order) {
  return D >= 0 && D <= (int64_t(1) << 24) && n >= 1 && n <= kMaxN && m >= 1 && m <= n && (order == 2 || order == 4);
}

}  // namespace

extern "C" {

int exo_laplace_points_f64(const double* x, int64_t n_chain, int32_t n, const int32_t* free_index, int32_t m, const double* scale,
                           int32_t scale_per_chain, const double* hess, double delta, int32_t order, double* points, double* dx,
                           void* stream) {
  if (!sizes_ok(n_chain, n, m, order) || (hess && !(delta > 0.0))) return EXO_ERR_INVALID_ARGUMENT;
  if (n_chain == 0) return EXO_OK;
  if (!x || !free_index || !points || !dx) return EXO_ERR_INVALID_ARGUMENT;
  const int64_t total = n_chain * order * m * n;       // (at most 2^24 * 256 * 64 = 2^38 elements)
  hipLaunchKernelGGL(laplace_points_kernel, dim3((unsigned)((total + kPointThreads - 1) / kPointThreads)), dim3(kPointThreads), 0,
                     (hipStream_t)stream, x, n_chain, (int)n, free_index, (int)m, scale, scale_per_chain ? (int)n : 0, hess, delta,
                     (int)order, points, dx);
  return launch_status();
}

int exo_laplace_factor_f64(const double* grad, const double* dx, const double* logp, int64_t n_chain, int32_t n,
                           const int32_t* free_index, int32_t m, int32_t order, double* hess, double* cov, double* sd, double* logdet,
                           double* log_evidence, double* asymmetry, double* fd_error, int32_t* status, void* stream) {
  if (!sizes_ok(n_chain, n, m, order)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_chain == 0) return EXO_OK;
  if (!grad || !dx || !logp || !free_index || !hess || !cov || !sd || !logdet || !log_evidence || !asymmetry || !fd_error || !status)
    return EXO_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(laplace_factor_kernel, dim3((unsigned)n_chain), dim3(kWave), 0, (hipStream_t)stream, grad, dx, logp, (int)n,
                     free_index, (int)m, (int)order, hess, cov, sd, logdet, log_evidence, asymmetry, fd_error, status);
  return launch_status();
}

}  // extern "C"
