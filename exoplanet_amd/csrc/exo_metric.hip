// exo_metric.hip -- the dense metric of HMC / NUTS (exoplanet_amd/sampling.py): the change of variables q = c + L x around the
// likelihood of a leaf (exo_metric_apply_f64), the sums of a warm-up window (exo_metric_accumulate_f64) and the metric of the
// next window from them (exo_metric_update_f64).  The arithmetic is exo_metric_core.hpp's, shared with tests/metric_harness.cpp;
// no atomics, no workspace, nothing but kernels enqueued: every entry may be captured into a hipGraph.
//
// apply: a workgroup is one wave, a lane owns a chain.  The lower triangle of L lies packed in LDS (16.6 KB at n = 64; all
// lanes read the same element at the same time: a broadcast) beside the centre, and the wave's 64 rows are staged in LDS,
// n | 1 doubles apart -- an odd stride, so that the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs --, loaded
// and stored coalesced, transformed in place by the lane that owns them: nothing is indexed dynamically in registers.
// 50 KB of LDS at n = 64, 4.7 KB at n = 8; D / 64 workgroups.
// accumulate: a thread owns ONE running sum (a first moment or a product (i, j), j <= i) and adds the rows to it in their
// order, from tiles of 64 shifted rows in LDS that every workgroup stages for itself: (n + n (n + 1) / 2) / 256 workgroups.
// update: one wave.  Sigma and L packed in LDS (33 KB at n = 64); the factor column by column, lane i the entry (i, j) -- the
// entry's own sum is the core's, so the numbers are those of the host's row-by-row loop --, written out only on success.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_metric_core.hpp"

namespace {

using namespace metric;

static_assert(kMaxN == EXO_METRIC_MAX_N, "the header's constant is the core's");
static_assert(kForward == EXO_METRIC_FORWARD && kTransposed == EXO_METRIC_TRANSPOSED && kSolve == EXO_METRIC_SOLVE, "modes");
static_assert(kOk == EXO_METRIC_STATUS_OK && kTooFew == EXO_METRIC_STATUS_TOO_FEW && kNotFinite == EXO_METRIC_STATUS_NOT_FINITE &&
              kNotPositive == EXO_METRIC_STATUS_NOT_POSITIVE, "status words");

constexpr int kWave = 64;
constexpr int kSumThreads = 256;

// the lower triangle of the row-major (n, n) array `chol` into its packed copy: row i by the lanes j <= i
__device__ __forceinline__ void load_packed(const double* __restrict__ chol, int n, double* packed) {
  for (int i = 0; i < n; ++i)
    if ((int)threadIdx.x <= i) packed[i * (i + 1) / 2 + threadIdx.x] = chol[i * n + threadIdx.x];
}

inline size_t apply_lds_bytes(int n) { return sizeof(double) * (size_t)(n * (n + 1) / 2 + n + kWave * (n | 1)); }

__global__ __launch_bounds__(kWave) void metric_apply_kernel(const double* __restrict__ chol, const double* __restrict__ center,
                                                             const double* in, double* out, int64_t D, int n, int mode) {
  extern __shared__ double sh[];
  double* Lp = sh;
  double* c = Lp + packed_size(n);
  double* rows = c + n;
  const int stride = n | 1, t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kWave;
  const int nrows = D - base < kWave ? (int)(D - base) : kWave;
  load_packed(chol, n, Lp);
  if (t < n) c[t] = mode == kTransposed ? 0.0 : center[t];
  for (int k = t; k < nrows * n; k += kWave) {
    const int r = k / n;
    rows[r * stride + (k - r * n)] = in[base * n + k];
  }
  __syncthreads();
  if (t < nrows) apply_row(Packed{Lp}, c, n, mode, rows + t * stride);
  __syncthreads();
  for (int k = t; k < nrows * n; k += kWave) {
    const int r = k / n;
    out[base * n + k] = rows[r * stride + (k - r * n)];
  }
}

__global__ __launch_bounds__(kSumThreads) void metric_accumulate_kernel(const double* __restrict__ q, int64_t D, int n,
                                                                        const double* __restrict__ shift, double* sum1,
                                                                        double* sum2, int64_t* count) {
  __shared__ double tile[kWave * kMaxN];
  __shared__ double s[kMaxN];
  __shared__ int bad[kWave];
  const int t = threadIdx.x;
  const int e = blockIdx.x * kSumThreads + t;          // the running sum this thread owns
  const bool live = e < n + packed_size(n);
  int i = e, j = -1;
  if (live && e >= n) {
    const int p = e - n;
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    j = p - i * (i + 1) / 2;
  }
  double* target = !live ? nullptr : (j < 0 ? sum1 + i : sum2 + i * n + j);
  double acc = live ? *target : 0.0;
  int64_t kept = 0;
  if (t < n) s[t] = shift[t];
  for (int64_t base = 0; base < D; base += kWave) {
    const int nrows = D - base < kWave ? (int)(D - base) : kWave;
    if (t < kWave) bad[t] = 0;
    __syncthreads();
    for (int k = t; k < nrows * n; k += kSumThreads) {
      const int r = k / n;
      const double v = q[base * n + k];
      if (!isfinite(v)) bad[r] = 1;                    // (several threads may store the same 1)
      tile[k] = v - s[k - r * n];
    }
    __syncthreads();
    if (live)
      for (int r = 0; r < nrows; ++r)
        if (!bad[r]) acc = accumulate_term(acc, tile + r * n, i, j);
    if (e == 0)
      for (int r = 0; r < nrows; ++r) kept += bad[r] ? 0 : 1;
    __syncthreads();
  }
  if (live) *target = acc;
  if (e == 0) *count += kept;
}

__global__ __launch_bounds__(kWave) void metric_update_kernel(const double* __restrict__ sum1, const double* __restrict__ sum2,
                                                              const int64_t* __restrict__ count, const double* __restrict__ shift,
                                                              int n, double* cov, double* chol, double* center, int32_t* status) {
  __shared__ double Sig[kMaxN * (kMaxN + 1) / 2];
  __shared__ double Lp[kMaxN * (kMaxN + 1) / 2];
  __shared__ double m[kMaxN];
  __shared__ int fail;
  const int t = threadIdx.x;
  const int64_t kept = *count;
  if (kept < 2) {
    if (t == 0) *status = kTooFew;
    return;
  }
  const double N = (double)kept;
  if (t == 0) fail = kOk;
  __syncthreads();
  if (t < n) {
    m[t] = update_center(shift[t], sum1[t], N);
    if (!isfinite(m[t])) fail = kNotFinite;
  }
  for (int i = 0; i < n; ++i)
    if (t <= i) {
      const double v = update_cov(sum2[i * n + t], sum1[i], sum1[t], N, i == t, true);
      Sig[i * (i + 1) / 2 + t] = v;
      if (!isfinite(v)) fail = kNotFinite;
    }
  __syncthreads();
  bool failed = fail != kOk;
  for (int j = 0; j < n && !failed; ++j) {
    const int jj = j * (j + 1) / 2 + j;
    if (t == 0) {
      const double pivot = cholesky_entry(Packed{Lp}, Sig[jj], j, j);
      if (!isfinite(pivot)) fail = kNotFinite;
      else if (!(pivot > 0.0)) fail = kNotPositive;
      Lp[jj] = sqrt(pivot);
    }
    __syncthreads();
    failed = fail != kOk;
    if (!failed && t > j && t < n) Lp[t * (t + 1) / 2 + j] = cholesky_entry(Packed{Lp}, Sig[t * (t + 1) / 2 + j], t, j);
    __syncthreads();
  }
  if (t == 0) *status = fail;
  if (failed) return;                                  // (nothing but the status: the previous metric stays in force)
  if (t < n) center[t] = m[t];
  for (int i = 0; i < n; ++i)
    if (t <= i) {
      const int p = i * (i + 1) / 2 + t;
      cov[i * n + t] = Sig[p];
      cov[t * n + i] = Sig[p];
      chol[i * n + t] = Lp[p];
      if (t < i) chol[t * n + i] = 0.0;
    }
}

}  // namespace

extern "C" {

int exo_metric_apply_f64(const double* chol, const double* center, const double* in, double* out, int64_t n_row, int32_t n,
                         int32_t mode, void* stream) {
  if (n_row < 0 || n < 1 || n > kMaxN || mode < kForward || mode > kSolve || n_row > (int64_t(1) << 36))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_row == 0) return EXO_OK;
  if (!chol || !in || !out || (mode != kTransposed && !center)) return EXO_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(metric_apply_kernel, dim3((unsigned)((n_row + kWave - 1) / kWave)), dim3(kWave), apply_lds_bytes(n),
                     (hipStream_t)stream, chol, center, in, out, n_row, (int)n, (int)mode);
  return launch_status();
}

int exo_metric_accumulate_f64(const double* q, int64_t n_row, int32_t n, const double* shift, double* sum1, double* sum2,
                              int64_t* count, void* stream) {
  if (n_row < 0 || n < 1 || n > kMaxN) return EXO_ERR_INVALID_ARGUMENT;
  if (n_row == 0) return EXO_OK;
  if (!q || !shift || !sum1 || !sum2 || !count) return EXO_ERR_INVALID_ARGUMENT;
  const int sums = n + n * (n + 1) / 2;
  hipLaunchKernelGGL(metric_accumulate_kernel, dim3((unsigned)((sums + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads), 0,
                     (hipStream_t)stream, q, n_row, (int)n, shift, sum1, sum2, count);
  return launch_status();
}

int exo_metric_update_f64(const double* sum1, const double* sum2, const int64_t* count, const double* shift, int32_t n,
                          double* cov, double* chol, double* center, int32_t* status, void* stream) {
  if (n < 1 || n > kMaxN || !sum1 || !sum2 || !count || !shift || !cov || !chol || !center || !status)
    return EXO_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(metric_update_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, sum1, sum2, count, shift, (int)n, cov,
                     chol, center, status);
  return launch_status();
}

}  // extern "C"
