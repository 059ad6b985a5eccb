// exo_psis.hip -- PSIS-LOO and WAIC per column of an (S, N) array of pointwise log-likelihoods, along the strided axis
// (exoplanet_amd/comparison.py; exo_column_psis_f64).  No sort of the array, no workspace, no atomics on floating-point
// numbers: the arithmetic of exo_psis_core.hpp (shared with tests/psis_harness.cpp) in the tile of exo_predictive.hip.
//
// A workgroup of 8 waves owns a tile of CW adjacent columns and ALL its rows; lane t reads column t % CW in the rows t / CW,
// + RL, + 2 RL, ... (RL = 512 / CW lanes per column).  Integers and keys are merged in LDS and every lane of a column repeats
// the decisions; floating sums over rows are formed per lane in row order and merged in the fixed order of the lanes.
// Passes over the tile: (1) count, extreme keys and the sum; (2) the bisection for the one order statistic l_(M) that sets the
// cut-off, 3 bits of the widest column's key interval per pass; (3) the gather of the tail {l_min - l > c} into LDS -- an
// integer LDS counter per column hands out the positions, the sort that follows makes the order definite -- and in the same
// sweep the sums that need nothing from the fit: the variance's, exp(l - l_max) and exp(x) of the rows outside the tail.
// Then, in LDS alone: a bitonic network over the column's lanes (the tail padded with +inf to a power of two), the m <= 62
// trial values of the Zhang-Stephens fit spread over the lanes of the column -- each lane walks the sorted tail in ascending
// order, so a trial's sum is the one-lane core's --, the weights, the posterior k and sigma, the smoothed tail and its sums.
// The tile's tails are tail[position][column]: CW = 32 columns for tails of up to 512, 16 for up to 1024 (128 KiB), beside
// 14 KiB of merge room.  Layout, resources, times: DESIGN.md section 25.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_psis_core.hpp"

namespace {

using namespace psis;
using namespace predictive;

static_assert(kMaxTail == EXO_PSIS_MAX_TAIL, "the header's constant is the core's");

constexpr int kThreads = 512;          // 8 waves: 256 registers a lane for exp, log1p and expm1 in double
// loads a lane keeps in flight in the counting passes.  Measured: 16 against 4 is 37.2 against 38.9 ms at
// 2000 x 150 000 on the 32-column tile, and 36.5 against 16.1 ms at 100 000 x 1000 on the 16-column one
template <int CW>
constexpr int loads_in_flight() { return CW == 32 ? 16 : 4; }
constexpr int kMerge = 28;             // bytes of merge room per thread: 7 counters; a count, two keys and a sum; three sums

#ifndef EXO_PSIS_TILE_BUDGET_MIB
#define EXO_PSIS_TILE_BUDGET_MIB 192   // tiles in flight are kept below this many MiB where that leaves enough workgroups
#endif
#ifndef EXO_PSIS_MIN_GRID
#define EXO_PSIS_MIN_GRID 256          // ... but never fewer workgroups than this (one per compute unit)
#endif

template <int CW>
constexpr int max_cap() { return CW == 32 ? 512 : 1024; }   // tail positions a tile of CW columns may hold (128 KiB)

constexpr int trial_cap(int cap) {
  int r = 0;
  while ((r + 1) * (r + 1) <= cap) ++r;
  return 30 + r;
}

template <int CW>
size_t lds_bytes(int cap) { return (size_t)kMerge * kThreads + 4 * CW + 16 + (size_t)cap * CW * sizeof(double); }

// the j-th smallest of a column's tail in LDS, and the trial table of a column
template <int CW>
struct Strided {
  double* p;
  __device__ __forceinline__ double& operator[](int j) const { return p[j * CW]; }
};

template <int CW>
__global__ __launch_bounds__(kThreads) void column_psis_kernel(const double* __restrict__ x, int64_t n_rows, int64_t n_cols,
                                                               int64_t row_stride, int32_t M, int32_t cap, int64_t n_tiles,
                                                               double* __restrict__ out_elpd, double* __restrict__ out_k,
                                                               double* __restrict__ out_lppd, double* __restrict__ out_var,
                                                               int32_t* __restrict__ out_n_tail) {
  constexpr int T = kThreads, RL = T / CW, K = (1 << kBits) - 1;
  constexpr int kLoads = loads_in_flight<CW>();
  constexpr int NT = (kMaxTrial + RL - 1) / RL;                       // trial values a lane walks the tail with
  static_assert(trial_cap(max_cap<CW>()) * CW * 8 <= kMerge * T, "the trial table reuses the merge room");
  static_assert(K * 4 <= kMerge && 3 * 8 <= kMerge, "a pass's counters, and three sums, fit the merge room");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int32_t* const sh_i = (int32_t*)lds;                               // [K or 1][T]
  uint64_t* const sh_k = (uint64_t*)(lds + 4 * T);                   // [2][T] (behind one row of counts)
  double* const sh_s = (double*)(lds + 20 * T);                      // [T]    (behind the keys)
  double* const sh_d = (double*)lds;                                 // [3][T]
  int32_t* const cnt = (int32_t*)(lds + kMerge * T);                 // [CW], then the tile's number of passes
  int32_t& tile_passes = cnt[CW];
  double* const tails = (double*)(lds + kMerge * T + 4 * CW + 16);   // [cap][CW]
  const int t = threadIdx.x;
  const int cc = t % CW, rl = t / CW;
  const Strided<CW> tail{tails + cc}, table{(double*)lds + cc};

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t col = tile * CW + cc;
    const bool live = col < n_cols;
    // (a lane past the last column reads the last column and writes nothing: the loops below stay uniform)
    const Column v{x + (live ? col : n_cols - 1), row_stride};

    // ---- pass 1: the count, the extreme keys and the sum
    Extent own = extent_empty();
    double own_sum = 0.0;
#pragma unroll kLoads
    for (int64_t i = rl; i < n_rows; i += RL) {
      const double vi = v[i];
      extent_add(own, vi);
      own_sum += vi;
    }
    if (t == 0) tile_passes = 0;
    if (t < CW) cnt[t] = 0;
    sh_i[t] = own.m;
    sh_k[t] = own.kmin;
    sh_k[T + t] = own.kmax;
    sh_s[t] = own_sum;
    __syncthreads();
    Extent e = extent_empty();
    double sum = 0.0;
#pragma unroll 4
    for (int j = 0; j < RL; ++j) {
      extent_merge(e, sh_i[j * CW + cc], sh_k[j * CW + cc], sh_k[T + j * CW + cc]);
      sum += sh_s[j * CW + cc];
    }
    const bool bad = extent_bad(e, n_rows);
    const double lmin = key_double(e.kmin) + 0.0, lmax = key_double(e.kmax) + 0.0;
    const double mean = sum / (double)n_rows;
    const Rank rank = cut_rank(n_rows, M);
    Bisect<1> s;
    bisect_begin<1>(s, e, &rank);
    // the widest column of the tile sets the number of passes (integers in LDS); a column that is not computed asks for none
    if (rl == 0) atomicMax(&tile_passes, bad ? 0 : passes_needed(e, kBits));
    __syncthreads();
    const int need = tile_passes;
    __syncthreads();   // (the counters of the passes below reuse these bytes)

    // ---- pass 2, need times: the bisection for l_(M)
    for (int pass = 0; pass < need; ++pass) {
      double trial[K];
      int32_t c[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        trial[j] = bisect_trial<K>(s, 0, j + 1);
        c[j] = 0;
      }
#pragma unroll kLoads
      for (int64_t i = rl; i < n_rows; i += RL) {
        const double vi = v[i];
#pragma unroll
        for (int j = 0; j < K; ++j) c[j] += (vi < trial[j]) ? 1 : 0;
      }
#pragma unroll
      for (int j = 0; j < K; ++j) sh_i[j * T + t] = c[j];
      __syncthreads();
      int32_t total[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        total[j] = 0;
#pragma unroll 4
        for (int r = 0; r < RL; ++r) total[j] += sh_i[j * T + r * CW + cc];
      }
      bisect_decide<K>(s, 0, total);
      __syncthreads();
    }
    // (a column that is not computed gathers nothing: no x is above +inf, and a NaN is above nothing)
    const double c = bad ? INFINITY : cut_off(lmin, bisect_value<1>(s, 0));
    const double ec = exp(c);

    // ---- pass 3: the tail into LDS, and the sums over the rows
    double own_var = 0.0, own_exp = 0.0, own_body = 0.0;
#pragma unroll 4
    for (int64_t i = rl; i < n_rows; i += RL) {
      const double vi = v[i];
      const double xi = lmin - vi, d = vi - mean;
      own_var += d * d;
      own_exp += exp(vi - lmax);
      if (xi > c) {
        const int pos = atomicAdd(&cnt[cc], 1);
        if (pos < cap) tail[pos] = xi;                     // (pos < M <= cap: #{x > x_(S-M-1)} <= M)
      } else {
        own_body += exp(xi);
      }
    }
    sh_d[t] = own_var;
    sh_d[T + t] = own_exp;
    sh_d[2 * T + t] = own_body;
    __syncthreads();
    double var = 0.0, sum_exp = 0.0, body = 0.0;
#pragma unroll 4
    for (int j = 0; j < RL; ++j) {
      var += sh_d[j * CW + cc];
      sum_exp += sh_d[T + j * CW + cc];
      body += sh_d[2 * T + j * CW + cc];
    }
    const int n = cnt[cc] < cap ? cnt[cc] : cap;
    for (int pos = n + rl; pos < cap; pos += RL) tail[pos] = INFINITY;
    __syncthreads();

    // ---- the tail ascending: a bitonic network over the lanes of the column
    for (int k = 2; k <= cap; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int idx = rl; idx < cap / 2; idx += RL) {
          const int lo = ((idx / j) * 2 * j) + (idx % j), hi = lo + j;
          const bool up = (lo & k) == 0;
          const double a = tail[lo], b = tail[hi];
          if ((a > b) == up) {
            tail[lo] = b;
            tail[hi] = a;
          }
        }
        __syncthreads();
      }

    // ---- the fit: trial i of the column goes to lane i % RL
    const bool fit = !bad && n > 4;
    const int m = trial_count(n);
    double uq = 1.0, ul = 1.0;
    if (fit) {
      uq = excess(tail, quartile_index(n), ec);
      ul = excess(tail, n - 1, ec);
      double b[NT], kk[NT];
#pragma unroll
      for (int r = 0; r < NT; ++r) b[r] = rl + r * RL < m ? trial_b(rl + r * RL + 1, m, uq, ul) : 0.0;
      mean_log1p<NT>(tail, n, ec, b, kk);
#pragma unroll
      for (int r = 0; r < NT; ++r)
        if (rl + r * RL < m) table[rl + r * RL] = trial_L(b[r], kk[r], n);
    }
    __syncthreads();
    double w[NT];
#pragma unroll
    for (int r = 0; r < NT; ++r) w[r] = fit && rl + r * RL < m ? trial_weight(table, m, rl + r * RL) : 0.0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NT; ++r)
      if (fit && rl + r * RL < m) table[rl + r * RL] = w[r];
    __syncthreads();
    Fit f{INFINITY, 0.0};
    if (fit) {
      const double b = posterior_b(table, m, uq, ul);
      double k1;
      mean_log1p<1>(tail, n, ec, &b, &k1);
      f = fit_finish(k1, b, n);
    }
    __syncthreads();   // (the merges below reuse the table's bytes)

    // ---- the smoothed tail and the last sums: a lane takes every RL-th tail value, the lanes merge in their order
    double own_mx = -INFINITY;
    for (int j = rl; j < n; j += RL) {
      const double tj = tail_value(tail, j, n, f, ec) + (lmin - tail[j]);
      own_mx = tj > own_mx ? tj : own_mx;
    }
    sh_d[t] = own_mx;
    __syncthreads();
    double mx = n < n_rows ? lmin : -INFINITY;
#pragma unroll 4
    for (int j = 0; j < RL; ++j) mx = sh_d[j * CW + cc] > mx ? sh_d[j * CW + cc] : mx;
    __syncthreads();
    double own_tail = 0.0, own_acc = 0.0;
    for (int j = rl; j < n; j += RL) {
      const double xs = tail_value(tail, j, n, f, ec);
      own_tail += exp(xs);
      own_acc += exp(xs + (lmin - tail[j]) - mx);
    }
    sh_d[t] = own_tail;
    sh_d[T + t] = own_acc;
    __syncthreads();
    double tail_sum = 0.0, acc = n < n_rows ? (double)(n_rows - n) * exp(lmin - mx) : 0.0;
#pragma unroll 4
    for (int j = 0; j < RL; ++j) {
      tail_sum += sh_d[j * CW + cc];
      acc += sh_d[T + j * CW + cc];
    }
    if (live && rl == 0) {
      out_elpd[col] = bad ? NAN : elpd_finish(body, tail_sum, acc, mx);
      out_k[col] = bad ? NAN : f.k;
      out_lppd[col] = bad ? NAN : lppd_finish(sum_exp, lmax, n_rows);
      out_var[col] = bad ? NAN : var / (double)n_rows;
      out_n_tail[col] = bad ? 0 : n;
    }
    __syncthreads();   // (the next tile writes the merge room and the counters at once)
  }
}

// workgroups for n_tiles tiles of tile_bytes each: all of them, unless that many tiles in flight outgrow the budget -- then as
// many as the budget holds, and at least EXO_PSIS_MIN_GRID (exo_predictive.hip, grid_for)
int64_t grid_for(int64_t n_tiles, int64_t tile_bytes) {
  int64_t most = ((int64_t)EXO_PSIS_TILE_BUDGET_MIB << 20) / (tile_bytes > 0 ? tile_bytes : 1);
  if (most < EXO_PSIS_MIN_GRID) most = EXO_PSIS_MIN_GRID;
  if (most > (int64_t(1) << 30)) most = int64_t(1) << 30;
  return n_tiles < most ? n_tiles : most;
}

template <int CW>
int launch(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, int32_t M, int32_t cap, double* out_elpd,
           double* out_k, double* out_lppd, double* out_var, int32_t* out_n_tail, hipStream_t stream) {
  const size_t bytes = lds_bytes<CW>(cap);
  if (!allow_dynamic_lds(column_psis_kernel<CW>, bytes)) return EXO_ERR_LAUNCH;
  const int64_t n_tiles = (n_cols + CW - 1) / CW;
  const int64_t grid = grid_for(n_tiles, n_rows * CW * (int64_t)sizeof(double));
  hipLaunchKernelGGL((column_psis_kernel<CW>), dim3((unsigned)grid), dim3(kThreads), bytes, stream, x, n_rows, n_cols, row_stride, M,
                     cap, n_tiles, out_elpd, out_k, out_lppd, out_var, out_n_tail);
  return launch_status();
}

}  // namespace

extern "C" {

int exo_column_psis_f64(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, int32_t n_tail_max, double* out_elpd,
                        double* out_k, double* out_lppd, double* out_var, int32_t* out_n_tail, void* stream) {
  if (n_rows < 0 || n_cols < 0 || n_rows >= (int64_t(1) << 31) || n_tail_max < 1 || n_tail_max > kMaxTail)
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_cols == 0) return EXO_OK;
  if (row_stride < n_cols || !out_elpd || !out_k || !out_lppd || !out_var || !out_n_tail || (n_rows > 0 && !x))
    return EXO_ERR_INVALID_ARGUMENT;
  int32_t cap = 16;                    // positions per column: a power of two, for the sorting network
  while (cap < n_tail_max) cap <<= 1;
  if (cap <= max_cap<32>())
    return launch<32>(x, n_rows, n_cols, row_stride, n_tail_max, cap, out_elpd, out_k, out_lppd, out_var, out_n_tail, (hipStream_t)stream);
  return launch<16>(x, n_rows, n_cols, row_stride, n_tail_max, cap, out_elpd, out_k, out_lppd, out_var, out_n_tail, (hipStream_t)stream);
}

}  // extern "C"
