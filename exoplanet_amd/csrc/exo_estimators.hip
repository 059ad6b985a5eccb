// exo_estimators.hip -- period search (exoplanet_amd/estimators.py): the box-least-squares periodogram, its limb-darkened
// twin (transit least squares: a template in place of the box) and the exact floating-mean Lomb-Scargle periodogram of a
// batch of series on one time axis.  Pre-fit utilities beside the per-step path: a translation unit of its own, so that
// none of the likelihood's kernels changes.  The arithmetic of one period lives in exo_estimators_core.hpp (tested on the
// host); definitions, resources and timings: DESIGN.md sections 9 and 18.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_draw_block.hpp"
#include "exo_estimators_core.hpp"
#include "exo_estimators_launch.hpp"

namespace {

using namespace est;
using exo::draw::kWave;
using exo::draw::wave_sum;

constexpr int kPrepThreads = 1024;
constexpr int kBlsThreads = 256;     // histogram in LDS: one workgroup per (period, series)
constexpr int kSlabThreads = 1024;   // histogram in the workspace: persistent workgroups, one slab each
constexpr int kMaxSlabs = 256;
// 64 KiB of LDS per workgroup: two fp64 arrays of n_bins + 1 entries beside the 4 KiB + 32 B of the reductions
constexpr int64_t kLdsBins = (64 * 1024 - 2 * kBlsThreads * 8 - 64) / 16 - 1;
constexpr int kMaxDur = EXO_BLS_MAX_DURATIONS;
constexpr int kLsFreq = 4;           // frequencies per workgroup, their 28 sums in registers
constexpr int kLsThreads = 256;

struct Durations {
  int32_t m[kMaxDur];  // boxes of m[k] bins, computed on the host
};

struct Templates {
  int32_t off[kMaxDur + 1];  // template k of the template search: entries off[k] .. off[k] + m[k] - 1 of the flat table
};

// workspace, in doubles: [0] t_min, [1] t_max, [2 + 2 b] Y_b, [3 + 2 b] W_b, then tt[n], w[n_w][n], wy[n_series][n], then the slabs
struct Layout {
  int64_t n, n_series, n_w;
  __host__ __device__ int64_t head() const { return (2 + 2 * n_series + 7) / 8 * 8; }
  __host__ __device__ int64_t tt() const { return head(); }
  __host__ __device__ int64_t w(int64_t b) const { return head() + n + (n_w > 1 ? b : 0) * n; }
  __host__ __device__ int64_t wy(int64_t b) const { return head() + n + n_w * n + b * n; }
  __host__ __device__ int64_t slabs() const { return head() + n + n_w * n + n_series * n; }
};

// sum over the workgroup, valid in thread 0 (scratch: one double per wave)
__device__ __forceinline__ double block_sum(double v, double* scratch) {
  v = wave_sum(v);
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n_wave = blockDim.x / kWave;
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < n_wave; ++i) r += scratch[i];
  return r;
}

// t_min and t_max (one workgroup)
__global__ __launch_bounds__(kPrepThreads) void est_range_kernel(const double* __restrict__ t, int64_t n, double* __restrict__ ws) {
  __shared__ double lo_s[kPrepThreads / kWave], hi_s[kPrepThreads / kWave];
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
    lo = fmin(lo, t[i]);
    hi = fmax(hi, t[i]);
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_down(lo, o, kWave));
    hi = fmax(hi, __shfl_down(hi, o, kWave));
  }
  if (threadIdx.x % kWave == 0) {
    lo_s[threadIdx.x / kWave] = lo;
    hi_s[threadIdx.x / kWave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kPrepThreads / kWave; ++i) {
      lo = fmin(lo, lo_s[i]);
      hi = fmax(hi, hi_s[i]);
    }
    ws[0] = lo;
    ws[1] = hi;
  }
}

// the columns a search reads: tt = t - origin (origin: t_min, or the mid-time with `centre`), w = 1 / yerr^2 (1 without), w y;
// and the totals Y_b = sum w y, W_b = sum w, in a fixed order (no atomics).  One workgroup per series.
// The columns are stored in the order j -> cadence (j * stride) mod n, stride coprime to n and about n / 61: the searches sum
// over the cadences in any order, and the 64 cadences that a wave of the box search reads together then lie a sixty-first of
// the series apart instead of side by side -- in sorted times neighbours share a phase bin, and their atomic adds to one
// LDS address would be served one after the other.
__global__ __launch_bounds__(kPrepThreads) void est_prepare_kernel(const double* __restrict__ t, const double* __restrict__ y,
                                                                   const double* __restrict__ yerr, int64_t n_yerr, Layout L,
                                                                   int centre, int64_t stride, double* __restrict__ ws) {
  __shared__ double scratch[kPrepThreads / kWave];
  const int64_t b = blockIdx.x, n = L.n;
  const double origin = centre ? 0.5 * (ws[0] + ws[1]) : ws[0];
  const double* e = yerr ? yerr + (n_yerr > 1 ? b : 0) * n : nullptr;
  const bool write_w = L.n_w > 1 || b == 0;
  double* tt = ws + L.tt();
  double* w = ws + L.w(b);
  double* wy = ws + L.wy(b);
  double sy = 0.0, sw = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
    const int64_t i = (j * stride) % n;
    const double wi = e ? 1.0 / (e[i] * e[i]) : 1.0, wyi = wi * y[b * n + i];
    if (b == 0) tt[j] = t[i] - origin;
    if (write_w) w[j] = wi;
    wy[j] = wyi;
    sy += wyi;
    sw += wi;
  }
  sy = block_sum(sy, scratch);
  sw = block_sum(sw, scratch);
  if (threadIdx.x == 0) {
    ws[2 + 2 * b] = sy;
    ws[3 + 2 * b] = sw;
  }
}

// a no-return fp64 add: ds_add_f64 on LDS, global_atomic_add_f64 on the workspace (both native on gfx950: DESIGN.md 9.3).
// The order in which the lanes' adds arrive is not fixed, so a bin's sum may differ in its last bits from run to run.
__device__ __forceinline__ void add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }

// The histogram pass of one period of one series, shared by the box search and the template search: zero, histogram of
// (w y, w) over the bins of the folded time, the wrap-around copy.  hy, hw: n_bins + 1 entries each, in LDS or in a slab of
// the workspace that this workgroup alone uses (kGlobal: the fences that make its atomics visible to its own plain loads).
template <bool kGlobal>
__device__ __forceinline__ void bls_histogram(double* hy, double* hw, int64_t n_bins, const double* __restrict__ tt,
                                              const double* __restrict__ w, const double* __restrict__ wy, int64_t n, double p,
                                              double delta, int oversample) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int64_t i = tid; i <= n_bins; i += nt) {
    hy[i] = 0.0;
    hw[i] = 0.0;
  }
  if (kGlobal) __threadfence();
  __syncthreads();
  const double inv_p = 1.0 / p, inv_delta = 1.0 / delta;
  for (int64_t i = tid; i < n; i += nt) {
    const int64_t b = bls_bin_index(tt[i], p, inv_p, delta, inv_delta, n_bins);
    add_f64(hy + b, wy[i]);
    add_f64(hw + b, w[i]);
  }
  if (kGlobal) __threadfence();
  __syncthreads();
  // bins 1 .. oversample once more behind the last phase bin: a box may straddle phase zero
  for (int64_t i = 1 + tid; i <= oversample; i += nt) {
    hy[n_bins - oversample + i] = hy[i];
    hw[n_bins - oversample + i] = hw[i];
  }
  __syncthreads();
}

// the arg-max of the workgroup from every lane's own (first maximiser in (k, s) order): shuffles, then LDS; valid in thread 0
__device__ __forceinline__ BlsBest block_best(BlsBest best, double* red_d, int64_t* red_i) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double obj = __shfl_down(best.obj, o, kWave);
    const int64_t key = __shfl_down((long long)best.key, o, kWave);
    bls_best_take(best, obj, key);
  }
  if (tid % kWave == 0) {
    red_d[tid / kWave] = best.obj;
    red_i[tid / kWave] = best.key;
  }
  __syncthreads();
  if (tid == 0)
    for (int i = 1; i < nt / kWave; ++i) bls_best_take(best, red_d[i], red_i[i]);
  return best;
}

// The two searches: what differs after the shared histogram pass.  Each is passed by value as a kernel argument and says how
// many doubles of `red_d` a workgroup of `threads` needs, what a lane's best candidate is, and what thread 0 writes at the
// workgroup's maximiser.  The template search's table is NOT in its struct: as a `const double* __restrict__` kernel
// parameter of its own (`table`; the box search is handed a null pointer and ignores it) its reads, under an index that is
// uniform across the wave, stay scalar loads on the slab path too, where the histogram shares the global address space with it.

// The box search: inclusive prefix sums in place, then the search over (duration, start).
struct BoxSearch {
  Durations dur;
  int n_dur;
  static constexpr int red_doubles(int threads) { return 2 * threads; }  // the lanes' totals of both prefix sums

  __device__ __forceinline__ BlsBest lane_best(double* hy, double* hw, int64_t n_bins, const double*, double Y, double W,
                                               int objective, double* red_d) const {
    const int tid = threadIdx.x, nt = blockDim.x;
    // inclusive prefix sums: each lane its own stretch, the lanes' totals scanned by lane 0's wave, then the offsets added
    const int64_t per = (n_bins + nt) / nt, lo = 1 + (int64_t)tid * per, hi = lo + per < n_bins + 1 ? lo + per : n_bins + 1;
    double ay = 0.0, aw = 0.0;
    for (int64_t i = lo; i < hi; ++i) {
      ay += hy[i];
      aw += hw[i];
      hy[i] = ay;
      hw[i] = aw;
    }
    double* tot_y = red_d;
    double* tot_w = red_d + nt;
    tot_y[tid] = ay;
    tot_w[tid] = aw;
    __syncthreads();
    if (tid == 0) {
      double cy = 0.0, cw = 0.0;
      for (int i = 0; i < nt; ++i) {
        const double y0 = tot_y[i], w0 = tot_w[i];
        tot_y[i] = cy;
        tot_w[i] = cw;
        cy += y0;
        cw += w0;
      }
    }
    __syncthreads();
    const double oy = tot_y[tid], ow = tot_w[tid];
    for (int64_t i = lo; i < hi; ++i) {
      hy[i] += oy;
      hw[i] += ow;
    }
    __syncthreads();
    return bls_search(hy, hw, n_bins, dur.m, n_dur, Y, W, objective, tid, nt);
  }

  __device__ __forceinline__ void outputs(double* hy, double* hw, int64_t n_bins, const double*, double Y, double W, int objective,
                                          BlsBest best, double p, double delta, double t_min, double* out, int64_t out_stride) const {
    bls_outputs(hy, hw, n_bins, dur.m, Y, W, objective, best, p, delta, t_min, out, out_stride);
  }
};

// The template search: the correlation of the histogram itself with every template -- lanes over the
// starts s, strided by the workgroup, so that neighbouring lanes read neighbouring bins; k outer, j inner.  g: the flat table
// in global memory, read under an index that is uniform across the wave.
struct TemplateSearch {
  Durations dur;
  Templates tpl;
  int n_dur;
  static constexpr int red_doubles(int threads) { return threads / kWave; }  // block_best's alone

  __device__ __forceinline__ BlsBest lane_best(const double* hy, const double* hw, int64_t n_bins, const double* __restrict__ g,
                                               double Y, double W, int objective, double*) const {
    return tls_search(hy, hw, n_bins, dur.m, tpl.off, n_dur, g, Y, W, objective, threadIdx.x, blockDim.x);
  }

  __device__ __forceinline__ void outputs(const double* hy, const double* hw, int64_t n_bins, const double* __restrict__ g, double Y,
                                          double W, int objective, BlsBest best, double p, double delta, double t_min, double* out,
                                          int64_t out_stride) const {
    tls_outputs(hy, hw, n_bins, dur.m, tpl.off, g, Y, W, objective, best, p, delta, t_min, out, out_stride);
  }
};

// One period of one series: the histogram pass, every lane its share of the candidates, the arg-max of the wave and of the
// workgroup (first maximiser in (k, s) order), and the outputs.
template <class Search, bool kGlobal>
__device__ __forceinline__ void period(const Search& search, const double* __restrict__ table, double* hy, double* hw,
                                       int64_t n_bins, const double* __restrict__ tt, const double* __restrict__ w,
                                       const double* __restrict__ wy, int64_t n, double p, double delta, int oversample, double Y,
                                       double W, double t_min, int objective, double* out, int64_t out_stride, double* red_d,
                                       int64_t* red_i) {
  bls_histogram<kGlobal>(hy, hw, n_bins, tt, w, wy, n, p, delta, oversample);
  const BlsBest best = block_best(search.lane_best(hy, hw, n_bins, table, Y, W, objective, red_d), red_d, red_i);
  if (threadIdx.x == 0) search.outputs(hy, hw, n_bins, table, Y, W, objective, best, p, delta, t_min, out, out_stride);
  __syncthreads();
}

// a period whose histogram has no room: NaN in its seven planes
__device__ __forceinline__ void fill_nan(double* o, int64_t plane) {
  if (threadIdx.x == 0)
    for (int i = 0; i < 7; ++i) o[i * plane] = NAN;
}

// periods whose histogram fits the LDS: workgroup (period, series)
template <class Search>
__global__ __launch_bounds__(kBlsThreads) void search_lds_kernel(const double* __restrict__ periods, int64_t n_period, Layout L,
                                                                 double delta, int oversample, Search search,
                                                                 const double* __restrict__ table, int objective, int64_t lds_bins,
                                                                 const double* __restrict__ ws, double* __restrict__ out) {
  extern __shared__ double hist[];
  __shared__ double red_d[Search::red_doubles(kBlsThreads)];
  __shared__ int64_t red_i[kBlsThreads / kWave];
  const int64_t ip = blockIdx.x, b = blockIdx.y;
  const double p = periods[ip];
  const int64_t n_bins = bls_n_bins(p, delta, oversample);
  if (n_bins > kLdsBins) return;  // the slab kernel's
  double* o = out + b * n_period + ip;
  if (n_bins > lds_bins) {  // (more bins than the caller's max_bins announced: nothing is written past the histogram)
    fill_nan(o, L.n_series * n_period);
    return;
  }
  period<Search, false>(search, table, hist, hist + n_bins + 1, n_bins, ws + L.tt(), ws + L.w(b), ws + L.wy(b), L.n, p, delta, oversample,
                        ws[2 + 2 * b], ws[3 + 2 * b], ws[0], objective, o, L.n_series * n_period, red_d, red_i);
}

// the others: the histogram in a slab of the workspace, one slab per workgroup, the workgroups walking the (period, series) pairs
template <class Search>
__global__ __launch_bounds__(kSlabThreads) void search_slab_kernel(const double* __restrict__ periods, int64_t n_period, Layout L,
                                                                   double delta, int oversample, Search search,
                                                                   const double* __restrict__ table, int objective, int64_t max_bins,
                                                                   double* __restrict__ ws, double* __restrict__ out) {
  __shared__ double red_d[Search::red_doubles(kSlabThreads)];
  __shared__ int64_t red_i[kSlabThreads / kWave];
  double* slab = ws + L.slabs() + (int64_t)blockIdx.x * 2 * (max_bins + 1);
  for (int64_t item = blockIdx.x; item < n_period * L.n_series; item += gridDim.x) {
    const int64_t ip = item % n_period, b = item / n_period;
    const double p = periods[ip];
    const int64_t n_bins = bls_n_bins(p, delta, oversample);
    if (n_bins <= kLdsBins) continue;
    double* o = out + b * n_period + ip;
    if (n_bins > max_bins) {  // (the host sized the slabs from these very periods: not reached)
      fill_nan(o, L.n_series * n_period);
      continue;
    }
    period<Search, true>(search, table, slab, slab + n_bins + 1, n_bins, ws + L.tt(), ws + L.w(b), ws + L.wy(b), L.n, p, delta, oversample,
                         ws[2 + 2 * b], ws[3 + 2 * b], ws[0], objective, o, L.n_series * n_period, red_d, red_i);
  }
}

// kLsFreq frequencies per workgroup, lanes over the cadences, series over blockIdx.y
__global__ __launch_bounds__(kLsThreads) void lomb_scargle_kernel(const double* __restrict__ freq, int64_t n_freq, Layout L,
                                                                  const double* __restrict__ ws, double* __restrict__ out) {
  __shared__ double red[kLsThreads / kWave][kLsFreq][7];
  const int64_t f0 = (int64_t)blockIdx.x * kLsFreq, b = blockIdx.y, n = L.n;
  const double* __restrict__ tt = ws + L.tt();
  const double* __restrict__ w = ws + L.w(b);
  const double* __restrict__ wy = ws + L.wy(b);
  const double span = ws[1] - ws[0];
  double f[kLsFreq], kappa[kLsFreq];
  LsSums a[kLsFreq];
#pragma unroll
  for (int j = 0; j < kLsFreq; ++j) {
    f[j] = freq[f0 + j < n_freq ? f0 + j : n_freq - 1];
    kappa[j] = ls_kappa(f[j], span);
    a[j] = LsSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  }
  for (int64_t i = threadIdx.x; i < n; i += kLsThreads) {
    const double ti = tt[i], wi = w[i], wyi = wy[i];
#pragma unroll
    for (int j = 0; j < kLsFreq; ++j) {
      double sn, cs;
      sincospi(2.0 * ls_phase_turns(f[j], ti), &sn, &cs);
      ls_accumulate(a[j], wi, wyi, sn, cs, kappa[j]);
    }
  }
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
  for (int j = 0; j < kLsFreq; ++j) {
    const double v[7] = {wave_sum(a[j].ys), wave_sum(a[j].yc), wave_sum(a[j].s), wave_sum(a[j].c),
                         wave_sum(a[j].ss), wave_sum(a[j].cc), wave_sum(a[j].sc)};
    if (lane == 0)
      for (int q = 0; q < 7; ++q) red[wave][j][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < kLsFreq && f0 + threadIdx.x < n_freq) {
    double v[7];
    for (int q = 0; q < 7; ++q) {
      v[q] = 0.0;
      for (int i = 0; i < kLsThreads / kWave; ++i) v[q] += red[i][threadIdx.x][q];
    }
    out[b * n_freq + f0 + threadIdx.x] = ls_power(LsSums{v[0], v[1], v[2], v[3], v[4], v[5], v[6]}, ws[3 + 2 * b], ws[2 + 2 * b]);
  }
}

inline bool series_ok(int64_t n, int64_t n_series, int64_t n_yerr) {
  return n >= 1 && n <= INT32_MAX && n_series >= 1 && n_series <= 65535 && (n_yerr == 0 || n_yerr == 1 || n_yerr == n_series);
}

inline Layout layout(int64_t n, int64_t n_series, int64_t n_yerr) { return Layout{n, n_series, n_yerr > 1 ? n_series : 1}; }

inline int64_t n_slabs(int64_t n_series, int64_t n_period, int64_t max_bins) {
  if (max_bins <= kLdsBins) return 0;
  const int64_t items = n_series * n_period;
  return items < kMaxSlabs ? items : kMaxSlabs;
}

inline int64_t gcd(int64_t a, int64_t b) { return b ? gcd(b, a % b) : a; }

inline void prepare(const double* t, const double* y, const double* yerr, int64_t n_yerr, const Layout& L, int centre, double* ws,
                    hipStream_t stream) {
  int64_t stride = L.n / 61 + 1;  // (n < 2^31 * 61: j * stride stays far inside int64)
  while (gcd(stride, L.n) != 1) ++stride;
  hipLaunchKernelGGL(est_range_kernel, dim3(1), dim3(kPrepThreads), 0, stream, t, L.n, ws);
  hipLaunchKernelGGL(est_prepare_kernel, dim3((unsigned)L.n_series), dim3(kPrepThreads), 0, stream, t, y, yerr, n_yerr, L, centre,
                     stride, ws);
}

// the arguments that exo_bls_power_f64 and exo_tls_power_f64 share
struct SearchCall {
  const double *t, *y, *yerr;
  int64_t n_yerr, n, n_series;
  const double* periods;
  int64_t n_period, min_bins, max_bins;
  const int32_t* duration_bins;
  int32_t n_duration;
  double delta;
  int32_t oversample, objective;
  double* out;
  void* workspace;
  int64_t workspace_bytes;
  void* stream;
};

inline bool search_args_ok(const SearchCall& c) {
  return series_ok(c.n, c.n_series, c.n_yerr) && c.n_period >= 0 && c.n_period <= INT32_MAX && c.t && c.y &&
         (c.n_yerr <= 0 || c.yerr) && c.periods && c.duration_bins && c.n_duration >= 1 && c.n_duration <= kMaxDur &&
         c.delta > 0.0 && c.oversample >= 1 && (c.objective == EXO_BLS_LIKELIHOOD || c.objective == EXO_BLS_SNR) &&
         c.min_bins >= 1 && c.max_bins >= c.min_bins && c.out && c.workspace;
}

// the durations into `search`, the workspace, the columns, and the search's kernel pair over the periods (table: the template
// search's, else null)
template <class Search>
inline int launch_search(Search search, const double* table, const SearchCall& c) {
  search.dur = Durations{};
  search.n_dur = (int)c.n_duration;
  for (int k = 0; k < c.n_duration; ++k) {
    if (c.duration_bins[k] < 1) return EXO_ERR_INVALID_ARGUMENT;
    search.dur.m[k] = c.duration_bins[k];
  }
  if (c.workspace_bytes < exo_bls_workspace_bytes(c.n, c.n_series, c.n_period, c.max_bins)) return EXO_ERR_WORKSPACE;
  const Layout L = layout(c.n, c.n_series, c.n_yerr);
  double* ws = (double*)c.workspace;
  hipStream_t s = (hipStream_t)c.stream;
  prepare(c.t, c.y, c.n_yerr > 0 ? c.yerr : nullptr, c.n_yerr, L, 0, ws, s);
  // which kernel a period takes depends on its bin count alone (bls_n_bins, the same division on both sides)
  if (c.min_bins <= kLdsBins) {
    const int64_t bins = c.max_bins < kLdsBins ? c.max_bins : kLdsBins;
    hipLaunchKernelGGL(search_lds_kernel<Search>, dim3((unsigned)c.n_period, (unsigned)c.n_series), dim3(kBlsThreads),
                       (size_t)(16 * (bins + 1)), s, c.periods, c.n_period, L, c.delta, (int)c.oversample, search, table,
                       (int)c.objective, bins, (const double*)ws, c.out);
  }
  if (c.max_bins > kLdsBins)
    hipLaunchKernelGGL(search_slab_kernel<Search>, dim3((unsigned)n_slabs(c.n_series, c.n_period, c.max_bins)), dim3(kSlabThreads), 0,
                       s, c.periods, c.n_period, L, c.delta, (int)c.oversample, search, table, (int)c.objective, c.max_bins, ws, c.out);
  return launch_status();
}

}  // namespace

extern "C" {

int64_t exo_bls_workspace_bytes(int64_t n, int64_t n_series, int64_t n_period, int64_t max_bins) {
  if (n < 1 || n_series < 1 || n_period < 0 || max_bins < 0) return -1;
  // (sized for per-series weights, the larger of the two layouts)
  const Layout L = layout(n, n_series, n_series);
  return 8 * (L.slabs() + n_slabs(n_series, n_period, max_bins) * 2 * (max_bins + 1));
}

int exo_bls_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                      const double* periods, int64_t n_period, int64_t min_bins, int64_t max_bins, const int32_t* duration_bins,
                      int32_t n_duration, double delta, int32_t oversample, int32_t objective, double* out, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  const SearchCall c{t, y, yerr, n_yerr, n, n_series, periods, n_period, min_bins, max_bins, duration_bins, n_duration, delta,
                     oversample, objective, out, workspace, workspace_bytes, stream};
  if (n_period == 0) return EXO_OK;
  if (!search_args_ok(c)) return EXO_ERR_INVALID_ARGUMENT;
  return launch_search(BoxSearch{}, nullptr, c);
}

int exo_tls_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                      const double* periods, int64_t n_period, int64_t min_bins, int64_t max_bins, const int32_t* duration_bins,
                      int32_t n_duration, double delta, int32_t oversample, int32_t objective, const double* templates,
                      const int32_t* template_offsets, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
  const SearchCall c{t, y, yerr, n_yerr, n, n_series, periods, n_period, min_bins, max_bins, duration_bins, n_duration, delta,
                     oversample, objective, out, workspace, workspace_bytes, stream};
  if (n_period == 0) return EXO_OK;
  if (!search_args_ok(c) || !templates || !template_offsets || template_offsets[0] < 0) return EXO_ERR_INVALID_ARGUMENT;
  TemplateSearch search{};
  search.tpl.off[0] = template_offsets[0];
  for (int k = 0; k < n_duration; ++k) {
    // template k holds duration_bins[k] entries (in int64: an offset near INT32_MAX must not wrap into a match)
    if ((int64_t)template_offsets[k] + duration_bins[k] != template_offsets[k + 1] || template_offsets[k + 1] > EXO_TLS_MAX_TEMPLATE)
      return EXO_ERR_INVALID_ARGUMENT;
    search.tpl.off[k + 1] = template_offsets[k + 1];
  }
  return launch_search(search, templates, c);
}

int exo_lomb_scargle_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                               const double* frequencies, int64_t n_frequency, double* power, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  if (n_frequency == 0) return EXO_OK;
  if (!series_ok(n, n_series, n_yerr) || n_frequency < 0 || !t || !y || (n_yerr > 0 && !yerr) || !frequencies || !power ||
      !workspace)
    return EXO_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < exo_bls_workspace_bytes(n, n_series, 0, 0)) return EXO_ERR_WORKSPACE;
  const Layout L = layout(n, n_series, n_yerr);
  double* ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  prepare(t, y, n_yerr > 0 ? yerr : nullptr, n_yerr, L, 1, ws, s);
  hipLaunchKernelGGL(lomb_scargle_kernel, dim3((unsigned)((n_frequency + kLsFreq - 1) / kLsFreq), (unsigned)n_series),
                     dim3(kLsThreads), 0, s, frequencies, n_frequency, L, (const double*)ws, power);
  return launch_status();
}

}  // extern "C"
