// exo_keplerian.hip -- the Keplerian periodogram of a batch of radial-velocity series on one time axis
// (exoplanet_amd/estimators.py: keplerian_power, keplerian_estimator): at every frequency the best of a grid of
// (eccentricity, phase of periastron) candidates, each a linear least-squares fit of  c_k + A cos nu + B sin nu  with one
// constant per instrument.  A translation unit of its own: none of the other kernels changes.  The arithmetic lives in
// exo_keplerian_core.hpp (tested on the host); definition, layout, resources and timings: DESIGN.md section 22.  Compiled
// with -ffp-contract=off, as the host build of the core is.
//
// The search: a workgroup owns one (frequency, series).  The epochs arrive sorted by instrument; a tile of kTile of them --
// the reduced phase f (t - t_min) in turns, w and w y -- is staged in LDS, and lane l takes the candidates l, l + threads, ...:
// for each it walks all epochs in order, segment by segment, every lane reading the same LDS address (a broadcast), with the
// five running sums, the two sums of the open segment and its reference values in registers.  Every sum therefore has one
// fixed order: no atomics, no sums across lanes.  The only reduction is the arg-max of (power, lowest candidate number) over
// the wave and then the workgroup.  The winner's sums are then formed once more, the lanes solving Kepler's equation for a tile of epochs side by
// side and lane 0 adding them up in the order of the search, which gives the constants of the instruments without a
// per-instrument accumulator in any lane of the search.  Nothing but kernels is enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_keplerian_core.hpp"

namespace {

using namespace kep;

constexpr int kWave = 64;
constexpr int kMaxThreads = 256;
constexpr int kTile = 256;  // epochs staged at a time: N is not capped by LDS
constexpr int kPrepThreads = 256;
constexpr int kMaxInst = EXO_KEP_MAX_INSTRUMENTS;
constexpr int kMaxEcc = EXO_KEP_MAX_ECC;

// the segments of the instruments, epochs off[k] .. off[k + 1] - 1 (checked on the host: 0 = off[0] < off[1] < ... = n), and
// the eccentricity grid: both travel by value in the kernel arguments
struct Segments {
  int32_t n_inst;
  int32_t off[kMaxInst + 1];
};
struct EccGrid {
  int32_t n;
  double e[kMaxEcc];
};

// workspace, in doubles: tt[n], w[n_w][n], w y[n_series][n], then per series W_k, Y_k of the kMaxInst segments
struct Layout {
  int64_t n, n_series, n_w;
  __host__ __device__ int64_t tt() const { return 0; }
  __host__ __device__ int64_t w(int64_t b) const { return n + (n_w > 1 ? b : 0) * n; }
  __host__ __device__ int64_t wy(int64_t b) const { return n + n_w * n + b * n; }
  __host__ __device__ int64_t totals(int64_t b) const { return n + n_w * n + n_series * n + b * 2 * kMaxInst; }
  __host__ __device__ int64_t size() const { return totals(n_series); }
};

// The columns the search reads -- tt = t - t_min, w = 1 / yerr^2 (1 without), w y -- and the totals of every segment, summed
// in a fixed shape (lane partials over the segment's epochs, then a tree).  One workgroup per series.
__global__ __launch_bounds__(kPrepThreads) void keplerian_prepare_kernel(const double* __restrict__ t, const double* __restrict__ y,
                                                                         const double* __restrict__ yerr, int64_t n_yerr, Layout L,
                                                                         Segments seg, double* __restrict__ ws) {
  __shared__ double red_a[kPrepThreads], red_b[kPrepThreads];
  const int64_t b = blockIdx.x, n = L.n;
  const int lane = threadIdx.x;
  double lo = INFINITY;
  for (int64_t i = lane; i < n; i += kPrepThreads) lo = fmin(lo, t[i]);
  red_a[lane] = lo;
  __syncthreads();
  for (int o = kPrepThreads / 2; o > 0; o >>= 1) {
    if (lane < o) red_a[lane] = fmin(red_a[lane], red_a[lane + o]);
    __syncthreads();
  }
  const double t_min = red_a[0];
  __syncthreads();  // (the reduction's array is used again below)
  const double* e = yerr ? yerr + (n_yerr > 1 ? b : 0) * n : nullptr;
  const bool write_w = L.n_w > 1 || b == 0;
  double* tt = ws + L.tt();
  double* w = ws + L.w(b);
  double* wy = ws + L.wy(b);
  double* totals = ws + L.totals(b);
  for (int k = 0; k < seg.n_inst; ++k) {
    double sw = 0.0, swy = 0.0;
    for (int64_t i = seg.off[k] + lane; i < seg.off[k + 1]; i += kPrepThreads) {
      const double wi = e ? 1.0 / (e[i] * e[i]) : 1.0, wyi = wi * y[b * n + i];
      if (b == 0) tt[i] = t[i] - t_min;
      if (write_w) w[i] = wi;
      wy[i] = wyi;
      sw += wi;
      swy += wyi;
    }
    red_a[lane] = sw;
    red_b[lane] = swy;
    __syncthreads();
    for (int o = kPrepThreads / 2; o > 0; o >>= 1) {
      if (lane < o) {
        red_a[lane] += red_a[lane + o];
        red_b[lane] += red_b[lane + o];
      }
      __syncthreads();
    }
    if (lane == 0) {
      totals[2 * k] = red_a[0];
      totals[2 * k + 1] = red_b[0];
    }
    __syncthreads();
  }
}

// what a candidate needs beside the staged epochs
struct Candidate {
  double e, se, pe, phi;
  bool live;
};

__device__ __forceinline__ Candidate candidate_of(int c, int n_cand, int n_phase, const double* e_s) {
  Candidate r;
  const int j = c / n_phase, k = c - j * n_phase;
  const double e = c < n_cand ? e_s[j] : -1.0;
  r.live = c < n_cand && is_candidate(e, k);
  r.e = r.live ? e : 0.5;
  r.se = sqrt(1.0 - r.e);
  r.pe = sqrt(1.0 + r.e);
  r.phi = (double)k / (double)n_phase;
  return r;
}

// The search and the winner's record.  grid: (frequencies, series); blockDim: 64, 128 or 256.
__global__ __launch_bounds__(kMaxThreads) void keplerian_kernel(const double* __restrict__ freq, Layout L, Segments seg, EccGrid grid,
                                                                int32_t n_phase, const double* __restrict__ ws,
                                                                double* __restrict__ power, int32_t* __restrict__ candidate,
                                                                double* __restrict__ coef) {
  __shared__ double turns_s[kTile], w_s[kTile], wy_s[kTile], sn_s[kTile], cs_s[kTile];
  __shared__ double e_s[kMaxEcc], red_p[kMaxThreads / kWave];
  __shared__ int32_t red_c[kMaxThreads / kWave];
  __shared__ Segment seg_g[kMaxInst];  // (the winner's segments as they were folded: lane 0 alone)
  const int64_t jf = blockIdx.x, n_freq = gridDim.x, b = blockIdx.y, n = L.n;
  const int lane = threadIdx.x, nt = blockDim.x;
  const double f = freq[jf];
  const double* __restrict__ tt = ws + L.tt();
  const double* __restrict__ w = ws + L.w(b);
  const double* __restrict__ wy = ws + L.wy(b);
  const double* __restrict__ totals = ws + L.totals(b);
  const int n_cand = grid.n * n_phase;
  for (int q = lane; q < grid.n; q += nt) e_s[q] = grid.e[q];
  double W = 0.0;
  for (int k = 0; k < seg.n_inst; ++k) W += totals[2 * k];
  __syncthreads();

  // ---- the search: this lane's candidates, ascending, so that a strict > keeps the lowest of equal maxima
  Best best = best_init();
  for (int c0 = 0; c0 < n_cand; c0 += nt) {
    const int c = c0 + lane;
    const Candidate cd = candidate_of(c, n_cand, n_phase, e_s);
    Sums a = {0.0, 0.0, 0.0, 0.0, 0.0};
    Segment g = {0.0, 0.0, 0.0, 0.0};
    for (int64_t lo = 0; lo < n; lo += kTile) {
      const int len = (int)(n - lo < kTile ? n - lo : kTile);
      __syncthreads();  // (every lane is done with the tile before)
      for (int i = lane; i < len; i += nt) {
        turns_s[i] = est::ls_phase_turns(f, tt[lo + i]);
        w_s[i] = w[lo + i];
        wy_s[i] = wy[lo + i];
      }
      __syncthreads();
      if (cd.live) {
        for (int k = 0; k < seg.n_inst; ++k) {
          const int64_t end = seg.off[k + 1];
          const int i0 = (int)((seg.off[k] > lo ? seg.off[k] : lo) - lo), i1 = (int)((end < lo + len ? end : lo + len) - lo);
          for (int i = i0; i < i1; ++i) {
            double sn, cs;
            true_anomaly(turns_s[i], cd.phi, cd.e, cd.se, cd.pe, &sn, &cs);
            accumulate(a, g, lo + i == seg.off[k], w_s[i], wy_s[i], sn, cs);
          }
          if (end > lo && end <= lo + len) fold(a, g, totals[2 * k], totals[2 * k + 1]);
        }
      }
    }
    if (cd.live) best_take(best, fit(a, W).power, c);
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double p = __shfl_down(best.power, o, kWave);
    const int32_t c = __shfl_down(best.candidate, o, kWave);
    best_take(best, p, c);
  }
  if (lane % kWave == 0) {
    red_p[lane / kWave] = best.power;
    red_c[lane / kWave] = best.candidate;
  }
  __syncthreads();
  best = best_init();
  for (int i = 0; i < nt / kWave; ++i) best_take(best, red_p[i], red_c[i]);

  // ---- the winner's record: power, candidate, A, B and the constants of the instruments
  const int64_t slot = b * n_freq + jf;
  const int n_coef = 2 + seg.n_inst;
  if (best.candidate == INT32_MAX) {  // (no candidate with a finite power: -inf, the rest NaN)
    if (lane == 0) {
      power[slot] = -INFINITY;
      candidate[slot] = -1;
      for (int q = 0; q < n_coef; ++q) coef[slot * n_coef + q] = NAN;
    }
    return;
  }
  const Candidate cd = candidate_of(best.candidate, n_cand, n_phase, e_s);
  Sums a = {0.0, 0.0, 0.0, 0.0, 0.0};
  Segment g = {0.0, 0.0, 0.0, 0.0};
  for (int64_t lo = 0; lo < n; lo += kTile) {
    const int len = (int)(n - lo < kTile ? n - lo : kTile);
    __syncthreads();
    for (int i = lane; i < len; i += nt) {
      double sn, cs;
      true_anomaly(est::ls_phase_turns(f, tt[lo + i]), cd.phi, cd.e, cd.se, cd.pe, &sn, &cs);
      sn_s[i] = sn;
      cs_s[i] = cs;
      w_s[i] = w[lo + i];
      wy_s[i] = wy[lo + i];
    }
    __syncthreads();
    if (lane == 0) {
      for (int k = 0; k < seg.n_inst; ++k) {
        const int64_t end = seg.off[k + 1];
        const int i0 = (int)((seg.off[k] > lo ? seg.off[k] : lo) - lo), i1 = (int)((end < lo + len ? end : lo + len) - lo);
        for (int i = i0; i < i1; ++i) accumulate(a, g, lo + i == seg.off[k], w_s[i], wy_s[i], sn_s[i], cs_s[i]);
        if (end > lo && end <= lo + len) {
          seg_g[k] = g;
          fold(a, g, totals[2 * k], totals[2 * k + 1]);
        }
      }
    }
  }
  if (lane != 0) return;
  const Fit r = fit(a, W);
  power[slot] = r.power;
  candidate[slot] = best.candidate;
  coef[slot * n_coef] = r.A;
  coef[slot * n_coef + 1] = r.B;
  for (int k = 0; k < seg.n_inst; ++k)
    coef[slot * n_coef + 2 + k] = constant(totals[2 * k], totals[2 * k + 1], seg_g[k], r.A, r.B);
}

inline Layout layout(int64_t n, int64_t n_series, int64_t n_yerr) { return Layout{n, n_series, n_yerr > 1 ? n_series : 1}; }

// lanes per workgroup: of 256, 128 and 64 the count whose passes over the candidates leave the fewest lanes idle (the larger
// of equals)
inline int threads_for(int64_t n_cand) {
  int best = kMaxThreads;
  for (int nt = kMaxThreads; nt >= kWave; nt /= 2)
    if ((n_cand + nt - 1) / nt * nt < (n_cand + best - 1) / best * best) best = nt;
  return best;
}

}  // namespace

extern "C" {

int64_t exo_keplerian_workspace_bytes(int64_t n, int64_t n_series) {
  if (n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535) return -1;
  // (sized for per-series weights, the larger of the two layouts)
  return 8 * layout(n, n_series, n_series).size();
}

int exo_keplerian_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                            const int32_t* segment_offsets, int32_t n_instrument, const double* frequencies, int64_t n_frequency,
                            const double* ecc, int32_t n_ecc, int32_t n_phase, double* power, int32_t* candidate, double* coef,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_frequency == 0) return EXO_OK;
  if (!t || !y || (n_yerr > 0 && !yerr) || !segment_offsets || !frequencies || !ecc || !power || !candidate || !coef ||
      !workspace || n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535 ||
      (n_yerr != 0 && n_yerr != 1 && n_yerr != n_series) || n_frequency < 0 || n_frequency > INT32_MAX || n_instrument < 1 ||
      n_instrument > kMaxInst || n_ecc < 1 || n_ecc > kMaxEcc || n_phase < 1 || n_phase > EXO_KEP_MAX_PHASES)
    return EXO_ERR_INVALID_ARGUMENT;
  Segments seg = {};
  seg.n_inst = n_instrument;
  for (int k = 0; k <= n_instrument; ++k) {
    // every instrument holds an epoch, and the segments tile 0 .. n
    if (k == 0 ? segment_offsets[0] != 0 : segment_offsets[k] <= segment_offsets[k - 1]) return EXO_ERR_INVALID_ARGUMENT;
    seg.off[k] = segment_offsets[k];
  }
  if (segment_offsets[n_instrument] != n) return EXO_ERR_INVALID_ARGUMENT;
  EccGrid grid = {};
  grid.n = n_ecc;
  for (int j = 0; j < n_ecc; ++j) {
    if (!(ecc[j] >= 0.0 && ecc[j] < 1.0)) return EXO_ERR_INVALID_ARGUMENT;
    grid.e[j] = ecc[j];
  }
  if (workspace_bytes < exo_keplerian_workspace_bytes(n, n_series)) return EXO_ERR_WORKSPACE;
  const Layout L = layout(n, n_series, n_yerr);
  double* ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(keplerian_prepare_kernel, dim3((unsigned)n_series), dim3(kPrepThreads), 0, s, t, y, n_yerr > 0 ? yerr : nullptr,
                     n_yerr, L, seg, ws);
  hipLaunchKernelGGL(keplerian_kernel, dim3((unsigned)n_frequency, (unsigned)n_series), dim3(threads_for((int64_t)n_ecc * n_phase)), 0,
                     s, frequencies, L, seg, grid, n_phase, (const double*)ws, power, candidate, coef);
  return launch_status();
}

}  // extern "C"
