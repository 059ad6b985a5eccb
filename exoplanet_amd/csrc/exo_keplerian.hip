// exo_keplerian.hip -- the Keplerian periodogram of a batch of radial-velocity series on one time axis
// (exoplanet_amd/estimators.py: keplerian_power, keplerian_estimator): at every frequency the best of a grid of
// (eccentricity, phase of periastron) candidates, each a linear least-squares fit of  c_k + A cos nu + B sin nu  with one
// constant per instrument.  A translation unit of its own: none of the other kernels changes.  The arithmetic lives in
// exo_keplerian_core.hpp (tested on the host), the search over the candidates in exo_orbit_search.hpp; definition, layout,
// resources and timings: DESIGN.md section 22.  Beside it the highest peak of every series without the periodogram
// (keplerian_max_power, false_alarm): groups of series that share every solve of Kepler's equation, exo_keplerian_max.hpp and
// DESIGN.md section 26.  Compiled with -ffp-contract=off, as the host builds of the two headers are.  Nothing but kernels is
// enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_keplerian_core.hpp"
#include "exo_keplerian_max.hpp"
#include "exo_orbit_search.hpp"

namespace {

using namespace kep;
using namespace orb;

constexpr int kMaxInst = EXO_KEP_MAX_INSTRUMENTS;

// the segments of the instruments, epochs off[k] .. off[k + 1] - 1 (checked on the host: 0 = off[0] < off[1] < ... = n): they
// travel by value in the kernel arguments
struct Segments {
  int32_t n_inst;
  int32_t off[kMaxInst + 1];
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
  __shared__ double red[kPrepThreads];
  const int64_t b = blockIdx.x, n = L.n;
  const int lane = threadIdx.x;
  const double t_min = block_min(t, n, red);
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
    const double Wk = block_sum(sw, red), Yk = block_sum(swy, red);
    if (lane == 0) {
      totals[2 * k] = Wk;
      totals[2 * k + 1] = Yk;
    }
  }
}

// the problem of exo_orbit_search.hpp: a tile carries w and w y; a candidate keeps the five sums and the open segment, all
// zero at first; its score is the power of the 2 x 2 fit; a lane keeps nothing of its best (the winner is walked again)
struct KeplerianProblem {
  const double* __restrict__ w;
  const double* __restrict__ wy;
  const double* __restrict__ totals;
  double* w_s;
  double* wy_s;
  const Segments& seg;
  double W;

  struct State {
    Sums a;
    Segment g;
  };
  using Fit = kep::Fit;

  __device__ __forceinline__ void stage(int64_t lo, int i) const {
    w_s[i] = w[lo + i];
    wy_s[i] = wy[lo + i];
  }
  __device__ __forceinline__ void walk(State& s, const Candidate& cd, const double* turns_s, int64_t lo, int len) const {
    for (int k = 0; k < seg.n_inst; ++k) {
      const int64_t end = seg.off[k + 1];
      const int i0 = (int)((seg.off[k] > lo ? seg.off[k] : lo) - lo), i1 = (int)((end < lo + len ? end : lo + len) - lo);
      for (int i = i0; i < i1; ++i) {
        double sn, cs;
        true_anomaly(turns_s[i], cd.phi, cd.e, cd.se, cd.pe, &sn, &cs);
        accumulate(s.a, s.g, lo + i == seg.off[k], w_s[i], wy_s[i], sn, cs);
      }
      if (end > lo && end <= lo + len) fold(s.a, s.g, totals[2 * k], totals[2 * k + 1]);
    }
  }
  __device__ __forceinline__ Fit fit(const State& s) const { return kep::fit(s.a, W); }
  __device__ __forceinline__ bool counts(const Fit&) const { return true; }
};

// The search and the winner's record.  grid: (frequencies, series); blockDim: 64, 128 or 256.
__global__ __launch_bounds__(kMaxThreads) void keplerian_kernel(const double* __restrict__ freq, Layout L, Segments seg, EccGrid grid,
                                                                int32_t n_phase, const double* __restrict__ ws,
                                                                double* __restrict__ power, int32_t* __restrict__ candidate,
                                                                double* __restrict__ coef) {
  __shared__ SearchLds sh;
  __shared__ double w_s[kTile], wy_s[kTile], sn_s[kTile], cs_s[kTile];
  __shared__ Segment seg_g[kMaxInst];  // (the winner's segments as they were folded: lane 0 alone)
  const int64_t jf = blockIdx.x, n_freq = gridDim.x, b = blockIdx.y, n = L.n;
  const int lane = threadIdx.x, nt = blockDim.x;
  const double f = freq[jf];
  const double* __restrict__ tt = ws + L.tt();
  const double* __restrict__ totals = ws + L.totals(b);
  double W = 0.0;
  for (int k = 0; k < seg.n_inst; ++k) W += totals[2 * k];
  const KeplerianProblem problem = {ws + L.w(b), ws + L.wy(b), totals, w_s, wy_s, seg, W};
  Fit unused;
  const Best best = block_best(lane_search(problem, sh, grid, n_phase, f, tt, n, unused), sh);

  // ---- the winner's record: power, candidate, A, B and the constants of the instruments.  The search keeps no sums per
  // instrument (eight pairs per lane would be an indexed array), so the winner's are formed once more: the lanes solve Kepler's
  // equation for a tile of epochs side by side, and lane 0 adds them up in the order of the search
  const int64_t slot = b * n_freq + jf;
  const int n_coef = 2 + seg.n_inst;
  if (best.candidate == INT32_MAX) {  // (no candidate with a finite power: -inf, the rest NaN)
    write_no_candidate(-INFINITY, slot, n_coef, power, candidate, coef);
    return;
  }
  const Candidate cd = candidate_of(best.candidate, grid.n * n_phase, n_phase, sh.e);
  Sums a = {};
  Segment g = {};
  for (int64_t lo = 0; lo < n; lo += kTile) {
    const int len = (int)(n - lo < kTile ? n - lo : kTile);
    __syncthreads();
    for (int i = lane; i < len; i += nt) {
      true_anomaly(est::ls_phase_turns(f, tt[lo + i]), cd.phi, cd.e, cd.se, cd.pe, &sn_s[i], &cs_s[i]);
      problem.stage(lo, i);
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

// ---- the highest peak of every series, without the periodogram -----------------------------------------

using kepmax::Best3;
constexpr int kMaxTile = kepmax::kTile;
constexpr int kTotals = kepmax::kTotals;
constexpr int kMaxWaves = kMaxThreads / kWave;

// the partial results behind the columns of `ws`: per (series, block of frequencies) a power, then a (frequency, candidate) pair
struct Partials {
  int64_t at, n_series, n_block;  // `at`: the doubles before them, Layout::size()
  __host__ __device__ int64_t power(int64_t b, int64_t blk) const { return at + b * n_block + blk; }
  // (counted in int32)
  __host__ __device__ int64_t index(int64_t b, int64_t blk) const { return 2 * (at + n_series * n_block + b * n_block + blk); }
  __host__ __device__ int64_t bytes() const { return 8 * at + 16 * n_series * n_block; }
};

// epochs lo .. lo + len - 1 of the group's columns into the tile: w and w y of a series side by side, the series of an epoch
// next to each other (kepmax::group_walk)
template <int G>
__device__ __forceinline__ void stage_pairs(const double* __restrict__ ws, const Layout& L, int64_t b0, int64_t lo, int len,
                                            double* pair_s) {
  for (int q = threadIdx.x; q < len * G; q += blockDim.x) {
    const int g = q / len, i = q - g * len;
    const int64_t b = kepmax::group_series(b0, g, L.n_series);
    pair_s[(i * G + g) * 2] = ws[L.w(b) + lo + i];
    pair_s[(i * G + g) * 2 + 1] = ws[L.wy(b) + lo + i];
  }
}

// The search of a block of `per_block` consecutive frequencies for a group of G series.  grid: (blocks of frequencies, groups
// of series); blockDim: that of keplerian_kernel for the same candidates, so that a lane owns the candidates it owns there and
// a candidate's power is the one found there.  Per frequency: every lane walks its candidates for the G series at once
// (kepmax::group_walk); the workgroup's arg-max over the candidates, per series, ends in lane g for series g (block_best's
// rule: over the wave by shuffles, over the waves through LDS); that lane keeps the series' best over the block's frequencies
// and writes it at the end.  A winner of e = 0 is walked once more by the whole workgroup, every lane on that one candidate,
// as keplerian_kernel walks every winner for its record: the solver's circular branch is taken when a whole wave is circular,
// which the record's walk is and the search's, one candidate to a lane, is not, and the power the periodogram holds is the
// record's.
template <int G>
__global__ __launch_bounds__(kMaxThreads) void keplerian_max_kernel(const double* __restrict__ freq, int32_t n_freq, int32_t per_block,
                                                                    Layout L, Segments seg, EccGrid grid, int32_t n_phase,
                                                                    double* __restrict__ ws, Partials P) {
  __shared__ double turns_s[kMaxTile], sn_s[kMaxTile], cs_s[kMaxTile], e_s[kMaxEcc];
  __shared__ __align__(16) double pair_s[kMaxTile * G * 2];
  __shared__ double tot_s[G * kTotals], W_s[G];
  __shared__ double red_p[G][kMaxWaves];
  __shared__ int32_t red_c[G][kMaxWaves];
  const int lane = threadIdx.x, nt = blockDim.x;
  const int64_t blk = blockIdx.x, b0 = (int64_t)blockIdx.y * G, n = L.n;
  const int n_cand = grid.n * n_phase;
  const double* __restrict__ tt = ws + L.tt();
  for (int q = lane; q < grid.n; q += nt) e_s[q] = grid.e[q];
  for (int q = lane; q < G * kTotals; q += nt)
    tot_s[q] = q % kTotals < 2 * seg.n_inst ? ws[L.totals(kepmax::group_series(b0, q / kTotals, L.n_series)) + q % kTotals] : 0.0;
  __syncthreads();
  if (lane < G) W_s[lane] = kepmax::total_weight(tot_s + lane * kTotals, seg.n_inst);
  __syncthreads();

  Best3 mine = kepmax::best3_init();  // (lane g < G: series b0 + g over the block's frequencies)
  const int64_t jf0 = blk * per_block, jf1 = jf0 + per_block < n_freq ? jf0 + per_block : n_freq;
  for (int32_t jf = (int32_t)jf0; jf < jf1; ++jf) {
    const double f = freq[jf];
    Best best[G];
#pragma unroll
    for (int g = 0; g < G; ++g) best[g] = best_init();
    for (int c0 = 0; c0 < n_cand; c0 += nt) {
      const int c = c0 + lane;
      const Candidate cd = candidate_of(c, n_cand, n_phase, e_s);
      kepmax::GroupState<G> st = {};
      for (int64_t lo = 0; lo < n; lo += kMaxTile) {
        const int len = (int)(n - lo < kMaxTile ? n - lo : kMaxTile);
        __syncthreads();  // (every lane is done with the tile before)
        for (int i = lane; i < len; i += nt) turns_s[i] = est::ls_phase_turns(f, tt[lo + i]);
        stage_pairs<G>(ws, L, b0, lo, len, pair_s);
        __syncthreads();
        if (cd.live) kepmax::group_walk<G>(st, cd, turns_s, pair_s, tot_s, seg.off, seg.n_inst, lo, len);
      }
      if (cd.live) {
#pragma unroll
        for (int g = 0; g < G; ++g) best_take(best[g], kep::fit(st.a[g], W_s[g]).power, c);
      }
    }
    // the arg-max over the candidates: series g's into lane g
#pragma unroll
    for (int g = 0; g < G; ++g) {
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const double p = __shfl_down(best[g].power, o, kWave);
        const int32_t c = __shfl_down(best[g].candidate, o, kWave);
        best_take(best[g], p, c);
      }
      if (lane % kWave == 0) {
        red_p[g][lane / kWave] = best[g].power;
        red_c[g][lane / kWave] = best[g].candidate;
      }
    }
    __syncthreads();
    Best win = best_init();
    if (lane < G)
      for (int i = 0; i < nt / kWave; ++i) best_take(win, red_p[lane][i], red_c[lane][i]);
    const bool found = win.candidate != INT32_MAX;
    const bool circular = found && e_s[win.candidate / n_phase] == 0.0;
    if (__syncthreads_or(circular)) {
      // (every winner of e = 0 is this candidate, whatever its number: phase 0 alone is one where e = 0)
      const Candidate cd = {0.0, 1.0, 1.0, 0.0, true};
      Sums a = {};
      Segment sg = {};
      for (int64_t lo = 0; lo < n; lo += kMaxTile) {
        const int len = (int)(n - lo < kMaxTile ? n - lo : kMaxTile);
        __syncthreads();
        for (int i = lane; i < len; i += nt)
          true_anomaly(est::ls_phase_turns(f, tt[lo + i]), cd.phi, cd.e, cd.se, cd.pe, &sn_s[i], &cs_s[i]);
        stage_pairs<G>(ws, L, b0, lo, len, pair_s);
        __syncthreads();
        if (circular) {
          for (int k = 0; k < seg.n_inst; ++k) {
            const int64_t end = seg.off[k + 1];
            const int i0 = (int)((seg.off[k] > lo ? seg.off[k] : lo) - lo), i1 = (int)((end < lo + len ? end : lo + len) - lo);
            for (int i = i0; i < i1; ++i)
              accumulate(a, sg, lo + i == seg.off[k], pair_s[(i * G + lane) * 2], pair_s[(i * G + lane) * 2 + 1], sn_s[i], cs_s[i]);
            if (end > lo && end <= lo + len) fold(a, sg, tot_s[lane * kTotals + 2 * k], tot_s[lane * kTotals + 2 * k + 1]);
          }
        }
      }
      if (circular) win.power = kep::fit(a, W_s[lane]).power;
    }
    if (found) kepmax::best3_take(mine, win.power, jf, win.candidate);
  }
  if (lane < G && b0 + lane < L.n_series) {
    ws[P.power(b0 + lane, blk)] = mine.power;
    int32_t* index = (int32_t*)ws + P.index(b0 + lane, blk);
    index[0] = mine.frequency;
    index[1] = mine.candidate;
  }
}

// a series' partials into its result, by the same rule: one wave per series, the blocks strided over its lanes
__global__ __launch_bounds__(kWave) void keplerian_max_finish_kernel(const double* __restrict__ ws, Partials P,
                                                                     double* __restrict__ max_power,
                                                                     int32_t* __restrict__ frequency_index,
                                                                     int32_t* __restrict__ candidate) {
  const int64_t b = blockIdx.x;
  const int32_t* index = (const int32_t*)ws;
  Best3 m = kepmax::best3_init();
  for (int64_t blk = threadIdx.x; blk < P.n_block; blk += kWave) {
    const int64_t at = P.index(b, blk);
    kepmax::best3_take(m, ws[P.power(b, blk)], index[at], index[at + 1]);
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double p = __shfl_down(m.power, o, kWave);
    const int32_t jf = __shfl_down(m.frequency, o, kWave), c = __shfl_down(m.candidate, o, kWave);
    kepmax::best3_take(m, p, jf, c);
  }
  if (threadIdx.x == 0) {
    max_power[b] = m.power;
    frequency_index[b] = m.frequency;
    candidate[b] = m.candidate;
  }
}

// the series of a group: the width measured fastest (another one for a measurement: -DEXO_KEP_MAX_GROUP=G)
#ifndef EXO_KEP_MAX_GROUP
#define EXO_KEP_MAX_GROUP 8
#endif
constexpr int kGroup = EXO_KEP_MAX_GROUP;

// Frequencies per block when the caller leaves them to the host: the longest block that still gives the device 64 workgroups
// per compute unit (256 of them).  The kernel keeps two waves per SIMD, so the device holds some 2048 waves at a time and a
// grid of about as many runs one round and most of a second for little; with 64 per compute unit the last round is a few
// per cent of the work (measured: DESIGN.md 26.5), and a block still amortises what a workgroup loads once.
inline int64_t block_length(int64_t n_series, int64_t n_frequency, int32_t per_block) {
  if (per_block > 0) return per_block;
  const int64_t groups = (n_series + kGroup - 1) / kGroup, blocks = (64 * 256 + groups - 1) / groups;
  return n_frequency / blocks > 1 ? n_frequency / blocks : 1;
}

inline Partials partials(int64_t n, int64_t n_series, int64_t n_yerr, int64_t n_frequency, int32_t per_block) {
  const int64_t len = block_length(n_series, n_frequency, per_block);
  return Partials{layout(n, n_series, n_yerr).size(), n_series, (n_frequency + len - 1) / len};
}

template <int G>
void launch_max(int64_t n_series, int64_t n_cand, hipStream_t s, const double* frequencies, int32_t n_freq, int32_t per_block,
                const Layout& L, const Segments& seg, const EccGrid& grid, int32_t n_phase, double* ws, const Partials& P) {
  hipLaunchKernelGGL(keplerian_max_kernel<G>, dim3((unsigned)P.n_block, (unsigned)((n_series + G - 1) / G)), dim3(threads_for(n_cand)),
                     0, s, frequencies, n_freq, per_block, L, seg, grid, n_phase, ws, P);
}

// what the two entry points check alike, and the segments and the grid by value
inline int keplerian_arguments(int64_t n, int64_t n_series, int64_t n_yerr, const int32_t* segment_offsets, int32_t n_instrument,
                               int64_t n_frequency, const double* ecc, int32_t n_ecc, int32_t n_phase, Segments* seg, EccGrid* grid) {
  if (!sizes_ok(n, n_series, n_frequency, n_ecc, n_phase) || (n_yerr != 0 && n_yerr != 1 && n_yerr != n_series) || n_instrument < 1 ||
      n_instrument > kMaxInst)
    return EXO_ERR_INVALID_ARGUMENT;
  *seg = Segments{};
  seg->n_inst = n_instrument;
  for (int k = 0; k <= n_instrument; ++k) {
    // every instrument holds an epoch, and the segments tile 0 .. n
    if (k == 0 ? segment_offsets[0] != 0 : segment_offsets[k] <= segment_offsets[k - 1]) return EXO_ERR_INVALID_ARGUMENT;
    seg->off[k] = segment_offsets[k];
  }
  if (segment_offsets[n_instrument] != n) return EXO_ERR_INVALID_ARGUMENT;
  *grid = EccGrid{};
  return ecc_grid(ecc, n_ecc, grid) ? EXO_OK : EXO_ERR_INVALID_ARGUMENT;
}

}  // namespace

extern "C" {

int64_t exo_keplerian_workspace_bytes(int64_t n, int64_t n_series) {
  if (!series_ok(n, n_series)) return -1;
  // (sized for per-series weights, the larger of the two layouts)
  return 8 * layout(n, n_series, n_series).size();
}

int exo_keplerian_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                            const int32_t* segment_offsets, int32_t n_instrument, const double* frequencies, int64_t n_frequency,
                            const double* ecc, int32_t n_ecc, int32_t n_phase, double* power, int32_t* candidate, double* coef,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_frequency == 0) return EXO_OK;
  if (!t || !y || (n_yerr > 0 && !yerr) || !segment_offsets || !frequencies || !ecc || !power || !candidate || !coef || !workspace)
    return EXO_ERR_INVALID_ARGUMENT;
  Segments seg;
  EccGrid grid;
  const int bad = keplerian_arguments(n, n_series, n_yerr, segment_offsets, n_instrument, n_frequency, ecc, n_ecc, n_phase, &seg, &grid);
  if (bad) return bad;
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

int64_t exo_keplerian_max_workspace_bytes(int64_t n, int64_t n_series, int64_t n_frequency, int32_t frequencies_per_block) {
  if (!series_ok(n, n_series) || n_frequency < 0 || n_frequency > INT32_MAX || frequencies_per_block < 0) return -1;
  // (sized for per-series weights, the larger of the two layouts)
  return partials(n, n_series, n_series, n_frequency, frequencies_per_block).bytes();
}

int exo_keplerian_max_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                          const int32_t* segment_offsets, int32_t n_instrument, const double* frequencies, int64_t n_frequency,
                          const double* ecc, int32_t n_ecc, int32_t n_phase, int32_t frequencies_per_block, double* max_power,
                          int32_t* frequency_index, int32_t* candidate, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!t || !y || (n_yerr > 0 && !yerr) || !segment_offsets || !frequencies || !ecc || !max_power || !frequency_index || !candidate ||
      !workspace || frequencies_per_block < 0)
    return EXO_ERR_INVALID_ARGUMENT;
  Segments seg;
  EccGrid grid;
  const int bad = keplerian_arguments(n, n_series, n_yerr, segment_offsets, n_instrument, n_frequency, ecc, n_ecc, n_phase, &seg, &grid);
  if (bad) return bad;
  if (workspace_bytes < exo_keplerian_max_workspace_bytes(n, n_series, n_frequency, frequencies_per_block)) return EXO_ERR_WORKSPACE;
  const Layout L = layout(n, n_series, n_yerr);
  // (the partials lie behind the larger layout, whichever the call uses: the workspace's size does not depend on n_yerr)
  const Partials P = partials(n, n_series, n_series, n_frequency, frequencies_per_block);
  const int32_t per_block = (int32_t)block_length(n_series, n_frequency, frequencies_per_block);
  double* ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(keplerian_prepare_kernel, dim3((unsigned)n_series), dim3(kPrepThreads), 0, s, t, y, n_yerr > 0 ? yerr : nullptr,
                     n_yerr, L, seg, ws);
  // (no frequency: no block, and every series gets the finish kernel's "none")
  if (P.n_block > 0)
    launch_max<kGroup>(n_series, (int64_t)n_ecc * n_phase, s, frequencies, (int32_t)n_frequency, per_block, L, seg, grid, n_phase, ws, P);
  hipLaunchKernelGGL(keplerian_max_finish_kernel, dim3((unsigned)n_series), dim3(kWave), 0, s, (const double*)ws, P, max_power,
                     frequency_index, candidate);
  return launch_status();
}

}  // extern "C"
