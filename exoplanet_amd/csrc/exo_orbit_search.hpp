// exo_orbit_search.hpp -- what the searches over a grid of orbits share (exo_keplerian.hip, exo_astrometric.hip): at every
// (frequency, series) the best of a grid of (eccentricity, phase of periastron) candidates, each a linear least-squares fit
// whose sums run over the epochs in a fixed order, the result the arg-max of (power, lowest candidate number).  A search
// differs in the columns an epoch carries, the sums a candidate keeps and what the winner's record holds: its problem type
// (below).  Three parts: the arithmetic of the candidate grid, which also compiles for the host with EXO_HOST_BUILD (the
// harnesses of tests/ walk it without a GPU); the host side of an entry point; the device side of a kernel.  No device code
// crosses translation units: each unit that includes this gets a copy of its own.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_core.hpp"

namespace orb {

// ---- the candidate grid (host and device) ------------------------------------------------------------------------------------

constexpr double kTwoPi = 6.283185307179586;
constexpr int kWave = 64;
constexpr int kMaxThreads = 256;
constexpr int kTile = 256;  // epochs staged at a time: N is not capped by LDS
constexpr int kPrepThreads = 256;
constexpr int kMaxEcc = EXO_KEP_MAX_ECC;

// a candidate's number j * n_phase + k, phase fastest; where e_j == 0 only k = 0 is one (every phase is the same model there)
EXO_EST_HD bool is_candidate(double e, int k) { return e >= 0.0 && e < 1.0 && (e != 0.0 || k == 0); }

// what a candidate needs beside the staged epochs: se = sqrt(1 - e), pe = sqrt(1 + e), phi = k / n_phase.  One that is not
// live (c past the grid, or a phase of e = 0 other than the first) carries e = 0.5 and is not to be walked.
struct Candidate {
  double e, se, pe, phi;
  bool live;
};
EXO_EST_HD Candidate candidate_of(int c, int n_cand, int n_phase, const double* ecc) {
  Candidate r;
  const int j = c / n_phase, k = c - j * n_phase;
  const double e = c < n_cand ? ecc[j] : -1.0;
  r.live = c < n_cand && is_candidate(e, k);
  r.e = r.live ? e : 0.5;
  r.se = sqrt(1.0 - r.e);
  r.pe = sqrt(1.0 + r.e);
  r.phi = (double)k / (double)n_phase;
  return r;
}

// the arg-max as one value: a larger power wins, an equal one only with a lower candidate number, NaN never
struct Best {
  double power;
  int32_t candidate;
};
EXO_EST_HD Best best_init() { return Best{-INFINITY, INT32_MAX}; }
EXO_EST_HD void best_take(Best& a, double power, int32_t candidate) {
  if (power > a.power || (power == a.power && candidate < a.candidate)) {
    a.power = power;
    a.candidate = candidate;
  }
}

// ---- the host side of an entry point ------------------------------------------------------------------------------------------

// the eccentricity grid: it travels by value in the kernel arguments
struct EccGrid {
  int32_t n;
  double e[kMaxEcc];
};

// the grid, copied; false: an eccentricity outside [0, 1) (a NaN is outside)
inline bool ecc_grid(const double* ecc, int32_t n_ecc, EccGrid* grid) {
  grid->n = n_ecc;
  for (int j = 0; j < n_ecc; ++j) {
    if (!(ecc[j] >= 0.0 && ecc[j] < 1.0)) return false;
    grid->e[j] = ecc[j];
  }
  return true;
}

// the sizes a workspace is laid out for, and those of a call
inline bool series_ok(int64_t n, int64_t n_series) { return n >= 1 && n <= INT32_MAX && n_series >= 1 && n_series <= 65535; }
inline bool sizes_ok(int64_t n, int64_t n_series, int64_t n_frequency, int32_t n_ecc, int32_t n_phase) {
  return series_ok(n, n_series) && n_frequency >= 0 && n_frequency <= INT32_MAX && n_ecc >= 1 && n_ecc <= kMaxEcc && n_phase >= 1 &&
         n_phase <= EXO_KEP_MAX_PHASES;
}

// lanes per workgroup: of 256, 128 and 64 the count whose passes over the candidates leave the fewest lanes idle (the larger
// of equals)
inline int threads_for(int64_t n_cand) {
  int best = kMaxThreads;
  for (int nt = kMaxThreads; nt >= kWave; nt /= 2)
    if ((n_cand + nt - 1) / nt * nt < (n_cand + best - 1) / best * best) best = nt;
  return best;
}

#ifndef EXO_HOST_BUILD

// ---- the device side of a kernel ----------------------------------------------------------------------------------------------

// v of every lane of a workgroup of kPrepThreads combined by a tree of one fixed shape -- kMin: the smallest, else the sum
// -- and known to every lane; red[kPrepThreads] is free again on return
template <bool kMin>
__device__ __forceinline__ double block_tree(double v, double* red) {
  const int lane = threadIdx.x;
  red[lane] = v;
  __syncthreads();
  for (int o = kPrepThreads / 2; o > 0; o >>= 1) {
    if (lane < o) red[lane] = kMin ? fmin(red[lane], red[lane + o]) : red[lane] + red[lane + o];
    __syncthreads();
  }
  const double all = red[0];
  __syncthreads();
  return all;
}
__device__ __forceinline__ double block_sum(double v, double* red) { return block_tree<false>(v, red); }
__device__ __forceinline__ double block_min(const double* __restrict__ t, int64_t n, double* red) {
  double lo = INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) lo = fmin(lo, t[i]);
  return block_tree<true>(lo, red);
}

// the LDS of a search that every problem needs, beside the columns of its own
struct SearchLds {
  double turns[kTile];  // the reduced phase f (t - t_min) of the staged epochs, in turns
  double e[kMaxEcc];
  double red_p[kMaxThreads / kWave];
  int32_t red_c[kMaxThreads / kWave];
};

// The search of one workgroup at the frequency f: lane l takes the candidates l, l + threads, ..., ascending, so that a strict
// > keeps the lowest of equal maxima; for each, a tile of kTile epochs at a time is staged and walked, every lane reading the
// same LDS address (a broadcast).  -> the lane's own best; `kept`: the fit of that candidate, stored only when that best
// changes.  The problem type supplies
//   State (a candidate's sums: zero at first) and Fit (with .power);
//   void stage(lo, i): epoch lo + i of its columns into slot i of its tiles;
//   void walk(State&, cd, turns, lo, len): the staged epochs lo .. lo + len - 1 into the candidate's sums, in order;
//   Fit fit(State);  bool counts(Fit): the fit is a candidate's.
template <class Problem>
__device__ __forceinline__ Best lane_search(const Problem& p, SearchLds& sh, const EccGrid& grid, int n_phase, double f,
                                            const double* __restrict__ tt, int64_t n, typename Problem::Fit& kept) {
  const int lane = threadIdx.x, nt = blockDim.x;
  const int n_cand = grid.n * n_phase;
  for (int q = lane; q < grid.n; q += nt) sh.e[q] = grid.e[q];
  __syncthreads();
  Best best = best_init();
  for (int c0 = 0; c0 < n_cand; c0 += nt) {
    const int c = c0 + lane;
    const Candidate cd = candidate_of(c, n_cand, n_phase, sh.e);
    typename Problem::State a{};
    for (int64_t lo = 0; lo < n; lo += kTile) {
      const int len = (int)(n - lo < kTile ? n - lo : kTile);
      __syncthreads();  // (every lane is done with the tile before)
      for (int i = lane; i < len; i += nt) {
        sh.turns[i] = est::ls_phase_turns(f, tt[lo + i]);
        p.stage(lo, i);
      }
      __syncthreads();
      if (cd.live) p.walk(a, cd, sh.turns, lo, len);
    }
    if (cd.live) {
      const typename Problem::Fit r = p.fit(a);
      if (p.counts(r)) {
        const int32_t before = best.candidate;
        best_take(best, r.power, c);
        if (best.candidate != before) kept = r;
      }
    }
  }
  return best;
}

// the arg-max over the workgroup, in every lane: over the wave by shuffles, over the waves through LDS
__device__ __forceinline__ Best block_best(Best best, SearchLds& sh) {
  const int lane = threadIdx.x, nt = blockDim.x;
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double p = __shfl_down(best.power, o, kWave);
    const int32_t c = __shfl_down(best.candidate, o, kWave);
    best_take(best, p, c);
  }
  if (lane % kWave == 0) {
    sh.red_p[lane / kWave] = best.power;
    sh.red_c[lane / kWave] = best.candidate;
  }
  __syncthreads();
  best = best_init();
  for (int i = 0; i < nt / kWave; ++i) best_take(best, sh.red_p[i], sh.red_c[i]);
  return best;
}

// the record of a (frequency, series) without a candidate, by lane 0: the problem's power for that, candidate -1, the rest NaN
__device__ __forceinline__ void write_no_candidate(double none, int64_t slot, int n_coef, double* __restrict__ power,
                                                   int32_t* __restrict__ candidate, double* __restrict__ coef) {
  if (threadIdx.x != 0) return;
  power[slot] = none;
  candidate[slot] = -1;
  for (int q = 0; q < n_coef; ++q) coef[slot * n_coef + q] = NAN;
}

#endif  // EXO_HOST_BUILD

}  // namespace orb

// The names under which exo_keplerian_core.hpp exported the arithmetic of the grid before it moved here: host harnesses
// written against either core header name them so, and go on compiling against this one.
namespace kep {
using orb::Best;
using orb::best_init;
using orb::best_take;
using orb::is_candidate;
}  // namespace kep
