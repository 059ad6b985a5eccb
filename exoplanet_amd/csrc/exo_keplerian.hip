// exo_keplerian.hip -- the Keplerian periodogram of a batch of radial-velocity series on one time axis
// (exoplanet_amd/estimators.py: keplerian_power, keplerian_estimator): at every frequency the best of a grid of
// (eccentricity, phase of periastron) candidates, each a linear least-squares fit of  c_k + A cos nu + B sin nu  with one
// constant per instrument.  A translation unit of its own: none of the other kernels changes.  The arithmetic lives in
// exo_keplerian_core.hpp (tested on the host), the search over the candidates in exo_orbit_search.hpp; definition, layout,
// resources and timings: DESIGN.md section 22.  Compiled with -ffp-contract=off, as the host build of the core is.  Nothing
// but kernels is enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_estimators_launch.hpp"
#include "exo_keplerian_core.hpp"
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
  if (!t || !y || (n_yerr > 0 && !yerr) || !segment_offsets || !frequencies || !ecc || !power || !candidate || !coef ||
      !workspace || !sizes_ok(n, n_series, n_frequency, n_ecc, n_phase) ||
      (n_yerr != 0 && n_yerr != 1 && n_yerr != n_series) || n_instrument < 1 || n_instrument > kMaxInst)
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
  if (!ecc_grid(ecc, n_ecc, &grid)) return EXO_ERR_INVALID_ARGUMENT;
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
