// exo_transit_runs.hpp -- the RUN-ENUMERATION PATH of the light-curve sweep (exo_transit.hip), enumerate -> runs -> finish:
// sorted times and one exposure time (or none) for all cadences.  Its kernels and its workspace layout (RunWs / carve_runs).
//
// Where a planet can overlap the disk is known in closed form (the conjunction windows of transit_window_kernel), the
// windows are periodic in mean anomaly, and t is sorted: so instead of testing every (draw, cadence) -- 1.5e8 phase tests
// per sweep of C2, 0.12 ms -- each window's run of cadences [lo, hi) is found by binary search in t (a few thousand
// searches per sweep).  The heavy kernel then works through the runs densely, in full fp64 (no fp32 pre-filter: a cadence
// in a window but off the disk costs one Kepler solve and returns 0), writes each cadence's flux to a compact per-(draw,
// planet) value array in run order, and -- dense output -- zero-fills its share of the flux array WHILE it computes (a few
// 1 KB non-temporal stores per wave and round: the store stream of the dense output hides under the fp64 work instead of
// preceding it); a last small kernel copies the runs' values to their cadences and sums the gradient partials.  With
// EXO_FLAG_SPARSE the flux array is never touched: the runs and the value array ARE the output.
//   t unsorted, a window that cannot be bounded, windows that overlap each other or more than kRunMax windows in the
//   series: that list becomes the single run [0, n_cad) (every cadence solved).
#pragma once
#include "exo_pack_core.hpp"
#include "exo_transit_sample.hpp"
#include "exo_transit_window.hpp"

namespace {

struct Run {
  int32_t lo, a, b, hi;   // cadences [lo, a) and [b, hi): may touch the limb; [a, b): small disk wholly inside (a hint)
};
constexpr int kRunMax = 4096;     // windows per list
#ifndef EXO_RUN_SEG
#define EXO_RUN_SEG 256
#endif
constexpr int kSeg = EXO_RUN_SEG;  // runs of one list a heavy block holds in LDS at a time (a power of two)

struct RunLists {
  int32_t* nrun;     // [n_list]                 windows of list = (draw, planet, event)
  Run* runs;         // [n_list][r_max]
  int32_t* pre_in;   // [n_list][r_max + 1]      exclusive prefix sums of b - a
  int32_t* pre_all;  // [n_list][r_max + 1]      exclusive prefix sums of hi - lo (= position in the value array)
  int32_t* rbin;     // [n_list][r_max]          timing tables: the bin every cadence AND sub-exposure of the run falls
                     //                          in, or -1 (looked up sample by sample)
  double* grun;      // [n_list][r_max]          timing tables, reverse sweep: d(sum)/d(shift) collected run by run
  int r_max;
};

// exclusive prefix sums of the run lengths a list's wave left in s_len: a lane takes a contiguous share of the runs
__device__ __forceinline__ void enum_prefix(int (*s_len)[kRunMax + 1], int K, int lane, int32_t* __restrict__ pin,
                                            int32_t* __restrict__ pall, int32_t* __restrict__ nrun_dst) {
  const int per = (K + 63) / 64, k0 = lane * per, k1 = (k0 + per < K) ? k0 + per : K;
  int sum_in = 0, sum_all = 0;
  for (int k = k0; k < k1; ++k) { sum_in += s_len[0][k]; sum_all += s_len[1][k]; }
  int ex_in = sum_in, ex_all = sum_all;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int o_in = __shfl_up(ex_in, m, 64), o_all = __shfl_up(ex_all, m, 64);
    if (lane >= m) { ex_in += o_in; ex_all += o_all; }
  }
  int run_in = ex_in - sum_in, run_all = ex_all - sum_all;
  for (int k = k0; k < k1; ++k) {
    pin[k] = run_in; pall[k] = run_all;
    run_in += s_len[0][k]; run_all += s_len[1][k];
  }
  if (lane == 63) { pin[K] = ex_in; pall[K] = ex_all; *nrun_dst = K; }
}

// ---- what the enumeration kernels share: a wave (lane = 0 .. 63) per list ----
// did every block of transit_window_kernel's check find its cadences in order?
__device__ __forceinline__ bool sorted_vote(const int32_t* __restrict__ sorted, int n_sorted, int lane) {
  bool srt = true;
  for (int i = lane; i < n_sorted; i += 64) srt = srt && (sorted[i] != 0);
  return __all(srt);
}

// The list "every cadence", as pieces of >= 1024 (the heavy blocks of a draw share a list run by run).  rbin (timing
// tables, else nullptr): no run carries a bin.  Returns the number of pieces.
__device__ __forceinline__ int every_cadence(int64_t n_cad, int r_max, int lane, Run* __restrict__ runs,
                                             int32_t* __restrict__ rbin, int (*s_len)[kRunMax + 1]) {
  int64_t piece = (n_cad + r_max - 1) / r_max;
  piece = piece < 1024 ? 1024 : piece;
  const int K = (int)((n_cad + piece - 1) / piece);
  for (int k = lane; k < K; k += 64) {
    const int64_t lo = k * piece, hi = (lo + piece < n_cad) ? lo + piece : n_cad;
    runs[k] = Run{(int32_t)lo, (int32_t)lo, (int32_t)lo, (int32_t)hi};
    if (rbin) rbin[k] = -1;
    s_len[0][k] = 0;
    s_len[1][k] = (int)(hi - lo);
  }
  return K;
}

// The cadences of a window, by search in the ascending times.  A cadence's phase is fma(t, nrev, c0) + off, in
// revolutions; off: the occultation's distance from the transit, or -shift nrev of a timing bin.
struct PhaseSearch {
  const double* __restrict__ t;
  double nrev, c0, off;
  // First i in [lo, hi) with phase >= thr (strict: > thr).  Series are nearly always evenly sampled: the position
  // guess(thr) -- from the mean sampling rate, if the series has one (`rated`) -- is confirmed by its two neighbours (two
  // independent loads instead of a chain of log2(n) dependent ones); anything else is searched for.
  template <class Guess>
  __device__ __forceinline__ int first_not(double thr, bool strict, int lo, int hi, bool rated, Guess guess) const {
    if (rated && hi > lo) {
      const double gq = guess(thr);
      const int g = gq < (double)lo ? lo : (gq > (double)hi ? hi : (int)gq);
      const double xa = g > lo ? fma(t[g - 1], nrev, c0) + off : 0.0, xb = g < hi ? fma(t[g], nrev, c0) + off : 0.0;
      const bool left_before = g == lo || (strict ? (xa <= thr) : (xa < thr));
      const bool here_not = g == hi || !(strict ? (xb <= thr) : (xb < thr));
      if (left_before && here_not) return g;
    }
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double xi = fma(t[mid], nrev, c0) + off;
      const bool before = strict ? (xi <= thr) : (xi < thr);
      lo = before ? mid + 1 : lo;
      hi = before ? hi : mid;
    }
    return lo;
  }
  // The window centred on phase kc -> run k of the list: the cadences within h of the centre, among them those within
  // hin (the "inside" hint; 0: none), and the two lengths enum_prefix sums.
  template <class Guess>
  __device__ __forceinline__ void window_run(double kc, double h, double hin, int n_cad, bool rated, Guess guess, int k,
                                             Run* __restrict__ runs, int (*s_len)[kRunMax + 1]) const {
    Run r;
    r.lo = first_not(kc - h, false, 0, n_cad, rated, guess);
    r.hi = first_not(kc + h, true, r.lo, n_cad, rated, guess);
    if (hin > 0.0) {
      r.a = first_not(kc - hin, false, r.lo, r.hi, rated, guess);
      r.b = first_not(kc + hin, true, r.a, r.hi, rated, guess);
    } else {
      r.a = r.b = r.lo;
    }
    runs[k] = r;
    s_len[0][k] = r.b - r.a;
    s_len[1][k] = r.hi - r.lo;
  }
};

// One wave per list (draw, planet, event: 0 = transits, 1 = occultations).
// FUSED (EXO_FLAG_SORTED_TIMES: the caller vouches for non-decreasing times, so nothing has to be checked before the
// searches): the wave works its record's conjunction windows out itself -- every group of eight lanes the same record, lane 0
// and lane 2 hold the result -- and the list of event 0 leaves them in `windows_out` for the sweep: no transit_window_kernel
// launch (each of these short kernels is ~5 us of dispatch and dependent memory round trips before its first useful cycle).
// PACK (with FUSED; exo_transit_flux_cols_vjp_f64): the wave is handed the constructor's COLUMNS and packs its record itself
// (exo_pack_core.hpp: lane 0; the list of event 0 writes it out for the sweep, the first list of a draw the limb-darkening
// coefficients too, on lane 1) -- no pack_kernel launch in front (C2: packing 5.9 + enumeration 10.2 us -> 14.5 us).
// (The packing VJP was folded into the sweep's last kernel as well -- the block that sums a draw's record cotangents taking them
// back to the columns -- measured, and removed: one thread's serial chain at the tail of every block cost the sweep 12.7 us at C2,
// the 1024-lane packing-VJP kernel it replaced costs 7.2.)
struct PackIn {
  exo_pack::ColsSrc src;
  uint32_t flags;          // pack flags
  int n_planet;
  double* params;          // out [n_draw][n_planet][EXO_NPAR]
  double* ld;              // out [n_draw][3 | 6]
};
template <bool FUSED, bool PACK = false>
__global__ __launch_bounds__(64) void transit_enum_kernel(const double* __restrict__ t, int64_t n_cad,
    const double* __restrict__ texp, int64_t n_texp, const double* __restrict__ stencil_dt, int n_sub, uint32_t flags,
    const double* __restrict__ windows, const int32_t* __restrict__ sorted, int n_sorted, int n_ev, RunLists rl,
    const double* __restrict__ params = nullptr, double* __restrict__ windows_out = nullptr, PackIn pk = PackIn{}) {
  static_assert(!PACK || FUSED, "packing rides on the fused windows + enumeration launch");
  __shared__ int s_len[2][kRunMax + 1];
  __shared__ double s_rec[PACK ? EXO_NPAR : 1];
  const int64_t list = blockIdx.x, rec = list / n_ev;
  const int ev = (int)(list - rec * n_ev), lane = threadIdx.x;
  if (PACK) {
    const int64_t draw = rec / pk.n_planet;
    const int planet = (int)(rec - draw * pk.n_planet);
    if (lane == 0) {
      double o[EXO_NPAR];
      exo_pack::pack_record(pk.src, rec, draw, planet, pk.flags, o);
#pragma unroll
      for (int k = 0; k < EXO_NPAR; ++k) s_rec[k] = o[k];
      if (ev == 0) {
#pragma unroll
        for (int k = 0; k < EXO_NPAR; ++k) pk.params[rec * EXO_NPAR + k] = o[k];
      }
    }
    if (lane == 1 && ev == 0 && planet == 0)
      exo_pack::pack_ld(pk.src, draw, pk.flags, pk.ld + draw * ((pk.flags & EXO_FLAG_SECONDARY) ? 6 : 3));
    __syncthreads();
  }
  double wv[kWin];
  if (FUSED) {
    double w[kWin] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    window_lanes(PACK ? s_rec : params + rec * EXO_NPAR, flags, lane & 7, w);
    const bool every = flags & EXO_FLAG_WINDOW;   // (every lane holds all seven)
#pragma unroll
    for (int q = 0; q < kWin; ++q) wv[q] = __shfl(w[q], (!every && (q == 4 || q == 6)) ? 2 : 0, 64);
    if (ev == 0 && lane == 0) {
#pragma unroll
      for (int q = 0; q < kWin; ++q) windows_out[kWin * rec + q] = wv[q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < kWin; ++q) wv[q] = windows[kWin * rec + q];
  }
  const double nrev = wv[0], c0 = wv[1], dmid = wv[2];
  // the windows are widened by the half-span of the exposure stencil; the reference widens its
  // contact windows by texp / 2 whatever the stencil (keplerian.py:765-769)
  const double span = (flags & EXO_FLAG_WINDOW) ? 0.5 : (stencil_dt ? stencil_reach(stencil_dt, n_sub) : 0.0);
  const double te = n_texp ? texp[0] : 0.0;
  const double widen = fabs(te) * span * fabs(nrev);
  const double h0 = wv[3] + widen, h1 = wv[4] + widen;
  bool srt;
  if (!FUSED) {
    srt = sorted_vote(sorted, n_sorted, lane);
  } else {
    // the caller's word covers the order of NEIGHBOURING cadences; the series as a whole is looked at here, coarsely: 65
    // evenly spaced cadences must ascend (a NaN fails), else the list is "every cadence".  What this catches is a time
    // buffer refilled with another, unordered series under a flag that was baked into a captured launch; two swapped
    // neighbours it cannot see (that is what the unflagged sweep's own check is for).  Two independent loads per lane.
    const int64_t i0 = (n_cad - 1) * lane / 64, i1 = (n_cad - 1) * (lane + 1) / 64;
    srt = __all(t[i0] <= t[i1]);
  }
  // the list degenerates to "every cadence" unless its windows are bounded, periodic in t and disjoint
  // (the decision is the same for both events of a planet: it only uses what they share)
  const double x_first = fma(t[0], nrev, c0), x_last = fma(t[n_cad - 1], nrev, c0);
  bool full = !srt || !(nrev > 0.0) || !(x_first == x_first) || !(x_last == x_last) || !(fabs(x_first) < 1e15) ||
              !(fabs(x_last) < 1e15) || !(h0 < 0.5);
  if (n_ev == 2) {
    const double sep = fabs(frac_rev(dmid));   // transit and occultation centres, in revolutions
    full = full || !(h1 < 0.5) || !(h0 + h1 < sep);
  }
  double kmin[2] = {0.0, 0.0}, kcnt[2] = {0.0, 0.0};
  if (!full) {
    for (int e = 0; e < n_ev; ++e) {
      const double off = e ? dmid : 0.0, h = e ? h1 : h0;
      kmin[e] = ceil((x_first + off) - h);
      kcnt[e] = floor((x_last + off) + h) - kmin[e] + 1.0;
      full = full || (kcnt[e] > (double)rl.r_max);
    }
  }
  Run* __restrict__ runs = rl.runs + list * rl.r_max;
  int32_t* __restrict__ pin = rl.pre_in + list * (rl.r_max + 1);
  int32_t* __restrict__ pall = rl.pre_all + list * (rl.r_max + 1);
  int K;
  if (full) {
    K = ev == 0 ? every_cadence(n_cad, rl.r_max, lane, runs, nullptr, s_len) : 0;
  } else {
    K = kcnt[ev] > 0.0 ? (int)kcnt[ev] : 0;
    const double off = ev ? dmid : 0.0, h = ev ? h1 : h0, hin = wv[5 + ev];
    // the guess: phases per cadence
    const double x_rate = (x_last - x_first) / (double)(n_cad > 1 ? n_cad - 1 : 1);
    const auto guess = [&](double thr) { return ceil((thr - off - x_first) / x_rate); };
    const PhaseSearch ps{t, nrev, c0, off};
    for (int k = lane; k < K; k += 64)
      ps.window_run(kmin[ev] + (double)k, h, hin, (int)n_cad, x_rate > 0.0, guess, k, runs, s_len);
  }
  __syncthreads();
  enum_prefix(s_len, K, lane, pin, pall, rl.nrun + list);
}

// The same with timing tables (one list per (draw, planet): transits only).  Within a timing bin the warp is a plain
// shift, so the windows of bin k are periodic in t - shift[k]: every bin's windows are enumerated on their own.  A
// list is TRUSTED when each of its windows, widened by the exposure's reach, lies strictly inside its bin -- then every
// cadence of a run and every one of its sub-exposures shares the run's bin (rbin), no sample needs a table lookup and
// d/d(shift) can be collected run by run.  Anything else (a transit across a bin edge, more bins or windows than the
// tables hold, unsorted times) degenerates to "every cadence", each sample looking its own bin up (rbin = -1).
__global__ __launch_bounds__(64) void transit_enum_ttv_kernel(const double* __restrict__ t, int64_t n_cad,
    const double* __restrict__ texp, int64_t n_texp, const double* __restrict__ stencil_dt, int n_sub, uint32_t flags,
    const double* __restrict__ windows, const int32_t* __restrict__ sorted, int n_sorted, RunLists rl, Ttv ttv) {
  __shared__ int s_len[2][kRunMax + 1];
  __shared__ int s_first[kRunMax + 2], s_mlo[kRunMax + 1];
  const int64_t list = blockIdx.x;
  const int lane = threadIdx.x;
  const double* wv = windows + kWin * list;
  const double nrev = wv[0], c0 = wv[1], hin = wv[5];
  const double reach = stencil_dt ? stencil_reach(stencil_dt, n_sub) : 0.0;
  const double span = (flags & EXO_FLAG_WINDOW) ? 0.5 : reach;
  const double te = n_texp ? texp[0] : 0.0;
  const double h0 = wv[3] + fabs(te) * span * fabs(nrev);
  const bool srt = sorted_vote(sorted, n_sorted, lane);
  const TtvRow row(ttv, list);
  const int nfin = row.bin(__builtin_inf());   // (the padding is +inf)
  const double t_first = t[0], t_last = t[n_cad - 1];
  const double inf = __builtin_inf();
  bool full = !srt || !(nrev > 0.0) || !(h0 < 0.5) || (nfin + 1 > kRunMax) || !(t_first == t_first) ||
              !(t_last == t_last) || !(fabs(t_first) < inf) || !(fabs(t_last) < inf);
  const double hw_t = h0 / nrev, r_t = n_texp ? fabs(te) * reach : 0.0;
  int K = 0;
  if (!full) {
    bool bad = false;
    int base = 0;
    for (int k0 = 0; k0 <= nfin; k0 += 64) {
      const int k = k0 + lane;
      int cnt = 0, mlo = 0;
      if (k <= nfin) {
        const double lo_t = k > 0 ? row.edges[k - 1] : -inf, hi_t = k < nfin ? row.edges[k] : inf;   // the bin: (lo_t, hi_t]
        const double sh = row.shift[k];
        const double lo_c = fmax(lo_t, t_first), hi_c = fmin(hi_t, t_last);
        if (lo_c <= hi_c) {
          const double x_lo = fma(lo_c - sh, nrev, c0), x_hi = fma(hi_c - sh, nrev, c0);
          if (!(fabs(x_lo) < 1e9) || !(fabs(x_hi) < 1e9)) {
            bad = true;
          } else {
            const double a = ceil(x_lo - h0), b = floor(x_hi + h0);
            if (b >= a) {
              const double n = b - a + 1.0;
              if (n > (double)rl.r_max) {
                bad = true;
              } else {
                cnt = (int)n;
                mlo = (int)a;
              }
              // the bin's first and last window, the exposure's reach included, strictly inside it
              const double tc_a = (a - c0) / nrev + sh, tc_b = (b - c0) / nrev + sh;
              const double slack = 1e-9 * (fabs(tc_a) + fabs(tc_b) + 1.0);
              if (!(tc_a - hw_t - r_t - slack > lo_t) || !(tc_b + hw_t + r_t + slack < hi_t)) bad = true;
            }
          }
        } else if (!(lo_c == lo_c) || !(hi_c == hi_c)) {
          bad = true;
        }
      }
      int ex = cnt;
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(ex, m, 64);
        if (lane >= m) ex += o;
      }
      if (k <= nfin) { s_first[k] = base + ex - cnt; s_mlo[k] = mlo; }
      base += __shfl(ex, 63, 64);
      if (base > rl.r_max) bad = true;
    }
    K = base;
    full = __any(bad) || K > rl.r_max;
  }
  Run* __restrict__ runs = rl.runs + list * rl.r_max;
  int32_t* __restrict__ rbin = rl.rbin + list * rl.r_max;
  int32_t* __restrict__ pin = rl.pre_in + list * (rl.r_max + 1);
  int32_t* __restrict__ pall = rl.pre_all + list * (rl.r_max + 1);
  __syncthreads();
  if (full) {
    K = every_cadence(n_cad, rl.r_max, lane, runs, rbin, s_len);
  } else {
    const double t_rate = (t_last - t_first) / (double)(n_cad > 1 ? n_cad - 1 : 1);
    for (int r = lane; r < K; r += 64) {
      int lo_k = 0, hi_k = nfin + 1;     // the run's bin: the last one whose first run is <= r
      while (hi_k - lo_k > 1) {
        const int mid = (lo_k + hi_k) >> 1;
        if (s_first[mid] <= r) lo_k = mid; else hi_k = mid;
      }
      const int k = lo_k;
      const double kc = (double)(s_mlo[k] + (r - s_first[k]));
      // the warped phase of a cadence; the guess: the threshold as a time, cadences per day
      const double sh = row.shift[k];
      const auto guess = [&](double thr) { return ceil(((thr - c0) / nrev + sh - t_first) / t_rate); };
      const PhaseSearch ps{t, nrev, c0, -sh * nrev};
      ps.window_run(kc, h0, hin, (int)n_cad, t_rate > 0.0, guess, r, runs, s_len);
      rbin[r] = k;
    }
  }
  __syncthreads();
  enum_prefix(s_len, K, lane, pin, pall, rl.nrun + list);
}

// this wave's share of a block's zero-fill: 1 KB pieces (64 lanes x 16 B, non-temporal), a few per round.
// Everything that steers the stream is WAVE-UNIFORM and lives in scalar registers -- the piece pointer, the count of
// pieces left -- and a store is `global_store_dwordx4 v_lane_offset, v_zero, s[piece]` with no vector arithmetic at
// all (round 2 carried the cursor per lane: 64-bit vector adds, two vector compares and four moves of the zero per
// store, ~200 vector instructions per round of a 1024-draw sweep -- a sixth of the kernel's VALU work).
struct FillCursor {
  typedef double v2d __attribute__((ext_vector_type(2)));
  char* base;      // the block's 16-B aligned share (block-uniform: derived from kernel arguments and block indices)
  int64_t off;     // byte offset of this wave's next full piece (wave-uniform)
  int left;        // full pieces this wave still owes (wave-uniform)
  uint32_t loff;   // lane * 16
  v2d zero;
  __device__ __forceinline__ FillCursor(double* dst, int64_t n) : base(nullptr), off(0), left(0), loff((threadIdx.x & 63) * 16) {
    zero = v2d{0.0, 0.0};
    asm volatile("" : "+v"(zero));   // (an opaque value: kept in four registers, not re-materialised before every store)
    if (!dst || n <= 0) return;
    const int64_t head = (reinterpret_cast<uintptr_t>(dst) & 8) ? 1 : 0;
    if (threadIdx.x == 0 && head) dst[0] = 0.0;
    if (threadIdx.x == 0 && ((n - head) & 1)) dst[n - 1] = 0.0;
    v2d* q2 = reinterpret_cast<v2d*>(dst + head);
    const int64_t n2 = (n - head) >> 1;            // 16-B units
    const int64_t nfull = n2 >> 6;                 // full 1-KB pieces; the partial one goes now
    const int rem = (int)(n2 & 63);
    if ((int)threadIdx.x < rem) __builtin_nontemporal_store(zero, q2 + (nfull << 6) + threadIdx.x);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    left = nfull > w ? (int)((nfull - w + kWaves - 1) / kWaves) : 0;
    left = __builtin_amdgcn_readfirstlane(left);
    base = reinterpret_cast<char*>(q2);
    off = (int64_t)w * 1024;
  }
  __device__ __forceinline__ int pieces_left() const { return left; }
  __device__ __forceinline__ void issue(int count) {   // `count`: wave-uniform
    const int k = count < left ? count : left;
    for (int s = 0; s < k; ++s) {
      __builtin_nontemporal_store(zero, reinterpret_cast<v2d*>(base + off + loff));
      off += kWaves * 1024;
    }
    left -= k;
  }
};

// Last kernel of a sweep on the run-enumeration path, one block per draw: (GRAD) block partials ->
// gparams, gld, sum(gflux * flux), in block order; (dense output) the runs' values to their cadences,
// planet by planet (summed flux: a later planet adds to what the earlier ones left).
// (1024 threads per block for batches of at most 256 draws: the scatter of a draw's values is one block's work, and
// with few draws the loads it keeps in flight are what bounds it -- C4 at 64 draws: 34 -> 10 us)
// (also the tail of transit_runs_kernel when a draw is one block's work -- no restrict on what that kernel wrote)
// NOISE (exo_transit_noise[_ttv]_vjp_f64): two more per-draw sums ride the same reductions -- sum w f (gmean) and
// sum w^2 (f^2 - 2 f r) (gjit2) over the solved cadences.  Single-pass route: the limb-darkening slots 3 and 4 of the
// partials, which only an occultation uses and that route has none; three-sweep route: two more rows of block partials
// behind the misfit's ([3][n_draw][n_chi2_part]), each summed by a thread of its own in block order.
struct NoiseOut {
  double* gmean;
  double* gjit2;
};
template <bool NOISE = false>
__device__ __forceinline__ void finish_draw(
    int64_t draw, const double* partial, int nblk, int n_planet, bool secondary, double* __restrict__ gparams,
    double* __restrict__ gld, double* __restrict__ flux_dot, int64_t n_cad, uint32_t flags, int n_ev, const RunLists& rl,
    const double* vals, const int32_t* vcad, double* flux,
    const double* __restrict__ chi2_part, int n_chi2_part, double* __restrict__ chi2_out, const Ttv& ttv,
    int64_t cm_draws = 0,     // cm_draws: 0, or n_draw -- the summed flux is cadence-major, [n_cad][n_draw]
    NoiseOut nzo = NoiseOut{nullptr, nullptr}, int64_t n_draw = 0) {
  if (ttv.gshift) {
    // timing tables, lists whose runs carry their bins: the runs' sums to their bins, in run order (the bins of a
    // list's runs ascend); the samples of any other list added to gshift themselves
    for (int p = 0; p < n_planet; ++p) {
      const int64_t list = draw * n_planet + p;
      const int K = rl.nrun[list];
      const int32_t* __restrict__ rbin = rl.rbin + list * rl.r_max;
      if (K == 0 || rbin[0] < 0) continue;
      const double* grun = rl.grun + list * rl.r_max;
      double* __restrict__ dst = ttv.gshift + list * (int64_t)(ttv.n_edge + 1);
      for (int k = threadIdx.x; k <= ttv.n_edge; k += (int)blockDim.x) {
        int lo = 0, hi = K;   // first run of a bin >= k
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rbin[mid] < k) lo = mid + 1; else hi = mid;
        }
        double v = 0.0;
        for (int r = lo; r < K && rbin[r] == k; ++r) v += grun[r];
        dst[k] = v;
      }
    }
  }
  if (chi2_out && threadIdx.x == blockDim.x - 1) {   // block partials of transit_residual_kernel, in block order
    double v = 0.0;
    for (int b = 0; b < n_chi2_part; ++b) v += chi2_part[draw * n_chi2_part + b];
    chi2_out[draw] = v;
  }
  if (NOISE && chi2_out && (threadIdx.x == blockDim.x - 2 || threadIdx.x == blockDim.x - 3)) {
    const int q = (int)(blockDim.x - 1 - threadIdx.x);   // 1: gmean, 2: gjit2
    double v = 0.0;
    for (int b = 0; b < n_chi2_part; ++b) v += chi2_part[(q * n_draw + draw) * n_chi2_part + b];
    (q == 1 ? nzo.gmean : nzo.gjit2)[draw] = v;
  }
  if (partial) {
    // (NOISE, single-pass route: its two sums rode in the limb-darkening slots of the occultation)
    partials_to_gradients(draw, partial, nblk, n_planet, secondary, (int)blockDim.x, gparams, gld, flux_dot, [&](int k, double v) {
      if (NOISE && !chi2_out && k == 3) nzo.gmean[draw] = v;
      if (NOISE && !chi2_out && k == 4) nzo.gjit2[draw] = v;
    });
  }
  if (!flux || !vals) return;
  // a thread per value: value and cadence arrays are read contiguously, four loads in flight per thread.  Summed flux of
  // several planets: planet 0 stores, every later planet ADDS with the hardware's fp64 atomic (no load of the target:
  // read-modify-write in the thread made each planet a load and a store round trip, C4 at 64 draws 15.8 us) behind a
  // block barrier -- planets in order, so the sums stay bit-reproducible (a planet's transits and occultations never
  // share a cadence) -- and the next batch of values is loaded before the current one is written.
  const bool per_planet = flags & EXO_FLAG_PER_PLANET;
  const int nthr = (int)blockDim.x;
  // the planets' value counts, all at once (two dependent loads each: one after the other they were the kernel)
  __shared__ int s_total[EXO_MAX_PLANETS];
  if ((int)threadIdx.x < n_planet) {
    int total = 0;
    for (int ev = 0; ev < n_ev; ++ev) {
      const int64_t list = (draw * n_planet + threadIdx.x) * n_ev + ev;
      total += rl.pre_all[list * (rl.r_max + 1) + rl.nrun[list]];
    }
    s_total[threadIdx.x] = total;
  }
  __syncthreads();
  auto total_of = [&](int p) { return s_total[p]; };
  auto load = [&](int p, int cb, int total, double* v, int* i) {
    const int64_t vbase = (draw * n_planet + p) * n_cad;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = cb + (int)threadIdx.x + u * nthr;
      v[u] = e < total ? vals[vbase + e] : 0.0;
      i[u] = e < total ? vcad[vbase + e] : -1;
    }
  };
  // batches (planet, first value) in order; `advance` steps to the next non-empty one
  int pl = 0, cb = -4 * nthr, total = total_of(0);
  auto advance = [&](int& p, int& c, int& tot) {
    c += 4 * nthr;
    while (p < n_planet && c >= tot) {
      ++p; c = 0;
      tot = p < n_planet ? total_of(p) : 0;
    }
  };
  advance(pl, cb, total);
  if (pl >= n_planet) return;
  double v[4];
  int i[4];
  load(pl, cb, total, v, i);
  for (;;) {
    int np = pl, ncb = cb, ntotal = total;
    advance(np, ncb, ntotal);
    const bool more = np < n_planet;
    double nv[4] = {0.0, 0.0, 0.0, 0.0};
    int ni[4] = {-1, -1, -1, -1};
    if (more) load(np, ncb, ntotal, nv, ni);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i[u] < 0) continue;
      if (per_planet) {
        flux[(draw * n_cad + i[u]) * n_planet + pl] = v[u];
      } else {
        double* dst = cm_draws ? flux + (int64_t)i[u] * cm_draws + draw : flux + draw * n_cad + i[u];
        if (pl == 0) *dst = v[u]; else unsafeAtomicAdd(dst, v[u]);
      }
    }
    if (!more) break;
    if (!per_planet && np != pl) __syncthreads();   // planets in order
    pl = np; cb = ncb; total = ntotal;
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[u] = nv[u]; i[u] = ni[u]; }
  }
}

__global__ __launch_bounds__(1024) void transit_finish_kernel(const double* __restrict__ partial, int nblk, int n_planet,
    bool secondary, double* __restrict__ gparams, double* __restrict__ gld, double* __restrict__ flux_dot, int64_t n_cad,
    uint32_t flags, int n_ev, RunLists rl, const double* __restrict__ vals, const int32_t* __restrict__ vcad,
    double* __restrict__ flux, const double* __restrict__ chi2_part, int n_chi2_part, double* __restrict__ chi2_out,
    Ttv ttv = Ttv{nullptr, nullptr, nullptr, 0}) {
  finish_draw(blockIdx.x, partial, nblk, n_planet, secondary, gparams, gld, flux_dot, n_cad, flags, n_ev, rl, vals, vcad, flux,
              chi2_part, n_chi2_part, chi2_out, ttv,
              ((flags & EXO_FLAG_CADENCE_MAJOR) && !(flags & EXO_FLAG_PER_PLANET)) ? (int64_t)gridDim.x : 0);
}

// the same with the two sums of the sampled-mean / jitter likelihood (grid: one block per draw)
__global__ __launch_bounds__(1024) void transit_finish_noise_kernel(const double* __restrict__ partial, int nblk,
    int n_planet, double* __restrict__ gparams, double* __restrict__ gld, double* __restrict__ chi2_direct, int64_t n_cad,
    uint32_t flags, int n_ev, RunLists rl, const int32_t* __restrict__ vcad, const double* __restrict__ chi2_part,
    int n_chi2_part, double* __restrict__ chi2_out, Ttv ttv, NoiseOut nzo) {
  finish_draw<true>(blockIdx.x, partial, nblk, n_planet, (flags & EXO_FLAG_SECONDARY) != 0, gparams, gld, chi2_direct, n_cad, flags,
                    n_ev, rl, nullptr, vcad, nullptr, chi2_part, n_chi2_part, chi2_out, ttv, 0, nzo, (int64_t)gridDim.x);
}

struct FinishArgs {
  double* gparams;
  double* gld;
  double* flux_dot;
  int fold;        // the runs kernel finishes its draws itself: no transit_finish_kernel launch
  int32_t* done;   // [n_draw] blocks of the draw that are through (zeroed by transit_window_kernel)
};
// NOISE: the draw's mean and jitter^2 ([1] or [n_draw]; n_jit = 0: none) and where its two extra sums go
struct NoiseIn {
  const double* mean;
  const double* jit2;
  int64_t n_mean, n_jit;
  NoiseOut out;
};

// CHI2 (one planet, one sample per cadence): gflux is the observed series [n_cad], gsparse its weights ([1] or [n_cad],
// `chi2_nw` says which); the "sum(gflux * flux)" slot of the partials carries sum w ((F - obs)^2 - obs^2) instead.
// TTV (one event per planet): `ttv` holds the timing tables; a trusted list's runs carry their bin (rl.rbin), its
// samples are shifted by the run's shift and d/d(shift) is summed run by run (wave partials in LDS, combined in a fixed
// order into rl.grun: bit-reproducible); the samples of any other list look their bins up and add to gshift atomically.
// Occupancy: THREE blocks per CU (three waves per SIMD: 168 registers, <= 53 KB of LDS per block).  The fp64 work of
// a sample is one long dependency chain (8 cycles per dependent operation against 4 of issue); a third wave per SIMD is
// worth ~1.2x of two.  It fits because (a) this translation unit is built with -mllvm -disable-machine-licm
// (__graft_entry__.py): hoisted out of the cadence loop, the ~60 fp64 constants of the polynomials sat in ~110 vector
// registers for the whole kernel (256 registers + scratch, two waves); re-materialised where they are used the kernel
// needs 168; (b) kSeg = 256 runs per batch keeps the LDS under a third of the CU's.  Variants whose LDS does not fit
// three blocks (timing tables) get the registers of two waves from the compiler; so do the light-delay variants (two
// Kepler solves alive at once: 250 B of scratch at 168 registers, measured slower than two waves without).
#ifndef EXO_RUNS_MIN_WAVES
#define EXO_RUNS_MIN_WAVES 3
#endif
// JAC (round 4; GRAD with a UNIT cotangent, value sweep of exo_transit_flux_fwd_jac_f64): a light curve that is the mean of a GP
// is swept before its cotangent exists, and used to be swept AGAIN for the gradient once it did.  The cotangent enters
// linearly -- gparams = sum over cadences of g x dF / dparams -- so this sweep leaves, next to every solved cadence's value, its
// sixteen derivatives (ten record slots, six limb-darkening coefficients: kJac doubles at `partial`, which is the Jacobian
// array here) and the second sweep becomes a contraction (transit_jac_vjp_kernel).  With an exposure stencil a cadence is
// n_sub Kepler solves and still one row of sixteen: C5 (7 sub-exposures) 238 us -> a few.
constexpr int kJac = 16;
__device__ __forceinline__ int jac_slot(int s) {   // LDS gradient column -> position in the row (-1: not kept)
  return s < G_PAD ? s : (s == G_SINI ? 9 : (s >= kNG && s < kNG + 6 ? 10 + (s - kNG) : -1));
}
// NOISE (CHI2 with a per-draw mean and jitter, exo_transit_noise[_ttv]_vjp_f64): gflux is the observed series y, gsparse
// the VARIANCES ([1] or [n_cad]); the residual r = y - mean_d and the weight w = 1 / (var + jit2_d) are formed where CHI2
// loads obs and ivar (mean_d, jit2_d: scalar registers), and the two extra sums go to the free limb-darkening slots 3 and 4.
template <bool GRAD, bool SECONDARY, bool LDELAY = false, bool CHI2 = false, bool TTV = false, bool JAC = false, bool NOISE = false>
__global__ __launch_bounds__(kBlock, LDELAY ? 2 : EXO_RUNS_MIN_WAVES) void transit_runs_kernel(
    const double* __restrict__ t, int64_t n_cad, const double* __restrict__ texp, int64_t n_texp,
    const double* __restrict__ stencil_dt, const double* __restrict__ stencil_w, int n_sub,
    const double* __restrict__ params, const double* __restrict__ ld, int n_planet, uint32_t flags, int n_ev, RunLists rl,
    const double* __restrict__ gflux, const double* __restrict__ gsparse, double* __restrict__ vals,
    int32_t* __restrict__ vcad, double* __restrict__ fill, double* __restrict__ partial, int64_t chi2_nw = 0,
    Ttv ttv = Ttv{nullptr, nullptr, nullptr, 0}, FinishArgs fin = FinishArgs{nullptr, nullptr, nullptr, 0, nullptr},
    NoiseIn nz = NoiseIn{nullptr, nullptr, 0, 0, NoiseOut{nullptr, nullptr}}) {
  static_assert(!NOISE || (CHI2 && GRAD && !SECONDARY && !JAC), "the sampled-mean / jitter likelihood is a CHI2 sweep");
  __shared__ Shared sh;
  __shared__ Run s_run[kSeg];
  __shared__ int2 s_pre[kSeg + 1];   // positions of a batch's runs among its "inside" items (.x) and its limb items (.y)
  __shared__ int s_all[kSeg + 1];    // position of a run's first cadence in the value array
  __shared__ int s_bin[TTV ? kSeg : 1];
  __shared__ double s_shift[TTV ? kSeg : 1];
  __shared__ double s_grun[(TTV && GRAD) ? kWaves : 1][(TTV && GRAD) ? kSeg : 1];
  __shared__ int s_rounds[2 * EXO_MAX_PLANETS];
  __shared__ double lds_acc[kNG + 7][kBlock];
  const int64_t draw = blockIdx.y;
  const int hb = gridDim.x, bx = blockIdx.x;
  stage_constants(sh, params, ld, stencil_dt, stencil_w, n_sub, n_planet, draw, SECONDARY);
  const bool per_planet = flags & EXO_FLAG_PER_PLANET;
  const int n_lists = n_planet * n_ev;
  // this block's slice of every list, and the rounds of 256 cadences it will take in all
  auto slice = [&](int K, int& k0, int& k1) {
    k0 = (int)((int64_t)K * bx / hb);
    k1 = (int)((int64_t)K * (bx + 1) / hb);
  };
  if ((int)threadIdx.x < n_lists) {
    const int64_t list = draw * n_lists + threadIdx.x;
    int k0, k1;
    slice(rl.nrun[list], k0, k1);
    const int32_t* pall = rl.pre_all + list * (rl.r_max + 1);
    int rounds = 0;
    for (int kb = k0; kb < k1; kb += kSeg) {
      const int ke = (kb + kSeg < k1) ? kb + kSeg : k1;
      rounds += (pall[ke] - pall[kb] + kBlock - 1) / kBlock;
    }
    s_rounds[threadIdx.x] = rounds;
  }
  __syncthreads();
  int total_rounds = 0;
  for (int l = 0; l < n_lists; ++l) total_rounds += s_rounds[l];
  // dense output: this block zeroes its share of the draw's flux, a few pieces per round
  const int64_t npl = per_planet ? n_planet : 1, n_fill = n_cad * npl;
  const int64_t f0 = n_fill * bx / hb, f1 = n_fill * (bx + 1) / hb;
  FillCursor fc(fill ? fill + draw * n_fill + f0 : nullptr, f1 - f0);
  const int per_round =
      __builtin_amdgcn_readfirstlane(total_rounds > 0 ? (fc.pieces_left() + total_rounds - 1) / total_rounds : 0);   // (wave-uniform)

  static_assert(!JAC || (GRAD && !LDELAY && !CHI2 && !TTV), "the Jacobian sweep is the plain value + gradient evaluation");
  const int ng_draw = n_planet * kNG + 7;
  double* __restrict__ pout = (GRAD && !JAC) ? partial + ((int64_t)draw * hb + bx) * ng_draw : nullptr;
  double* __restrict__ jac = JAC ? partial : nullptr;
  const GradAcc acc{GRAD ? &lds_acc[0][threadIdx.x] : nullptr};
  if (GRAD) {
#pragma unroll
    for (int s = 0; s < kNG + 7; ++s) lds_acc[s][threadIdx.x] = 0.0;
  }
  double cld[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) cld[k] = uniform((SECONDARY || k < 3) ? sh.c[k] : 0.0);
  const double te = (n_texp == 0) ? 0.0 : texp[0];
  const double sdt0 = uniform(sh.sdt[0]), sw0 = uniform(sh.sw[0]);
  const double nz_mean = NOISE ? uniform(nz.mean[nz.n_mean == 1 ? 0 : draw]) : 0.0;
  const double nz_jit2 = (NOISE && nz.n_jit > 0) ? uniform(nz.jit2[nz.n_jit == 1 ? 0 : draw]) : 0.0;
  for (int p = 0; p < n_planet; ++p) {
    const PlanetS c(sh.pc[p]);
    if (GRAD && p > 0) {
#pragma unroll
      for (int s = 0; s < kNG; ++s) lds_acc[s][threadIdx.x] = 0.0;
    }
    int64_t vbase = (draw * n_planet + p) * n_cad;   // the planet's values: transits first, occultations behind them
    const TtvRow row(ttv, TTV ? draw * n_planet + p : 0);
    double* __restrict__ grow = (TTV && GRAD) ? ttv.gshift + (draw * n_planet + p) * (int64_t)(ttv.n_edge + 1) : nullptr;
    const TtvGrad tgrad{(GRAD && TTV) ? &lds_acc[0][threadIdx.x] : nullptr, grow, nullptr};
    for (int ev = 0; ev < n_ev; ++ev) {
      const int64_t list = (draw * n_planet + p) * n_ev + ev;
      const int K = rl.nrun[list];
      const Run* __restrict__ runs = rl.runs + list * rl.r_max;
      const int32_t* __restrict__ pin = rl.pre_in + list * (rl.r_max + 1);
      const int32_t* __restrict__ pall = rl.pre_all + list * (rl.r_max + 1);
      int k0, k1;
      slice(K, k0, k1);
      for (int kb = k0; kb < k1; kb += kSeg) {
        const int m = (kb + kSeg < k1) ? kSeg : k1 - kb;
        __syncthreads();   // (the previous batch is done with the tables)
        const int in0 = pin[kb], all0 = pall[kb];
        for (int q = threadIdx.x; q <= m; q += kBlock) {
          const int pi = pin[kb + q] - in0, pa = pall[kb + q];
          s_pre[q] = make_int2(pi, (pa - all0) - pi);
          s_all[q] = pa;
          if (q < m) s_run[q] = runs[kb + q];
          if (TTV && q < m) {
            const int kq = rl.rbin[list * rl.r_max + kb + q];
            s_bin[q] = kq;
            s_shift[q] = kq >= 0 ? row.shift[kq] : 0.0;
            if (GRAD) {
#pragma unroll
              for (int w = 0; w < kWaves; ++w) s_grun[w][q] = 0.0;
            }
          }
        }
        __syncthreads();
        const bool trusted = TTV && s_bin[0] >= 0;   // (all runs of a list or none)
        const int tin = s_pre[m].x, total = tin + s_pre[m].y;
        // dense index j of the batch -> cadence i and position v in the value array: "inside" parts of all
        // runs first, then the limb parts, so that a wave's vote on the arc geometry is nearly unanimous.
        // Which run?  Transits recur: the runs of a list are nearly equally long, so position x runs / items is
        // the run or a neighbour of it; a wave steps its lanes to the right run (a vote per step) and only an uneven
        // list -- gaps in the series, the every-cadence fallback -- pays for a binary search (round 2 paid for one per
        // item: ~100 of the kernel's ~1100 vector instructions per cadence).
        const float g_in = tin > 0 ? (float)m / (float)tin : 0.0f;
        const float g_lim = total > tin ? (float)m / (float)(total - tin) : 0.0f;
        struct Item { int i, v, q; double tv, g, w; };
        auto locate = [&](int j, int& i, int& v, int& qrun) {
          const bool in = j < tin;
          const int jj = in ? j : j - tin;
          int q = (int)((float)jj * (in ? g_in : g_lim));
          q = q < m - 1 ? q : m - 1;
          int2 pa = s_pre[q], pb = s_pre[q + 1];
          int lo = in ? pa.x : pa.y, hi = in ? pb.x : pb.y;
          int tries = 0;
          while (EXO_WAVE_ANY((jj < lo) | (jj >= hi))) {
            if (++tries > 4) {
              q = 0;
#pragma unroll
              for (int step = kSeg / 2; step > 0; step >>= 1) {
                const int c2 = q + step;
                if (c2 < m) {
                  const int2 pc = s_pre[c2];
                  q = (jj >= (in ? pc.x : pc.y)) ? c2 : q;
                }
              }
              pa = s_pre[q];
              lo = in ? pa.x : pa.y;
              break;
            }
            q += (jj < lo) ? -1 : ((jj >= hi) ? 1 : 0);
            pa = s_pre[q]; pb = s_pre[q + 1];
            lo = in ? pa.x : pa.y; hi = in ? pb.x : pb.y;
          }
          const Run r = s_run[q];
          const int off = jj - lo;
          i = in ? r.a + off : ((off < r.a - r.lo) ? r.lo + off : r.b + (off - (r.a - r.lo)));
          v = s_all[q] + (i - r.lo);
          qrun = q;
        };
        auto load_item = [&](int j) -> Item {
          Item it{0, 0, 0, 0.0, 0.0, 0.0};   // lanes past the end of the batch: cadence 0 with a zero cotangent
          if (j < total) locate(j, it.i, it.v, it.q);
          it.tv = t[it.i];
          // the cotangent of the cadence's flux: dense [draw][cadence] (x planet), or -- gsparse -- at the value's own
          // position in the value array (transit_residual_kernel wrote it there)
          if (JAC) {
            it.g = (j < total) ? 1.0 : 0.0;   // unit cotangent: the row of derivatives itself
          } else if (NOISE) {
            if (j < total) {
              it.g = gflux[it.i] - nz_mean;
              it.w = exo::fast_rcp(gsparse[chi2_nw == 1 ? 0 : it.i] + nz_jit2);
            }
          } else if (CHI2) {
            if (j < total) { it.g = gflux[it.i]; it.w = gsparse[chi2_nw == 1 ? 0 : it.i]; }
          } else if (GRAD && j < total)
            it.g = gsparse ? gsparse[vbase + it.v]
                           : (per_planet ? gflux[(draw * n_cad + it.i) * n_planet + p]
                                         : ((flags & EXO_FLAG_CADENCE_MAJOR) ? gflux[(int64_t)it.i * gridDim.y + draw]
                                                                             : gflux[draw * n_cad + it.i]));
          return it;
        };
        Item nxt = load_item(threadIdx.x);
        for (int j0 = 0; j0 < total; j0 += kBlock) {
          const int j = j0 + threadIdx.x;
          const bool has = j < total;
          const Item cur = nxt;
          if (j0 + kBlock < total) nxt = load_item(j + kBlock);   // in flight while this round computes
          fc.issue(per_round);
          double f = 0.0;
          const double dsh = TTV ? s_shift[TTV ? cur.q : 0] : 0.0;
          for (int k = 0; k < n_sub; ++k) {
            // (the first sub-exposure's offset and weight sit in scalar registers: without an exposure time there is
            // no LDS read -- and no wait for one -- at the top of a round)
            const double sdt_k = (k == 0) ? sdt0 : sh.sdt[k], sw_k = (k == 0) ? sw0 : sh.sw[k];
            double tt = fma(te, sdt_k, cur.tv);
            int ks = 0;
            if (TTV) {
              double sh_k = dsh;
              if (!trusted) {
                ks = row.bin(tt);
                sh_k = row.shift[ks];
              }
              tt -= sh_k;
            }
            const double gw = cur.g * sw_k;
            const double F = eval_sample<GRAD, SECONDARY, LDELAY, CHI2>(tt, c, cld, CHI2 ? cur.g : gw, acc, cur.w);
            f = fma(sw_k, F, f);
            if (CHI2) {
              const double r = F - cur.g;
              acc.add(kNG + 6, cur.w * (r * r - cur.g * cur.g));
              if (NOISE) {
                acc.add(kNG + 3, cur.w * F);
                acc.add(kNG + 4, cur.w * cur.w * (r * r - cur.g * cur.g));
              }
            } else if (GRAD && !JAC) {
              acc.add(kNG + 6, gw * F);
            }
            if (TTV && GRAD && !trusted) tgrad.flush_lane(ks);
          }
          if (TTV && GRAD && trusted) tgrad.flush_runs(cur.q, &s_grun[0][0], kSeg);
          if (JAC) {
            // this cadence's row: the thread's gradient columns hold sum_k w_k dF_k / d(slot); out they go, and back to zero
            double row[kJac];
#pragma unroll
            for (int q = 0; q < kJac; ++q) row[q] = 0.0;
#pragma unroll
            for (int sl = 0; sl < kNG + 6; ++sl) {
              if (jac_slot(sl) >= 0) {
                row[jac_slot(sl)] = lds_acc[sl][threadIdx.x];
                lds_acc[sl][threadIdx.x] = 0.0;
              }
            }
            if (has) {
              double2* __restrict__ dst = reinterpret_cast<double2*>(jac + (vbase + cur.v) * kJac);
#pragma unroll
              for (int q = 0; q < kJac / 2; ++q) dst[q] = make_double2(row[2 * q], row[2 * q + 1]);
            }
          }
          if (vals && has) {
            vals[vbase + cur.v] = f;
            if (vcad) vcad[vbase + cur.v] = cur.i;   // (dense output: where the last kernel puts it)
          }
        }
        if (TTV && GRAD && trusted) {
          __syncthreads();   // the waves' tables of this batch, in wave order
          for (int q = threadIdx.x; q < m; q += kBlock) {
            double v = s_grun[0][q];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += s_grun[(TTV && GRAD) ? w : 0][q];
            rl.grun[list * rl.r_max + kb + q] = v;
          }
        }
      }
      vbase += pall[K];
    }
    if (GRAD && TTV) {
      // every sample's t_periastron term went to its bin; the planet's total is in G_PAD
      lds_acc[G_TP][threadIdx.x] = lds_acc[G_PAD][threadIdx.x];
      lds_acc[G_PAD][threadIdx.x] = 0.0;
    }
    if (GRAD && !JAC) reduce_columns(lds_acc, sh.red, 0, kNG, pout + p * kNG);
  }
  if (GRAD && !JAC) reduce_columns(lds_acc, sh.red, kNG, 7, pout + n_planet * kNG);
  fc.issue(1 << 30);   // whatever is left of the fill (all of it for a block without work)
  if (fin.fold) {
    // the block owns its draw (hb = 1): partials -> gradients, values -> their cadences -- what transit_finish_kernel does
    // otherwise, without its launch; a block barrier is all the hand-shake its own stores need
    __syncthreads();
    finish_draw<NOISE>(draw, (GRAD && !JAC) ? partial : nullptr, hb, n_planet, SECONDARY, fin.gparams, fin.gld, fin.flux_dot, n_cad,
                       flags, n_ev, rl, vals, vcad, fill, nullptr, 0, nullptr,
                       (TTV && GRAD) ? ttv : Ttv{nullptr, nullptr, nullptr, 0}, 0, nz.out);
  }
}

// The second half of the Jacobian route (transit_runs_kernel<.., JAC>): gparams, gld and sum(gflux flux) of a draw from the rows
// the value sweep left -- one block per draw, the planets in turn, every thread its share of the planet's solved cadences
// (the cotangent gathered through the cadence index of the value array), a fixed-order sum over the block: bit-reproducible.
// Output: the draw's partials in the layout of the runs kernel with ONE block per draw (transit_finish_kernel turns them
// into gparams / gld / flux_dot as it does for the sweep's).
__global__ __launch_bounds__(kBlock) void transit_jac_vjp_kernel(int64_t n_cad, int n_planet, int n_ev, uint32_t flags,
    RunLists rl, const double* __restrict__ vals, const int32_t* __restrict__ vcad, const double* __restrict__ jac,
    const double* __restrict__ gflux, int64_t n_draw, double* __restrict__ partial) {
  // (EXO_FLAG_SPARSE: gflux is the cotangent of the VALUES, in their layout -- what the sparse GP entries return)
  __shared__ double red[kJac + 1][kBlock];
  const int64_t draw = blockIdx.y;
  const int nb = gridDim.x, bx = blockIdx.x;       // a draw's cadences in nb contiguous shares (as the sweep's blocks share them)
  const int ng_draw = n_planet * kNG + 7;
  double* __restrict__ pout = partial + (draw * nb + bx) * ng_draw;
  const bool cmaj = flags & EXO_FLAG_CADENCE_MAJOR, gsp = flags & EXO_FLAG_SPARSE;
  double keep = 0.0;   // threads 10 .. 15: the running sum over planets of limb-darkening coefficient (thread - 10); thread 16: the dot
  for (int p = 0; p < n_planet; ++p) {
    int n_vals = 0;
    for (int ev = 0; ev < n_ev; ++ev) {
      const int64_t list = (draw * n_planet + p) * n_ev + ev;
      n_vals += rl.pre_all[list * (rl.r_max + 1) + rl.nrun[list]];
    }
    const int64_t vbase = (draw * n_planet + p) * n_cad;
    double acc[kJac + 1];
#pragma unroll
    for (int q = 0; q <= kJac; ++q) acc[q] = 0.0;
    const int v0 = (int)((int64_t)n_vals * bx / nb), v1 = (int)((int64_t)n_vals * (bx + 1) / nb);
    for (int v = v0 + threadIdx.x; v < v1; v += kBlock) {
      double g;
      if (gsp) {
        g = gflux[vbase + v];
      } else {
        const int64_t i = vcad[vbase + v];
        g = cmaj ? gflux[i * n_draw + draw] : gflux[draw * n_cad + i];
      }
      const double2* __restrict__ row = reinterpret_cast<const double2*>(jac + (vbase + v) * kJac);
#pragma unroll
      for (int q = 0; q < kJac / 2; ++q) {
        const double2 r2 = row[q];
        acc[2 * q] = fma(g, r2.x, acc[2 * q]);
        acc[2 * q + 1] = fma(g, r2.y, acc[2 * q + 1]);
      }
      acc[kJac] = fma(g, vals[vbase + v], acc[kJac]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q <= kJac; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    if (threadIdx.x <= kJac) {
      double v = 0.0;
      for (int k = 0; k < kBlock; ++k) v += red[threadIdx.x][k];
      const int q = threadIdx.x;
      if (q < 10) {
        pout[p * kNG + (q < 9 ? q : G_SINI)] = v;
      } else {
        keep += v;
      }
    }
    if (threadIdx.x < kNG && (threadIdx.x == G_PAD || threadIdx.x == G_CL)) pout[p * kNG + threadIdx.x] = 0.0;
  }
  if (threadIdx.x >= 10 && threadIdx.x <= kJac) pout[n_planet * kNG + (threadIdx.x - 10)] = keep;
}

// White-noise likelihood on the sparse output (exo_transit_chi2_vjp_f64), between the value sweep and the gradient
// sweep: for every value (cadence i of a run of list l = (planet, event) of the draw) the draw's TOTAL flux at i --
// its own value plus whatever the draw's other lists hold for that cadence (simultaneous transits: a binary search
// over each other list's runs) -- the residual r = total - obs[i], the cotangent 2 w_i r of the flux at i (written at
// the value's own position, where the gradient sweep reads it) and the draw's chi^2 relative to an empty light curve,
//     sum over solved cadences of  w_i ((total_i - obs_i)^2 - obs_i^2),
// each cadence counted once (by the first list that holds it).  Block partials in a fixed order (bit-reproducible).
// NOISE: obs is the series y and ivar holds the VARIANCES; r = y - mean_d, w = 1 / (var + jit2_d), and two more sums over the
// same cadences: sum w total (row 1 of the block partials) and sum w^2 ((total - r)^2 - r^2) (row 2).
constexpr int kResidualBlocks = 16;   // per draw
template <bool NOISE = false>
__global__ __launch_bounds__(kBlock) void transit_residual_kernel(int64_t n_cad, int n_planet, int n_ev, RunLists rl,
    const double* __restrict__ vals, const int32_t* __restrict__ vcad, const double* __restrict__ obs,
    const double* __restrict__ ivar, int64_t n_ivar, double* __restrict__ gvals, double* __restrict__ chi2_part,
    NoiseIn nz = NoiseIn{nullptr, nullptr, 0, 0, NoiseOut{nullptr, nullptr}}) {
  __shared__ double red[NOISE ? 3 : 1][kBlock];
  const int64_t draw = blockIdx.y;
  const int nb = gridDim.x, n_lists = n_planet * n_ev;
  double acc = 0.0, acc_m = 0.0, acc_j = 0.0;
  const double nz_mean = NOISE ? nz.mean[nz.n_mean == 1 ? 0 : draw] : 0.0;
  const double nz_jit2 = (NOISE && nz.n_jit > 0) ? nz.jit2[nz.n_jit == 1 ? 0 : draw] : 0.0;
  // value of list l2 at cadence i (0 if none of its runs holds it); `hit` says whether one does
  auto lookup = [&](int l2, int i, bool& hit) -> double {
    const int64_t list = draw * n_lists + l2;
    const int K = rl.nrun[list];
    const Run* __restrict__ runs = rl.runs + list * rl.r_max;
    int lo = 0, hi = K;                       // first run with run.lo > i
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (runs[mid].lo <= i) lo = mid + 1; else hi = mid;
    }
    hit = false;
    if (lo == 0) return 0.0;
    const Run r = runs[lo - 1];
    if (i >= r.hi) return 0.0;
    hit = true;
    const int p2 = l2 / n_ev, ev2 = l2 - p2 * n_ev;
    int64_t base = ((int64_t)draw * n_planet + p2) * n_cad;
    if (ev2 > 0) { const int64_t l0 = list - ev2; base += rl.pre_all[l0 * (rl.r_max + 1) + rl.nrun[l0]]; }
    return vals[base + rl.pre_all[list * (rl.r_max + 1) + lo - 1] + (i - r.lo)];
  };
  for (int l = 0; l < n_lists; ++l) {
    const int64_t list = draw * n_lists + l;
    const int p = l / n_ev, ev = l - p * n_ev;
    int64_t vbase = ((int64_t)draw * n_planet + p) * n_cad;
    if (ev > 0) { const int64_t l0 = list - ev; vbase += rl.pre_all[l0 * (rl.r_max + 1) + rl.nrun[l0]]; }
    const int total = rl.pre_all[list * (rl.r_max + 1) + rl.nrun[list]];
    for (int e = blockIdx.x * kBlock + threadIdx.x; e < total; e += nb * kBlock) {
      const int i = vcad[vbase + e];
      double tot = vals[vbase + e];
      bool first = true;
      for (int l2 = 0; l2 < n_lists; ++l2) {
        if (l2 == l) continue;
        bool hit;
        tot += lookup(l2, i, hit);
        first = first && !(hit && l2 < l);
      }
      const double o = NOISE ? obs[i] - nz_mean : obs[i];
      const double w = NOISE ? exo::fast_rcp(ivar[n_ivar == 1 ? 0 : i] + nz_jit2) : ivar[n_ivar == 1 ? 0 : i];
      const double r = tot - o;
      gvals[vbase + e] = 2.0 * w * r;
      if (first) acc += w * (r * r - o * o);
      if (NOISE && first) {
        acc_m += w * tot;
        acc_j += w * w * (r * r - o * o);
      }
    }
  }
  red[0][threadIdx.x] = acc;
  if (NOISE) {
    red[NOISE ? 1 : 0][threadIdx.x] = acc_m;
    red[NOISE ? 2 : 0][threadIdx.x] = acc_j;
  }
  __syncthreads();
  for (int m = kBlock / 2; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) {
      red[0][threadIdx.x] += red[0][threadIdx.x + m];
      if (NOISE) {
        red[NOISE ? 1 : 0][threadIdx.x] += red[NOISE ? 1 : 0][threadIdx.x + m];
        red[NOISE ? 2 : 0][threadIdx.x] += red[NOISE ? 2 : 0][threadIdx.x + m];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) chi2_part[draw * nb + blockIdx.x] = red[0][0];
  if (NOISE && threadIdx.x == 0) {
    const int64_t n_draw = gridDim.y;
    chi2_part[(n_draw + draw) * nb + blockIdx.x] = red[NOISE ? 1 : 0][0];
    chi2_part[(2 * n_draw + draw) * nb + blockIdx.x] = red[NOISE ? 2 : 0][0];
  }
}

// A DENSE flux array kept across steps (exo_transit_sparse_scatter_f64): the summed flux of the cadences in a sparse output's
// runs written into -- or, CLEAR, zeroed in -- a dense [n_draw][n_cad] array that is otherwise left alone.  A step of a sampler
// solves the same few per cent of the cadences as the step before it: clear the last step's, write this one's, and the
// dense result costs the sparse sweep plus two passes over the solved cadences instead of a fill of every cadence (1.2 GB at
// C2).  A block per draw; a wave per run (its cadences are consecutive: coalesced); planets in order with a block barrier,
// the first one storing and the later ones adding with the hardware's fp64 atomic -- the dense sweep's own order, so the
// same bits.
template <bool CLEAR>
__global__ __launch_bounds__(kBlock) void transit_scatter_runs_kernel(RunLists rl, const double* __restrict__ vals,
    int64_t n_cad, int n_planet, int n_ev, double* __restrict__ flux) {
  const int64_t draw = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_wave = kBlock / 64;
  double* __restrict__ row = flux + draw * n_cad;
  for (int p = 0; p < n_planet; ++p) {
    int64_t vbase = (draw * n_planet + p) * n_cad;      // the planet's values: transits first, occultations behind them
    for (int ev = 0; ev < n_ev; ++ev) {
      const int64_t list = (draw * n_planet + p) * n_ev + ev;
      // (a workspace that is not a sparse output -- never zeroed, never swept -- must not become a wild store: counts and
      // cadences are held to the arrays' bounds)
      int K = rl.nrun[list];
      K = K < 0 ? 0 : (K > rl.r_max ? rl.r_max : K);
      const Run* __restrict__ runs = rl.runs + list * rl.r_max;
      const int32_t* __restrict__ pall = rl.pre_all + list * (rl.r_max + 1);
      for (int k = wave; k < K; k += n_wave) {
        int lo = runs[k].lo, len = runs[k].hi - lo;
        const int pk = pall[k];
        if (lo < 0 || len < 0 || (int64_t)lo + len > n_cad || pk < 0 || (int64_t)pk + len > n_cad) continue;
        const int64_t v0 = vbase + pk;
        for (int i = lane; i < len; i += 64) {
          if (CLEAR) row[lo + i] = 0.0;
          // (planet 0 stores for BOTH events: a planet's transit and occultation lists never share a cadence -- the enumeration
          // keeps two lists only when the windows are disjoint, h0 + h1 < their separation; otherwise event 0 is "every
          // cadence" and event 1 is empty: transit_enum_kernel.  The dense sweep relies on the same invariant, finish_draw.)
          else if (p == 0) row[lo + i] = vals[v0 + i];
          else unsafeAtomicAdd(row + lo + i, vals[v0 + i]);
        }
      }
      const int tot = pall[K];
      vbase += (tot < 0 || tot > n_cad) ? 0 : tot;
    }
    if (!CLEAR && p + 1 < n_planet) __syncthreads();   // planets in order
  }
}

// ---- run-enumeration path -------------------------------------------------------------------------
// heavy blocks per draw.  A round of a block (256 cadences through eval_sample) takes ~8 us whatever its fill, 512
// blocks are resident at once (two per CU), and every (planet, inside / limb) segment of a block ends in a partly
// filled round: one generation of fuller blocks beats two generations of emptier ones (C4 at 64 draws: 11 round
// times at 8 blocks per draw against 18 at 16).
// A draw that is ONE block's work (hb = 1: batches of >= 512 draws) is finished by that block -- no transit_finish_kernel launch.
// (Draws shared by several blocks finished by the last block to arrive -- fence + counter -- were measured in round 3 and
// removed in round 5: the device-scope release each block then needs writes the L2's dirty zero-fill lines back before it
// returns, heavy kernel 54 -> 147 us at 128 draws, 102 -> 225 us on C4 at 64.)
#ifndef EXO_RUNS_TARGET_BLOCKS
#define EXO_RUNS_TARGET_BLOCKS 512
#endif
inline int runs_blocks_per_draw(int64_t n_draw) {
  int64_t hb = (EXO_RUNS_TARGET_BLOCKS + n_draw - 1) / n_draw;
  return (int)(hb < 1 ? 1 : (hb > 64 ? 64 : hb));
}
inline int runs_r_max(int64_t n_cad) { return (int)(n_cad < kRunMax ? (n_cad < 16 ? 16 : n_cad) : kRunMax); }

// scratch layout of the run-enumeration path (sized for two events per planet whatever the flags)
struct RunWs {
  double* partial;
  double* windows;
  int32_t* sorted;
  RunLists rl;
  double* vals;
  int32_t* vcad;   // cadence of every value (dense output, chi^2)
  double* gvals;   // chi^2: cotangent of every value
  double* chi2_part;
  int32_t* done;   // [n_draw] blocks of a draw that are through with it
  int hb, n_sorted;
  int64_t off_nrun, off_runs, off_pre_all, off_vals;   // byte offsets (exo_transit_flux_sparse_layout)
  int64_t bytes;
};
inline RunWs carve_runs(void* base, int64_t n_cad, int64_t n_draw, int n_planet) {
  RunWs w;
  w.hb = runs_blocks_per_draw(n_draw);
  w.n_sorted = (int)((n_cad + kSortBlock - 1) / kSortBlock);
  w.rl.r_max = runs_r_max(n_cad);
  const int64_t n_list = n_draw * n_planet * 2;
  auto up16 = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
  char* p = (char*)base;
  int64_t off = 0;
  w.partial = (double*)(p + off); off = up16(off + 8 * n_draw * w.hb * (int64_t)(n_planet * kNG + 7));
  w.windows = (double*)(p + off); off = up16(off + 8 * (int64_t)kWin * n_draw * n_planet);
  w.sorted = (int32_t*)(p + off); off = up16(off + 4 * (int64_t)w.n_sorted);
  w.off_nrun = off; w.rl.nrun = (int32_t*)(p + off); off = up16(off + 4 * n_list);
  w.off_runs = off; w.rl.runs = (Run*)(p + off); off = up16(off + (int64_t)sizeof(Run) * n_list * w.rl.r_max);
  w.rl.pre_in = (int32_t*)(p + off); off = up16(off + 4 * n_list * (int64_t)(w.rl.r_max + 1));
  w.off_pre_all = off; w.rl.pre_all = (int32_t*)(p + off); off = up16(off + 4 * n_list * (int64_t)(w.rl.r_max + 1));
  w.rl.rbin = (int32_t*)(p + off); off = up16(off + 4 * n_draw * n_planet * (int64_t)w.rl.r_max);
  w.rl.grun = (double*)(p + off); off = up16(off + 8 * n_draw * n_planet * (int64_t)w.rl.r_max);
  w.off_vals = off; w.vals = (double*)(p + off); off = up16(off + 8 * n_draw * n_planet * n_cad);
  w.vcad = (int32_t*)(p + off); off = up16(off + 4 * n_draw * n_planet * n_cad);
  w.gvals = (double*)(p + off); off = up16(off + 8 * n_draw * n_planet * n_cad);
  w.chi2_part = (double*)(p + off); off = up16(off + 8 * n_draw * kResidualBlocks * 3);   // (the misfit; NOISE: + gmean, gjit2)
  w.done = (int32_t*)(p + off); off = up16(off + 4 * n_draw);
  w.bytes = off;
  return w;
}

}  // namespace
