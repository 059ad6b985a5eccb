// exo_astrometric.hip -- the astrometric orbit search of a batch of (rho, theta) series on one time axis
// (exoplanet_amd/estimators.py: astrometric_power, astrometric_estimator): at every frequency the best of a grid of
// (eccentricity, phase of periastron) candidates, each a linear least-squares fit of the four Thiele-Innes constants to the
// sky-plane positions, with radial and tangential errors.  A translation unit of its own: none of the other kernels changes.
// The arithmetic lives in exo_astrometric_core.hpp (tested on the host); definition, layout, resources and timings:
// DESIGN.md section 23.  Compiled with -ffp-contract=off, as the host build of the core is.
//
// The search: a workgroup owns one (frequency, series).  A tile of kTile epochs -- the reduced phase f (t - t_min) in turns,
// the three numbers of the precision matrix P and the two of q = P (x, y) -- is staged in LDS, and lane l takes the candidates
// l, l + threads, ...: for each it walks all epochs in order, every lane reading the same LDS address (a broadcast), with the
// thirteen running sums in registers, and solves its 4 x 4 system.  Every sum therefore has one fixed order: no atomics, no
// sums across lanes.  A lane keeps the power, the number and the four constants of its best candidate; the only reduction
// is the arg-max of (power, lowest candidate number) over the wave and then the workgroup, and the lane that owns the winner
// writes the record.  Nothing but kernels is enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_astrometric_core.hpp"
#include "exo_estimators_launch.hpp"

namespace {

using namespace ast;

constexpr int kWave = 64;
constexpr int kMaxThreads = 256;
constexpr int kTile = 256;  // epochs staged at a time: N is not capped by LDS
constexpr int kPrepThreads = 256;
constexpr int kMaxEcc = EXO_KEP_MAX_ECC;
constexpr int kCoef = EXO_AST_NCOEF;

// the eccentricity grid travels by value in the kernel arguments
struct EccGrid {
  int32_t n;
  double e[kMaxEcc];
};

// workspace, in doubles: tt[n], then per series the columns pxx, pxy, pyy, qx, qy [5][n], then t_min and per series chi2_0
struct Layout {
  int64_t n, n_series;
  __host__ __device__ int64_t tt() const { return 0; }
  __host__ __device__ int64_t col(int64_t b, int k) const { return n + (5 * b + k) * n; }
  __host__ __device__ int64_t t_min() const { return n + 5 * n_series * n; }
  __host__ __device__ int64_t chi2_0(int64_t b) const { return t_min() + 1 + b; }
  __host__ __device__ int64_t size() const { return chi2_0(n_series); }
};

// The columns the search reads -- tt = t - t_min and, per epoch, the precision matrix of the radial and the tangential error
// in the sky plane and its product with the measured position -- and chi2_0 = sum (x, y) P (x, y)^T, summed in a fixed shape
// (lane partials over the epochs, then a tree).  One workgroup per series.
__global__ __launch_bounds__(kPrepThreads) void astrometric_prepare_kernel(const double* __restrict__ t, const double* __restrict__ rho,
                                                                           const double* __restrict__ rho_err, int64_t n_rho_err,
                                                                           const double* __restrict__ theta,
                                                                           const double* __restrict__ theta_err, int64_t n_theta_err,
                                                                           Layout L, double* __restrict__ ws) {
  __shared__ double red[kPrepThreads];
  const int64_t b = blockIdx.x, n = L.n;
  const int lane = threadIdx.x;
  double lo = INFINITY;
  for (int64_t i = lane; i < n; i += kPrepThreads) lo = fmin(lo, t[i]);
  red[lane] = lo;
  __syncthreads();
  for (int o = kPrepThreads / 2; o > 0; o >>= 1) {
    if (lane < o) red[lane] = fmin(red[lane], red[lane + o]);
    __syncthreads();
  }
  const double t_min = red[0];
  __syncthreads();  // (the reduction's array is used again below)
  const double* re = rho_err + (n_rho_err > 1 ? b : 0) * n;
  const double* te = theta_err + (n_theta_err > 1 ? b : 0) * n;
  double* tt = ws + L.tt();
  double *pxx = ws + L.col(b, 0), *pxy = ws + L.col(b, 1), *pyy = ws + L.col(b, 2), *qx = ws + L.col(b, 3), *qy = ws + L.col(b, 4);
  double part = 0.0;
  for (int64_t i = lane; i < n; i += kPrepThreads) {
    const double r = rho[b * n + i];
    double s, c;
    sincos(theta[b * n + i], &s, &c);
    const double x = r * c, y = r * s;
    const double rt = r * te[i];
    const double wr = 1.0 / (re[i] * re[i]), wt = 1.0 / (rt * rt);  // (the MEASURED rho: the problem stays linear)
    const double xx = fma(wr * c, c, wt * s * s), xy = (wr - wt) * c * s, yy = fma(wr * s, s, wt * c * c);
    const double ax = fma(xx, x, xy * y), ay = fma(xy, x, yy * y);
    if (b == 0) tt[i] = t[i] - t_min;
    pxx[i] = xx;
    pxy[i] = xy;
    pyy[i] = yy;
    qx[i] = ax;
    qy[i] = ay;
    part += fma(x, ax, y * ay);
  }
  red[lane] = part;
  __syncthreads();
  for (int o = kPrepThreads / 2; o > 0; o >>= 1) {
    if (lane < o) red[lane] += red[lane + o];
    __syncthreads();
  }
  if (lane == 0) {
    if (b == 0) ws[L.t_min()] = t_min;
    ws[L.chi2_0(b)] = red[0];
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
  r.live = c < n_cand && kep::is_candidate(e, k);
  r.e = r.live ? e : 0.5;
  r.se = sqrt(1.0 - r.e);
  r.pe = sqrt(1.0 + r.e);
  r.phi = (double)k / (double)n_phase;
  return r;
}

// The search and the winner's record.  grid: (frequencies, series); blockDim: 64, 128 or 256.
__global__ __launch_bounds__(kMaxThreads) void astrometric_kernel(const double* __restrict__ freq, Layout L, EccGrid grid, int32_t n_phase,
                                                                  const double* __restrict__ ws, double* __restrict__ power,
                                                                  int32_t* __restrict__ candidate, double* __restrict__ coef) {
  __shared__ double turns_s[kTile], pxx_s[kTile], pxy_s[kTile], pyy_s[kTile], qx_s[kTile], qy_s[kTile];
  __shared__ double e_s[kMaxEcc], red_p[kMaxThreads / kWave];
  __shared__ int32_t red_c[kMaxThreads / kWave];
  const int64_t jf = blockIdx.x, n_freq = gridDim.x, b = blockIdx.y, n = L.n;
  const int lane = threadIdx.x, nt = blockDim.x;
  const double f = freq[jf];
  const double* __restrict__ tt = ws + L.tt();
  const double* __restrict__ pxx = ws + L.col(b, 0);
  const double* __restrict__ pxy = ws + L.col(b, 1);
  const double* __restrict__ pyy = ws + L.col(b, 2);
  const double* __restrict__ qx = ws + L.col(b, 3);
  const double* __restrict__ qy = ws + L.col(b, 4);
  const int n_cand = grid.n * n_phase;
  for (int q = lane; q < grid.n; q += nt) e_s[q] = grid.e[q];
  __syncthreads();

  // ---- the search: this lane's candidates, ascending, so that a strict > keeps the lowest of equal maxima
  kep::Best mine = kep::best_init();
  double ta = NAN, tb = NAN, tf = NAN, tg = NAN;
  for (int c0 = 0; c0 < n_cand; c0 += nt) {
    const int c = c0 + lane;
    const Candidate cd = candidate_of(c, n_cand, n_phase, e_s);
    Sums a = sums_init();
    for (int64_t lo = 0; lo < n; lo += kTile) {
      const int len = (int)(n - lo < kTile ? n - lo : kTile);
      __syncthreads();  // (every lane is done with the tile before)
      for (int i = lane; i < len; i += nt) {
        turns_s[i] = est::ls_phase_turns(f, tt[lo + i]);
        pxx_s[i] = pxx[lo + i];
        pxy_s[i] = pxy[lo + i];
        pyy_s[i] = pyy[lo + i];
        qx_s[i] = qx[lo + i];
        qy_s[i] = qy[lo + i];
      }
      __syncthreads();
      if (cd.live) {
        for (int i = 0; i < len; ++i) {
          double xi, eta;
          orbit_plane(turns_s[i], cd.phi, cd.e, cd.se, cd.pe, &xi, &eta);
          accumulate(a, xi, eta, pxx_s[i], pxy_s[i], pyy_s[i], qx_s[i], qy_s[i]);
        }
      }
    }
    if (cd.live) {
      const Fit r = fit(a);
      if (r.ok) {
        const int32_t before = mine.candidate;
        kep::best_take(mine, r.power, c);
        if (mine.candidate != before) {
          ta = r.ta;
          tb = r.tb;
          tf = r.tf;
          tg = r.tg;
        }
      }
    }
  }
  kep::Best best = mine;
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double p = __shfl_down(best.power, o, kWave);
    const int32_t c = __shfl_down(best.candidate, o, kWave);
    kep::best_take(best, p, c);
  }
  if (lane % kWave == 0) {
    red_p[lane / kWave] = best.power;
    red_c[lane / kWave] = best.candidate;
  }
  __syncthreads();
  best = kep::best_init();
  for (int i = 0; i < nt / kWave; ++i) kep::best_take(best, red_p[i], red_c[i]);

  // ---- the winner's record: power, candidate, the four constants, the elements, t_periastron and chi2
  const int64_t slot = b * n_freq + jf;
  if (best.candidate == INT32_MAX) {  // (no candidate at this frequency: power 0, the rest NaN)
    if (lane == 0) {
      power[slot] = 0.0;
      candidate[slot] = -1;
      for (int q = 0; q < kCoef; ++q) coef[slot * kCoef + q] = NAN;
    }
    return;
  }
  if (mine.candidate != best.candidate) return;  // (candidate numbers are unique: one lane is left)
  const Elements el = campbell(ta, tb, tf, tg);
  const int k = best.candidate % n_phase;
  double* out = coef + slot * kCoef;
  power[slot] = best.power;
  candidate[slot] = best.candidate;
  out[0] = ta;
  out[1] = tb;
  out[2] = tf;
  out[3] = tg;
  out[4] = el.a_angular;
  out[5] = el.incl;
  out[6] = el.omega;
  out[7] = el.Omega;
  out[8] = ws[L.t_min()] + ((double)k / (double)n_phase) / f;
  out[9] = ws[L.chi2_0(b)] - 2.0 * best.power;
}

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

int64_t exo_astrometric_workspace_bytes(int64_t n, int64_t n_series) {
  if (n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535) return -1;
  return 8 * Layout{n, n_series}.size();
}

int exo_astrometric_power_f64(const double* t, const double* rho, const double* rho_err, int64_t n_rho_err, const double* theta,
                              const double* theta_err, int64_t n_theta_err, int64_t n, int64_t n_series, const double* frequencies,
                              int64_t n_frequency, const double* ecc, int32_t n_ecc, int32_t n_phase, double* power,
                              int32_t* candidate, double* coef, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_frequency == 0) return EXO_OK;
  if (!t || !rho || !rho_err || !theta || !theta_err || !frequencies || !ecc || !power || !candidate || !coef || !workspace ||
      n < 1 || n > INT32_MAX || n_series < 1 || n_series > 65535 || (n_rho_err != 1 && n_rho_err != n_series) ||
      (n_theta_err != 1 && n_theta_err != n_series) || n_frequency < 0 || n_frequency > INT32_MAX || n_ecc < 1 ||
      n_ecc > kMaxEcc || n_phase < 1 || n_phase > EXO_KEP_MAX_PHASES)
    return EXO_ERR_INVALID_ARGUMENT;
  EccGrid grid = {};
  grid.n = n_ecc;
  for (int j = 0; j < n_ecc; ++j) {
    if (!(ecc[j] >= 0.0 && ecc[j] < 1.0)) return EXO_ERR_INVALID_ARGUMENT;
    grid.e[j] = ecc[j];
  }
  if (workspace_bytes < exo_astrometric_workspace_bytes(n, n_series)) return EXO_ERR_WORKSPACE;
  const Layout L = {n, n_series};
  double* ws = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(astrometric_prepare_kernel, dim3((unsigned)n_series), dim3(kPrepThreads), 0, s, t, rho, rho_err, n_rho_err, theta,
                     theta_err, n_theta_err, L, ws);
  hipLaunchKernelGGL(astrometric_kernel, dim3((unsigned)n_frequency, (unsigned)n_series), dim3(threads_for((int64_t)n_ecc * n_phase)), 0,
                     s, frequencies, L, grid, n_phase, (const double*)ws, power, candidate, coef);
  return launch_status();
}

}  // extern "C"
