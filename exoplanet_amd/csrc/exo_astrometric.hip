// exo_astrometric.hip -- the astrometric orbit search of a batch of (rho, theta) series on one time axis
// (exoplanet_amd/estimators.py: astrometric_power, astrometric_estimator): at every frequency the best of a grid of
// (eccentricity, phase of periastron) candidates, each a linear least-squares fit of the four Thiele-Innes constants to the
// sky-plane positions, with radial and tangential errors.  A translation unit of its own: none of the other kernels changes.
// The arithmetic lives in exo_astrometric_core.hpp (tested on the host), the search over the candidates in
// exo_orbit_search.hpp; definition, layout, resources and timings: DESIGN.md section 23.  Compiled with -ffp-contract=off, as
// the host build of the core is.  Nothing but kernels is enqueued.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_astrometric_core.hpp"
#include "exo_estimators_launch.hpp"
#include "exo_orbit_search.hpp"

namespace {

using namespace ast;
using namespace orb;

constexpr int kCoef = EXO_AST_NCOEF;

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
  const double t_min = block_min(t, n, red);
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
  const double chi2_0 = block_sum(part, red);
  if (lane == 0) {
    if (b == 0) ws[L.t_min()] = t_min;
    ws[L.chi2_0(b)] = chi2_0;
  }
}

// the problem of exo_orbit_search.hpp: a tile carries the five columns; a candidate keeps the thirteen sums, all zero at
// first; its score is the power of the 4 x 4 fit where that has every pivot; of the lane's best the four constants are used
struct AstrometricProblem {
  const double* __restrict__ col;  // pxx, pxy, pyy, qx, qy of the series: [5][n]
  int64_t n;
  double (*col_s)[kTile];

  using State = Sums;
  using Fit = ast::Fit;

  __device__ __forceinline__ void stage(int64_t lo, int i) const {
    for (int k = 0; k < 5; ++k) col_s[k][i] = col[k * n + lo + i];
  }
  __device__ __forceinline__ void walk(State& a, const Candidate& cd, const double* turns_s, int64_t, int len) const {
    for (int i = 0; i < len; ++i) {
      double xi, eta;
      orbit_plane(turns_s[i], cd.phi, cd.e, cd.se, cd.pe, &xi, &eta);
      accumulate(a, xi, eta, col_s[0][i], col_s[1][i], col_s[2][i], col_s[3][i], col_s[4][i]);
    }
  }
  __device__ __forceinline__ Fit fit(const State& a) const { return ast::fit(a); }
  __device__ __forceinline__ bool counts(const Fit& r) const { return r.ok; }
};

// The search and the winner's record.  grid: (frequencies, series); blockDim: 64, 128 or 256.
__global__ __launch_bounds__(kMaxThreads) void astrometric_kernel(const double* __restrict__ freq, Layout L, EccGrid grid, int32_t n_phase,
                                                                  const double* __restrict__ ws, double* __restrict__ power,
                                                                  int32_t* __restrict__ candidate, double* __restrict__ coef) {
  __shared__ SearchLds sh;
  __shared__ double col_s[5][kTile];
  const int64_t jf = blockIdx.x, n_freq = gridDim.x, b = blockIdx.y;
  const double f = freq[jf];
  const AstrometricProblem problem = {ws + L.col(b, 0), L.n, col_s};
  Fit beta;  // (of this lane's best candidate: set where the lane has one)
  const Best mine = lane_search(problem, sh, grid, n_phase, f, ws + L.tt(), L.n, beta);
  const Best best = block_best(mine, sh);

  // ---- the winner's record: power, candidate, the four constants, the elements, t_periastron and chi2
  const int64_t slot = b * n_freq + jf;
  if (best.candidate == INT32_MAX) {  // (no candidate at this frequency: power 0, the rest NaN)
    write_no_candidate(0.0, slot, kCoef, power, candidate, coef);
    return;
  }
  if (mine.candidate != best.candidate) return;  // (candidate numbers are unique: one lane is left)
  const Elements el = campbell(beta.ta, beta.tb, beta.tf, beta.tg);
  const int k = best.candidate % n_phase;
  double* out = coef + slot * kCoef;
  power[slot] = best.power;
  candidate[slot] = best.candidate;
  out[0] = beta.ta;
  out[1] = beta.tb;
  out[2] = beta.tf;
  out[3] = beta.tg;
  out[4] = el.a_angular;
  out[5] = el.incl;
  out[6] = el.omega;
  out[7] = el.Omega;
  out[8] = ws[L.t_min()] + ((double)k / (double)n_phase) / f;
  out[9] = ws[L.chi2_0(b)] - 2.0 * best.power;
}

}  // namespace

extern "C" {

int64_t exo_astrometric_workspace_bytes(int64_t n, int64_t n_series) {
  if (!series_ok(n, n_series)) return -1;
  return 8 * Layout{n, n_series}.size();
}

int exo_astrometric_power_f64(const double* t, const double* rho, const double* rho_err, int64_t n_rho_err, const double* theta,
                              const double* theta_err, int64_t n_theta_err, int64_t n, int64_t n_series, const double* frequencies,
                              int64_t n_frequency, const double* ecc, int32_t n_ecc, int32_t n_phase, double* power,
                              int32_t* candidate, double* coef, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_frequency == 0) return EXO_OK;
  if (!t || !rho || !rho_err || !theta || !theta_err || !frequencies || !ecc || !power || !candidate || !coef || !workspace ||
      !sizes_ok(n, n_series, n_frequency, n_ecc, n_phase) || (n_rho_err != 1 && n_rho_err != n_series) ||
      (n_theta_err != 1 && n_theta_err != n_series))
    return EXO_ERR_INVALID_ARGUMENT;
  EccGrid grid = {};
  if (!ecc_grid(ecc, n_ecc, &grid)) return EXO_ERR_INVALID_ARGUMENT;
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
