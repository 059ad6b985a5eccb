// Host build of exoplanet_amd/csrc/exo_noise_core.hpp for tests/test_noise_terms_host.py: the same per-element arithmetic
// and the same order of summation as the kernels of exo_noise.hip (`lanes` strided accumulators, then the lanes in turn),
// without a GPU.
#define EXO_HOST_BUILD 1
#include "../exoplanet_amd/csrc/exo_noise_core.hpp"

#include <vector>

using namespace nz;

static double lane_sum(const std::vector<double>& v) {
  double s = 0.0;
  for (double x : v) s += x;
  return s;
}

extern "C" {

int harness_renorm_every() { return kRenorm; }

// series[8] as noise_series_kernel leaves it
void harness_series(const double* y, const double* var, int64_t n, int one_var, int lanes, double* series) {
  std::vector<Pass1> p1(lanes, Pass1{0.0, 0.0});
  for (int64_t i = 0; i < n; ++i) pass1_add(p1[i % lanes], y[i], one_var ? 1.0 : rcp(var[i]));
  double su = 0.0, suy = 0.0;
  for (const Pass1& p : p1) su += p.u;
  for (const Pass1& p : p1) suy += p.uy;
  const double ybar = suy / su;
  std::vector<Pass2> p2(lanes, Pass2{0.0, 0.0, 0.0, 0.0, 0.0});
  std::vector<LogProd> lp(lanes, logprod_one());
  std::vector<int> cnt(lanes, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int l = (int)(i % lanes);
    const double v = one_var ? 1.0 : var[i];
    pass2_add(p2[l], y[i], one_var ? 1.0 : rcp(v), ybar);
    logprod_mul(lp[l], v);
    if (++cnt[l] == kRenorm) { logprod_renorm(lp[l]); cnt[l] = 0; }
  }
  series[0] = ybar; series[1] = su;
  for (int q = 2; q < kSeries; ++q) series[q] = 0.0;
  for (int l = 0; l < lanes; ++l) series[2] += p2[l].S1;
  for (int l = 0; l < lanes; ++l) series[3] += p2[l].S2;
  for (int l = 0; l < lanes; ++l) series[4] += p2[l].T0;
  for (int l = 0; l < lanes; ++l) series[5] += p2[l].T1;
  for (int l = 0; l < lanes; ++l) series[6] += p2[l].T2;
  for (int l = 0; l < lanes; ++l) series[7] += logprod_value(lp[l]);
}

// terms [5][n_draw]; the regime from n_var / n_jit alone, as exo_white_noise_terms_f64 picks it.  Returns the regime (0: series
// sums, 1: element by element)
int harness_terms(const double* y, const double* var, int64_t n, int64_t n_var, const double* mean, int64_t n_mean,
                  const double* jit2, int64_t n_jit, int64_t n_draw, int lanes, double* terms) {
  const bool separable = n > 0 && (n_jit == 0 || n_var == 1);
  if (separable) {
    double s[kSeries];
    harness_series(y, var, n, n_var == 1, lanes, s);
    const Series ser{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
    for (int64_t d = 0; d < n_draw; ++d) {
      double out[kTerms];
      from_series(ser, n_var == 1, n_var == 1 ? var[0] : 0.0, (double)n, mean[n_mean == 1 ? 0 : d],
                  n_jit == 0 ? 0.0 : jit2[n_jit == 1 ? 0 : d], out);
      for (int q = 0; q < kTerms; ++q) terms[q * n_draw + d] = out[q];
    }
    return 0;
  }
  for (int64_t d = 0; d < n_draw; ++d) {
    const double mu = mean[n_mean == 1 ? 0 : d], s2 = n_jit == 0 ? 0.0 : jit2[n_jit == 1 ? 0 : d];
    std::vector<Acc> acc(lanes, acc_zero());
    std::vector<int> cnt(lanes, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int l = (int)(i % lanes);
      acc_add(acc[l], y[i], var[i], mu, s2);
      if (++cnt[l] == kRenorm) { logprod_renorm(acc[l].lam); cnt[l] = 0; }
    }
    std::vector<double> col(lanes);
    for (int q = 0; q < kTerms; ++q) {
      for (int l = 0; l < lanes; ++l)
        col[l] = q == kQ ? acc[l].Q : q == kLam ? logprod_value(acc[l].lam) : q == kG ? acc[l].G : q == kH ? acc[l].H : acc[l].A;
      terms[q * n_draw + d] = lane_sum(col);
    }
  }
  return 1;
}

// sum of log(x_i): 0 -- one logarithm per element, 1 -- the running product of mantissas (one lane)
double harness_sum_log(const double* x, int64_t n, int product) {
  if (!product) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += log(x[i]);
    return s;
  }
  LogProd p = logprod_one();
  int cnt = 0;
  for (int64_t i = 0; i < n; ++i) {
    logprod_mul(p, x[i]);
    if (++cnt == kRenorm) { logprod_renorm(p); cnt = 0; }
  }
  return logprod_value(p);
}

}  // extern "C"
