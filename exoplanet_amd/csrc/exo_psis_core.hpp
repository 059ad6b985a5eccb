// exo_psis_core.hpp -- the per-column arithmetic of PSIS-LOO and WAIC (exoplanet_amd/comparison.py, loo / waic;
// exo_column_psis_f64): from one column l_s of an (S, N) array of pointwise log-likelihoods, along the strided axis, the
// Pareto-smoothed leave-one-out density, the Pareto k, the lppd and the variance over the draws.  Definition: DESIGN.md
// section 25 and tests/psis_oracle.py.  Compiles for the device (exo_psis.hip) and, with EXO_HOST_BUILD, for the host
// (tests/psis_harness.cpp checks it against the numpy statement without a GPU).
//
// The log ratios are x_s = l_min - l_s <= 0.  A rounded subtraction is monotone, so the j-th smallest x is l_min minus the
// j-th largest l: the cut-off x_(S-M-1) is l_min - l_(M), and l_(M) is ONE order statistic of the column as it lies in memory
// -- the selection by counting passes of exo_predictive_core.hpp (Extent, Bisect<1>, Column) finds it, B = 3 bits of the
// interval of keys per pass.  The tail {x > c}, at most M <= 1024 values, is then gathered, sorted and fitted (Zhang &
// Stephens 2009, as ArviZ's _gpdfit applies it); everything outside the tail enters the sums as exp(x_s) and as a count.
// The pieces below are written against any tail accessor T with T[j] = the j-th smallest x of the tail, so that the kernel,
// whose tail lies in LDS with the rows shared out over lanes, calls the same functions as the one-lane routine at the end.
#pragma once
#include <math.h>
#include <stdint.h>

#include "exo_predictive_core.hpp"

#define EXO_PSIS_HD EXO_PRED_HD

namespace psis {

using predictive::Bisect;
using predictive::Column;
using predictive::Extent;
using predictive::Rank;

constexpr int kMaxTail = 1024;                           // EXO_PSIS_MAX_TAIL
constexpr int kMaxTrial = 62;                            // m = 30 + floor(sqrt(n)), n <= 1024
constexpr int kBits = 3;                                 // bits of the key interval a counting pass settles (7 trial values)
constexpr double kEps = 2.220446049250313e-16;           // DBL_EPSILON
constexpr double kLogDblMin = -708.3964185322641;        // log(DBL_MIN), rounded to double

struct Result {
  double elpd, k, lppd, var;
  int32_t n_tail;
};

EXO_PSIS_HD Result result_nan() { return Result{NAN, NAN, NAN, NAN, 0}; }

// a column with a NaN or an infinity (or no row at all) is not computed
EXO_PSIS_HD bool extent_bad(const Extent& e, int64_t n_rows) {
  return n_rows == 0 || e.m < n_rows || e.kmin <= detrend::kKeyNegInf || e.kmax >= detrend::kKeyPosInf;
}

// the order statistic of l that sets the cut-off: l_(min(M, S - 1)), i.e. x_(max(S - M - 1, 0))
EXO_PSIS_HD Rank cut_rank(int64_t n_rows, int32_t M) { return Rank{(int32_t)(M < n_rows - 1 ? M : n_rows - 1), 0}; }

EXO_PSIS_HD double cut_off(double lmin, double l_at_rank) {
  const double c = lmin - l_at_rank;
  return c > kLogDblMin ? c : kLogDblMin;
}

// ---- the generalised-Pareto fit ------------------------------------------------------------------------------------------------
EXO_PSIS_HD int trial_count(int n) {
  int r = 0;
  while ((r + 1) * (r + 1) <= n) ++r;                    // floor(sqrt(n)) in whole numbers
  return 30 + r;
}

EXO_PSIS_HD int quartile_index(int n) { return (n + 2) / 4 - 1; }   // floor(n / 4 + 0.5) - 1

template <class T>
EXO_PSIS_HD double excess(T xt, int j, double ec) { return exp(xt[j]) - ec; }

// b_i, i = 1 .. m
EXO_PSIS_HD double trial_b(int i, int m, double u_quart, double u_last) {
  return (1.0 - sqrt((double)m / ((double)i - 0.5))) / (3.0 * u_quart) + 1.0 / u_last;
}

// k_i = (1 / n) sum_j log1p(-b_i u_j) for NT values of b at once, j ascending, one term after the other
template <int NT, class T>
EXO_PSIS_HD void mean_log1p(T xt, int n, double ec, const double* b, double* out) {
  double acc[NT];
  for (int r = 0; r < NT; ++r) acc[r] = 0.0;
  for (int j = 0; j < n; ++j) {
    const double u = excess(xt, j, ec);
    for (int r = 0; r < NT; ++r) acc[r] += log1p(-b[r] * u);
  }
  for (int r = 0; r < NT; ++r) out[r] = acc[r] / (double)n;
}

EXO_PSIS_HD double trial_L(double b, double k, int n) { return (double)n * (log(-b / k) - k - 1.0); }

// w_i = 1 / sum_i' exp(L_i' - L_i), i' ascending (an overflow to inf: weight 0)
template <class A>
EXO_PSIS_HD double trial_weight(A L, int m, int i) {
  const double Li = L[i];
  double acc = 0.0;
  for (int q = 0; q < m; ++q) acc += exp(L[q] - Li);
  return 1.0 / acc;
}

// b = sum_i b_i w_i / (sum of the kept w), the weights below 10 eps dropped
template <class A>
EXO_PSIS_HD double posterior_b(A w, int m, double u_quart, double u_last) {
  double total = 0.0;
  for (int i = 0; i < m; ++i) total += (w[i] >= 10.0 * kEps) ? w[i] : 0.0;
  double b = 0.0;
  for (int i = 0; i < m; ++i)
    if (w[i] >= 10.0 * kEps) b += trial_b(i + 1, m, u_quart, u_last) * (w[i] / total);
  return b;
}

struct Fit {
  double k, sigma;
};

EXO_PSIS_HD Fit fit_finish(double k1, double b, int n) {
  return Fit{((double)n * k1 + 5.0) / ((double)n + 10.0), -k1 / b};
}

// ---- the smoothed tail ---------------------------------------------------------------------------------------------------------
// the j-th of n smoothed log ratios (k finite)
EXO_PSIS_HD double smoothed(int j, int n, Fit f, double ec) {
  const double p = ((double)j + 0.5) / (double)n;
  const double q = fabs(f.k) < kEps ? -f.sigma * log1p(-p) : f.sigma * expm1(-f.k * log1p(-p)) / f.k;
  const double v = log(q + ec);
  return v > 0.0 ? 0.0 : v;
}

EXO_PSIS_HD bool is_finite(double v) { return v - v == 0.0; }

// x'_j: smoothed where the fit gave a finite k, the value itself otherwise
template <class T>
EXO_PSIS_HD double tail_value(T xt, int j, int n, Fit f, double ec) { return is_finite(f.k) ? smoothed(j, n, f, ec) : xt[j]; }

// ---- the last step -------------------------------------------------------------------------------------------------------------
// body = sum of exp(x_s) outside the tail, tail_sum = sum_j exp(x'_j), mx = the largest term of the elpd sum, acc = the sum of
// the terms' exp(. - mx) with the S - n draws outside the tail as (S - n) exp(l_min - mx)
EXO_PSIS_HD double elpd_finish(double body, double tail_sum, double acc, double mx) { return log(acc) + mx - log(body + tail_sum); }

EXO_PSIS_HD double lppd_finish(double sum_exp, double lmax, int64_t n_rows) { return log(sum_exp) + lmax - log((double)n_rows); }

// ---- the per-column routine ----------------------------------------------------------------------------------------------------
// One lane owning the whole column; `tail`: room for M doubles.  The kernel runs the same steps with the rows and the trial
// values shared out and a merge after each.
template <class A>
EXO_PSIS_HD void sort_ascending(A v, int n) {               // (heap sort: in place, no recursion)
  for (int start = n / 2 - 1, end = n; end > 1;) {
    double t;
    int root;
    if (start >= 0) {
      root = start--;
      t = v[root];
    } else {
      --end;
      t = v[end];
      v[end] = v[0];
      root = 0;
    }
    for (int child = 2 * root + 1; child < end; child = 2 * root + 1) {
      if (child + 1 < end && v[child] < v[child + 1]) ++child;
      if (!(t < v[child])) break;
      v[root] = v[child];
      root = child;
    }
    v[root] = t;
  }
}

template <class P>
EXO_PSIS_HD Result column_psis(P col, int64_t n_rows, int32_t M, double* tail) {
  using namespace predictive;
  Extent e = extent_empty();
  double sum = 0.0;
  for (int64_t i = 0; i < n_rows; ++i) {
    const double v = col[i];
    extent_add(e, v);
    sum += v;
  }
  if (extent_bad(e, n_rows)) return result_nan();
  const double lmin = key_double(e.kmin) + 0.0, lmax = key_double(e.kmax) + 0.0;
  const double mean = sum / (double)n_rows;
  // the cut-off
  const Rank rank = cut_rank(n_rows, M);
  Bisect<1> s;
  bisect_begin<1>(s, e, &rank);
  constexpr int K = (1 << kBits) - 1;
  for (int pass = passes_needed(e, kBits); pass > 0; --pass) {
    double x[K];
    int32_t c[K];
    for (int j = 0; j < K; ++j) x[j] = bisect_trial<K>(s, 0, j + 1), c[j] = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
      const double v = col[i];
      for (int j = 0; j < K; ++j) c[j] += (v < x[j]) ? 1 : 0;
    }
    bisect_decide<K>(s, 0, c);
  }
  const double c = cut_off(lmin, bisect_value<1>(s, 0));
  const double ec = exp(c);
  // the tail, and every sum over the rows
  int n = 0;
  double body = 0.0, sum_exp = 0.0, var = 0.0;
  for (int64_t i = 0; i < n_rows; ++i) {
    const double v = col[i];
    const double x = lmin - v, d = v - mean;
    var += d * d;
    sum_exp += exp(v - lmax);
    if (x > c) {
      if (n < M) tail[n] = x;
      ++n;
    } else {
      body += exp(x);
    }
  }
  if (n > M) return result_nan();                            // (cannot happen: #{x > x_(S-M-1)} <= M)
  sort_ascending(tail, n);
  Fit f{INFINITY, 0.0};
  if (n > 4) {
    const int m = trial_count(n);
    const double uq = excess(tail, quartile_index(n), ec), ul = excess(tail, n - 1, ec);
    double L[kMaxTrial], w[kMaxTrial];
    for (int i = 0; i < m; ++i) {
      const double b = trial_b(i + 1, m, uq, ul);
      double k;
      mean_log1p<1>(tail, n, ec, &b, &k);
      L[i] = trial_L(b, k, n);
    }
    for (int i = 0; i < m; ++i) w[i] = trial_weight(L, m, i);
    const double b = posterior_b(w, m, uq, ul);
    double k1;
    mean_log1p<1>(tail, n, ec, &b, &k1);
    f = fit_finish(k1, b, n);
  }
  double mx = n < n_rows ? lmin : -INFINITY;
  for (int j = 0; j < n; ++j) {
    const double t = tail_value(tail, j, n, f, ec) + (lmin - tail[j]);
    mx = t > mx ? t : mx;
  }
  double tail_sum = 0.0, acc = n < n_rows ? (double)(n_rows - n) * exp(lmin - mx) : 0.0;
  for (int j = 0; j < n; ++j) tail_sum += exp(tail_value(tail, j, n, f, ec));
  for (int j = 0; j < n; ++j) acc += exp(tail_value(tail, j, n, f, ec) + (lmin - tail[j]) - mx);
  return Result{elpd_finish(body, tail_sum, acc, mx), f.k, lppd_finish(sum_exp, lmax, n_rows), var / (double)n_rows, n};
}

}  // namespace psis
