// exo_metric_core.hpp -- the arithmetic of the dense metric of HMC / NUTS (exoplanet_amd/sampling.py, set_metric and
// adapt_mass="dense"; exo_metric_apply_f64, exo_metric_accumulate_f64, exo_metric_update_f64).  A metric is a covariance
// Sigma = L L^T (L lower triangular) and a centre c; the samplers run at unit masses in x, q = c + L x.  Definition: DESIGN.md
// section 27 and tests/metric_oracle.py.  Compiles for the device (exo_metric.hip) and, with EXO_HOST_BUILD, for the host
// (tests/metric_harness.cpp checks it against the long-double numpy statement without a GPU).
//
// Every sum has ONE order, stated at the function, and no product is contracted into a fused multiply-add (both builds are
// compiled with -ffp-contract=off), so the kernels and the host build give the same bits.  The functions are written against
// any lower-triangle accessor T with T(i, j) = L[i][j], j <= i: the host reads the row-major (n, n) array as it lies in
// memory, the kernels a packed copy in LDS.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_MET_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_MET_HD __device__ __forceinline__
#endif

namespace metric {

constexpr int kMaxN = 64;                                // EXO_METRIC_MAX_N
constexpr int kForward = 0, kTransposed = 1, kSolve = 2; // EXO_METRIC_FORWARD, _TRANSPOSED, _SOLVE
constexpr int kOk = 0, kTooFew = 1, kNotFinite = 2, kNotPositive = 3;   // EXO_METRIC_STATUS_*
constexpr double kShrinkCount = 5.0;                     // Stan's regularisation, weight 5 / (N + 5), ...
constexpr double kShrinkTarget = 1e-3;                   // ... on 1e-3 times the DIAGONAL of S (Stan: times the identity)

// the lower triangle of a row-major (n, n) array
struct Dense {
  const double* p;
  int n;
  EXO_MET_HD double operator()(int i, int j) const { return p[i * n + j]; }
};

// the lower triangle packed row after row: (i, j) at i (i + 1) / 2 + j
struct Packed {
  const double* p;
  EXO_MET_HD double operator()(int i, int j) const { return p[i * (i + 1) / 2 + j]; }
};

EXO_MET_HD int packed_size(int n) { return n * (n + 1) / 2; }

// ---- the three maps of one row, IN PLACE (r[0 .. n - 1]) ----------------------------------------------------------------------
// q_i = c_i + (((L_i0 x_0) + L_i1 x_1) + ... + L_ii x_i): the sum starts at the first product and takes j ascending, the centre
// is added last.  i runs downwards, so that q_i replaces x_i after every row that reads it.
template <class T>
EXO_MET_HD void forward_row(const T& L, const double* c, int n, double* r) {
  for (int i = n - 1; i >= 0; --i) {
    double acc = L(i, 0) * r[0];
    for (int j = 1; j <= i; ++j) acc += L(i, j) * r[j];
    r[i] = c[i] + acc;
  }
}

// gx_j = ((gq_j L_jj) + gq_{j+1} L_{j+1,j}) + ... + gq_{n-1} L_{n-1,j}: i ascending from j; j runs upwards, in place
template <class T>
EXO_MET_HD void transposed_row(const T& L, int n, double* r) {
  for (int j = 0; j < n; ++j) {
    double acc = r[j] * L(j, j);
    for (int i = j + 1; i < n; ++i) acc += r[i] * L(i, j);
    r[j] = acc;
  }
}

// L x = q - c by forward substitution: x_i = ((((q_i - c_i) - L_i0 x_0) - L_i1 x_1) - ...) / L_ii, j ascending, in place
template <class T>
EXO_MET_HD void solve_row(const T& L, const double* c, int n, double* r) {
  for (int i = 0; i < n; ++i) {
    double acc = r[i] - c[i];
    for (int j = 0; j < i; ++j) acc -= L(i, j) * r[j];
    r[i] = acc / L(i, i);
  }
}

template <class T>
EXO_MET_HD void apply_row(const T& L, const double* c, int n, int mode, double* r) {
  if (mode == kForward) forward_row(L, c, n, r);
  else if (mode == kTransposed) transposed_row(L, n, r);
  else solve_row(L, c, n, r);
}

// ---- the window's sums ---------------------------------------------------------------------------------------------------------
// one more row of shifted positions dq = q - s into one running sum: the first moments (j < 0) or the product (i, j)
EXO_MET_HD double accumulate_term(double sum, const double* dq, int i, int j) { return j < 0 ? sum + dq[i] : sum + dq[i] * dq[j]; }

EXO_MET_HD bool row_finite(const double* q, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(q[i])) return false;
  return true;
}

// ---- the update ----------------------------------------------------------------------------------------------------------------
// the centre, m_i = s_i + sum1_i / N
EXO_MET_HD double update_center(double s_i, double sum1_i, double N) { return s_i + sum1_i / N; }

// Sigma_ij = N / (N + 5) S_ij + [i == j] 1e-3 (5 / (N + 5)) S_ii, S_ij = (sum2_ij - sum1_i sum1_j / N) / (N - 1); shrink false
// (the tests' rank-deficient window): Sigma = S.  Stan adds 1e-3 (5 / (N + 5)) itself, which presumes parameters of order one;
// a transit model's period or flux level has a posterior variance of 1e-9 or less in its own units, and that floor -- 1e-6 --
// would BE the metric in those directions.  Relative to the parameter's own variance the shrinkage keeps its weight and its
// purpose (the off-diagonal part is damped, the correlation matrix stays away from singular) in any units.
EXO_MET_HD double update_cov(double sum2_ij, double sum1_i, double sum1_j, double N, bool diagonal, bool shrink) {
  const double S = (sum2_ij - sum1_i * sum1_j / N) / (N - 1.0);
  if (!shrink) return S;
  const double v = N / (N + kShrinkCount) * S;
  return diagonal ? v + kShrinkTarget * (kShrinkCount / (N + kShrinkCount)) * S : v;
}

// entry (i, j), j <= i, of the Cholesky factor from Sigma_ij and the entries before it in rows i and j: Sigma_ij less the
// products L_ik L_jk one after the other, k ascending; off the diagonal divided by L_jj; on it the PIVOT, whose square root the
// caller takes after looking at its sign.  Row by row (host) or column by column (kernel), an entry is the same number.
template <class T>
EXO_MET_HD double cholesky_entry(const T& L, double sigma_ij, int i, int j) {
  double acc = sigma_ij;
  for (int k = 0; k < j; ++k) acc -= L(i, k) * L(j, k);
  return i == j ? acc : acc / L(j, j);
}

}  // namespace metric
