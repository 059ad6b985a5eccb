// Host build of exoplanet_amd/csrc/exo_laplace_core.hpp for tests/test_laplace_host.py (g++, no GPU): the stencil's points
// element by element and the factorisation chain by chain, entry by entry -- the loops of the kernels of exo_laplace.hip in
// another nesting, every number formed by the same core function.
#define EXO_HOST_BUILD
#include "../exoplanet_amd/csrc/exo_laplace_core.hpp"

extern "C" {

int harness_points(const double* x, int64_t n_chain, int32_t n, const int32_t* free_index, int32_t m, const double* scale,
                   int32_t scale_per_chain, const double* hess, double delta, int32_t order, double* points, double* dx) {
  using namespace laplace;
  if (n < 1 || n > kMaxN || m < 1 || m > n || (order != 2 && order != 4)) return 1;
  const int rows = order * m;
  for (int64_t d = 0; d < n_chain; ++d)
    for (int r = 0; r < rows; ++r) {
      const int s = r / m, k = r - s * m, jf = free_index[k];
      double* row = points + (d * rows + r) * n;
      for (int j = 0; j < n; ++j) row[j] = x[d * n + j];
      const double xv = x[d * n + jf];
      const double h = step(xv, scale != nullptr, scale ? scale[d * (scale_per_chain ? n : 0) + jf] : 0.0, hess != nullptr,
                            hess ? hess[(d * m + k) * m + k] : 0.0, delta);
      row[jf] = xv + offset(s, h);
      dx[d * rows + r] = row[jf] - xv;
    }
  return 0;
}

int harness_factor(const double* grad, const double* dx, const double* logp, int64_t n_chain, int32_t n, const int32_t* free_index,
                   int32_t m, int32_t order, double* hess, double* cov, double* sd, double* logdet, double* log_evidence,
                   double* asymmetry, double* fd_error, int32_t* status) {
  using namespace laplace;
  if (n < 1 || n > kMaxN || m < 1 || m > n || (order != 2 && order != 4)) return 1;
  static double Hp[kMaxN * (kMaxN + 1) / 2], Rp[kMaxN * (kMaxN + 1) / 2], Tp[kMaxN * (kMaxN + 1) / 2];
  double hd[kMaxN], sc[kMaxN];
  const int rows = order * m;
  const int* F = free_index;
  for (int64_t d = 0; d < n_chain; ++d) {
    const double* g = grad + d * rows * n;
    const double* h = dx + d * rows;
    double *H = hess + d * m * m, *C = cov + d * m * m;
    bool not_finite = false, not_positive = false;
    for (int r = 0; r < rows; ++r) {
      if (!isfinite(h[r])) not_finite = true;
      for (int i = 0; i < m; ++i)
        if (!isfinite(g[r * n + F[i]])) not_finite = true;
    }
    for (int k = 0; k < m; ++k) {
      if (h[k] - h[m + k] == 0.0) not_finite = true;
      if (order == 4 && h[2 * m + k] - h[3 * m + k] == 0.0) not_finite = true;
    }
    for (int i = 0; i < m; ++i)
      for (int k = 0; k <= i; ++k) {
        const int p = i * (i + 1) / 2 + k;
        const double a1_ik = raw_entry(g[k * n + F[i]], g[(m + k) * n + F[i]], h[k], h[m + k]);
        const double a1_ki = raw_entry(g[i * n + F[k]], g[(m + i) * n + F[k]], h[i], h[m + i]);
        double a_ik = a1_ik, a_ki = a1_ki, step_diff = NAN;
        if (order == 4) {
          const double a2_ik = raw_entry(g[(2 * m + k) * n + F[i]], g[(3 * m + k) * n + F[i]], h[2 * m + k], h[3 * m + k]);
          const double a2_ki = raw_entry(g[(2 * m + i) * n + F[k]], g[(3 * m + i) * n + F[k]], h[2 * m + i], h[3 * m + i]);
          a_ik = richardson(a1_ik, a2_ik);
          a_ki = richardson(a1_ki, a2_ki);
          step_diff = symmetrise(a1_ik, a1_ki) - symmetrise(a2_ik, a2_ki);
        }
        Hp[p] = symmetrise(a_ik, a_ki);
        Tp[p] = a_ik - a_ki;
        Rp[p] = step_diff;
      }
    double asym = 0.0, fd = 0.0;
    for (int i = 0; i < m; ++i)
      for (int k = 0; k <= i; ++k) {
        const int p = i * (i + 1) / 2 + k;
        const double hii = Hp[i * (i + 1) / 2 + i], hkk = Hp[k * (k + 1) / 2 + k];
        if (k < i) asym = max_of(asym, scaled_abs(Tp[p], hii, hkk));
        if (order == 4) fd = max_of(fd, scaled_abs(Rp[p], hii, hkk));
        H[i * m + k] = H[k * m + i] = Hp[p];
      }
    asymmetry[d] = asym;
    fd_error[d] = order == 4 ? fd : NAN;
    for (int i = 0; i < m; ++i) {
      hd[i] = Hp[i * (i + 1) / 2 + i];
      if (!isfinite(hd[i])) not_finite = true;
      else if (!(hd[i] > 0.0)) not_positive = true;
    }
    if (!not_finite && !not_positive) {
      for (int i = 0; i < m; ++i) sc[i] = inv_sqrt(hd[i]);
      for (int i = 0; i < m; ++i)
        for (int k = 0; k <= i; ++k) Hp[i * (i + 1) / 2 + k] = scaled_entry(sc[i], Hp[i * (i + 1) / 2 + k], sc[k], i == k);
      for (int i = 0; i < m && !not_positive; ++i) {
        for (int j = 0; j < i; ++j) Rp[i * (i + 1) / 2 + j] = cholesky_entry(Packed{Rp}, Hp[i * (i + 1) / 2 + j], i, j);
        const double pivot = cholesky_entry(Packed{Rp}, Hp[i * (i + 1) / 2 + i], i, i);
        if (!pivot_ok(pivot, m)) not_positive = true;
        Rp[i * (i + 1) / 2 + i] = sqrt(pivot);
      }
    }
    if (not_finite || not_positive) {
      for (int k = 0; k < m * m; ++k) C[k] = NAN;
      for (int i = 0; i < m; ++i) sd[d * m + i] = NAN;
      logdet[d] = log_evidence[d] = NAN;
      status[d] = not_finite ? kNotFinite : kNotPositive;
      continue;
    }
    for (int i = 0; i < m; ++i)
      for (int k = 0; k <= i; ++k) Tp[i * (i + 1) / 2 + k] = inverse_entry(Packed{Rp}, Packed{Tp}, i, k);
    for (int i = 0; i < m; ++i)
      for (int k = 0; k <= i; ++k) {
        C[i * m + k] = C[k * m + i] = cov_entry(sc[i], sc[k], gram_entry(Packed{Tp}, m, i, k));
        if (k == i) sd[d * m + i] = sqrt(C[i * m + i]);
      }
    logdet[d] = log_det(hd, Packed{Rp}, m);
    log_evidence[d] = laplace::log_evidence(logp[d], m, logdet[d]);
    status[d] = kOk;
  }
  return 0;
}

}  // extern "C"
