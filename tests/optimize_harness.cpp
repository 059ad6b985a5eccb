// Host build of exoplanet_amd/csrc/exo_optimize_core.hpp -- the per-chain arithmetic of the batched L-BFGS -- in double and in
// long double, for tests/test_optimize_host.py and tests/make_optimize_golden.py: ONE call of a phase on the state of one
// chain (history stride 1).  The long double run converts the state, runs the same template and rounds the result to double.
// Compiled on its own (-DOPTIMIZE_HARNESS_MAIN) it is a program that runs both phases on a small state: what an address /
// undefined-behaviour sanitizer build checks.
#define EXO_HOST_BUILD
#include <stdint.h>

#include <vector>

#include "../exoplanet_amd/csrc/exo_optimize_core.hpp"

namespace {

struct State {
  double *x, *g, *xt, *gt, *d, *free, *hs, *hy, *hsy, *coef, *logp, *lpt, *alpha, *gamma, *grad_max;
  int32_t *status, *n_iter, *n_eval, *m, *head, *n_rej, *n_small;
};

template <typename T>
void run(const State& s, int n, int n_hist, int max_linesearch, double c1, double gtol, double ftol, int phase) {
  // the arrays of the state in T, in the order of `sizes`
  double* const src[15] = {s.x, s.g, s.xt, s.gt, s.d, s.free, s.hs, s.hy, s.hsy, s.coef, s.logp, s.lpt, s.alpha, s.gamma, s.grad_max};
  const int sizes[15] = {n, n, n, n, n, n, n_hist * n, n_hist * n, n_hist, n_hist, 1, 1, 1, 1, 1};
  std::vector<std::vector<T>> v(15);
  for (int k = 0; k < 15; ++k) v[k].assign(src[k], src[k] + sizes[k]);
  lbfgs::Chain<T> c;
  c.x = v[0].data(); c.g = v[1].data(); c.xt = v[2].data(); c.gt = v[3].data(); c.d = v[4].data(); c.free = v[5].data();
  c.hs = v[6].data(); c.hy = v[7].data(); c.hsy = v[8].data(); c.coef = v[9].data();
  c.stride = 1;
  c.logp = v[10].data(); c.lpt = v[11].data(); c.alpha = v[12].data(); c.gamma = v[13].data(); c.grad_max = v[14].data();
  c.status = s.status; c.n_iter = s.n_iter; c.n_eval = s.n_eval; c.m = s.m; c.head = s.head; c.n_rej = s.n_rej; c.n_small = s.n_small;
  const lbfgs::Rules<T> r{n, n_hist, max_linesearch, (T)c1, (T)gtol, (T)ftol};
  if (phase == 0) lbfgs::start(c, r);
  else lbfgs::decide(c, r);
  for (int k = 0; k < 15; ++k)
    for (int i = 0; i < sizes[k]; ++i) src[k][i] = (double)v[k][i];
}

}  // namespace

extern "C" {

int harness_max_history() { return lbfgs::kMaxHistory; }

void harness_phase(int long_double, double* x, double* g, double* xt, double* gt, double* d, double* free, double* hs, double* hy,
                   double* hsy, double* coef, double* logp, double* lpt, double* alpha, double* gamma, double* grad_max,
                   int32_t* status, int32_t* n_iter, int32_t* n_eval, int32_t* m, int32_t* head, int32_t* n_rej, int32_t* n_small,
                   int n, int n_hist, int max_linesearch, double c1, double gtol, double ftol, int phase) {
  const State s{x, g, xt, gt, d, free, hs, hy, hsy, coef, logp, lpt, alpha, gamma, grad_max, status, n_iter, n_eval, m, head, n_rej,
                n_small};
  if (long_double) run<long double>(s, n, n_hist, max_linesearch, c1, gtol, ftol, phase);
  else run<double>(s, n, n_hist, max_linesearch, c1, gtol, ftol, phase);
}

}  // extern "C"

#ifdef OPTIMIZE_HARNESS_MAIN
#include <stdio.h>

// f = sum_i w_i x_i^2 / 2 from a fixed start, evaluated here: phase 0, then phase 1 until the chain stops -- every array at
// its exact size, so that an access outside one is seen
int main() {
  const int n = 5, H = 3;
  for (int long_double = 0; long_double < 2; ++long_double) {
    std::vector<double> x(n), g(n), xt(n), gt(n), d(n), free(n, 1.0), hs(H * n), hy(H * n), hsy(H), coef(H);
    double logp = 0, lpt = 0, alpha = 0, gamma = 0, grad_max = 0;
    int32_t status = 0, n_iter = 0, n_eval = 0, m = 0, head = 0, n_rej = 0, n_small = 0;
    free[3] = 0.0;
    for (int i = 0; i < n; ++i) x[i] = xt[i] = 1.0 + 0.5 * i;
    for (int tick = 0; tick < 200 && status == 0; ++tick) {
      lpt = 0.0;
      for (int i = 0; i < n; ++i) {
        const double w = 1.0 + 30.0 * i;
        lpt -= 0.5 * w * xt[i] * xt[i];
        gt[i] = -w * xt[i];
      }
      harness_phase(long_double, x.data(), g.data(), xt.data(), gt.data(), d.data(), free.data(), hs.data(), hy.data(), hsy.data(),
                    coef.data(), &logp, &lpt, &alpha, &gamma, &grad_max, &status, &n_iter, &n_eval, &m, &head, &n_rej, &n_small,
                    n, H, 20, 1e-4, 1e-5, 2.220446049250313e-09, tick == 0 ? 0 : 1);
    }
    printf("%s: status %d after %d evaluations, logp %.6g, x[3] %.3g\n", long_double ? "long double" : "double", status, n_eval,
           logp, x[3]);
    if ((status != 1 && status != 2) || x[3] != 2.5) return 1;
  }
  return 0;
}
#endif
