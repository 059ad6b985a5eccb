// exo_optimize_core.hpp -- the per-chain arithmetic of the batched L-BFGS (exoplanet_amd/optimize.py: LBFGS -- the torch
// statement there is the definition): what one chain does after an evaluation of f = -logp at its
// trial point.  Compiled for the device (exo_optimize.hip: one thread per chain) and for the host
// (tests/optimize_harness.cpp, with EXO_HOST_BUILD), templated on the scalar type: the host build in long double is what
// tests/golden/lbfgs_phase.npz holds.
//
// A chain's rows of the trajectory arrays are contiguous ([n]); its history is strided -- element i of pair k at
// hs[(k * n + i) * stride], the per-pair scalars at [k * stride] -- so that on the device, where stride is the number of
// chains, the lanes of a wave read consecutive addresses.  The two-loop recursion keeps its per-pair coefficients in the
// workspace row `coef` and its vector in `d`: no per-thread array, whatever n and the history length.
// Every sum runs over i = 0 .. n - 1 in turn, written without fused multiply-adds (both builds compile with contraction
// off): the double build on the host and the kernel do the same IEEE operations in the same order.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef EXO_HOST_BUILD
#define EXO_OPT_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_OPT_HD __device__ __forceinline__
#endif

namespace lbfgs {

constexpr int kMaxHistory = 32;      // EXO_LBFGS_MAX_HISTORY of include/exoplanet_amd.h
enum Status : int32_t { kRunning = 0, kGradient = 1, kValue = 2, kLineSearch = 3, kBadStart = 4 };

template <typename T>
struct Chain {
  // trajectory, [n] each: position, gradient of f there (masked), trial point, direction
  T *x, *g, *xt, *d;
  T* gt;               // [n] in: gradient of logp at xt as evaluated; out: gradient of f there, masked
  const T* free;       // [n] 0 / 1: a column with 0 never moves
  // history of the chain (strided, see above): pairs s, y [n_hist][n]; s.y [n_hist]; workspace [n_hist]
  T *hs, *hy, *hsy, *coef;
  int64_t stride;
  // scalars of the chain
  T* logp;             // -f at x
  const T* lpt;        // logp at xt as evaluated
  T *alpha, *gamma, *grad_max;
  int32_t *status, *n_iter, *n_eval, *m, *head, *n_rej;
  int32_t* n_small;    // accepted steps in a row, up to now, whose decrease was below ftol
};

template <typename T>
struct Rules {
  int n, n_hist, max_linesearch;
  T c1, gtol, ftol;
};

template <typename T>
EXO_OPT_HD T abs_of(T v) { return v < T(0) ? -v : v; }
template <typename T>
EXO_OPT_HD T max_of(T a, T b) { return a > b ? a : b; }
template <typename T>
EXO_OPT_HD bool finite(T v) { return v - v == T(0); }          // (inf - inf and NaN - NaN are NaN)

constexpr double kCurvatureEps = 2.220446049250313e-16;        // a pair with s.y <= eps y.y is not stored (scipy's rule)

// gt <- -(gradient of logp) * free; (largest |.|, sum of |.|, all finite) of the result
template <typename T>
EXO_OPT_HD bool mask_gradient(const Chain<T>& c, int n, T* gmax, T* gsum) {
  bool ok = true;
  T mx = T(0), sm = T(0);
  for (int i = 0; i < n; ++i) {
    const T v = c.free[i] != T(0) ? -c.gt[i] * c.free[i] : T(0);
    c.gt[i] = v;
    ok = ok && finite(v);
    mx = max_of(mx, abs_of(v));
    sm += abs_of(v);
  }
  *gmax = mx;
  *gsum = sm;
  return ok;
}

// steepest descent from the gradient in g: d = -g, the first step min(1, 1 / sum |g|)
template <typename T>
EXO_OPT_HD void steepest(const Chain<T>& c, int n, T gsum) {
  for (int i = 0; i < n; ++i) c.d[i] = -c.g[i];
  *c.alpha = gsum > T(1) ? T(1) / gsum : T(1);
}

template <typename T>
EXO_OPT_HD void trial_point(const Chain<T>& c, int n) {
  const T a = *c.alpha;
  for (int i = 0; i < n; ++i) c.xt[i] = c.x[i] + a * c.d[i];
}
template <typename T>
EXO_OPT_HD void stay(const Chain<T>& c, int n) {                // a chain that has stopped is evaluated at its own x
  for (int i = 0; i < n; ++i) c.xt[i] = c.x[i];
}

// d = -H g by the two-loop recursion over the *c.m newest pairs (newest first: slots head - 1, head - 2, ... mod n_hist),
// first scaling per column; returns d.g
template <typename T>
EXO_OPT_HD T two_loop(const Chain<T>& c, const Rules<T>& r) {
  const int n = r.n, H = r.n_hist, m = *c.m, head = *c.head;
  const int64_t st = c.stride;
  for (int i = 0; i < n; ++i) c.d[i] = c.g[i];
  for (int j = 0; j < m; ++j) {
    const int k = (head - 1 - j + 2 * H) % H;
    const T* s = c.hs + (int64_t)k * n * st;
    const T* y = c.hy + (int64_t)k * n * st;
    T sq = T(0);
    for (int i = 0; i < n; ++i) sq += s[i * st] * c.d[i];
    const T a = sq / c.hsy[k * st];
    c.coef[j * st] = a;
    for (int i = 0; i < n; ++i) c.d[i] -= a * y[i * st];
  }
  // the first scaling, per column: the diagonal that fits the stored pairs, sum_k s_i y_i / sum_k y_i^2 (exact for a separable
  // quadratic, and what brings columns of very different widths to one scale); gamma of the newest pair where that is not positive
  const T gamma = *c.gamma;
  for (int i = 0; i < n; ++i) {
    T num = T(0), den = T(0);
    for (int j = 0; j < m; ++j) {
      const int64_t at = ((int64_t)((head - 1 - j + 2 * H) % H) * n + i) * st;
      num += c.hs[at] * c.hy[at];
      den += c.hy[at] * c.hy[at];
    }
    c.d[i] *= (num > T(0) && den > T(0)) ? num / den : gamma;
  }
  for (int j = m - 1; j >= 0; --j) {
    const int k = (head - 1 - j + 2 * H) % H;
    const T* s = c.hs + (int64_t)k * n * st;
    const T* y = c.hy + (int64_t)k * n * st;
    T yr = T(0);
    for (int i = 0; i < n; ++i) yr += y[i * st] * c.d[i];
    const T w = c.coef[j * st] - yr / c.hsy[k * st];
    for (int i = 0; i < n; ++i) c.d[i] += w * s[i * st];
  }
  T dg = T(0);
  for (int i = 0; i < n; ++i) {
    c.d[i] = -c.d[i];
    dg += c.d[i] * c.g[i];
  }
  return dg;
}

// phase 0: after the evaluation at the starting point (xt == x)
template <typename T>
EXO_OPT_HD void start(const Chain<T>& c, const Rules<T>& r) {
  const int n = r.n;
  T gmax, gsum;
  const bool ok = mask_gradient(c, n, &gmax, &gsum) && finite(*c.lpt);
  for (int i = 0; i < n; ++i) {
    c.g[i] = c.gt[i];
    c.d[i] = T(0);
  }
  *c.logp = *c.lpt;
  *c.grad_max = gmax;
  *c.alpha = T(0);
  *c.gamma = T(1);
  *c.n_iter = 0; *c.n_eval = 1; *c.m = 0; *c.head = 0; *c.n_rej = 0; *c.n_small = 0;
  if (!ok) { *c.status = kBadStart; return; }
  if (gmax <= r.gtol) { *c.status = kGradient; return; }
  *c.status = kRunning;
  steepest(c, n, gsum);
  trial_point(c, n);
}

// phase 1: the decision after the evaluation at the trial point, and the next trial point
template <typename T>
EXO_OPT_HD void decide(const Chain<T>& c, const Rules<T>& r) {
  if (*c.status != kRunning) return;            // (a chain that has stopped rides along: nothing of its state changes)
  const int n = r.n, H = r.n_hist;
  const int64_t st = c.stride;
  *c.n_eval += 1;
  T gmax, gsum;
  const bool ok = mask_gradient(c, n, &gmax, &gsum) && finite(*c.lpt);
  const T f = -*c.logp, ft = -*c.lpt, a = *c.alpha;
  T gd = T(0);
  for (int i = 0; i < n; ++i) gd += c.g[i] * c.d[i];
  if (ok && ft <= f + r.c1 * a * gd) {
    // accept: the pair (s, y) joins the history; if its curvature is not positive it does not, and the history goes
    T sy = T(0), yy = T(0);
    for (int i = 0; i < n; ++i) {
      const T s = c.xt[i] - c.x[i], y = c.gt[i] - c.g[i];
      sy += s * y;
      yy += y * y;
    }
    if (sy > T(kCurvatureEps) * yy) {
      const int k = *c.head;
      for (int i = 0; i < n; ++i) {
        c.hs[((int64_t)k * n + i) * st] = c.xt[i] - c.x[i];
        c.hy[((int64_t)k * n + i) * st] = c.gt[i] - c.g[i];
      }
      c.hsy[k * st] = sy;
      *c.gamma = sy / yy;
      *c.head = (k + 1) % H;
      if (*c.m < H) *c.m += 1;
    } else {
      *c.m = 0;        // f is not convex along the step: the pairs describe another place, and backtracking alone never mends them
    }
    for (int i = 0; i < n; ++i) {
      c.x[i] = c.xt[i];
      c.g[i] = c.gt[i];
    }
    *c.logp = *c.lpt;
    *c.grad_max = gmax;
    *c.n_iter += 1;
    *c.n_rej = 0;
    const T af = abs_of(f), aft = abs_of(ft);
    if (gmax <= r.gtol) { *c.status = kGradient; return; }       // (xt == x already)
    // (one small decrease says little: a step that settles the stiff directions of a badly scaled f decreases it by next to
    // nothing while the gradient along the soft ones is as large as ever.  Status 2 takes a history's worth of small decreases
    // in a row: then every pair the model is built from comes from a step that achieved nothing)
    *c.n_small = f - ft <= r.ftol * max_of(max_of(af, aft), T(1)) ? *c.n_small + 1 : 0;
    if (*c.n_small >= H) { *c.status = kValue; return; }
    if (*c.m > 0 && !(two_loop(c, r) < T(0))) *c.m = 0;          // not a descent direction: the history goes
    if (*c.m > 0) *c.alpha = T(1);
    else steepest(c, n, gsum);
    trial_point(c, n);
    return;
  }
  // reject (a NaN or an infinite value: the trial left the support): half the step; after max_linesearch of them in a
  // row a chain with history drops it and restarts along -g, one without gives up
  *c.n_rej += 1;
  *c.alpha = T(0.5) * a;
  if (*c.n_rej >= r.max_linesearch) {
    if (*c.m == 0) {
      // (a line search that fails right after small decreases has met the rounding of f, not an obstacle)
      *c.status = *c.n_small > 0 ? kValue : kLineSearch;
      stay(c, n);
      return;
    }
    *c.m = 0;
    *c.n_rej = 0;
    T sum = T(0);
    for (int i = 0; i < n; ++i) sum += abs_of(c.g[i]);
    steepest(c, n, sum);
  }
  trial_point(c, n);
}

}  // namespace lbfgs
