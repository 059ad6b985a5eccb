// exo_astrometry_core.hpp -- the per-epoch arithmetic of the astrometric likelihood (exo_astrometry.hip): what one epoch of
// separation and position angle adds to the value, to the cotangent of the orbit's record and to the gradients of the two
// jitters, and the constants that fix the order of summation.  Compiled for gfx950 by exo_astrometry.hip and for the host by
// tests/astrometry_harness.cpp (EXO_HOST_BUILD), which walks a draw in the kernel's order, so that the same lines are held to
// the multiprecision fixture (tests/golden/astrometry_mp.npz) on a machine without a GPU.  The Keplerian part is
// exo_rv_core.hpp's ov_sample<0> / ov_vjp_term<0>.  Definitions: include/exoplanet_amd.h, exo_astrometry_loglike_vjp_f64.
#pragma once
#include "../../include/exoplanet_amd.h"
#include "exo_draw_block.hpp"
#include "exo_math.hpp"
#include "exo_rv_core.hpp"

namespace exo {
namespace ast {

using draw::block_threads;
using draw::kNarrow;
using draw::kNarrowCad;
using draw::kWave;
using draw::kWide;
#ifndef EXO_HOST_BUILD
using draw::wave_sum;
#endif

// slots of the per-draw reduction: the halves of the value, the record's cotangent, the two jitters
constexpr int kChiR = 0, kLogR = 1, kChiT = 2, kLogT = 3, kRec = 4, kJitR = kRec + EXO_OV_NPAR, kJitT = kJitR + 1,
              kSlots = kJitT + 1;

struct Acc {
  double v[kSlots];
};

EXO_HD void acc_zero(Acc& a) {
#pragma unroll
  for (int k = 0; k < kSlots; ++k) a.v[k] = 0.0;
}

// what one epoch adds.  (c, s) = (cos, sin) of the observed position angle; s2r, s2t the two variances, jitters included.
// The angle residual is atan2(Y c - X s, X c + Y s): the model's angle minus the observed one wrapped into (-pi, pi], without
// forming the model's angle.  A separation of exactly zero (no direction, no derivative) is NaN.
template <bool WITH_REC>
EXO_HD void epoch_add(Acc& a, double t, const double* __restrict__ rec, double rho, double c, double s, double s2r, double s2t) {
  const OvSample sm = ov_sample<0>(t, rec);
  const double amp = rec[EXO_OV_AMP];
  const double X = amp * sm.X, Y = amp * sm.Y;
  const double rho2 = X * X + Y * Y;
  const double rho_m = rho2 > 0.0 ? sqrt(rho2) : __builtin_nan("");
  const double delta = atan2(Y * c - X * s, X * c + Y * s);
  const double wr = 1.0 / s2r, r = rho - rho_m, kappa = wr * r;
  const double wt = 1.0 / s2t, lambda = -wt * delta;
  a.v[kChiR] += kappa * r;
  a.v[kLogR] += log(s2r);
  a.v[kChiT] -= lambda * delta;
  a.v[kLogT] += log(s2t);
  a.v[kJitR] += kappa * kappa - wr;
  a.v[kJitT] += lambda * lambda - wt;
  if (WITH_REC) {
    const double irho = 1.0 / rho_m, kr = kappa * irho, lr = lambda * irho * irho;
    ov_vjp_term<0>(t, rec, kr * X - lr * Y, kr * Y + lr * X, 0.0, a.v + kRec);
  }
}

EXO_HD double loglike_from(double chi_r, double log_r, double chi_t, double log_t, int64_t n_cad) {
  return -0.5 * ((chi_r + log_r) + (chi_t + log_t)) - (double)n_cad * 1.8378770664093454836;   // log(2 pi), once per datum
}

}  // namespace ast
}  // namespace exo
