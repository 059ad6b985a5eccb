// exo_rv_like_core.hpp -- the per-epoch arithmetic of the radial-velocity likelihood (exo_rv_like.hip): the model of one epoch,
// what that epoch adds to the value and to the gradients of the trend, the zero points and the jitters, and the constants that
// fix the order of summation.  Compiled for gfx950 by exo_rv_like.hip and for the host by tests/rv_like_harness.cpp
// (EXO_HOST_BUILD), which walks a draw in the kernel's order, so that the same lines are held to the multiprecision fixture
// (tests/golden/rv_like_mp.npz) on a machine without a GPU.  The Keplerian part is exo_rv_core.hpp's rv_sample / rv_vjp_term.
// Definitions: include/exoplanet_amd.h, exo_rv_loglike_vjp_f64.
#pragma once
#include "../../include/exoplanet_amd.h"
#include "exo_draw_block.hpp"
#include "exo_math.hpp"
#include "exo_rv_core.hpp"

namespace exo {
namespace rvl {

using draw::block_threads;
using draw::kNarrow;
using draw::kNarrowCad;
using draw::kWave;
using draw::kWide;
#ifndef EXO_HOST_BUILD
using draw::wave_sum;
#endif

constexpr int kTile = 1024;       // epochs whose rho is kept (LDS) between the two passes

// slots of the per-draw reduction: the two halves of the value, then the gradients
constexpr int kChi = 0, kLog = 1, kTrend = 2, kOff = kTrend + EXO_RV_MAX_TREND, kJit = kOff + EXO_RV_MAX_INST,
              kScalars = kJit + EXO_RV_MAX_INST;

struct Acc {
  double v[kScalars];
};

EXO_HD void acc_zero(Acc& a) {
#pragma unroll
  for (int k = 0; k < kScalars; ++k) a.v[k] = 0.0;
}

// m of one epoch: the planets in turn, the trend by increasing power, the zero point
EXO_HD double model(double t, double tau, const double* __restrict__ recs, int n_planet, const double* __restrict__ trend,
                    int n_trend, double offset) {
  double m = 0.0;
  for (int p = 0; p < n_planet; ++p) {
    const double* __restrict__ rec = recs + p * EXO_RV_NPAR;
    m += rec[EXO_RV_AMP] * rv_sample(t, rec).g;
  }
  double pw = 1.0;
#pragma unroll
  for (int k = 0; k < EXO_RV_MAX_TREND; ++k) {
    if (k < n_trend) m += trend[k] * pw;
    pw *= tau;
  }
  return m + offset;
}

// what one epoch adds; returns rho.  `inst` outside [0, EXO_RV_MAX_INST) adds to no instrument (the caller has made rho NaN)
EXO_HD double epoch_add(Acc& a, double rv, double m, double s2, double tau, int n_trend, int inst) {
  const double w = 1.0 / s2, r = rv - m, rho = w * r;
  a.v[kChi] += rho * r;
  a.v[kLog] += log(s2);
  double pw = 1.0;
#pragma unroll
  for (int k = 0; k < EXO_RV_MAX_TREND; ++k) {
    if (k < n_trend) a.v[kTrend + k] += rho * pw;
    pw *= tau;
  }
  const double j = rho * rho - w;
#pragma unroll
  for (int i = 0; i < EXO_RV_MAX_INST; ++i) {   // (a select per instrument: no indexed register, an empty instrument adds 0.0)
    a.v[kOff + i] += inst == i ? rho : 0.0;
    a.v[kJit + i] += inst == i ? j : 0.0;
  }
  return rho;
}

EXO_HD double loglike_from(double chi, double lg, int64_t n_cad) {
  return -0.5 * (chi + lg) - 0.5 * (double)n_cad * 1.8378770664093454836;   // log(2 pi)
}

}  // namespace rvl
}  // namespace exo
