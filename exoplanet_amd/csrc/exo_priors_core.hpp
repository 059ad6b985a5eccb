// exo_priors_core.hpp -- the arithmetic of one block of a ParameterSpace (exoplanet_amd/distributions.py): unconstrained
// coordinates -> constrained values and the block's share of the log prior (log-Jacobians included), and the reverse of
// that map.  Definitions: include/exoplanet_amd.h (the table above exo_prior_transform_f64) and DESIGN.md section 10.
// Compiles for the device (exo_priors.hip) and, with EXO_HOST_BUILD, with a host compiler alone
// (tests/priors_harness.cpp holds it to the multiprecision fixture without a GPU).
//
// Numerics: s(z), s(-z), log s(z) and log s(-z) all come from ONE exp(-|z|) and ONE log1p of it, each with full relative
// precision on both sides of zero; no log is taken of a rounded s(z) where the log s form exists, and on a bounded interval
// e and 1 - e are each summed from non-negative parts.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_math.hpp"

#ifdef EXO_HOST_BUILD
#define EXO_PRI_HD inline
#else
#include <hip/hip_runtime.h>
#define EXO_PRI_HD __host__ __device__ __forceinline__
#endif

namespace pri {

constexpr double kHalfLog2Pi = 0.91893853320467274178;    // log(2 pi) / 2
constexpr double kLog2Pi = 1.83787706640934548356;
constexpr double kHalfLog2OverPi = -0.22579135264472743236;  // log(2 / pi) / 2
constexpr double kSqrtHalf = 0.70710678118654752440;

struct Sig {
  double s, sm, ls, lsm;  // s(z), s(-z), log s(z), log s(-z)
};

EXO_PRI_HD Sig sig(double z) {
  const double a = fabs(z), t = exp(-a), d = 1.0 / (1.0 + t), l = log1p(t);
  Sig r;
  if (z >= 0.0) {
    r.s = d; r.sm = t * d; r.ls = -l; r.lsm = -a - l;
  } else {
    r.s = t * d; r.sm = d; r.ls = -a - l; r.lsm = -l;
  }
  return r;
}

EXO_PRI_HD double clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// UNIT_DISK after rounding.  x * x + y * y <= 1 has to hold as the caller evaluates it in fp64, and y has to keep its accuracy
// where 1 - x^2 is tiny.  So x is taken 2^-49 (relative) towards zero -- more than the roundings between exp and x^2 can add up
// to, which leaves y = (s(z2) - s(-z2)) w its room next to |x| = 1 -- and |y| is capped at the largest value that passes the
// caller's test: y^2 <= 1 - fl(x^2) + 2^-54 (the sum then rounds to 1 at most), taken down by the roundings of the difference,
// the root, this product and the caller's square.  Away from |x| = 1 the cap moves y by a few ulp at most.  The square is
// rounded on its own: contracted into an fma the difference would be that of the exact x^2, not of the caller's rounded one.
constexpr double kDiskShrink = 1.0 - 0x1p-49;

EXO_PRI_HD double disk_ymax(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  const double x2 = __dmul_rn(x, x);
#else
  const double x2 = x * x;
#endif
  return sqrt(fmax(1.0 - x2, 0.0) + 0x1p-54) * (1.0 - 0x1p-51);
}

// digamma for x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the asymptotic series (its first
// neglected term, x^-14 / 12, is below 1e-15 there)
EXO_PRI_HD double digamma(double x) {
  double r = 0.0;
  while (x < 10.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double i = 1.0 / x, i2 = i * i;
  const double series = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0))))));
  return r + log(x) - 0.5 * i - series;
}

// log of the normal distribution function, log Phi(x)
EXO_PRI_HD double log_ncdf(double x) { return log(0.5 * erfc(-x * kSqrtHalf)); }

EXO_PRI_HD int n_hyper(int kind) { return kind == EXO_PRIOR_KIPPING13_HYPER ? 2 : kind == EXO_PRIOR_VANEYLEN19_HYPER ? 3 : 0; }
EXO_PRI_HD int n_coord(int kind) { return (kind == EXO_PRIOR_ANGLE || kind == EXO_PRIOR_UNIT_DISK || kind == EXO_PRIOR_QUAD_LIMB_DARK) ? 2 : 1; }
EXO_PRI_HD int n_value(int kind) { return (kind == EXO_PRIOR_UNIT_DISK || kind == EXO_PRIOR_QUAD_LIMB_DARK) ? 2 : 1; }
EXO_PRI_HD int n_free(const exo_prior_block& b) { return n_hyper(b.kind) + b.count * n_coord(b.kind); }
EXO_PRI_HD int n_out(int kind) { return n_value(kind) + n_hyper(kind); }

// ---- the eccentricity priors: one element given the (hyper)parameters ---------------------------------------------------------

struct Ecc {
  double e, de;          // value, de/dz
  double lp, dlp;        // log prior (Jacobian in; the Beta's normalisation out), d/dz
  double da, db;         // d lp / d(first, second shape parameter): Beta alpha, beta; mixture sg, sr
  double wa, wb;         // mixture weights of the two components: d lp / d log(1-f), d lp / d log f
};

// Beta(alpha, beta) on [lo, hi] without its normalising constant
EXO_PRI_HD Ecc kipping_elem(double z, bool bounded, double lo, double hi, double alpha, double beta) {
  const Sig g = sig(z);
  Ecc r;
  r.wa = r.wb = 0.0;
  if (!bounded) {
    r.e = g.s; r.de = g.s * g.sm;
    r.lp = alpha * g.ls + beta * g.lsm;
    r.dlp = alpha * g.sm - beta * g.s;
    r.da = g.ls; r.db = g.lsm;
    return r;
  }
  const double w = hi - lo, e = lo + w * g.s, em = (1.0 - hi) + w * g.sm, J = w * g.s * g.sm;
  const double loge = log(e), log1me = log(em);
  r.e = clamp(e, lo, hi); r.de = J;
  r.lp = (alpha - 1.0) * loge + (beta - 1.0) * log1me + (g.ls + g.lsm);
  r.dlp = (alpha - 1.0) * (e > 0.0 ? J / e : g.sm) - (beta - 1.0) * (em > 0.0 ? J / em : g.s) + (g.sm - g.s);
  r.da = loge; r.db = log1me;
  return r;
}

// the mixture of a half-normal (width sg, weight 1 - f) and a Rayleigh distribution (width sr, weight f); log1mf = log(1 - f), logf = log f
EXO_PRI_HD Ecc vaneylen_elem(double z, double lo, double hi, double sg, double sr, double log1mf, double logf) {
  const Sig g = sig(z);
  const double w = hi - lo, e = lo + w * g.s, J = w * g.s * g.sm;
  const double loge = lo == 0.0 ? log(w) + g.ls : log(e);
  const double Je = lo == 0.0 ? g.sm : J / e;                 // (de/dz) / e
  const double isg2 = 1.0 / (sg * sg), isr2 = 1.0 / (sr * sr);
  const double A = log1mf + kHalfLog2OverPi - log(sg) - 0.5 * e * e * isg2;
  const double B = logf + loge - 2.0 * log(sr) - 0.5 * e * e * isr2;
  const double m = fmax(A, B);
  double lse, wa, wb;
  if (m == -INFINITY) {
    lse = m; wa = wb = 0.5;
  } else {
    const double ea = exp(A - m), eb = exp(B - m), sum = ea + eb;
    lse = m + log(sum); wa = ea / sum; wb = eb / sum;
  }
  Ecc r;
  r.e = clamp(e, lo, hi); r.de = J;
  r.lp = (g.ls + g.lsm) + lse;
  r.dlp = (g.sm - g.s) - wa * e * isg2 * J + wb * (Je - e * isr2 * J);
  r.da = wa * (e * e * isg2 - 1.0) / sg;
  r.db = wb * (e * e * isr2 - 2.0) / sr;
  r.wa = wa; r.wb = wb;
  return r;
}

// a hyperparameter x = exp(z) > 0 under a normal(mu, sd) truncated below at 0: (x, log prior with the log-Jacobian z, d/dz)
struct Hyper {
  double x, dx, lp, dlp;
};

EXO_PRI_HD Hyper positive_hyper(double z, double mu, double sd) {
  Hyper h;
  h.x = exp(z); h.dx = h.x;
  const double u = (h.x - mu) / sd;
  h.lp = -0.5 * u * u - log(sd) - kHalfLog2Pi - log_ncdf(mu / sd) + z;
  h.dlp = -u / sd * h.x + 1.0;
  return h;
}

// f = s(z) in [0, 1] under a normal(mu, sd) truncated to [0, 1]; g: sig(z)
EXO_PRI_HD Hyper fraction_hyper(const Sig& g, double mu, double sd) {
  Hyper h;
  h.x = g.s; h.dx = g.s * g.sm;
  const double u = (h.x - mu) / sd;
  const double mass = 0.5 * (erfc(-(1.0 - mu) / sd * kSqrtHalf) - erfc(mu / sd * kSqrtHalf));
  h.lp = -0.5 * u * u - log(sd) - kHalfLog2Pi - log(mass) + (g.ls + g.lsm);
  h.dlp = -u / sd * h.dx + (g.sm - g.s);
  return h;
}

// ---- one element of a block without hyperparameters -----------------------------------------------------------------------------

struct Elem {
  double v0, v1;              // the value(s)
  double d00, d01, d10, d11;  // dIJ = d v_I / d z_J
  double lp, l0, l1;          // log prior and d/dz
  double dr;                  // d v0 / d ror (IMPACT_PARAMETER)
};

EXO_PRI_HD Elem elem(int kind, int flags, const double* p, double z0, double z1, double ror) {
  Elem e;
  e.v0 = e.v1 = e.d00 = e.d01 = e.d10 = e.d11 = e.lp = e.l0 = e.l1 = e.dr = 0.0;
  switch (kind) {
    case EXO_PRIOR_NORMAL:
    case EXO_PRIOR_LOGNORMAL: {
      const double u = (z0 - p[0]) / p[1];
      e.v0 = kind == EXO_PRIOR_NORMAL ? z0 : exp(z0);
      e.d00 = kind == EXO_PRIOR_NORMAL ? 1.0 : e.v0;
      e.lp = -0.5 * u * u - log(p[1]) - kHalfLog2Pi;
      e.l0 = -u / p[1];
      break;
    }
    case EXO_PRIOR_UNIFORM: {
      const Sig g = sig(z0);
      const double w = p[1] - p[0];
      e.v0 = clamp(p[0] + w * g.s, p[0], p[1]);
      e.d00 = w * g.s * g.sm;
      e.lp = g.ls + g.lsm;
      e.l0 = g.sm - g.s;
      break;
    }
    case EXO_PRIOR_ANGLE: {
      const double r2 = z0 * z0 + z1 * z1, ir2 = r2 > 0.0 ? 1.0 / r2 : 0.0;
      e.v0 = atan2(z0, z1);
      e.d00 = z1 * ir2;
      e.d01 = -z0 * ir2;
      e.lp = -0.5 * r2 - kLog2Pi;
      e.l0 = -z0;
      e.l1 = -z1;
      if (flags & 1) {
        e.lp += p[0] * log(r2);
        e.l0 += 2.0 * p[0] * z0 * ir2;
        e.l1 += 2.0 * p[0] * z1 * ir2;
      }
      break;
    }
    case EXO_PRIOR_UNIT_DISK: {
      const Sig a = sig(z0), b = sig(z1);
      const double w = 2.0 * sqrt(a.s * a.sm), t = b.s - b.sm, La = a.ls + a.lsm;
      e.v0 = (a.s - a.sm) * kDiskShrink;
      e.v1 = clamp(t * w, -disk_ymax(e.v0), disk_ymax(e.v0));
      e.d00 = 2.0 * a.s * a.sm;
      e.d10 = e.v1 * 0.5 * (a.sm - a.s);
      e.d11 = w * 2.0 * b.s * b.sm;
      e.lp = La + (b.ls + b.lsm) + (exo::kLn2 + 0.5 * La);
      e.l0 = 1.5 * (a.sm - a.s);
      e.l1 = b.sm - b.s;
      break;
    }
    case EXO_PRIOR_QUAD_LIMB_DARK: {
      const Sig a = sig(z0), b = sig(z1);
      const double sq = sqrt(a.s);
      e.v0 = 2.0 * sq * b.s;
      e.v1 = clamp(sq * (b.sm - b.s), -0.5 * e.v0, 1.0 - e.v0);   // the triangle's edges u1 + 2 u2 >= 0, u1 + u2 <= 1, after rounding
      e.d00 = e.v0 * 0.5 * a.sm;
      e.d10 = e.v1 * 0.5 * a.sm;
      e.d01 = 2.0 * sq * b.s * b.sm;
      e.d11 = -e.d01;
      e.lp = (a.ls + a.lsm) + (b.ls + b.lsm);
      e.l0 = a.sm - a.s;
      e.l1 = b.sm - b.s;
      break;
    }
    case EXO_PRIOR_IMPACT_PARAMETER: {
      const Sig g = sig(z0);
      e.v0 = g.s * (1.0 + ror);
      e.d00 = (1.0 + ror) * g.s * g.sm;
      e.dr = g.s;
      e.lp = g.ls + g.lsm;
      e.l0 = g.sm - g.s;
      break;
    }
    case EXO_PRIOR_KIPPING13: {
      const Ecc r = kipping_elem(z0, flags & 1, p[2], p[3], p[0], p[1]);
      e.v0 = r.e; e.d00 = r.de; e.lp = r.lp + p[4]; e.l0 = r.dlp;
      break;
    }
    case EXO_PRIOR_VANEYLEN19: {
      const Ecc r = vaneylen_elem(z0, p[3], p[4], p[0], p[1], log1p(-p[2]), log(p[2]));
      e.v0 = r.e; e.d00 = r.de; e.lp = r.lp; e.l0 = r.dlp;
      break;
    }
    default:
      break;
  }
  return e;
}

// the value of element j of the block an IMPACT_PARAMETER block is linked to (one coordinate per element), and d/dz of it
EXO_PRI_HD double link_value(const exo_prior_block& lb, const double* zrow, int j, double* dr_dz) {
  const Elem e = elem(lb.kind, lb.flags, lb.p, zrow[lb.offset + (lb.count == 1 ? 0 : j)], 0.0, 0.0);
  *dr_dz = e.d00;
  return e.v0;
}

// ---- a block of one chain: forward ------------------------------------------------------------------------------------------------
// zrow: the chain's row of z; out: the output pointer list; returns the block's share of the chain's log prior
EXO_PRI_HD double block_fwd(const exo_prior_block& b, const exo_prior_block* table, const double* zrow, double* const* out,
                            int64_t chain) {
  const double* z = zrow + b.offset;
  const int n = b.count;
  double lp = 0.0;
  if (b.kind == EXO_PRIOR_KIPPING13_HYPER) {
    const Hyper ha = positive_hyper(z[0], b.p[0], b.p[1]), hb = positive_hyper(z[1], b.p[2], b.p[3]);
    const double logB = lgamma(ha.x) + lgamma(hb.x) - lgamma(ha.x + hb.x);
    for (int j = 0; j < n; ++j) {
      const Ecc r = kipping_elem(z[2 + j], false, 0.0, 1.0, ha.x, hb.x);
      out[b.out][chain * n + j] = r.e;
      lp += r.lp - logB;
    }
    out[b.out + 1][chain] = ha.x;
    out[b.out + 2][chain] = hb.x;
    return lp + ha.lp + hb.lp;
  }
  if (b.kind == EXO_PRIOR_VANEYLEN19_HYPER) {
    const Hyper hg = positive_hyper(z[0], b.p[0], b.p[1]), hr = positive_hyper(z[1], b.p[2], b.p[3]);
    const Sig gf = sig(z[2]);
    const Hyper hf = fraction_hyper(gf, b.p[4], b.p[5]);
    for (int j = 0; j < n; ++j) {
      const Ecc r = vaneylen_elem(z[3 + j], b.p[6], b.p[7], hg.x, hr.x, gf.lsm, gf.ls);
      out[b.out][chain * n + j] = r.e;
      lp += r.lp;
    }
    out[b.out + 1][chain] = hg.x;
    out[b.out + 2][chain] = hr.x;
    out[b.out + 3][chain] = hf.x;
    return lp + hg.lp + hr.lp + hf.lp;
  }
  const bool two = n_coord(b.kind) == 2, pair = n_value(b.kind) == 2;
  for (int j = 0; j < n; ++j) {
    double ror = b.p[0], unused;
    if (b.kind == EXO_PRIOR_IMPACT_PARAMETER && b.link >= 0) ror = link_value(table[b.link], zrow, j, &unused);
    const Elem e = elem(b.kind, b.flags, b.p, z[j], two ? z[n + j] : 0.0, ror);
    out[b.out][chain * n + j] = e.v0;
    if (pair) out[b.out + 1][chain * n + j] = e.v1;
    lp += e.lp;
  }
  return lp;
}

// ---- a block of one chain: reverse ------------------------------------------------------------------------------------------------
// gout: the cotangents of the outputs (a null entry: zero); glp: the cotangent of the chain's log prior; gzrow: the chain's row of
// gz.  The block's own coordinates are WRITTEN; db/dror of a linked IMPACT_PARAMETER block is ADDED to the coordinates of the
// block it is linked to, which lies earlier in the table and has therefore been written already, by this lane.
EXO_PRI_HD double cot(const double* const* gout, int at, int64_t i) { return gout[at] ? gout[at][i] : 0.0; }

EXO_PRI_HD void block_vjp(const exo_prior_block& b, const exo_prior_block* table, const double* zrow, const double* const* gout,
                          double glp, int64_t chain, double* gzrow) {
  const double* z = zrow + b.offset;
  double* gz = gzrow + b.offset;
  const int n = b.count;
  if (b.kind == EXO_PRIOR_KIPPING13_HYPER) {
    const Hyper ha = positive_hyper(z[0], b.p[0], b.p[1]), hb = positive_hyper(z[1], b.p[2], b.p[3]);
    const double psab = digamma(ha.x + hb.x), dBa = digamma(ha.x) - psab, dBb = digamma(hb.x) - psab;   // d log B / d alpha, d beta
    double da = 0.0, db = 0.0;
    for (int j = 0; j < n; ++j) {
      const Ecc r = kipping_elem(z[2 + j], false, 0.0, 1.0, ha.x, hb.x);
      gz[2 + j] = glp * r.dlp + cot(gout, b.out, chain * n + j) * r.de;
      da += r.da - dBa;
      db += r.db - dBb;
    }
    gz[0] = glp * (da * ha.dx + ha.dlp) + cot(gout, b.out + 1, chain) * ha.dx;
    gz[1] = glp * (db * hb.dx + hb.dlp) + cot(gout, b.out + 2, chain) * hb.dx;
    return;
  }
  if (b.kind == EXO_PRIOR_VANEYLEN19_HYPER) {
    const Hyper hg = positive_hyper(z[0], b.p[0], b.p[1]), hr = positive_hyper(z[1], b.p[2], b.p[3]);
    const Sig gf = sig(z[2]);
    const Hyper hf = fraction_hyper(gf, b.p[4], b.p[5]);
    double dg = 0.0, dr = 0.0, df = 0.0;
    for (int j = 0; j < n; ++j) {
      const Ecc r = vaneylen_elem(z[3 + j], b.p[6], b.p[7], hg.x, hr.x, gf.lsm, gf.ls);
      gz[3 + j] = glp * r.dlp + cot(gout, b.out, chain * n + j) * r.de;
      dg += r.da;
      dr += r.db;
      df += r.wb * gf.sm - r.wa * gf.s;          // through log f = log s(zf) and log(1 - f) = log s(-zf)
    }
    gz[0] = glp * (dg * hg.dx + hg.dlp) + cot(gout, b.out + 1, chain) * hg.dx;
    gz[1] = glp * (dr * hr.dx + hr.dlp) + cot(gout, b.out + 2, chain) * hr.dx;
    gz[2] = glp * (df + hf.dlp) + cot(gout, b.out + 3, chain) * hf.dx;
    return;
  }
  const bool two = n_coord(b.kind) == 2, pair = n_value(b.kind) == 2;
  for (int j = 0; j < n; ++j) {
    const bool linked = b.kind == EXO_PRIOR_IMPACT_PARAMETER && b.link >= 0;
    double ror = b.p[0], dr_dz = 0.0;
    if (linked) ror = link_value(table[b.link], zrow, j, &dr_dz);
    const Elem e = elem(b.kind, b.flags, b.p, z[j], two ? z[n + j] : 0.0, ror);
    const double g0 = cot(gout, b.out, chain * n + j), g1 = pair ? cot(gout, b.out + 1, chain * n + j) : 0.0;
    gz[j] = glp * e.l0 + g0 * e.d00 + g1 * e.d10;
    if (two) gz[n + j] = glp * e.l1 + g0 * e.d01 + g1 * e.d11;
    if (linked) {
      const exo_prior_block& lb = table[b.link];
      gzrow[lb.offset + (lb.count == 1 ? 0 : j)] += g0 * e.dr * dr_dz;
    }
  }
}

// the whole table of one chain
EXO_PRI_HD double chain_fwd(const exo_prior_block* table, int n_block, const double* zrow, double* const* out, int64_t chain) {
  double lp = 0.0;
  for (int k = 0; k < n_block; ++k) lp += block_fwd(table[k], table, zrow, out, chain);
  return lp;
}

EXO_PRI_HD void chain_vjp(const exo_prior_block* table, int n_block, int n_free_total, const double* zrow,
                          const double* const* gout, double glp, int64_t chain, double* gzrow) {
  int at = 0;   // the blocks come in the order of their coordinates (checked on the host): what lies between them is zero
  for (int k = 0; k < n_block; ++k) {
    for (; at < table[k].offset; ++at) gzrow[at] = 0.0;
    block_vjp(table[k], table, zrow, gout, glp, chain, gzrow);
    at = table[k].offset + n_free(table[k]);
  }
  for (; at < n_free_total; ++at) gzrow[at] = 0.0;
}

// ---- the argument checks of the two entry points (host) ------------------------------------------------------------------------
// returns the number of output pointers the table needs, or -1
inline int check_table(const exo_prior_block* table, int32_t n_block, int32_t n_free_total) {
  if (!table || n_block < 1 || n_block > EXO_PRIOR_MAX_BLOCKS || n_free_total < 1) return -1;
  int at = 0, n_outputs = 0;
  for (int k = 0; k < n_block; ++k) {
    const exo_prior_block& b = table[k];
    if (b.kind < 0 || b.kind >= EXO_PRIOR_N_KINDS || b.count < 1 || b.offset < at || b.count > n_free_total) return -1;
    // (64-bit: offset and count are the caller's, and their sum must not wrap before it is compared)
    const int64_t end = (int64_t)b.offset + n_hyper(b.kind) + (int64_t)b.count * n_coord(b.kind);
    if (end > (int64_t)n_free_total) return -1;
    at = (int)end;
    if (b.out < 0 || (int64_t)b.out + n_out(b.kind) > EXO_PRIOR_MAX_OUTPUTS) return -1;
    n_outputs = n_outputs > b.out + n_out(b.kind) ? n_outputs : b.out + n_out(b.kind);
    if (b.kind == EXO_PRIOR_IMPACT_PARAMETER && b.link >= 0) {
      if (b.link >= k) return -1;
      const exo_prior_block& lb = table[b.link];
      if (lb.kind != EXO_PRIOR_NORMAL && lb.kind != EXO_PRIOR_LOGNORMAL && lb.kind != EXO_PRIOR_UNIFORM) return -1;
      if (lb.count != 1 && lb.count != b.count) return -1;
    }
  }
  return n_outputs;
}

}  // namespace pri
