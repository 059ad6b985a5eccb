// exo_celerite_predict.hpp -- the predictive variance of a celerite GP at sorted query times, one lane per draw:
// the Kalman filter the factorisation already is (exo_celerite_lanegroup.hpp, "Time-parallel path"), followed by the matching
// smoother, in O((N + M) J^2) per draw.  Host + device, like exo_celerite_core.hpp, whose Fwd / Phi / DrawCoef it reuses:
// tests/gp_predict_var_harness.cpp runs the same functions with g++ against the dense definition.
//
// With A = K + diag = L diag(d) L^T as Fwd<J> computes it (S_i the state ENTERING cadence i, E(tau) = diag(exp(-c tau))):
//   forward:   d_i = diag_i + sum a - U_i^T S_i U_i,   W_i = (V_i - S_i U_i) / d_i,
//              S+_i = S_i + d_i W_i W_i^T,             S_(i+1) = E(t_(i+1) - t_i) S+_i E(t_(i+1) - t_i)
//   backward:  B_N = 0;  X = E(t_(i+1) - t_i) B_(i+1) E(t_(i+1) - t_i)  (X = 0 at the last cadence)
//              B_i = U_i U_i^T / d_i + (I - W_i U_i^T)^T X (I - W_i U_i^T)
//                  = X - U_i y^T - y U_i^T + (s + 1 / d_i) U_i U_i^T,    y = X W_i,  s = W_i^T y
//   query t* after cadence n (the last one with t_n <= t*, n = -1 if none), U*, V* = uv(t*) with the entries of the state
//   indices outside the predicted component set to zero:
//              S* = E(t* - t_n) S+_n E(t* - t_n)  (0 for n = -1),     r* = V* - S* U*
//              B* = E(t_(n+1) - t*) B_(n+1) E(t_(n+1) - t*)  (0 for n = N - 1)
//              var(t*) = k2(0) - U*^T S* U* - r*^T B* r*
// k2(0): the sum of the amplitudes of the predicted terms; U*^T S* U* is the filter's share, r*^T B* r* the smoother's.
// Neither S* nor B* is formed: with u~ = E(t* - t_n) U*,  U*^T S* U* = u~^T S_n u~ + d_n (W_n . u~)^2  and
// S* U* = E(t* - t_n) (S_n u~ + d_n W_n (W_n . u~)), one pass over the packed S_n.
#pragma once
#include "exo_celerite_core.hpp"

namespace gp {

// The workspace of one call: rows of J + 1 quantities, draws innermost ([row][quantity][draw]: the lanes of a wave store and
// load contiguous rows).  Rows 0 .. n - 1: cadence i -> (1 / d_i, W_i); rows n .. n + m - 1: query q -> (the filter's
// var, r*).  Written by the forward pass, read back by the backward pass of the same lane.
EXO_HDH int64_t predict_var_work_doubles(int64_t n, int64_t m, int J, int64_t n_draw) {
  return (n + m) * (int64_t)(J + 1) * n_draw;
}

// The backward pass carries B in double-double (an unevaluated sum hi + lo of two doubles, ~106 bits).  B holds the information
// of the data after a cadence: its entries reach 1 / d_i (1e4 at diag = 1e-4, 5e11 at a repeated time stamp under diag = 1e-12),
// and the update  X - U y^T - y U^T + s U U^T  as well as the query's  r*^T B r*  are differences of terms of that size whose
// result is of order 1 / k(0): in plain doubles the absolute error eps max |B_i| shows wherever r* is not small -- before the
// first datum, next to a repeated stamp -- at up to 1e-9 k(0).  The inputs (U, W, 1 / d, the
// propagators, r*) stay doubles: with them exact the result is within a few eps of the dense definition.
// The error-free transformations below rely on every product and sum being rounded as written: no contraction into fma
// across them (hipcc's default would fuse  p + e  with the product behind p, and the low word would be lost).
#if defined(__clang__)
#define EXO_DD_EXACT _Pragma("clang fp contract(off)")
#else
#define EXO_DD_EXACT
#endif
struct DD {
  double h, l;
};
EXO_HD DD dd_fast_two_sum(double a, double b) {   // |a| >= |b| or a == 0
  EXO_DD_EXACT
  const double s = a + b;
  return DD{s, b - (s - a)};
}
EXO_HD DD dd_two_sum(double a, double b) {
  EXO_DD_EXACT
  const double s = a + b, bb = s - a;
  return DD{s, (a - (s - bb)) + (b - bb)};
}
EXO_HD DD dd_add(DD a, DD b) {
  EXO_DD_EXACT
  DD s = dd_two_sum(a.h, b.h);
  const DD t = dd_two_sum(a.l, b.l);
  s = dd_fast_two_sum(s.h, s.l + t.h);
  return dd_fast_two_sum(s.h, s.l + t.l);
}
EXO_HD DD dd_sub(DD a, DD b) { return dd_add(a, DD{-b.h, -b.l}); }
EXO_HD DD dd_mul_d(DD a, double b) {
  EXO_DD_EXACT
  const double p = a.h * b;
  return dd_fast_two_sum(p, fma(a.l, b, fma(a.h, b, -p)));
}

// the predicted state indices: slot_mask (nullptr: all) holds one flag per real slot, then one per pair slot
template <int J, int NR>
EXO_HD double predict_keep(const DrawCoef<J, NR>& co, const Coefs& cf, const int32_t* EXO_RESTRICT slot_mask, double* keep) {
  double k0 = 0.0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int slot = j < cf.n_real ? j : cf.n_real + ((j - cf.n_real) >> 1);
    keep[j] = (slot_mask == nullptr || slot_mask[slot] != 0) ? 1.0 : 0.0;
    k0 += (co.is_real(j) || co.is_first(j)) ? keep[j] * co.k[j].a : 0.0;
  }
  return k0;
}

// var[draw][q] for sorted data times t[0 .. n) and sorted query times tq[0 .. m); n >= 1.  A draw whose factorisation
// meets d <= 0 (not positive definite) gets NaN everywhere, as dot_tril does.
template <int J>
EXO_HD void predict_var_lane(const double* EXO_RESTRICT t, const double* EXO_RESTRICT diag, int64_t n_diag, int64_t n,
                             const Coefs& cf, const int32_t* EXO_RESTRICT slot_mask, const double* EXO_RESTRICT tq, int64_t m,
                             double* EXO_RESTRICT var, double* EXO_RESTRICT work, int64_t n_draw, int64_t draw) {
  DrawCoef<J> co;
  co.init(cf, draw);
  const double asum = co.asum();
  double keep[J];
  const double k0 = predict_keep(co, cf, slot_mask, keep);
  const double* EXO_RESTRICT dg = diag_row(diag, n_diag, cf, draw, n);
  double* EXO_RESTRICT wk = work + draw;
  const int64_t row = (int64_t)(J + 1) * n_draw;   // (a row's quantity k: wk[r * row + k * n_draw])
  double Uq[J], Vq[J];
  // the query's U*, V* of the predicted component, its filter share from (S, W, d) of the cadence n before it -- with
  // ph = E(t* - t_n), or no cadence at all (have = false) -- and r* into the workspace
  auto query_fwd = [&](const Fwd<J>& f, const double* ph, bool have, int64_t q) {
    co.uv(tq[q], Uq, Vq);
    double u[J], su[J];
#pragma unroll
    for (int j = 0; j < J; ++j) u[j] = have ? ph[j] * Uq[j] * keep[j] : 0.0;
    double w = 0.0, quad = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) w = fma(f.W[j], u[j], w);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < J; ++l) s = fma(f.S(j, l), u[l], s);
      quad = fma(u[j], s, quad);
      su[j] = have ? ph[j] * fma(f.d * f.W[j], w, s) : 0.0;
    }
    quad = have ? fma(f.d * w, w, quad) : 0.0;
    double* EXO_RESTRICT o = wk + (n + q) * row;
    o[0] = k0 - quad;
#pragma unroll
    for (int j = 0; j < J; ++j) o[(j + 1) * n_draw] = Vq[j] * keep[j] - su[j];
  };
  // forward: the factorisation; every query is met right after the last cadence at or before it
  Fwd<J> f;
#pragma unroll
  for (int j = 0; j < J; ++j) f.F[j] = f.W[j] = f.U[j] = f.V[j] = 0.0;
#pragma unroll
  for (int k = 0; k < J * (J + 1) / 2; ++k) f.S.v[k] = 0.0;
  f.d = 1.0;
  double ph[J];
#pragma unroll
  for (int j = 0; j < J; ++j) ph[j] = 1.0;
  int64_t q = 0;
  bool ok = true;
#pragma unroll 1
  for (; q < m && tq[q] < t[0]; ++q) query_fwd(f, ph, false, q);
  Phi<J> phi;
#pragma unroll 1
  for (int64_t i = 0; i < n; ++i) {
    const double ti = t[i];
    if (i > 0) {
      phi.set(co, ti - t[i - 1]);
      f.advance(phi.v);
    }
    co.uv(ti, f.U, f.V);
    f.measure(0.0, dg[i] + asum);
    ok = ok && f.d > 0.0;
    double* EXO_RESTRICT o = wk + i * row;
    o[0] = f.id;
#pragma unroll
    for (int j = 0; j < J; ++j) o[(j + 1) * n_draw] = f.W[j];
    const double tnext = i + 1 < n ? t[i + 1] : INFINITY;
#pragma unroll 1
    for (; q < m && tq[q] < tnext; ++q) {
#pragma unroll
      for (int j = 0; j < J; ++j) ph[j] = exp(-co.k[j].c * (tq[q] - ti));
      query_fwd(f, ph, true, q);
    }
  }
  // backward: B from the last cadence down; a query after cadence i is finished while B is B_(i+1), at t_(i+1)
  double* EXO_RESTRICT out = var + draw * m;
  Sym<J> Bh, Bl;   // B = Bh + Bl
#pragma unroll
  for (int k = 0; k < J * (J + 1) / 2; ++k) Bh.v[k] = Bl.v[k] = 0.0;
  auto query_bwd = [&](int64_t q, bool have, double tb) {
    const double* EXO_RESTRICT o = wk + (n + q) * row;
    double r[J];
#pragma unroll
    for (int j = 0; j < J; ++j) r[j] = have ? o[(j + 1) * n_draw] * exp(-co.k[j].c * (tb - tq[q])) : 0.0;
    DD res{o[0], 0.0};
#pragma unroll
    for (int j = 0; j < J; ++j) {
      DD s{0.0, 0.0};
#pragma unroll
      for (int l = 0; l < J; ++l) s = dd_add(s, dd_mul_d(DD{Bh(j, l), Bl(j, l)}, r[l]));
      res = dd_sub(res, dd_mul_d(s, r[j]));
    }
    out[q] = ok ? res.h : __builtin_nan("");
  };
  Phi<J> phb;
  double U[J], V[J], W[J];
  q = m - 1;
#pragma unroll 1
  for (int64_t i = n - 1; i >= 0; --i) {
    const double ti = t[i];
#pragma unroll 1
    for (; q >= 0 && tq[q] >= ti; --q) query_bwd(q, i + 1 < n, i + 1 < n ? t[i + 1] : ti);
    if (i + 1 < n) {
      phb.set(co, t[i + 1] - ti);
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int l = j; l < J; ++l) {   // (one factor at a time: each product exact to the double-double's precision)
          const DD x = dd_mul_d(dd_mul_d(DD{Bh(j, l), Bl(j, l)}, phb.v[j]), phb.v[l]);
          Bh(j, l) = x.h;
          Bl(j, l) = x.l;
        }
    }
    co.uv(ti, U, V);
    const double* EXO_RESTRICT o = wk + i * row;
    const double id = o[0];
#pragma unroll
    for (int j = 0; j < J; ++j) W[j] = o[(j + 1) * n_draw];
    DD y[J], s{id, 0.0};
#pragma unroll
    for (int j = 0; j < J; ++j) {
      DD v{0.0, 0.0};
#pragma unroll
      for (int l = 0; l < J; ++l) v = dd_add(v, dd_mul_d(DD{Bh(j, l), Bl(j, l)}, W[l]));
      y[j] = v;
      s = dd_add(s, dd_mul_d(v, W[j]));
    }
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int l = j; l < J; ++l) {
        DD x = dd_mul_d(dd_mul_d(s, U[j]), U[l]);
        x = dd_sub(x, dd_add(dd_mul_d(y[l], U[j]), dd_mul_d(y[j], U[l])));
        x = dd_add(DD{Bh(j, l), Bl(j, l)}, x);
        Bh(j, l) = x.h;
        Bl(j, l) = x.l;
      }
  }
#pragma unroll 1
  for (; q >= 0; --q) query_bwd(q, true, t[0]);
}

// alpha = (K + diag)^-1 y per draw by the published recurrences, one lane per draw, sequential in time: the factorisation with
// the lower sweep beside it (Fwd<J>: z_i = y_i - U_i . F_i), z / d, then the upper sweep
//   G_i = E(t_(i+1) - t_i) (G_(i+1) + U_(i+1) alpha_(i+1)),   alpha_i = z_i / d_i - W_i . G_i.
// The likelihood's reverse pass gives the same vector as a gradient, but its backward error is not that of these sweeps
// (DESIGN.md section 13.3).  work: W_i, n J doubles per draw laid out [cadence][j][draw].  A draw that meets d <= 0: NaN.
EXO_HDH int64_t solve_work_doubles(int64_t n, int J, int64_t n_draw) { return n * (int64_t)J * n_draw; }

template <int J>
EXO_HD void solve_lane(const double* EXO_RESTRICT t, const double* EXO_RESTRICT diag, int64_t n_diag, int64_t n, const Coefs& cf,
                       const double* EXO_RESTRICT y, double* EXO_RESTRICT alpha, double* EXO_RESTRICT work, int64_t n_draw,
                       int64_t draw) {
  DrawCoef<J> co;
  co.init(cf, draw);
  const double asum = co.asum();
  const double* EXO_RESTRICT dg = diag_row(diag, n_diag, cf, draw, n);
  const double* EXO_RESTRICT yr = y + draw * n;
  double* EXO_RESTRICT ar = alpha + draw * n;
  double* EXO_RESTRICT wk = work + draw;
  const int64_t row = (int64_t)J * n_draw;
  Fwd<J> f;
#pragma unroll
  for (int j = 0; j < J; ++j) f.F[j] = f.W[j] = f.U[j] = f.V[j] = 0.0;
#pragma unroll
  for (int k = 0; k < J * (J + 1) / 2; ++k) f.S.v[k] = 0.0;
  f.d = 1.0;
  f.z = 0.0;
  Phi<J> phi;
  bool ok = true;
#pragma unroll 1
  for (int64_t i = 0; i < n; ++i) {
    const double ti = t[i];
    if (i > 0) {
      phi.set(co, ti - t[i - 1]);
      f.advance(phi.v);
    }
    co.uv(ti, f.U, f.V);
    f.measure(yr[i], dg[i] + asum);
    ok = ok && f.d > 0.0;
    ar[i] = f.z * f.id;
    double* EXO_RESTRICT o = wk + i * row;
#pragma unroll
    for (int j = 0; j < J; ++j) o[j * n_draw] = f.W[j];
  }
  double G[J], U[J], V[J];
#pragma unroll
  for (int j = 0; j < J; ++j) G[j] = 0.0;
  Phi<J> phb;
#pragma unroll 1
  for (int64_t i = n - 2; i >= 0; --i) {
    phb.set(co, t[i + 1] - t[i]);
    co.uv(t[i + 1], U, V);
    const double a1 = ar[i + 1];
    const double* EXO_RESTRICT o = wk + i * row;
    double acc = ar[i];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      G[j] = phb.v[j] * fma(U[j], a1, G[j]);
      acc = fma(-o[j * n_draw], G[j], acc);
    }
    ar[i] = acc;
  }
  if (!ok) {
#pragma unroll 1
    for (int64_t i = 0; i < n; ++i) ar[i] = __builtin_nan("");
  }
}

}  // namespace gp
