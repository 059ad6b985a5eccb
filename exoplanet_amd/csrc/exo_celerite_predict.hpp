// exo_celerite_predict.hpp -- the predictive variance of a celerite GP at sorted query times, one lane per draw:
// the Kalman filter the factorisation already is (exo_celerite.hip, "Time-parallel path"), followed by the matching
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
  const double* EXO_RESTRICT dg = diag + (n_diag == 1 ? 0 : cf.at(draw) * n);
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
  Sym<J> B;
#pragma unroll
  for (int k = 0; k < J * (J + 1) / 2; ++k) B.v[k] = 0.0;
  auto query_bwd = [&](int64_t q, bool have, double tb) {
    const double* EXO_RESTRICT o = wk + (n + q) * row;
    double r[J];
#pragma unroll
    for (int j = 0; j < J; ++j) r[j] = have ? o[(j + 1) * n_draw] * exp(-co.k[j].c * (tb - tq[q])) : 0.0;
    double quad = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < J; ++l) s = fma(B(j, l), r[l], s);
      quad = fma(r[j], s, quad);
    }
    out[q] = ok ? o[0] - quad : __builtin_nan("");
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
        for (int l = j; l < J; ++l) B(j, l) *= phb.v[j] * phb.v[l];
    }
    co.uv(ti, U, V);
    const double* EXO_RESTRICT o = wk + i * row;
    const double id = o[0];
#pragma unroll
    for (int j = 0; j < J; ++j) W[j] = o[(j + 1) * n_draw];
    double y[J], s = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < J; ++l) v = fma(B(j, l), W[l], v);
      y[j] = v;
      s = fma(W[j], v, s);
    }
    s += id;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int l = j; l < J; ++l) B(j, l) = fma(s * U[j], U[l], B(j, l) - fma(U[j], y[l], y[j] * U[l]));
  }
#pragma unroll 1
  for (; q >= 0; --q) query_bwd(q, true, t[0]);
}

}  // namespace gp
