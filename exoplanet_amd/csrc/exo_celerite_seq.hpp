// exo_celerite_seq.hpp -- the SEQUENTIAL kernels: the parallel pre-pass (U, V, P of every cadence), the forward recurrence
// and its hand-derived reverse, a draw on G lanes, one cadence after the other.  They serve calls without a state buffer,
// short series and the draws the time-parallel path hands back (flagged), and their unflagged lanes do the last step of
// the time-parallel path's sums.
#pragma once
#include "exo_celerite_state.hpp"

namespace {

// Pre-pass, fully parallel over (cadence, draw, state index): everything in the
// recurrences that does not depend on the recurrence itself.  One (cadence, draw, state index):
__device__ __forceinline__ void prep_one(const double* __restrict__ t, const Coefs& cf, const StateIdx& six, int64_t i, int64_t draw,
                                         int j, double* __restrict__ state) {
  const LaneCoef k = lane_coef(cf, draw, j, six.J);
  double U, V, cs, sn;
  const double ti = t[i];
  lane_uv(k, ti, &U, &V, &cs, &sn);
  state[six.uvp(0, i, draw, j)] = U;
  state[six.uvp(1, i, draw, j)] = V;
  state[six.uvp(2, i, draw, j)] = i > 0 ? exp(-k.c * (ti - t[i - 1])) : 1.0;
}
__global__ __launch_bounds__(256) void celerite_prep_kernel(const double* __restrict__ t, int64_t n,
                                                            Coefs cf,
                                                            int64_t n_draw, int J, double* __restrict__ state) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = n_draw * J;
  if (e >= n * per) return;
  const int64_t i = e / per, rem = e - i * per;
  const int64_t draw = rem / J;
  prep_one(t, cf, StateIdx{n, n_draw, J}, i, draw, (int)(rem - draw * J), state);
}

template <int J, bool SAVE>
__global__ __launch_bounds__(kWave) void celerite_fwd_kernel(
    const double* __restrict__ t, Series rs, const double* __restrict__ diag,
    int64_t n_diag, int64_t n, Coefs cf, int64_t n_draw, double* __restrict__ loglike,
    double* __restrict__ state, const double* __restrict__ only_flagged, ChunkGeom cg, int n_slice) {
  constexpr int G = Group<J>::G;
  const auto [j, draw, live_draw] = GroupLane<G>(n_draw);
  // after the time-parallel path: redo only the draws it could not take (see DeltaCoef)
  const bool mine = live_draw && (!only_flagged || only_flagged[draw] >= kFlagSeq);
  if (only_flagged) {
    // ... and every other draw's log-likelihood from the chunks' partial sums (n_slice of them per quantity, in the slots of
    // chunks 0 .. n_slice - 1: celerite_chunk_slice_sum_kernel) -- round 5: this launch is there anyway, a kernel of its own for
    // the sums' last step was 7 us of the step
    if (live_draw && !mine && j == 0) {
      const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
      double acc = 0.0, logdet = 0.0, bad = 0.0;
      for (int q = 0; q < n_slice; ++q) {
        acc += state[ws.part(q, 0, draw)];
        logdet += state[ws.part(q, 1, draw)];
        bad += state[ws.part(q, 2, draw)];
      }
      loglike[cf.at(draw)] = loglike_of(acc, logdet, bad > 0.0, n);
    }
    if (__ballot(mine) == 0) return;
  }
  const LaneCoef k = lane_coef(cf, draw, j, J);
  const bool store = SAVE && mine && k.live;
  // a_n = diag_n + sum of the a coefficients (first index of each term)
  const double asum = group_sum<G>((k.live && !k.odd) ? k.a : 0.0);
  const StateIdx six{n, n_draw, J};
  const SeriesRow y(rs, draw, n);
  const double* __restrict__ dg = diag_row(diag, n_diag, cf, draw, n);

  double Srow[J], Wall[J], Uall[J], Pall[J];
#pragma unroll
  for (int l = 0; l < J; ++l) { Srow[l] = 0.0; Pall[l] = 1.0; }
  double Fj = 0.0, Pj = 1.0, Uj, Vj, cs, sn;
  double tprev = t[0];
  const int jj = k.live ? j : 0;
  if (SAVE) {
    Uj = k.live ? state[six.uvp(0, 0, draw, jj)] : 0.0;
    Vj = k.live ? state[six.uvp(1, 0, draw, jj)] : 0.0;
  } else {
    lane_uv(k, tprev, &Uj, &Vj, &cs, &sn);
  }
  double d = dg[0] + asum;
  double z = y[0];
  bool bad = !(d > 0.0);
  double Wj = Vj / d;
  EXO_GROUP_GATHER(Wj, Wall);
  // sum log d_n = log prod d_n: carry the product as (mantissa, exponent) -- a multiply
  // and a frexp per cadence instead of a ~45-instruction log on the sequential chain
  double acc = z * z / d;
  int lexp;
  double lman = frexp(bad ? 1.0 : d, &lexp);
  int64_t lsum = lexp;
  double dt_prev = -1.0;
  if (store) {
    if (j == 0) *reinterpret_cast<double2*>(state + six.scal(0, 0, draw)) = double2{d, z};
    store_record<J>(state + six.rec(0, draw, j), six.piece(), Wj, 0.0, Srow);   // S_0 = 0
  }
  // software prefetch ring: the loads of cadence i + kPF are issued while cadence i
  // computes (one wave per SIMD and a serial chain: nothing else hides HBM latency)
  const int64_t vstride = n_draw * J;            // one cadence, in doubles, of a per-(draw, j) quantity (U, V, P)
  const int64_t qstride = n * vstride;           // one quantity (U, V, P)
  const int64_t rstride = vstride * (2 + J);     // one cadence of (W, F, S row) records
  double* __restrict__ p_vec = SAVE ? state + six.rec(0, draw, jj) : nullptr;
  double* __restrict__ p_scal = SAVE ? state + six.scal(0, 0, draw) : nullptr;
  const double* __restrict__ p_uvp = SAVE ? state + six.uvp(0, 0, draw, jj) : nullptr;
  constexpr int kPF = 4;
  double ring_t[kPF], ring_y[kPF], ring_g[kPF], ring_U[kPF], ring_V[kPF], ring_P[kPF];
#pragma unroll
  for (int q = 0; q < kPF; ++q) {
    const int64_t ii = 1 + q < n ? 1 + q : n - 1;
    ring_t[q] = t[ii]; ring_y[q] = y[ii]; ring_g[q] = dg[ii];
    if (SAVE) {
      const double* p = p_uvp + ii * vstride;
      ring_U[q] = k.live ? p[0] : 0.0;
      ring_V[q] = k.live ? p[qstride] : 0.0;
      ring_P[q] = k.live ? p[2 * qstride] : 0.0;
    }
  }
  const double* __restrict__ p_pf = SAVE ? p_uvp + (int64_t)kPF * vstride : nullptr;  // cadence i + kPF, i = 0
  for (int64_t i0 = 1; i0 < n; i0 += kPF) {
#pragma unroll
   for (int q = 0; q < kPF; ++q) {
    const int64_t i = i0 + q;
    if (i >= n) break;
    const double ti = ring_t[q];
    const double yi = ring_y[q];
    const double gi = ring_g[q];
    const double Ui = ring_U[q], Vi = ring_V[q], Pi = ring_P[q];
    {
      const int64_t ii = i + kPF < n ? i + kPF : n - 1;
      ring_t[q] = t[ii]; ring_y[q] = y[ii]; ring_g[q] = dg[ii];
      if (SAVE) {
        p_pf += vstride;                                   // -> cadence i + kPF
        const double* p = i + kPF < n ? p_pf : p_uvp + (n - 1) * vstride;
        ring_U[q] = k.live ? p[0] : 0.0;
        ring_V[q] = k.live ? p[qstride] : 0.0;
        ring_P[q] = k.live ? p[2 * qstride] : 0.0;
      }
    }
    const double dt = ti - tprev;
    tprev = ti;
    if (SAVE) {
      Pj = Pi;
      EXO_GROUP_GATHER(Pj, Pall);
    } else if (dt != dt_prev) {  // wave-uniform: evenly sampled series reuse P
      Pj = k.live ? exp(-k.c * dt) : 0.0;
      EXO_GROUP_GATHER(Pj, Pall);
      dt_prev = dt;
    }
    // row j of  S <- (P P^T) o (S + d W W^T) ;  F_j <- P_j (F_j + W_j z)
    Fj = Pj * fma(Wj, z, Fj);
    const double dwj = d * Wj;
#pragma unroll
    for (int l = 0; l < J; ++l) Srow[l] = Pj * Pall[l] * fma(dwj, Wall[l], Srow[l]);
    if (SAVE) { Uj = Ui; Vj = Vi; } else { lane_uv(k, ti, &Uj, &Vj, &cs, &sn); }
    EXO_GROUP_GATHER(Uj, Uall);
    double uj = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) uj = fma(Srow[l], Uall[l], uj);
    // the two dot products of the step share one butterfly
    const double pd = group_sum<G>(Uj * uj), pz = group_sum<G>(Uj * Fj);
    d = gi + asum - pd;
    z = yi - pz;
    bad = bad || !(d > 0.0);
    const double id = 1.0 / d;
    Wj = (Vj - uj) * id;
    EXO_GROUP_GATHER(Wj, Wall);
    acc = fma(z * z, id, acc);
    lman = frexp(lman * (d > 0.0 ? d : 1.0), &lexp);
    lsum += lexp;
    if (store) {
      // running pointers: one add per cadence instead of a 64-bit index product per access
      p_vec += rstride;
      p_scal += 2 * n_draw;
      if (j == 0) *reinterpret_cast<double2*>(p_scal) = double2{d, z};
      store_record<J>(p_vec, six.piece(), Wj, Fj, Srow);
    }
   }
  }
  if (mine && j == 0) loglike[cf.at(draw)] = loglike_of(acc, log(lman) + (double)lsum * exo::kLn2, bad, n);
}

// Reverse recurrence (hand-derived adjoint of the two recurrences above), same lane
// layout: lane j owns row j of the SYMMETRISED adjoint of S (S is symmetric, so only
// the symmetric part of its adjoint matters), Fb_j, Wb_j and the coefficient
// cotangents of its state index.
template <int J>
__global__ __launch_bounds__(kWave) void celerite_vjp_kernel(
    const double* __restrict__ t, const double* __restrict__ diag, int64_t n_diag, int64_t n,
    Coefs cf,
    int64_t n_draw, const double* __restrict__ gloglike, const double* __restrict__ state,
    double* __restrict__ gresid, double* __restrict__ gdiag, double* __restrict__ gdiag_sum,
    double* __restrict__ gcoef_real, double* __restrict__ gcoef_complex, const double* __restrict__ only_flagged,
    double gsign, Series rs, ChunkGeom cg) {   // rs: the series this is the cotangent of (its layout is the cotangent's: GradRow)
  constexpr int G = Group<J>::G;
  const int j = threadIdx.x & (G - 1);
  const int64_t lane_draw = ((int64_t)blockIdx.x * kWave + threadIdx.x) / G;
  const bool live_draw = (lane_draw < n_draw) && (!only_flagged || only_flagged[lane_draw < n_draw ? lane_draw : 0] >= kFlagSeq);
  if (only_flagged) {
    // ... and every other draw's coefficient cotangents from the sums over the chunks (totals in chunk 0's slots): gcoef_lane,
    // the combination of this kernel's own tail, on the lanes that would otherwise leave at once
    if (lane_draw < n_draw && !live_draw && j < J)
      gcoef_lane(cf, n, n_draw, state, cg, 1, gdiag_sum, gcoef_real, gcoef_complex, lane_draw, j);
    if (__ballot(live_draw) == 0) return;
  }
  const int64_t draw = lane_draw < n_draw ? lane_draw : n_draw - 1;
  const LaneCoef k = lane_coef(cf, draw, j, J);
  const int jj = k.live ? j : 0;  // idle lanes read a valid slot and contribute zeros
  const StateIdx six{n, n_draw, J};
  const double gL = gloglike[cf.at(draw)];
  const bool lead = live_draw && j == 0;
  GradRow grow(gresid, rs, draw, n);
  // the other state index of this lane's complex pair (itself for real terms / idle lanes)
  const int partner = (int)threadIdx.x + ((k.live && !k.real) ? (k.odd ? -1 : 1) : 0);

  double Sb[J];  // row j of the symmetric adjoint of S
#pragma unroll
  for (int l = 0; l < J; ++l) Sb[l] = 0.0;
  double Fb = 0.0, Wb = 0.0, db = 0.0, zb = 0.0, gasum = 0.0;
  double ga = 0.0, gb = 0.0, gc = 0.0, gd = 0.0;

  const int64_t vstride = n_draw * J, qstride = n * vstride;
  const double* __restrict__ sc0 = state + six.scal(0, 0, draw);
  const double* __restrict__ ve0 = state + six.rec(0, draw, jj);
  const double* __restrict__ uv0 = state + six.uvp(0, 0, draw, jj);
  const int64_t rstride = vstride * (2 + J);   // one cadence of (W, F, S row) records
  auto load = [&](int64_t i, double& d_, double& z_, double& W_, double& F_, double* S_) {
    const double2 dz = *reinterpret_cast<const double2*>(sc0 + i * 2 * n_draw);
    d_ = dz.x; z_ = dz.y;
    load_record<J>(ve0 + i * rstride, six.piece(), W_, F_, S_);   // idle lanes read lane 0's record: harmless, zeroed below
    if (!k.live) {
      W_ = F_ = 0.0;
#pragma unroll
      for (int l = 0; l < J; ++l) S_[l] = 0.0;
    }
  };
  double d_n, z_n, W_n, F_n, S_n[J];
  load(n - 1, d_n, z_n, W_n, F_n, S_n);
  double Pj = 1.0, Pall[J];
#pragma unroll
  for (int l = 0; l < J; ++l) Pall[l] = 1.0;
  // software prefetch ring over the saved factorisation: the loads of cadence
  // i - 1 - kPB are in flight while cadence i is processed (serial chain, one wave
  // per SIMD: nothing else hides the HBM latency of this 10 GB-scale stream)
  constexpr int kPB = J <= 2 ? 3 : 1;   // deeper rings cost more registers than they hide at larger J
  double r_d[kPB], r_z[kPB], r_W[kPB], r_F[kPB], r_S[kPB][J], r_t[kPB];
  double r_U[kPB], r_V[kPB], r_Vo[kPB], r_P[kPB];   // U, V, partner's V, P of the cadence being processed
  const int jp = k.live ? (partner - ((int)threadIdx.x - j)) : 0;   // partner's state index
  auto load_uvp = [&](int64_t i, double& U_, double& V_, double& Vo_, double& P_) {
    const double* pu = uv0 + i * vstride;
    U_ = k.live ? pu[0] : 0.0;
    V_ = k.live ? pu[qstride] : 0.0;
    Vo_ = k.live ? pu[qstride + (jp - jj)] : 0.0;
    P_ = k.live ? pu[2 * qstride] : 0.0;
  };
#pragma unroll
  for (int q = 0; q < kPB; ++q) {
    const int64_t ii = n - 2 - q >= 0 ? n - 2 - q : 0;
    load(ii, r_d[q], r_z[q], r_W[q], r_F[q], r_S[q]);
    r_t[q] = t[ii];
    load_uvp(ii + 1 < n ? ii + 1 : n - 1, r_U[q], r_V[q], r_Vo[q], r_P[q]);
  }
  double t_n = t[n - 1];

  for (int64_t i0 = n - 1; i0 >= 1; i0 -= kPB) {
#pragma unroll
   for (int q = 0; q < kPB; ++q) {
    const int64_t i = i0 - q;
    if (i < 1) break;
    const double d_p = r_d[q], z_p = r_z[q], W_p = r_W[q], F_p = r_F[q], t_p = r_t[q];
    double S_p[J];
#pragma unroll
    for (int l = 0; l < J; ++l) S_p[l] = r_S[q][l];
    const double Uj = r_U[q], Vj = r_V[q], Vo = r_Vo[q];
    Pj = r_P[q];
    {
      const int64_t ii = i - 1 - kPB >= 0 ? i - 1 - kPB : 0;
      load(ii, r_d[q], r_z[q], r_W[q], r_F[q], r_S[q]);
      r_t[q] = t[ii];
      load_uvp(ii + 1, r_U[q], r_V[q], r_Vo[q], r_P[q]);
    }
    const double ti = t_n;
    const double dt = ti - t_p;
    t_n = t_p;
    EXO_GROUP_GATHER(Pj, Pall);
    // cos / sin of this lane's complex pair: its own V and its partner's
    const double cs = k.odd ? Vo : Vj, sn = k.odd ? Vj : Vo;
    double Uall[J], Wpall[J];
    EXO_GROUP_GATHER(Uj, Uall);
    EXO_GROUP_GATHER(W_p, Wpall);
    const double id = 1.0 / d_n;
    // (5) log-likelihood terms, (4) z_n = y_n - U.F_n
    const double zbar = zb - gL * z_n * id;
    const double wdot = group_sum<G>(Wb * W_n);
    const double dbar = db + gL * (0.5 * z_n * z_n * id * id - 0.5 * id) - wdot * id;
    if (lead) {
      grow.store(i, gsign * zbar);
      if (gdiag) gdiag[cf.at(draw) * n + i] = dbar;
    }
    gasum += dbar;
    double Ub = -zbar * F_n;
    Fb = fma(-zbar, Uj, Fb);
    // (3) W_n = (V_n - u) / d_n ; d_n = a_n - U.u ; u = S_n U
    const double Vb = Wb * id;
    double uj = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) uj = fma(S_n[l], Uall[l], uj);
    Ub = fma(-dbar, uj, Ub);
    const double ubj = -Vb - dbar * Uj;
    double uball[J];
    EXO_GROUP_GATHER(ubj, uball);
    double acc_u = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      Sb[l] = fma(0.5, fma(ubj, Uall[l], uball[l] * Uj), Sb[l]);  // symmetrised  ub U^T
      acc_u = fma(S_n[l], uball[l], acc_u);                        // (S_n^T ub)_j, S symmetric
    }
    Ub += acc_u;
    // d loglike / d(oscillation rate of a complex pair): - sum over the links of dt x (the phase FLUX across the link), the flux
    // taken from what it is -- Fbar^T G F + < Sbar, G S + S G^T >, G = [[0, -1], [1, 0]] on the pair, the state entering this
    // cadence against its adjoint (phase_flux, exo_celerite_core.hpp) -- at EVERY link: no sum of phase cotangents weighted with
    // their distance from the origin (sum_i (t_i - t_0) g_i lost up to 4e-5 on kernels with aliased oscillation rates -- the
    // sequential recurrences of celerite2's formulation do; tools/gp_seq_dc_check.py).  Lane j of a pair has row j of S and of
    // Sbar; the partner lane (j ^ 1) supplies its row of Sbar and its own cross term.
    double flux = 0.0;
    if (G >= 2) {
      // the pair's other lane: j + 1 for its first index, j - 1 for its second (an odd number of real terms in front leaves
      // the pairs on odd lanes: not lane ^ 1) -- both moves by every lane, then the choice (dpp inside a branch: see grp_argmax8)
      auto other = [&](double v) {
        const double up = dpp_mov<0x101>(v), dn = dpp_mov<0x111>(v);   // row_shl 1: lane i reads i + 1; row_shr 1: i - 1
        return k.odd ? dn : up;
      };
      double cross = 0.0;
#pragma unroll
      for (int l = 0; l < J; ++l) cross = fma(other(Sb[l]), S_n[l], cross);
      const double cross_o = other(cross), F_o = other(F_n), Fb_o = other(Fb);
      flux = fma(Fb_o, F_n, -Fb * F_o) + 2.0 * (cross - cross_o);
    }
    // (2) F_n = P o G, G = F_p + W_p z_p   (1) S_n = P P^T o T, T = S_p + d_p W_p W_p^T
    const double Gj = fma(W_p, z_p, F_p);
    double Pb = Fb * Gj;
    const double Gb = Fb * Pj;
    double Wb_prev = Gb * z_p;
    const double zb_prev = group_sum<G>(Gb * W_p);
    double psum = 0.0, wsum = 0.0, dsum = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      const double T = fma(d_p * W_p, Wpall[l], S_p[l]);
      const double Tb = Sb[l] * Pj * Pall[l];       // adjoint of T (symmetric)
      psum = fma(2.0 * Sb[l] * T, Pall[l], psum);
      wsum = fma(2.0 * Tb, Wpall[l], wsum);
      dsum = fma(Tb, Wpall[l], dsum);
      Sb[l] = Tb;                                   // becomes the adjoint of S_{n-1}
    }
    Pb += psum;
    Wb_prev = fma(d_p, wsum, Wb_prev);
    const double db_prev = group_sum<G>(dsum * W_p);
    // parameter adjoints: P = exp(-c dt), U, V.  A complex pair's (a, b, d) cotangents
    // collect on its first lane: fetch the partner lane's Ub, Vb
    gc = fma(-dt * Pj, Pb, gc);
    if (k.live) {
      if (k.real) {
        ga += Ub;
      }
    }
    {
      const double Ub_o = __shfl(Ub, partner, 64);
      if (k.live && !k.real && !k.odd) {
        ga += Ub * cs + Ub_o * sn;
        gb += Ub * sn - Ub_o * cs;
        gd = fma(-dt, flux, gd);
      }
    }
    // shift to cadence n-1
    db = db_prev;
    zb = zb_prev;
    Fb = Gb;
    Wb = Wb_prev;
    d_n = d_p; z_n = z_p; W_n = W_p; F_n = F_p;
#pragma unroll
    for (int l = 0; l < J; ++l) S_n[l] = S_p[l];
   }
  }
  // cadence 0: d_0 = a_0, W_0 = V_0 / d_0, z_0 = y_0
  {
    const double id = 1.0 / d_n;
    const double zbar = zb - gL * z_n * id;
    const double wdot = group_sum<G>(Wb * W_n);
    const double dbar = db + gL * (0.5 * z_n * z_n * id * id - 0.5 * id) - wdot * id;
    if (lead) {
      grow.store(0, gsign * zbar);
      if (gdiag) gdiag[cf.at(draw) * n] = dbar;
    }
    gasum += dbar;
    // (cadence 0's phase cotangent has no link in front of it -- the phases are counted from t_0, Coefs::origin -- and its
    // U, V carry no other parameter: nothing more to collect)
  }
  // the decay rate of a complex pair is shared by its two state indices
  const double gc_o = __shfl(gc, partner, 64);
  if (!live_draw || !k.live) return;
  if (j == 0 && gdiag_sum) gdiag_sum[cf.at(draw)] = gasum;
  if (k.real) {
    // a real term of its own, or one of the two real terms of a pair slot (kind 1)
    double* o = k.slot < 0 ? gcoef_real + (cf.at(draw) * cf.n_real + j) * 2 : gcoef_complex + cf.at(draw) * cf.n_complex * 4 + k.slot;
    o[0] = ga + gasum;  // a_n = diag_n + sum a
    o[1] = gc;
  } else if (!k.odd) {
    double* o = gcoef_complex + (cf.at(draw) * cf.n_complex + ((j - cf.n_real) >> 1)) * 4;
    o[0] = ga + gasum;
    o[1] = gb;
    o[2] = gc + gc_o;
    o[3] = gd;
  }
}

}  // namespace
