// exo_celerite_lanegroup.hpp -- the TIME-PARALLEL path in lane-group form (J >= 7): which draws it can take (flag), the
// pre-pass for those it cannot, a lane's row of Delta (LaneDelta), the reference step of a chunk (LaneStepper), and the
// three kernels that work on all chunks at once, a draw on G lanes: elements (A), forward recurrence (C), reverse (C').
#pragma once
#include "exo_celerite_seq.hpp"

namespace {

// ===========================================================================
// Time-parallel path.  The recurrences above are a Kalman filter in disguise: with a
// symmetric Delta_n such that Delta_n U_n = V_n (the state covariance of the process the kernel
// describes, in the rotating frame celerite uses),
//     P_n = Delta_n - S_n   is the covariance of the one-step prediction of the state,
//     F_n                   is its mean,
//     d_n = diag_n + U_n^T P_n U_n,  W_n = P_n U_n / d_n,  z_n   the innovation variance, gain, innovation
// (diag_n = a_n - U_n^T V_n is the measurement variance).  A run of cadences therefore acts on
// (F, P) as a filtering element (A, b, C, eta, J) of Sarkka & Garcia-Fernandez (2021):
//     F' = A (I + P J)^-1 (F + P eta) + b,      P' = A (I + P J)^-1 P A^T + C,
// built by running the filter from (0, 0) next to two sensitivity matrices, and the run's
// log-likelihood as a function of its entering state has the closed form
//     const - 1/2 log det(I + P J) + 1/2 eta^T Y P eta + eta^T Y F - 1/2 F^T J Y F,  Y = (I + P J)^-1.
// So: split the series into C chunks; (A) build every chunk's element in parallel; (B) walk the
// C elements per draw to get the state ENTERING each chunk; (C) run the ordinary recurrences inside
// every chunk in parallel from that state.  The reverse pass needs the adjoint of the entering
// state of every chunk, and the chain rule across chunks only needs the same elements:
//     Fbar  += Y^T (eta - J F) gL + Abar^T Fbar',            Abar = A Y
//     Pbar  += 1/2 (w w^T - J Y) gL + Abar^T Pbar' Abar + sym(Abar^T Fbar' g^T),   g = eta - J Y (F + P eta)
// (B'), after which the ordinary reverse recurrence runs inside every chunk in parallel (C').
// Nothing is differentiated through (A), (B): they only supply boundary values of quantities the
// sequential algorithm also has, so the parameter cotangents are still summed by the ordinary
// reverse recurrence.  Work is ~2x the sequential algorithm's, spread over C x more lanes.
//
// Delta: a real term (a, c): 1 / a.  A complex pair (a, b, c, d) with (cs, sn) = (cos d t, sin d t):
// H Delta0 H, H = [[cs, sn], [sn, -cs]], Delta0 = [[p, q], [q, r]], r = a / (a^2 + b^2),
// q = -b / (a^2 + b^2), p = (a^2 + 2 b^2) / (a (a^2 + b^2)) -- the member of the family
// Delta0 (a, b)^T = (1, 0)^T for which the process noise Delta_{n+1} - phi^2 Delta_n is positive
// semi-definite exactly when the term is a valid kernel (|b d| <= a c).  Draws with a term outside
// a > 0, |b d| <= a c are flagged and handled by the sequential kernels.
// ===========================================================================

// which draws the time-parallel path cannot take (DeltaCoef::valid): kFlagSeq = redo sequentially (the element kernel adds
// its own verdicts on the conditioning: kFlagRobust / kFlagSeq, exo_celerite_core.hpp)
template <int J>
__global__ __launch_bounds__(kWave) void celerite_flag_kernel(Coefs cf,
                                                              int64_t n_draw, double* __restrict__ flag) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  DeltaCoef<J> dc;
  dc.init(cf, draw);
  flag[draw] = dc.valid ? kFlagClean : kFlagSeq;
}

// pre-pass for the flagged draws only (the sequential kernels read U, V, P from `state`; the
// time-parallel kernels recompute them: three fewer arrays across HBM four times)
__global__ __launch_bounds__(256) void celerite_prep_flagged_kernel(const double* __restrict__ t, int64_t n,
                                                                    Coefs cf, int64_t n_draw, int J,
                                                                    double* __restrict__ state,
                                                                    const double* __restrict__ flag) {
  const int64_t draw = blockIdx.y;
  if (flag[draw] < kFlagSeq) return;   // (clean, or finished on the robust route of the time-parallel path)
  const StateIdx six{n, n_draw, J};
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n * J; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / J;
    prep_one(t, cf, six, i, draw, (int)(e - i * J), state);
  }
}

// row j of Delta_n for the lane that owns state index j (see DeltaCoef for the formulas)
struct LaneDelta {
  double dp, dq, dr;
  __device__ __forceinline__ explicit LaneDelta(const LaneCoef& k) : dp(0.0), dq(0.0), dr(0.0) {
    if (!k.live) return;
    if (k.real) {
      dp = 1.0 / k.a;
    } else {
      const double h = 1.0 / (k.a * k.a + k.b * k.b);
      dr = k.a * h; dq = -k.b * h; dp = (k.a * k.a + 2.0 * k.b * k.b) * h / k.a;
    }
  }
  // cs, sn: cos / sin (d t_n) of the lane's pair (from lane_uv)
  // Branch-free: a row has its diagonal entry and, for a pair, the entry of the pair's other index -- two values worked out once,
  // then two selects per entry.  (A real or idle lane has dq = dr = 0 and (cs, sn) = (1, 0) from lane_uv: the pair formulas give
  // dp and 0 there.)  As nested ifs inside the unrolled loop this was ~4 divergent branch regions per ENTRY in the element
  // kernel's cadence loop: 47 of them per cadence at J = 10, a third of the 1030 instructions it issued.
  // the two entries of my row that are not zero: the diagonal one, vd, and (a pair) the one at the pair's other index, vo
  __device__ __forceinline__ void two(const LaneCoef& k, double cs, double sn, double* vd, double* vo) const {
    const double v_even = dp * cs * cs + 2.0 * dq * cs * sn + dr * sn * sn;
    const double v_odd = dp * sn * sn - 2.0 * dq * cs * sn + dr * cs * cs;
    const double v_off = (dp - dr) * cs * sn + dq * (sn * sn - cs * cs);
    *vd = k.live ? (k.real ? dp : (k.odd ? v_odd : v_even)) : 0.0;
    *vo = (k.live && !k.real) ? v_off : 0.0;
  }
  // the pair's other index (-1: none)
  static __device__ __forceinline__ int other(const LaneCoef& k, int j) { return (k.live && !k.real) ? (k.odd ? j - 1 : j + 1) : -1; }
  template <int J>
  __device__ __forceinline__ void row(const LaneCoef& k, int j, double cs, double sn, double* D) const {
    double vd, vo;
    two(k, cs, sn, &vd, &vo);
    const int jo = other(k, j);
#pragma unroll
    for (int l = 0; l < J; ++l) D[l] = (l == j) ? vd : ((l == jo) ? vo : 0.0);
  }
};

// U_j, V_j from the pair's (cos, sin) (lane_uv's last lines)
__device__ __forceinline__ void lane_uv_from(const LaneCoef& k, double cs, double sn, double* U, double* V) {
  *U = k.odd ? (k.a * sn - k.b * cs) : (k.a * cs + k.b * sn);
  *V = k.live ? (k.odd ? sn : cs) : 0.0;
}

// The REFERENCE STEP of a chunk for one state index (DrawCoef::step / rot_uv of the one-lane kernels, on a lane).  The lane-group
// kernels used to take sin / cos of d (t - t0) and exp(-c dt) afresh at every cadence -- ~130 of the 500-700 instructions a
// cadence issued at J = 10, the propagators re-evaluated two steps out of three because "evenly sampled" steps differ in their
// last bits.  Here the chunk's first step is the reference: exp(-c dt_ref), (cos, sin)(d dt_ref) once, and a step within 2^-20
// of it takes them corrected to second order in del = dt - dt_ref (exact to 1e-16 when max(|c|, |d|) dt_ref <= 8); the pair's
// (cos, sin) are ROTATED from the neighbouring cadence and taken exactly at every fourth cadence of the chunk (three rotations
// in a row drift by ~3e-16), at gaps, and for terms too fast for the correction.  Two equal steps off the reference in a row
// become the new reference.
#ifndef EXO_LG_REF_STEP
#define EXO_LG_REF_STEP 1
#endif
struct LaneStepper {
  double dt_ref = -1.0, dt_miss = -1.0, ph = 1.0, rc = 1.0, rs = 0.0;
  bool near_ok = false;
  __device__ __forceinline__ void set_ref(const LaneCoef& k, double dt) {
    dt_ref = dt;
    ph = k.live ? exp(-k.c * dt) : 0.0;
    rc = 1.0; rs = 0.0;
    if (k.live && !k.real) exo::sincos_any(k.d * dt, &rs, &rc);
    near_ok = fmax(fabs(k.c), fabs(k.d)) * dt <= 8.0 && dt > 0.0;
  }
  // the propagator of the step dt; true: the step is near the reference (rot / rot_back may follow)
  __device__ __forceinline__ bool step(const LaneCoef& k, double dt, double* P) {
    constexpr double kTol = 9.5367431640625e-07;   // 2^-20
    if (!EXO_LG_REF_STEP) {
      *P = k.live ? exp(-k.c * dt) : 0.0;
      return false;
    }
    if (dt_ref < 0.0) set_ref(k, dt);
    bool near = near_ok && fabs(dt - dt_ref) <= kTol * dt_ref;
    if (!near) {
      if (dt_miss > 0.0 && fabs(dt - dt_miss) <= kTol * dt_miss) {
        set_ref(k, dt);
        near = near_ok;
      }
      dt_miss = dt;
    }
    if (near) {
      const double x = k.c * (dt - dt_ref);
      *P = ph * fma(x, fma(0.5, x, -1.0), 1.0);
    } else {
      *P = k.live ? exp(-k.c * dt) : 0.0;
    }
    return near;
  }
  // the pair's (cos, sin) one near step dt LATER / EARLIER than the cadence they belong to (a real or idle lane's (1, 0) stays)
  __device__ __forceinline__ void rot(const LaneCoef& k, double dt, double& cs, double& sn) const {
    const double c1 = fma(cs, rc, -sn * rs), s1 = fma(sn, rc, cs * rs);
    const double e = k.d * (dt - dt_ref), h = fma(-0.5 * e, e, 1.0);
    cs = fma(-e, s1, c1 * h);
    sn = fma(e, c1, s1 * h);
  }
  __device__ __forceinline__ void rot_back(const LaneCoef& k, double dt, double& cs, double& sn) const {
    const double c1 = fma(cs, rc, sn * rs), s1 = fma(sn, rc, -cs * rs);
    const double e = k.d * (dt - dt_ref), h = fma(-0.5 * e, e, 1.0);
    cs = fma(e, s1, c1 * h);
    sn = fma(-e, c1, s1 * h);
  }
  // U, V of the cadence at time t, q cadences into its chunk; (cs, sn) come in as those of the cadence before it (the step dt up
  // to t) or, BACK, after it (the step dt on from t) and go out as its own: rotated where that step is near the reference, taken
  // exactly at every fourth cadence of the chunk and wherever it is not
  template <bool BACK>
  __device__ __forceinline__ void uv_from_neighbour(const LaneCoef& k, bool near, int64_t q, double dt, double t, double& cs, double& sn,
                                                    double* U, double* V) const {
    if (near && (q & 3) != 0) {
      if (BACK) rot_back(k, dt, cs, sn); else rot(k, dt, cs, sn);
      lane_uv_from(k, cs, sn, U, V);
    } else {
      lane_uv(k, t, U, V, &cs, &sn);
    }
  }
};

// (A) in lane-group form: the element of a (draw, chunk) on the draw's G lanes, lane j owning row j of
// A, Cm, Jm.  Same arithmetic as celerite_elem_kernel; the column sums A^T U travel by a butterfly,
// Cm U / the gain by DPP broadcasts.  A lane carries 3 J + 2 doubles of element state instead of
// 3 J^2 + 2 J (J = 6: the one-lane version needs 256 registers and scratch), and there are G times
// more lanes to hide the loads.  Used for J >= 3, and the only version for J = 7, 8.
template <int J>
__global__ __launch_bounds__(kWave) void celerite_elem_lg_kernel(
    const double* __restrict__ t, Series rs, const double* __restrict__ diag, int64_t n_diag,
    int64_t n, Coefs cf, int64_t n_draw, double* __restrict__ state, ChunkGeom cg, int64_t flag_at) {
  constexpr int G = Group<J>::G;
  const auto [j, draw, live_draw] = GroupLane<G>(n_draw);
  const int c = blockIdx.y;
  const bool empty = c * cg.L >= n;   // a fine chunk past the end of the series: the identity element
  const int64_t n0 = empty ? n - 1 : c * cg.L, n1 = empty ? n0 : ((n0 + cg.L < n) ? n0 + cg.L : n);
  const LaneCoef k = lane_coef(cf, draw, j, J);
  const bool live = k.live;
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const LaneDelta ld(k);
  const SeriesRow y(rs, draw, n);
  const double* __restrict__ dg = diag_row(diag, n_diag, cf, draw, n);
  // conditioning score (see celerite_elem_kernel)
  const double asum = group_sum<G>((live && !k.odd) ? fabs(k.a) : 0.0);
  double ba2 = (live && !k.real && !k.odd) ? (k.b * k.b) / (k.a * k.a) : 0.0;
  if (G >= 2) ba2 = fmax(ba2, xor_get<1>(ba2));
  if (G >= 4) ba2 = fmax(ba2, xor_get<2>(ba2));
  if (G >= 8) ba2 = fmax(ba2, xor_get<4>(ba2));
  if (G >= 16) ba2 = fmax(ba2, xor_get<8>(ba2));
  const double rmin = (1.0 + ba2) * asum * (1.0 / EXO_GP_COND_MAX);
  bool ok = true;

  // lane j holds COLUMN j of A (so that (A^T U)_j is a local dot product: no butterfly) and rows j of
  // Cm, Jm
  // (my row of Delta has two entries that are not zero -- LaneDelta::two: the previous cadence's are two doubles, not a row of J:
  // the kernel held 80 + 16 J registers, one wave per SIMD from J = 11 and two from J = 6)
  double Acol[J], Crow[J], Jrow[J], phiall[J];
#pragma unroll
  for (int l = 0; l < J; ++l) { Acol[l] = (live && l == j) ? 1.0 : 0.0; Crow[l] = 0.0; Jrow[l] = 0.0; phiall[l] = 1.0; }
  double bj = 0.0, etaj = 0.0, phi = 1.0;
  double ti = t[n0];
  double Uj, Vj, cs, sn;
  lane_uv(k, ti, &Uj, &Vj, &cs, &sn);
  const int jo = LaneDelta::other(k, j);
  double vd_l, vo_l;
  ld.two(k, cs, sn, &vd_l, &vo_l);
  LaneStepper stp;
#pragma unroll 1
  for (int64_t i = n0; i < n1; ++i) {
    const double yi = y[i], R = dg[i];
    ok = ok && (R >= rmin) && (R < INFINITY);
    double Uall[J];
    EXO_GROUP_GATHER(Uj, Uall);
    double rj = 0.0, cuj = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      rj = fma(Acol[l], Uall[l], rj);            // (A^T U)_j
      cuj = fma(Crow[l], Uall[l], cuj);          // (Cm U)_j
    }
    const double s = R + group_sum<G>(Uj * cuj);
    const double zeta = yi - group_sum<G>(Uj * bj);
    const double is = exo::fast_rcp(s);
    double rall[J];
    EXO_GROUP_GATHER(rj, rall);
    const double ris = rj * is;
    etaj = fma(ris, zeta, etaj);
#pragma unroll
    for (int l = 0; l < J; ++l) Jrow[l] = fma(ris, rall[l], Jrow[l]);
    if (i + 1 < n) {
      const double tn = t[i + 1], dt = tn - ti;
      ti = tn;
      const bool near = stp.step(k, dt, &phi);
      EXO_GROUP_GATHER(phi, phiall);
      stp.uv_from_neighbour<false>(k, near, i + 1 - n0, dt, tn, cs, sn, &Uj, &Vj);
      double vd_n, vo_n;
      ld.two(k, cs, sn, &vd_n, &vo_n);
      const double kj = cuj * is;            // the gain of my state index
      bj = phi * fma(kj, zeta, bj);
      // what the updates need of the OTHER indices is their gains k_l = (Cm U)_l / s (gathered once, instead of (Cm U)_l with a
      // multiplication by 1 / s per entry):  A[l][j] = phi_l (A[l][j] - k_l r_j),   Cm[j][l] = phi_j phi_l (Cm[j][l] - (Cm U)_j k_l) + Q
      double kall[J];
      EXO_GROUP_GATHER(kj, kall);
#pragma unroll
      for (int l = 0; l < J; ++l) {
        Acol[l] = phiall[l] * fma(-kall[l], rj, Acol[l]);
        const double dl = (l == j) ? vd_l : ((l == jo) ? vo_l : 0.0), dn = (l == j) ? vd_n : ((l == jo) ? vo_n : 0.0);
        Crow[l] = fma(phi * phiall[l], fma(-cuj, kall[l], Crow[l]) - dl, dn);   // + Q = Dn - phi phi Dl
      }
      vd_l = vd_n; vo_l = vo_n;
    }
  }
  if (!live_draw || !live) return;
  if (!ok && j == 0) state[(flag_at >= 0 ? flag_at : ws.off_flag()) + draw] = kFlagSeq;   // (no robust route on the lane-group path)
  const int E1 = J * J, E2 = J * J + J, E3 = 2 * J * J + J, E4 = 2 * J * J + 2 * J;
#pragma unroll
  for (int l = 0; l < J; ++l) {
    state[ws.elem(c, l * J + j, draw)] = Acol[l];          // A[l][j]
    state[ws.elem(c, E2 + j * J + l, draw)] = Crow[l];
    state[ws.elem(c, E4 + j * J + l, draw)] = Jrow[l];
  }
  state[ws.elem(c, E1 + j, draw)] = bj;
  state[ws.elem(c, E3 + j, draw)] = etaj;
}

// (C) the ordinary recurrences inside every chunk, from the entering state: same lane layout as
// celerite_fwd_kernel (a draw on G lanes), one wave per (64 / G draws, chunk).  With C x more
// waves than the sequential kernel the loads are hidden by occupancy: no prefetch ring.
template <int J>
__global__ __launch_bounds__(kWave) void celerite_chunk_fwd_kernel(
    const double* __restrict__ t, Series rs, const double* __restrict__ diag, int64_t n_diag,
    int64_t n,
    Coefs cf,
    int64_t n_draw, double* __restrict__ state, ChunkGeom cg) {
  constexpr int G = Group<J>::G;
  const auto [j, draw, live_draw] = GroupLane<G>(n_draw);
  const int c = blockIdx.y;
  const int64_t n0 = c * cg.L, n1 = (n0 + cg.L < n) ? n0 + cg.L : n;
  const LaneCoef k = lane_coef(cf, draw, j, J);
  const bool store = live_draw && k.live;
  const double asum = group_sum<G>((k.live && !k.odd) ? k.a : 0.0);
  const StateIdx six{n, n_draw, J};
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const SeriesRow y(rs, draw, n);
  const double* __restrict__ dg = diag_row(diag, n_diag, cf, draw, n);
  const int jj = k.live ? j : 0;

  double Srow[J], Wall[J], Uall[J], Pall[J];
  {
    // entering state from (B) as (F, P): S = Delta_{n0} - P
    const LaneDelta ld(k);
    double U_, V_, cs, sn;
    lane_uv(k, t[n0], &U_, &V_, &cs, &sn);
    ld.row<J>(k, j, cs, sn, Srow);
#pragma unroll
    for (int l = 0; l < J; ++l) { Srow[l] -= k.live ? state[ws.bnd(1, c, J + jj * J + l, draw)] : 0.0; Wall[l] = 0.0; }
  }
  double Fj = k.live ? state[ws.bnd(1, c, jj, draw)] : 0.0;
  double Wj = 0.0, d = 1.0, z = 0.0;
  bool bad = false;
  double acc = 0.0, lman = 1.0;
  int64_t lsum = 0;
  const int64_t rstride = n_draw * J * (int64_t)(2 + J);   // one cadence of (W, F, S row) records
  double* __restrict__ p_vec = state + six.rec(n0, draw, jj);
  double* __restrict__ p_scal = state + six.scal(0, n0, draw);
  double tprev = t[n0], Pj = 1.0;
  double cs_ = 1.0, sn_ = 0.0;
  LaneStepper stp;
#pragma unroll 1
  for (int64_t i = n0; i < n1; ++i) {
    // U, V, P recomputed, not read: three arrays fewer through HBM (LaneStepper: from the chunk's reference step)
    const double ti = t[i], dt = ti - tprev;
    tprev = ti;
    double Uj, Vj;
    bool near = false;
    if (i > n0) near = stp.step(k, dt, &Pj);
    stp.uv_from_neighbour<false>(k, near, i - n0, dt, ti, cs_, sn_, &Uj, &Vj);
    const double yi = y[i], gi = dg[i];
    if (i > n0) {
      EXO_GROUP_GATHER(Pj, Pall);
      Fj = Pj * fma(Wj, z, Fj);
      const double dwj = d * Wj;
#pragma unroll
      for (int l = 0; l < J; ++l) Srow[l] = Pj * Pall[l] * fma(dwj, Wall[l], Srow[l]);
    }
    EXO_GROUP_GATHER(Uj, Uall);
    double uj = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) uj = fma(Srow[l], Uall[l], uj);
    const double pd = group_sum<G>(Uj * uj), pz = group_sum<G>(Uj * Fj);
    d = gi + asum - pd;
    z = yi - pz;
    bad = bad || !(d > 0.0);
    const double id = exo::fast_rcp(d);
    Wj = (Vj - uj) * id;
    EXO_GROUP_GATHER(Wj, Wall);
    acc = fma(z * z, id, acc);
    int lexp;
    lman = frexp(lman * (d > 0.0 ? d : 1.0), &lexp);
    lsum += lexp;
#ifndef EXO_EXP_NOSTORE
    if (store) {
      if (j == 0) *reinterpret_cast<double2*>(p_scal) = double2{d, z};
      if ((i - n0) % lg_span<J>() == 0) store_record<J>(p_vec, six.piece(), Wj, Fj, Srow);   // a checkpoint: the S row too
      else store_record_wf<J>(p_vec, six.piece(), Wj, Fj);
    }
#endif
    p_vec += rstride; p_scal += 2 * n_draw;
  }
  if (live_draw && j == 0) {
    state[ws.part(c, 0, draw)] = acc;
    state[ws.part(c, 1, draw)] = log(lman) + (double)lsum * exo::kLn2;
    state[ws.part(c, 2, draw)] = bad ? 1.0 : 0.0;
  }
}

// (C') the ordinary reverse recurrence inside every chunk.  It starts from the adjoint of the state
// entering the NEXT chunk (from (B')) with the reverse of the propagation step into that chunk, and
// ends with the measurement half of the chunk's first cadence.
template <int J>
__global__ __launch_bounds__(kWave) void celerite_chunk_vjp_kernel(
    const double* __restrict__ t, int64_t n, Coefs cf, int64_t n_draw, const double* __restrict__ gloglike,
    double* __restrict__ state, ChunkGeom cg, double* __restrict__ gresid, double* __restrict__ gdiag,
    double gsign, Series rs) {
  constexpr int G = Group<J>::G;
  const bool gcm = rs.cm != 0 || rs.sp.nseg != nullptr;   // the cotangent is not a row of consecutive cadences: stored one by one
  const GroupLane<G> gl(n_draw);   // (not a structured binding: the lambdas below capture the three)
  const int j = gl.j; const int64_t draw = gl.draw; const bool live_draw = gl.live_draw;
  const int c = blockIdx.y;
  const int64_t n0 = c * cg.L, n1 = (n0 + cg.L < n) ? n0 + cg.L : n;
  const LaneCoef k = lane_coef(cf, draw, j, J);
  const int jj = k.live ? j : 0;
  const StateIdx six{n, n_draw, J};
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const double gL = gloglike[cf.at(draw)];
  const int partner = (int)threadIdx.x + ((k.live && !k.real) ? (k.odd ? -1 : 1) : 0);
  GradRow grow(gresid, rs, draw, n);

  const double gsc = cg.prep ? gL : 1.0;   // (ChunkGeom::prep: the scan's adjoints are those of a cotangent of one)
  double Sb[J];
#pragma unroll
  for (int l = 0; l < J; ++l) Sb[l] = k.live ? gsc * state[ws.bnd(2, c, J + jj * J + l, draw)] : 0.0;
  double Fb = k.live ? gsc * state[ws.bnd(2, c, jj, draw)] : 0.0;
  double Wb = 0.0, db = 0.0, zb = 0.0, gasum = 0.0;
  double ga = 0.0, gb = 0.0, gc = 0.0, gd = 0.0;

  const int64_t vstride = n_draw * J, qstride = n * vstride;
  const double* __restrict__ sc0 = state + six.scal(0, 0, draw);
  const double* __restrict__ ve0 = state + six.rec(0, draw, jj);
  const int64_t rstride = vstride * (2 + J);   // one cadence of (W, F, S row) records
  // (d, z, W, F) of cadence i; the S row of a CHECKPOINT cadence (lg_span: every span-th of a chunk)
  auto load_wf = [&](int64_t i, double& d_, double& z_, double& W_, double& F_) {
    const double2 dz = *reinterpret_cast<const double2*>(sc0 + i * 2 * n_draw);
    d_ = dz.x; z_ = dz.y;
    load_record_wf<J>(ve0 + i * rstride, six.piece(), W_, F_);   // idle lanes read lane 0's record: harmless, zeroed below
    if (!k.live) W_ = F_ = 0.0;
  };
  auto load_s = [&](int64_t i, double* S_) {
    load_record_s<J>(ve0 + i * rstride, six.piece(), S_);
    if (!k.live) {
#pragma unroll
      for (int l = 0; l < J; ++l) S_[l] = 0.0;
    }
  };
  LaneStepper stp, stf;   // (stf: the propagators of the recomputed steps, taken in forward order)
  bool near_last = false;   // the step reversed last -- (i - 1) -> i -- was near the reference: cadence i - 1's (cos, sin) by rot_back
  constexpr int kPer = G >= 8 ? 1 : 8 / G;   // (G = 16: lanes 0 .. 7 of the row keep one cadence each)
  double buf_r[kPer], buf_d[kPer];
  unsigned have = 0u;
#pragma unroll
  for (int q = 0; q < kPer; ++q) buf_r[q] = buf_d[q] = 0.0;
  // reverse of the step (i - 1) -> i :  F_i = P o (F_p + W_p z_p),  S_i = P P^T o (S_p + d_p W_p W_p^T);
  // on entry Sb, Fb are the adjoints of S_i, F_i; on exit those of S_{i-1}, F_{i-1}, and Wb, db, zb
  // those of W_{i-1}, d_{i-1}, z_{i-1}
  auto propagate_adjoint = [&](int64_t i, double d_p, double z_p, double W_p, double F_p, const double* S_p) {
    const double dt = t[i] - t[i - 1];
    double Pj;
    near_last = stp.step(k, dt, &Pj);
    double Pall[J], Wpall[J];
    EXO_GROUP_GATHER(Pj, Pall);
    EXO_GROUP_GATHER(W_p, Wpall);
    const double Gj = fma(W_p, z_p, F_p);
    double Pb = Fb * Gj;
    const double Gb = Fb * Pj;
    double Wb_prev = Gb * z_p;
    const double zb_prev = group_sum<G>(Gb * W_p);
    // (five operations per entry: q = Sb P_l serves the adjoint of T and the propagator's cotangent, and the two sums over
    // Tb W_l -- for Wb and for db -- are one sum; nine as first written, of the ~570 vector instructions a cadence issued at J = 10)
    double psum = 0.0, dsum = 0.0;
    const double dw = d_p * W_p;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      const double T = fma(dw, Wpall[l], S_p[l]);
      const double q = Sb[l] * Pall[l];
      const double Tb = q * Pj;
      psum = fma(q, T, psum);
      dsum = fma(Tb, Wpall[l], dsum);
      Sb[l] = Tb;
    }
    Pb = fma(2.0, psum, Pb);
    Wb_prev = fma(2.0 * d_p, dsum, Wb_prev);
    const double db_prev = group_sum<G>(dsum * W_p);
    gc = fma(-dt * Pj, Pb, gc);
    db = db_prev; zb = zb_prev; Fb = Gb; Wb = Wb_prev;
  };

  // d loglike / d(oscillation rate) as a phase FLUX (exo_celerite_core.hpp, phase_flux): the flux across the chunk's end boundary
  // from the state entering the next chunk (saved at cadence n1) and the adjoint the scan handed over; a pair's first lane keeps it,
  // the partner lane supplies the other row
  double flux = 0.0;
  if (n1 < n) {
    double d1, z1, W1, F1, S1[J];
    load_wf(n1, d1, z1, W1, F1);
    load_s(n1, S1);   // (the next chunk's first cadence: a checkpoint)
    const double Fb_o = __shfl(Fb, partner, 64), F1_o = __shfl(F1, partner, 64);
    double acc = Fb_o * F1 - Fb * F1_o;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      const double Sb_o = __shfl(Sb[l], partner, 64), S1_o = __shfl(S1[l], partner, 64);
      acc = fma(2.0, Sb_o * S1[l] - Sb[l] * S1_o, acc);
    }
    flux = (k.live && !k.real && !k.odd) ? acc : 0.0;
  }
  double cs = 1.0, sn = 0.0;
  // the measurement half of cadence i from its record (d, z, W, F, S row)
  auto measure = [&](int64_t i, double d_n, double z_n, double W_n, double F_n, const double* S_n) {
    // measurement half of cadence i
    const double ti = t[i];
    const double dt_next = (i + 1 < n) ? t[i + 1] - ti : 0.0;
    double Uj, Vj;
    stp.uv_from_neighbour<true>(k, i < n1 - 1 && near_last, i - n0, dt_next, ti, cs, sn, &Uj, &Vj);   // (from cadence i + 1's, one step back)
    double Uall[J];
    EXO_GROUP_GATHER(Uj, Uall);
    const double id = exo::fast_rcp(d_n);   // (seed + two Newton steps, as the one-lane kernels: a third of the IEEE sequence)
    const double zbar = zb - gL * z_n * id;
    const double wdot = group_sum<G>(Wb * W_n);
    const double dbar = db + gL * (0.5 * z_n * z_n * id * id - 0.5 * id) - wdot * id;
    // gresid / gdiag are [draw][cadence]: a store per cadence would touch one 8-B piece of a
    // different 64-B line for every draw of the wave.  The G lanes of a draw (zbar, dbar are the
    // same on all of them) each keep 8 / G consecutive cadences of an aligned block of 8 and the
    // block is written when it is complete (measured: 2.9x write amplification without this).
    if (gcm && live_draw && j == 0) grow.store(i, gsign * zbar);   // cadence-major: the wave's draws are neighbours (sparse: the few values)
    {
      const int owner = (int)(i & 7) / kPer, slot = (int)(i & 7) % kPer;
      if (live_draw && j == owner) {
#pragma unroll
        for (int q = 0; q < kPer; ++q)
          if (slot == q) { buf_r[q] = zbar; buf_d[q] = dbar; }
        have |= 1u << slot;
      }
      if ((i & 7) == 0 || i == n0) {
        const int64_t at = draw * n + (i & ~(int64_t)7) + j * kPer;
#pragma unroll
        for (int q = 0; q < kPer; ++q)
          if ((have >> q) & 1u) {
            if (!gcm) gresid[at + q] = gsign * buf_r[q];
            if (gdiag) gdiag[at + q + (cf.at(draw) - draw) * n] = buf_d[q];
          }
        have = 0u;
      }
    }
    gasum += dbar;
    double Ub = -zbar * F_n;
    Fb = fma(-zbar, Uj, Fb);
    const double Vb = Wb * id;
    double uj = 0.0;
#pragma unroll
    for (int l = 0; l < J; ++l) uj = fma(S_n[l], Uall[l], uj);
    Ub = fma(-dbar, uj, Ub);
    const double ubj = -Vb - dbar * Uj;
    double uball[J];
    EXO_GROUP_GATHER(ubj, uball);
    double acc_u = 0.0;
    const double ubh = 0.5 * ubj, Uh = 0.5 * Uj;
#pragma unroll
    for (int l = 0; l < J; ++l) {
      Sb[l] = fma(ubh, Uall[l], fma(uball[l], Uh, Sb[l]));   // symmetrised  ub U^T
      acc_u = fma(S_n[l], uball[l], acc_u);
    }
    Ub += acc_u;
    if (k.live && k.real) ga += Ub;
    {
      const double Ub_o = __shfl(Ub, partner, 64), Vb_o = __shfl(Vb, partner, 64);
      if (k.live && !k.real && !k.odd) {
        ga += Ub * cs + Ub_o * sn;
        gb += Ub * sn - Ub_o * cs;
        // the link behind this cadence carries the flux so far; this cadence's phase cotangent leaves it
        gd = fma(-dt_next, flux, gd);
        flux -= Ub * (-k.a * sn + k.b * cs) + Ub_o * (k.a * cs + k.b * sn) - Vb * sn + Vb_o * cs;
      }
    }
  };
  // Blocks of lg_span cadences, last to first.  A block's records are loaded at once (all in flight together), its S rows
  // recomputed forward from the checkpoint at its first cadence -- S_i = P_i P_i^T o (S_(i-1) + d_(i-1) W_(i-1) W_(i-1)^T), the
  // forward kernel's own line -- and its cadences walked backwards: the reverse of the step OUT of cadence i, then the
  // measurement half of cadence i, both from cadence i's record alone.
  constexpr int K = lg_span<J>();
  const int64_t nblk = (n1 - n0 + K - 1) / K;
#pragma unroll 1
  for (int64_t bb = nblk - 1; bb >= 0; --bb) {
    const int64_t b0 = n0 + bb * K;
    const int len = (int)((n1 - b0 < K) ? n1 - b0 : K);   // (block-uniform: c is blockIdx.y)
    double rd[K], rz[K], rW[K], rF[K], Sblk[K][J];
#pragma unroll
    for (int q = 0; q < K; ++q) {
      if (q < len) load_wf(b0 + q, rd[q], rz[q], rW[q], rF[q]);
      else { rd[q] = 1.0; rz[q] = rW[q] = rF[q] = 0.0; }
    }
    load_s(b0, Sblk[0]);
#pragma unroll
    for (int q = 1; q < K; ++q) {
      if (q < len) {
        double Pj;
        stf.step(k, t[b0 + q] - t[b0 + q - 1], &Pj);
        double Pall[J], Wall[J];
        EXO_GROUP_GATHER(Pj, Pall);
        EXO_GROUP_GATHER(rW[q - 1], Wall);
        const double dwj = rd[q - 1] * rW[q - 1];
#pragma unroll
        for (int l = 0; l < J; ++l) Sblk[q][l] = Pj * Pall[l] * fma(dwj, Wall[l], Sblk[q - 1][l]);
      } else {
#pragma unroll
        for (int l = 0; l < J; ++l) Sblk[q][l] = 0.0;
      }
    }
#pragma unroll
    for (int q = K - 1; q >= 0; --q) {
      if (q < len) {
        const int64_t i = b0 + q;
        if (i + 1 < n) propagate_adjoint(i + 1, rd[q], rz[q], rW[q], rF[q], Sblk[q]);   // reverse of the step i -> i + 1
        measure(i, rd[q], rz[q], rW[q], rF[q], Sblk[q]);
      }
    }
  }
  if (live_draw && k.live) {
    state[ws.gpart(c, 4 * j + 0, draw)] = ga;
    state[ws.gpart(c, 4 * j + 1, draw)] = gb;
    state[ws.gpart(c, 4 * j + 2, draw)] = gc;
    state[ws.gpart(c, 4 * j + 3, draw)] = gd;
    if (j == 0) state[ws.gpart(c, 4 * J, draw)] = gasum;
  }
}

}  // namespace
