// exo_celerite_scan.hpp -- the scans over the chunks, (B) and (B'): a level of a tree of element compositions per launch --
// one lane per item, a wave per composition in LDS, a block per item for wide states, two levels at once for J <= 2, items
// on groups of eight lanes with a serial top -- the adjoint elements of the wide and the group form, the state a forward
// scan starts from, and the ROBUST route's own scan of the entering states (serial chain, Newton iterations).
#pragma once
#include "exo_celerite_group.hpp"
#include "exo_celerite_lanegroup.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// The scans over the chunks as trees of element compositions (exo_celerite_core.hpp, "The scans (B), (B') as TREES").
// Everything runs one lane per item (celerite_tree_kernel below) except composing two FILTERING elements at J >= 3:
//     M = I + C1 J2,  X1 = M^-1 A1,  x2 = M^-1 (b1 + C1 eta2),  X3 = M^-1 C1,  N = I - J2 X3
//     A = A2 X1        b = A2 x2 + b2        C = A2 X3 A2^T + C2
//     eta = A1^T N (eta2 - J2 b1) + eta1     J = A1^T N J2 A1 + J1
// keeps ~5 J x J matrices alive around the solve -- one lane spills 2 KB at J = 6 and takes 76 us per level whatever
// its size.  Here: one wave per composition (a block), the matrices in LDS padded to 8 x 8, lane (j, l) owning entry
// (j, l) of every product, Gauss-Jordan with partial pivoting for the solve.  LDS-bandwidth-bound (~230 reads of
// 512 B per composition), ~40 us per level at 128 chains x 512 chunks.  Also used where the J > 2 lane-group path
// builds its elements on half chunks and composes them pairwise (ChunkGeom::fine).
// ---------------------------------------------------------------------------------------------
struct ComposeLds {
  double m[13][64];   // A1 C1 J1 A2 C2 J2 M R1 R3 T T2 T3 tmp
  double v[8][8];     // b1 eta1 b2 eta2 r2 v w tmp
};
__global__ __launch_bounds__(kWave) void celerite_compose_lds_kernel(TreeOp op, double* __restrict__ state) {
  __shared__ ComposeLds S;
  const int lane = threadIdx.x, j = lane >> 3, l = lane & 7;
  const int64_t item = blockIdx.x;                       // (index, draw), draws fastest
  const int J = op.J;
  const int64_t n_draw = op.n_draw;
  const int c = (int)(item / n_draw);
  const int64_t draw = item - (int64_t)c * n_draw;
  enum { A1 = 0, C1, J1, A2, C2, J2, MM, R1, R3, TT, T2, T3, TMP };
  enum { B1 = 0, E1, B2, E2, RR2, VV, WW, VT };
  const int E = 3 * J * J + 2 * J;
  const int oA = 0, ob = J * J, oC = J * J + J, oeta = 2 * J * J + J, oJ = 2 * J * J + 2 * J;
  const bool in = j < J && l < J;
  auto src = [&](int pos, int e) -> double {
    const int idx = op.src_rev ? op.src_len - 1 - pos : pos;
    return state[op.src_elem + ((int64_t)idx * E + e) * n_draw + draw];
  };
  // ---- load the two elements; missing ones are the identity
  const int p1 = 2 * c, p2 = 2 * c + 1;
  const bool has1 = p1 < op.src_n, has2 = p2 < op.src_n;
  const double idm = (j == l && in) ? 1.0 : 0.0;
  S.m[A1][lane] = in ? (has1 ? src(p1, oA + j * J + l) : idm) : 0.0;
  S.m[C1][lane] = (in && has1) ? src(p1, oC + j * J + l) : 0.0;
  S.m[J1][lane] = (in && has1) ? src(p1, oJ + j * J + l) : 0.0;
  S.m[A2][lane] = in ? (has2 ? src(p2, oA + j * J + l) : idm) : 0.0;
  S.m[C2][lane] = (in && has2) ? src(p2, oC + j * J + l) : 0.0;
  S.m[J2][lane] = (in && has2) ? src(p2, oJ + j * J + l) : 0.0;
  if (l == 0) {
    S.v[B1][j] = (j < J && has1) ? src(p1, ob + j) : 0.0;
    S.v[E1][j] = (j < J && has1) ? src(p1, oeta + j) : 0.0;
    S.v[B2][j] = (j < J && has2) ? src(p2, ob + j) : 0.0;
    S.v[E2][j] = (j < J && has2) ? src(p2, oeta + j) : 0.0;
  }
  __syncthreads();
  // dst[j][l] = sum_k X[j][k] Y[k][l]  (transposes by index)
  auto mm = [&](int X, bool tx, int Y, bool ty) -> double {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fma(tx ? S.m[X][k * 8 + j] : S.m[X][j * 8 + k], ty ? S.m[Y][l * 8 + k] : S.m[Y][k * 8 + l], acc);
    return acc;
  };
  auto mv = [&](int X, bool tx, int V) -> double {   // (X v)_j, computed by every lane of row j
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fma(tx ? S.m[X][k * 8 + j] : S.m[X][j * 8 + k], S.v[V][k], acc);
    return acc;
  };
  // M = I + C1 J2 ;  right-hand sides R1 = A1, r2 = b1 + C1 eta2, R3 = C1
  {
    const double m = mm(C1, false, J2, false) + (j == l ? 1.0 : 0.0);
    const double r2 = S.v[B1][j] + mv(C1, false, E2);
    S.m[MM][lane] = m;
    S.m[R1][lane] = S.m[A1][lane];
    S.m[R3][lane] = S.m[C1][lane];
    if (l == 0) S.v[RR2][j] = r2;
  }
  __syncthreads();
  // Gauss-Jordan with partial pivoting (padded rows / columns are the identity: never chosen, never changed)
  for (int k = 0; k < J; ++k) {
    int piv = k;
    double best = fabs(S.m[MM][k * 8 + k]);
    for (int i = k + 1; i < J; ++i) {
      const double a = fabs(S.m[MM][i * 8 + k]);
      if (a > best) { best = a; piv = i; }
    }
    // rows k and piv swapped on the way in; row k scaled, its multiples taken off the others
    const int srow = j == k ? piv : (j == piv ? k : j);
    const double ip = 1.0 / S.m[MM][piv * 8 + k];
    const double mk = S.m[MM][piv * 8 + l] * ip, ak = S.m[R1][piv * 8 + l] * ip, ck = S.m[R3][piv * 8 + l] * ip;
    const double rk = S.v[RR2][piv] * ip;
    const double f = j == k ? 0.0 : S.m[MM][srow * 8 + k];
    const double mj = S.m[MM][srow * 8 + l], aj = S.m[R1][srow * 8 + l], cj = S.m[R3][srow * 8 + l], rj = S.v[RR2][srow];
    __syncthreads();
    S.m[MM][lane] = j == k ? mk : fma(-f, mk, mj);
    S.m[R1][lane] = j == k ? ak : fma(-f, ak, aj);
    S.m[R3][lane] = j == k ? ck : fma(-f, ck, cj);
    if (l == 0) S.v[RR2][j] = j == k ? rk : fma(-f, rk, rj);
    __syncthreads();
  }
  // now R1 = X1, r2 = x2, R3 = X3
  const double A_new = mm(A2, false, R1, false);
  const double b_new = mv(A2, false, RR2) + S.v[B2][j];
  S.m[TT][lane] = mm(A2, false, R3, false);                          // A2 X3
  S.m[T2][lane] = (j == l ? 1.0 : 0.0) - mm(J2, false, R3, false);   // N = I - J2 X3
  if (l == 0) S.v[VV][j] = S.v[E2][j] - mv(J2, false, B1);           // eta2 - J2 b1
  __syncthreads();
  const double C_new = mm(TT, false, A2, true) + S.m[C2][lane];
  S.m[T3][lane] = mm(T2, false, J2, false);                          // N J2
  if (l == 0) S.v[WW][j] = mv(T2, false, VV);                        // N (eta2 - J2 b1)
  __syncthreads();
  S.m[TMP][lane] = mm(T3, false, A1, false);                         // N J2 A1
  const double eta_new = mv(A1, true, WW) + S.v[E1][j];
  __syncthreads();
  const double J_new = mm(A1, true, TMP, false) + S.m[J1][lane];
  // symmetrise C and J through LDS
  S.m[TT][lane] = C_new;
  S.m[T2][lane] = J_new;
  __syncthreads();
  const double C_sym = 0.5 * (C_new + S.m[TT][l * 8 + j]), J_sym = 0.5 * (J_new + S.m[T2][l * 8 + j]);
  if (!in) return;
  auto dst = [&](int e) -> double& { return state[op.dst_elem + ((int64_t)c * E + e) * n_draw + draw]; };
  dst(oA + j * J + l) = A_new;
  dst(oC + j * J + l) = C_sym;
  dst(oJ + j * J + l) = J_sym;
  if (l == 0) { dst(ob + j) = b_new; dst(oeta + j) = eta_new; }
}

// The same items, ONE LANE each (tree_item_lane, exo_celerite_core.hpp): (index, draw) pairs with draws fastest, so that
// the [index][quantity][draw] arrays are read and written coalesced.  An item touches ~3 J^2 doubles once; whatever
// spills costs a few loads, and a wave carries 64 items where the LDS kernel above carries one.
template <int J, bool ADJ, bool DOWN>
__global__ __launch_bounds__(kWave) void celerite_tree_kernel(TreeOp op, double* __restrict__ state) {
  const int64_t item = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (item >= (int64_t)op.n_item * op.n_draw) return;
  const int c = (int)(item / op.n_draw);
  tree_item_lane<J, ADJ, DOWN>(op, state, c, item - (int64_t)c * op.n_draw);
}

// WIDE STATES (J = 9 .. 16, round 6): an item of a scan level on a BLOCK of 256 threads, thread (j, l) owning entry (j, l) of every
// J x J matrix, the matrices in LDS padded to 16 x 16.  One lane per item (celerite_tree_kernel) holds an element's 3 J^2 + 2 J
// doubles -- 320 at J = 10, 800 at J = 16 -- in scratch and walks J^3 products through it: 0.4-1.4 ms per level at 128 chains x 128
// chunks, 21 of the 33 ms of a C5-shaped step at J = 10.  Same algebra as tree_compose / tree_apply (exo_celerite_core.hpp), the
// sums in the same order (k ascending); the solve is Gauss-Jordan with partial pivoting on [X | right-hand sides] in place (the
// one-lane code eliminates forward and substitutes back: the same pivots, other roundings at the 1e-16 level).  J is a RUN-TIME
// value here (op.J): one instantiation per (ADJ, DOWN) serves every width.
#ifndef EXO_GP_WIDE_LDS
#define EXO_GP_WIDE_LDS 1     // (0: the one-lane tree kernel for wide states too -- A/B)
#endif
struct WideLds {
  double m[14][256];
  double v[10][16];
  int piv;
};
template <bool ADJ, bool DOWN>
__global__ __launch_bounds__(256) void celerite_tree_wide_kernel(TreeOp op, double* __restrict__ state) {
  __shared__ WideLds S;
  const int tid = threadIdx.x, j = tid >> 4, l = tid & 15;
  const int J = op.J;
  const int64_t nd = op.n_draw;
  const int64_t item = blockIdx.x;                      // (index, draw), draws fastest
  const int c = (int)(item / nd);
  const int64_t draw = item - (int64_t)c * nd;
  const bool in = j < J && l < J;
  const int E = 3 * J * J + 2 * J, Bq = J + J * J;
  const int oA = 0, ob = J * J, oC = J * J + J, oeta = 2 * J * J + J, oJ = 2 * J * J + 2 * J;
  auto src = [&](int pos, int e) -> double {
    const int idx = op.src_rev ? op.src_len - 1 - pos : pos;
    return state[op.src_elem + ((int64_t)idx * E + e) * nd + draw];
  };
  // element `pos` into matrices (a, cm, jm) and vectors (b, eta); the identity past the end
  auto load_elem = [&](int pos, int a, int cm, int jm, int b, int eta) {
    const bool has = pos >= 0 && pos < op.src_n;
    S.m[a][tid] = in ? (has ? src(pos, oA + j * J + l) : (j == l ? 1.0 : 0.0)) : 0.0;
    S.m[cm][tid] = (in && has) ? src(pos, oC + j * J + l) : 0.0;
    S.m[jm][tid] = (in && has) ? src(pos, oJ + j * J + l) : 0.0;
    if (l == 0) {
      S.v[b][j] = (j < J && has) ? src(pos, ob + j) : 0.0;
      S.v[eta][j] = (j < J && has) ? src(pos, oeta + j) : 0.0;
    }
  };
  // sum_k op(X)[j][k] op(Y)[k][l], k ascending from `init`
  auto mm = [&](double init, int X, bool tx, int Y, bool ty) -> double {
    double acc = init;
    for (int k = 0; k < J; ++k)
      acc = fma(tx ? S.m[X][k * 16 + j] : S.m[X][j * 16 + k], ty ? S.m[Y][l * 16 + k] : S.m[Y][k * 16 + l], acc);
    return acc;
  };
  // (op(X) v)_j from `init`, computed by every thread of row j
  auto mv = [&](double init, int X, bool tx, int V) -> double {
    double acc = init;
    for (int k = 0; k < J; ++k) acc = fma(tx ? S.m[X][k * 16 + j] : S.m[X][j * 16 + k], S.v[V][k], acc);
    return acc;
  };
  // Gauss-Jordan with partial pivoting: X (matrix slot) against right-hand sides R1, R3 (matrix slots; R3 < 0: none) and r (vector
  // slot); on exit the right-hand sides hold the solutions.  Every thread of the block calls it.
  auto solve = [&](int X, int R1, int R3, int r) {
    for (int k = 0; k < J; ++k) {
      if (tid == 0) {
        int p = k;
        double best = fabs(S.m[X][k * 16 + k]);
        for (int i = k + 1; i < J; ++i) {
          const double a = fabs(S.m[X][i * 16 + k]);
          if (a > best) { best = a; p = i; }
        }
        S.piv = p;
      }
      __syncthreads();
      const int p = S.piv;
      if (p != k && j == k && l < J) {          // row k's sixteen threads swap rows k and p
        double tmp = S.m[X][k * 16 + l]; S.m[X][k * 16 + l] = S.m[X][p * 16 + l]; S.m[X][p * 16 + l] = tmp;
        tmp = S.m[R1][k * 16 + l]; S.m[R1][k * 16 + l] = S.m[R1][p * 16 + l]; S.m[R1][p * 16 + l] = tmp;
        if (R3 >= 0) { tmp = S.m[R3][k * 16 + l]; S.m[R3][k * 16 + l] = S.m[R3][p * 16 + l]; S.m[R3][p * 16 + l] = tmp; }
        if (l == 0) { tmp = S.v[r][k]; S.v[r][k] = S.v[r][p]; S.v[r][p] = tmp; }
      }
      __syncthreads();
      const double f = (in && j != k) ? S.m[X][j * 16 + k] / S.m[X][k * 16 + k] : 0.0;
      const double xk = in ? S.m[X][k * 16 + l] : 0.0, r1k = in ? S.m[R1][k * 16 + l] : 0.0;
      const double r3k = (in && R3 >= 0) ? S.m[R3][k * 16 + l] : 0.0, rk = S.v[r][k];
      __syncthreads();
      if (in && j != k) {
        S.m[X][tid] = fma(-f, xk, S.m[X][tid]);
        S.m[R1][tid] = fma(-f, r1k, S.m[R1][tid]);
        if (R3 >= 0) S.m[R3][tid] = fma(-f, r3k, S.m[R3][tid]);
        if (l == 0) S.v[r][j] = fma(-f, rk, S.v[r][j]);
      }
      __syncthreads();
    }
    if (in) {
      const double ip = 1.0 / S.m[X][j * 16 + j];
      S.m[R1][tid] *= ip;
      if (R3 >= 0) S.m[R3][tid] *= ip;
      if (l == 0) S.v[r][j] *= ip;
    }
    __syncthreads();
  };
  enum { A1 = 0, C1, J1, A2, C2, J2, MM, R1, R3, T1, T2, T3, T4, T5 };
  enum { B1 = 0, E1, B2, E2, RR, VW, VN, VX };
  if (DOWN) {
    // ---- child states 2c, 2c + 1 from parent state c and child element 2c
    const double mj = (l == 0 && j < J) ? state[op.par_state + ((int64_t)c * Bq + j) * nd + draw] : 0.0;
    const double pjl = in ? state[op.par_state + ((int64_t)c * Bq + J + j * J + l) * nd + draw] : 0.0;
    auto put = [&](int pos, double mval, double pval) {
      const int idx = op.dst_rev ? op.dst_len - 1 - pos : pos;
      double* __restrict__ q = state + op.dst_state + ((int64_t)idx * Bq) * nd + draw;
      if (l == 0 && j < J) q[(int64_t)j * nd] = mval;
      if (in) q[(int64_t)(J + j * J + l) * nd] = op.psign * pval;
    };
    put(2 * c, mj, pjl);
    if (2 * c + 1 >= op.dst_n) return;               // (uniform over the block)
    load_elem(2 * c, A1, C1, J1, B1, E1);
    S.m[T1][tid] = pjl;                               // P
    if (l == 0) S.v[VW][j] = mj;                      // m
    __syncthreads();
    if (ADJ) {
      // x = A^T m ;  T = P A ;  m2 = eta + x ;  P2 = Cm + A^T T + sym(x b^T)
      const double xj = mv(0.0, A1, true, VW);
      const double tv = mm(0.0, T1, false, A1, false);
      if (l == 0) S.v[VX][j] = xj;
      S.m[T2][tid] = tv;
      __syncthreads();
      const double cong = mm(S.m[C1][tid], A1, true, T2, false);
      const double p2 = in ? cong + 0.5 * (S.v[VX][j] * S.v[B1][l] + S.v[B1][j] * S.v[VX][l]) : 0.0;
      S.m[T3][tid] = p2;
      __syncthreads();
      put(2 * c + 1, S.v[E1][j] + S.v[VX][j], 0.5 * (S.m[T3][j * 16 + l] + S.m[T3][l * 16 + j]));
    } else {
      // X = I + P Jm ;  solve X [YP | ym] = [P | m + P eta] ;  m2 = b + A ym ;  P2 = Cm + (A YP) A^T
      const double xv = mm((j == l && in) ? 1.0 : 0.0, T1, false, J1, false);
      const double pe = mv(S.v[VW][j], T1, false, E1);
      S.m[MM][tid] = in ? xv : 0.0;
      S.m[R1][tid] = pjl;
      if (l == 0) S.v[RR][j] = (j < J) ? pe : 0.0;
      __syncthreads();
      solve(MM, R1, -1, RR);
      const double m2 = mv(S.v[B1][j], A1, false, RR);
      const double ay = mm(0.0, A1, false, R1, false);
      S.m[T2][tid] = ay;
      __syncthreads();
      S.m[T3][tid] = mm(S.m[C1][tid], T2, false, A1, true);
      __syncthreads();
      put(2 * c + 1, m2, 0.5 * (S.m[T3][j * 16 + l] + S.m[T3][l * 16 + j]));
    }
    return;
  }
  // ---- UP: dst element c = src elements 2c, 2c + 1 composed (2c acts first)
  load_elem(2 * c, A1, C1, J1, B1, E1);
  load_elem(2 * c + 1, A2, C2, J2, B2, E2);
  __syncthreads();
  double* __restrict__ dstp = state + op.dst_elem + ((int64_t)c * E) * nd + draw;
  auto dst = [&](int e, double val) { dstp[(int64_t)e * nd] = val; };
  if (ADJ) {
    // Abar = Abar1 Abar2 ;  g = g2 + Abar2^T g1 ;  lF = lF2 + Abar2^T lF1 ;  lP = lP2 + Abar2^T lP1 Abar2 + sym(Abar2^T lF1 g2^T)
    const double gj = mv(S.v[B2][j], A2, true, B1);
    const double vj = mv(0.0, A2, true, E1);
    const double a = mm(0.0, A1, false, A2, false);
    S.m[T1][tid] = mm(0.0, C1, false, A2, false);        // T = lP1 Abar2
    if (l == 0) S.v[VX][j] = vj;
    __syncthreads();
    const double cv = mm(in ? S.m[C2][tid] + 0.5 * (S.v[VX][j] * S.v[B2][l] + S.v[B2][j] * S.v[VX][l]) : 0.0, A2, true, T1, false);
    S.m[T2][tid] = cv;
    __syncthreads();
    if (in) {
      dst(oA + j * J + l, a);
      dst(oC + j * J + l, 0.5 * (S.m[T2][j * 16 + l] + S.m[T2][l * 16 + j]));
      dst(oJ + j * J + l, 0.0);
    }
    if (l == 0 && j < J) { dst(ob + j, gj); dst(oeta + j, S.v[E2][j] + vj); }
    return;
  }
  // filtering elements:  M = I + C1 J2 ;  solve M [X1 | X3 | x2] = [A1 | C1 | b1 + C1 eta2]
  {
    const double mval = mm((j == l && in) ? 1.0 : 0.0, C1, false, J2, false);
    const double r2 = mv(S.v[B1][j], C1, false, E2);
    S.m[MM][tid] = in ? mval : 0.0;
    S.m[R1][tid] = S.m[A1][tid];
    S.m[R3][tid] = S.m[C1][tid];
    if (l == 0) S.v[RR][j] = (j < J) ? r2 : 0.0;
    __syncthreads();
  }
  solve(MM, R1, R3, RR);                               // R1 = X1, R3 = X3, RR = x2
  {
    const double bj = mv(S.v[B2][j], A2, false, RR);                   // b = b2 + A2 x2
    const double wj = -mv(-S.v[E2][j], J2, false, B1);                 // w = eta2 - J2 b1  (same order: eta2, then -J2 b1 terms)
    const double a = mm(0.0, A2, false, R1, false);                    // A = A2 X1
    const double ax = mm(0.0, A2, false, R3, false);                   // A2 X3
    const double nv = -mm((j == l && in) ? -1.0 : 0.0, J2, false, R3, false);   // N = I - J2 X3
    S.m[T1][tid] = ax;
    S.m[T2][tid] = in ? nv : 0.0;
    if (l == 0) { S.v[VW][j] = wj; S.v[VN][j] = bj; }
    __syncthreads();
    const double nw = mv(0.0, T2, false, VW);                           // N w
    S.m[T3][tid] = mm(0.0, T2, false, J2, false);                       // N J2
    if (l == 0) S.v[VX][j] = nw;
    __syncthreads();
    S.m[T4][tid] = mm(0.0, T3, false, A1, false);                       // N J2 A1
    __syncthreads();
    const double ej = mv(S.v[E1][j], A1, true, VX);                     // eta = eta1 + A1^T N w
    const double cv = mm(S.m[C2][tid], T1, false, A2, true);            // C = C2 + (A2 X3) A2^T
    const double jv = mm(S.m[J1][tid], A1, true, T4, false);            // J = J1 + A1^T (N J2 A1)
    S.m[T5][tid] = cv;
    S.m[MM][tid] = jv;
    __syncthreads();
    if (in) {
      dst(oA + j * J + l, a);
      dst(oC + j * J + l, 0.5 * (S.m[T5][j * 16 + l] + S.m[T5][l * 16 + j]));
      dst(oJ + j * J + l, 0.5 * (S.m[MM][j * 16 + l] + S.m[MM][l * 16 + j]));
    }
    if (l == 0 && j < J) { dst(ob + j, S.v[VN][j]); dst(oeta + j, ej); }
  }
}

// (B') part 1 for wide states: the adjoint element of chunk c from its filtering element and the state entering it (badj_prep_lane:
// X = I + P Jm, Y = X^-1, ...), a block of 256 threads per (draw, chunk) like celerite_tree_wide_kernel -- one lane per item walks
// 5 KB of scratch (0.86 of a 9.8 ms step at J = 10).  Same sums in the same order; the element is overwritten in place.
__global__ __launch_bounds__(256) void celerite_badj_prep_wide_kernel(const double* __restrict__ gloglike, int64_t n, int64_t n_draw,
                                                                      int J, double* __restrict__ state, ChunkGeom cg,
                                                                      const int32_t* __restrict__ row) {
  __shared__ WideLds S;
  const int tid = threadIdx.x, j = tid >> 4, l = tid & 15;
  const int64_t draw = blockIdx.x;
  const int c = (int)blockIdx.y + 1;
  const bool in = j < J && l < J;
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const double gL = gloglike ? gloglike[row ? (int64_t)row[draw] : draw] : 1.0;   // (null: a cotangent of one -- ChunkGeom::prep)
  const int oA = 0, ob = J * J, oC = J * J + J, oeta = 2 * J * J + J, oJ = 2 * J * J + 2 * J;
  enum { MA = 0, MJ, MP, MX, MY, MT };
  enum { VM = 0, VETA, VU, VV, VW, VYV, VD };
  S.m[MA][tid] = in ? state[ws.elem(c, oA + j * J + l, draw)] : 0.0;
  S.m[MJ][tid] = in ? state[ws.elem(c, oJ + j * J + l, draw)] : 0.0;
  S.m[MP][tid] = in ? state[ws.bnd(1, c, J + j * J + l, draw)] : 0.0;
  S.m[MY][tid] = (in && j == l) ? 1.0 : 0.0;
  if (l == 0) {
    S.v[VM][j] = j < J ? state[ws.bnd(1, c, j, draw)] : 0.0;
    S.v[VETA][j] = j < J ? state[ws.elem(c, oeta + j, draw)] : 0.0;
    S.v[VD][j] = 0.0;
  }
  __syncthreads();
  auto mm = [&](double init, int X, bool tx, int Y, bool ty) -> double {
    double acc = init;
    for (int k = 0; k < J; ++k)
      acc = fma(tx ? S.m[X][k * 16 + j] : S.m[X][j * 16 + k], ty ? S.m[Y][l * 16 + k] : S.m[Y][k * 16 + l], acc);
    return acc;
  };
  auto mv = [&](double init, int X, bool tx, int V) -> double {
    double acc = init;
    for (int k = 0; k < J; ++k) acc = fma(tx ? S.m[X][k * 16 + j] : S.m[X][j * 16 + k], S.v[V][k], acc);
    return acc;
  };
  {
    const double xv = mm((j == l && in) ? 1.0 : 0.0, MP, false, MJ, false);      // X = I + P Jm
    const double uj = -mv(-S.v[VETA][j], MJ, false, VM);                        // u = eta - Jm m
    const double vj = mv(S.v[VM][j], MP, false, VETA);                          // v = m + P eta
    S.m[MX][tid] = in ? xv : 0.0;
    if (l == 0) { S.v[VU][j] = uj; S.v[VV][j] = vj; }
    __syncthreads();
  }
  // Y = X^-1: Gauss-Jordan with partial pivoting on [X | I] (celerite_tree_wide_kernel's solve, one right-hand side)
  for (int k = 0; k < J; ++k) {
    if (tid == 0) {
      int p = k;
      double best = fabs(S.m[MX][k * 16 + k]);
      for (int i = k + 1; i < J; ++i) {
        const double a = fabs(S.m[MX][i * 16 + k]);
        if (a > best) { best = a; p = i; }
      }
      S.piv = p;
    }
    __syncthreads();
    const int p = S.piv;
    if (p != k && j == k && l < J) {
      double tmp = S.m[MX][k * 16 + l]; S.m[MX][k * 16 + l] = S.m[MX][p * 16 + l]; S.m[MX][p * 16 + l] = tmp;
      tmp = S.m[MY][k * 16 + l]; S.m[MY][k * 16 + l] = S.m[MY][p * 16 + l]; S.m[MY][p * 16 + l] = tmp;
    }
    __syncthreads();
    const double f = (in && j != k) ? S.m[MX][j * 16 + k] / S.m[MX][k * 16 + k] : 0.0;
    const double xk = in ? S.m[MX][k * 16 + l] : 0.0, yk = in ? S.m[MY][k * 16 + l] : 0.0;
    __syncthreads();
    if (in && j != k) {
      S.m[MX][tid] = fma(-f, xk, S.m[MX][tid]);
      S.m[MY][tid] = fma(-f, yk, S.m[MY][tid]);
    }
    __syncthreads();
  }
  if (in) S.m[MY][tid] *= 1.0 / S.m[MX][j * 16 + j];
  __syncthreads();
  {
    const double wj = mv(0.0, MY, true, VU);                                    // w = Y^T u
    const double yv = mv(0.0, MY, false, VV);                                   // Y v
    const double a = mm(0.0, MA, false, MY, false);                             // A Y
    S.m[MT][tid] = mm(0.0, MJ, false, MY, false);                               // Jm Y
    if (l == 0) { S.v[VW][j] = wj; S.v[VYV][j] = yv; }
    __syncthreads();
    const double gj = -mv(-S.v[VETA][j], MJ, false, VYV);                       // g = eta - Jm (Y v)
    if (in) {
      state[ws.elem(c, oA + j * J + l, draw)] = a;
      state[ws.elem(c, oC + j * J + l, draw)] = 0.5 * gL * (S.v[VW][j] * S.v[VW][l] - 0.5 * (S.m[MT][j * 16 + l] + S.m[MT][l * 16 + j]));
    }
    if (l == 0 && j < J) {
      state[ws.elem(c, ob + j, draw)] = gj;
      state[ws.elem(c, oeta + j, draw)] = gL * S.v[VW][j];
    }
  }
}

// two levels of a scan in one launch, one lane per item of the upper one (tree_item4_*_lane; J <= 2)
#ifndef EXO_GP_TREE4
#define EXO_GP_TREE4 1
#endif
template <int J, bool ADJ, bool DOWN>
__global__ __launch_bounds__(kWave) void celerite_tree4_kernel(TreeOp a, TreeOp b, double* __restrict__ state) {
  const int64_t item = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (item >= (int64_t)b.n_item * b.n_draw) return;
  const int i = (int)(item / b.n_draw);
  const int64_t draw = item - (int64_t)i * b.n_draw;
  if (DOWN) tree_item4_down_lane<J, ADJ>(a, b, state, i, draw);
  else tree_item4_up_lane<J, ADJ>(a, b, state, i, draw);
}

// (A draw's scan in ONE launch -- a block per draw walking the levels with block barriers, all of them or the narrow top ones
// only -- was built in round 4, measured slower inside a replayed graph (C3 3.88 against 3.82 ms, C5 1.90 against 1.91: what a
// narrow level costs is its item's dependent latency, not its launch) and removed in round 5.)
// (Round 5, also measured and not kept: the narrow top as a SERIAL chain -- from the level with <= 128 positions up, one lane per
// draw applying that level's elements one after the other to the seed, elements prefetched four ahead, no compositions above
// it: a step costs ~0.5 us -- the 2 x 2 solve's divisions and a load latency the prefetch only partly hides -- so 128 positions
// are no cheaper than the 14 launches they replace: C3 3.63 ms against 3.57 (64 positions: 3.59, 256: 3.74).)
#ifndef EXO_GP_GROUP_TREES
#define EXO_GP_GROUP_TREES 1
#endif
#ifndef EXO_GP_FINE_GROUP
#define EXO_GP_FINE_GROUP 1   // the pairwise composition of the fine elements (ChunkGeom::fine; J = 7, 8) by celerite_tree_group_kernel too
#endif
constexpr int kScanBlock = 256;
// One level of a scan, items of J >= 3 on groups of eight lanes (tree_item_group): a block is 32 groups = 32 CONSECUTIVE
// DRAWS of one item (draws fastest), so that each of an item's ~100 strided accesses covers, per row, 64 contiguous bytes of
// eight draws (one lane per (item, draw) -- celerite_tree_kernel -- is fully coalesced but spills 2 KB per lane at J = 6; a
// block per draw -- the fused kernel below -- touches 64 lines per instruction and is SLOWER than the 34 launches it replaces).
#ifndef EXO_GROUP_WAVES
#define EXO_GROUP_WAVES 1
#endif
template <int J, bool ADJ, bool DOWN>
__global__ __launch_bounds__(kScanBlock, EXO_GROUP_WAVES) void celerite_tree_group_kernel(TreeOp op, double* state) {
  __shared__ double lds[(kScanBlock / 8) * GroupLds<J>::S];
  const int tid = threadIdx.x;
  const int64_t unit = (int64_t)blockIdx.x * (kScanBlock / 8) + (tid >> 3);
  if (unit >= (int64_t)op.n_item * op.n_draw) return;     // (whole groups leave; nothing below needs a block barrier)
  Grp<J> g;
  g.lds = lds + (tid >> 3) * GroupLds<J>::S;
  g.r = tid & 7;
  g.live = g.r < J;
  const int c = (int)(unit / op.n_draw);
  tree_item_group<J, ADJ, DOWN>(op, state, c, unit - (int64_t)c * op.n_draw, g);
}

// the adjoint elements (B') part 1 on groups of eight lanes, 32 draws per block (badj_prep_group; J = 7, 8)
// From J = 7: one lane per (draw, chunk) holds 512 registers + 1.8 KB of scratch there (137 us at the C5 shape, J = 8: this kernel
// ~35); at J = 6 the one-lane kernel takes all 65 408 units in one round of 40 us and THIS one, four rounds of two waves per SIMD,
// was slower (C5 1.895 -> 1.948 ms).
#ifndef EXO_GP_BADJ_GROUP_MIN_J
#define EXO_GP_BADJ_GROUP_MIN_J 7
#endif
template <int J>
__global__ __launch_bounds__(kScanBlock, EXO_GROUP_WAVES) void celerite_badj_prep_group_kernel(const double* __restrict__ gloglike, int64_t n,
                                                                                             int64_t n_draw, double* state, ChunkGeom cg,
                                                                                             const int32_t* __restrict__ row) {
  __shared__ double lds[(kScanBlock / 8) * GroupLds<J>::S];
  const int tid = threadIdx.x;
  const int64_t unit = (int64_t)blockIdx.x * (kScanBlock / 8) + (tid >> 3);
  if (unit >= (int64_t)(cg.C - 1) * n_draw) return;     // (whole groups leave; nothing below needs a block barrier)
  Grp<J> g;
  g.lds = lds + (tid >> 3) * GroupLds<J>::S;
  g.r = tid & 7;
  g.live = g.r < J;
  const int c = (int)(unit / n_draw) + 1;
  badj_prep_group<J>(gloglike, state, chunk_ws(n, n_draw, J, cg), c, unit - (int64_t)(c - 1) * n_draw, g, row);
}

// the narrow top of a scan as a serial chain on groups of eight lanes, 32 draws per block (tree_serial_group; J >= 3)
template <int J, bool ADJ>
__global__ __launch_bounds__(kScanBlock, EXO_GROUP_WAVES) void celerite_tree_serial_group_kernel(TreeOp op, double* state) {
  __shared__ double lds[(kScanBlock / 8) * GroupLds<J>::S];
  const int tid = threadIdx.x;
  const int64_t draw = (int64_t)blockIdx.x * (kScanBlock / 8) + (tid >> 3);
  if (draw >= op.n_draw) return;     // (whole groups leave; nothing below needs a block barrier)
  Grp<J> g;
  g.lds = lds + (tid >> 3) * GroupLds<J>::S;
  g.r = tid & 7;
  g.live = g.r < J;
  tree_serial_group<J, ADJ>(op, state, draw, g);
}


// the state the forward scan starts from: F = 0, P = Delta(t_0) (S_0 = 0)
template <int J>
__global__ __launch_bounds__(kWave) void celerite_scan_init_kernel(const double* __restrict__ t, Coefs cf, int64_t n_draw,
                                                                   double* __restrict__ dst) {
  constexpr int G = Group<J>::G;
  const int j = threadIdx.x & (G - 1);
  const int64_t draw = ((int64_t)blockIdx.x * kWave + threadIdx.x) / G;
  if (draw >= n_draw) return;
  if (J <= kLaneMaxJ) {
    // the one-lane path's own Delta (DeltaCoef: joint covariance of an over-damped SHO's pair of real terms included);
    // LaneDelta below serves the lane-group kernels (J = 7, 8), where such pairs stay flagged
    if (j == 0) scan_init_lane<J>(t, cf, n_draw, dst, draw);
    return;
  }
  const LaneCoef k = lane_coef(cf, draw, j, J);
  if (!k.live) return;
  const LaneDelta ld(k);
  double U_, V_, cs, sn, Prow[J];
  lane_uv(k, t[0], &U_, &V_, &cs, &sn);
  ld.row<J>(k, j, cs, sn, Prow);
  dst[(int64_t)j * n_draw + draw] = 0.0;
#pragma unroll
  for (int l = 0; l < J; ++l) dst[(int64_t)(J + j * J + l) * n_draw + draw] = Prow[l];
}

// ---- the ROBUST route (draws flagged kFlagRobust: exo_celerite_core.hpp, chunk_adj_lane) ---------------------------------
// (B) once more for those draws alone, as a serial chain over the chunks: a draw on one group of eight lanes for J >= 3
// (robust_fwd_chain_group), on one lane below.  Launched after the trees, whose boundary states of these draws it replaces.
template <int J>
__global__ __launch_bounds__(kWave) void celerite_robust_scan_kernel(const double* __restrict__ t, Coefs cf, int64_t n,
                                                                     ChunkGeom cg, int64_t n_draw, double* state) {
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  if constexpr (J >= 3) {
    __shared__ double lds[(kWave / 8) * ChainLds<J>::S];
    const int64_t draw = (int64_t)blockIdx.x * (kWave / 8) + (threadIdx.x >> 3);
    const bool mine = draw < n_draw && state[ws.off_flag() + (draw < n_draw ? draw : 0)] == kFlagRobust;
    if (__ballot(mine) == 0) return;
    if (!mine) return;     // (whole groups leave: nothing below needs a block barrier)
    robust_fwd_chain_group<J>(ws, state, draw, lds + (threadIdx.x >> 3) * ChainLds<J>::S, (int)(threadIdx.x & 7));
  } else {
    const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (draw >= n_draw || state[ws.off_flag() + draw] != kFlagRobust) return;
    bscan_lane<J>(t, cf, n, n_draw, state, cg, draw);
  }
}

// (B) once more for those draws as NEWTON ITERATIONS from the trees' states (exo_celerite_group.hpp, tan_linearise): one block per
// draw -- it leaves at once unless the draw is flagged kFlagRobust -- walks, per iteration, the level-0 items (tangent elements
// of the chunks at the current guess, composed pairwise), the levels of the corrections' scan up and down, and the level-0
// items again (corrections added), a block barrier between levels.  J >= 3; replaces the serial chain above (kept behind
// EXO_GP_ROBUST_NEWTON = 0: 1.34 ms at C5 against ~0.5).
#ifndef EXO_GP_ROBUST_NEWTON
#define EXO_GP_ROBUST_NEWTON 1
#endif
// Iterations: until one's corrections were below EXO_GP_NEWTON_TOL of the states (the next guess is then right to the square
// of that), at most EXO_GP_NEWTON_ITERS (tools/gp_lab_newton.py, 450 chunks, scores of 1e7 .. 1e8: the guess is off by up to
// 4e-2, one iteration leaves 4e-7, two 8e-9 -- the serial chain's own distance from the long-double definition)
#ifndef EXO_GP_NEWTON_ITERS
#define EXO_GP_NEWTON_ITERS 4
#endif
#ifndef EXO_GP_NEWTON_TOL
#define EXO_GP_NEWTON_TOL 1e-8
#endif
#ifndef EXO_GP_NEWTON_BLOCK
#define EXO_GP_NEWTON_BLOCK 256   // (512: 64 items at a time, but 256 registers a lane -- scratch at J = 6 -- and 0.54 ms against 0.43)
#endif
constexpr int kNewtonBlock = EXO_GP_NEWTON_BLOCK;   // threads of a draw's block: 8 per item of a level
template <int J>
__global__ __launch_bounds__(kNewtonBlock) void celerite_robust_newton_kernel(int64_t n, ChunkGeom cg, int64_t n_draw, double* state) {
  __shared__ double lds[(kNewtonBlock / 8) * GroupLds<J>::S];
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const int64_t draw = blockIdx.x;
  if (state[ws.off_flag() + draw] != kFlagRobust) return;     // (the whole block)
  const int tid = threadIdx.x, unit = tid >> 3, n_unit = kNewtonBlock / 8;
  Grp<J> g;
  g.lds = lds + unit * GroupLds<J>::S;
  g.r = tid & 7;
  g.live = g.r < J;
  const int top = ws.tree_top(), n1 = ws.tree_npos(1);
  __shared__ double s_err[kNewtonBlock / kWave];
  bool converged = false;
  for (int it = 0; it < EXO_GP_NEWTON_ITERS; ++it) {
    for (int i = unit; i < n1; i += n_unit) newton_up0<J>(ws, state, i, draw, g);
    __syncthreads();
    for (int f = 1; f + 1 < top; ++f) {
      const TreeOp op = scan_level_op(ws, J, false, f, false);
      for (int c = unit; c < op.n_item; c += n_unit) newton_item<J, false>(op, state, c, draw, g);
      __syncthreads();
    }
    {   // nothing to correct in front of the first chunk
      const int64_t seed = ws.tree_state(top);
      for (int k = tid; k < J + J * J; k += kNewtonBlock) state[seed + (int64_t)k * n_draw + draw] = 0.0;
    }
    __syncthreads();
    for (int f = top - 1; f >= 1; --f) {
      const TreeOp op = scan_level_op(ws, J, false, f, true);
      for (int c = unit; c < op.n_item; c += n_unit) newton_item<J, true>(op, state, c, draw, g);
      __syncthreads();
    }
    double err = 0.0;
    for (int i = unit; i < n1; i += n_unit) err = fmax(err, newton_down0<J>(ws, state, i, draw, g));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) err = fmax(err, __shfl_xor(err, m, 64));
    if ((tid & 63) == 0) s_err[tid >> 6] = err;
    __syncthreads();
    double all = 0.0;
#pragma unroll
    for (int w = 0; w < kNewtonBlock / kWave; ++w) all = fmax(all, s_err[w]);
    __syncthreads();
    if (all < EXO_GP_NEWTON_TOL) { converged = true; break; }     // (the same verdict in every thread)
  }
  // not there after the last iteration, or a NaN on the way (a guess the iterations could not start from): the elements applied
  // one after the other -- the serial chain needs no guess -- by the block's first eight lanes
  if (!converged && tid < 8) {
    static_assert(ChainLds<J>::S <= (kNewtonBlock / 8) * GroupLds<J>::S, "the chain's strip inside the block's LDS");
    robust_fwd_chain_group<J>(ws, state, draw, lds, tid);
  }
}

}  // namespace
