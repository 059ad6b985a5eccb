// exo_celerite_state.hpp -- the saved factorisation: where (d, z), the records (W, F, S row) and the pre-pass's U, V, P of a
// (cadence, draw, state index) lie in the caller's state buffer (StateIdx), the stores / loads of a record and of its
// parts, and at which cadences of a chunk the lane-group kernels keep the S row (lg_span).
#pragma once
#include "exo_celerite_dpp.hpp"

namespace {

// saved-state addressing.  Per (cadence, draw): the pair (d, z), 16 B; per (cadence, draw, j): one
// record (W_j, F_j, S_j0 .. S_j,J-1) of R = 2 + J doubles, stored PLANAR within the cadence: piece q
// of every (draw, j) is contiguous -- [cadence][piece][draw x j], pieces of 16 B for even R, of 8 B
// for odd R (whose cadence stride is not 16-B aligned): record_piece, the one place that says so.  Lanes of a wave are
// consecutive (draw, j), so every load / store instruction of a wave covers one contiguous kilobyte; record-major records
// made each instruction touch 16 B of every lane's record -- partial lines at the memory side.
constexpr int record_piece(int J) { return (2 + J) % 2 == 0 ? 2 : 1; }   // doubles per piece
struct StateIdx {
  int64_t n, n_draw;
  int J;
  __device__ __forceinline__ int64_t scal(int q, int64_t i, int64_t draw) const {  // q = 0 (d), 1 (z)
    return (i * n_draw + draw) * 2 + q;
  }
  // address of piece 0 of the record of (cadence i, draw, j); piece q is q * piece() doubles further
  __device__ __forceinline__ int64_t rec(int64_t i, int64_t draw, int j) const {
    const int64_t lanes = n_draw * J, lane = draw * J + j;
    return 2 * n * n_draw + i * lanes * (int64_t)(2 + J) + record_piece(J) * lane;
  }
  __device__ __forceinline__ int64_t piece() const { return n_draw * J * (int64_t)record_piece(J); }
  // U_n, V_n, P_n (q = 0, 1, 2) written by the parallel pre-pass: the sequential kernels
  // never evaluate a sin, cos or exp
  __device__ __forceinline__ int64_t uvp(int q, int64_t i, int64_t draw, int j) const {
    return (2 + (int64_t)(2 + J) * J) * n * n_draw + (((int64_t)q * n + i) * n_draw + draw) * J + j;
  }
};

// one record (W, F, S row): p = piece 0 (StateIdx::rec), ps = StateIdx::piece().  Non-temporal:
// written once per forward pass, read once by the reverse pass, 10 GB-scale.
template <int J>
__device__ __forceinline__ void store_record(double* __restrict__ p, int64_t ps, double W, double F, const double* S) {
  constexpr int R = 2 + J;
  double v[R];
  v[0] = W; v[1] = F;
#pragma unroll
  for (int l = 0; l < J; ++l) v[2 + l] = S[l];
  typedef double v2d __attribute__((ext_vector_type(2)));
  if (record_piece(J) == 2) {
#pragma unroll
    for (int q = 0; q < R / 2; ++q) {
      const v2d x = {v[2 * q], v[2 * q + 1]};
      __builtin_nontemporal_store(x, reinterpret_cast<v2d*>(p + q * ps));
    }
  } else {
#pragma unroll
    for (int q = 0; q < R; ++q) __builtin_nontemporal_store(v[q], p + q * ps);
  }
}
template <int J>
__device__ __forceinline__ void load_record(const double* __restrict__ p, int64_t ps, double& W, double& F, double* S) {
  constexpr int R = 2 + J;
  double v[R];
  if (record_piece(J) == 2) {
#pragma unroll
    for (int q = 0; q < R / 2; ++q) {
      const double2 x = *reinterpret_cast<const double2*>(p + q * ps);
      v[2 * q] = x.x; v[2 * q + 1] = x.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = p[q * ps];
  }
  W = v[0]; F = v[1];
#pragma unroll
  for (int l = 0; l < J; ++l) S[l] = v[2 + l];
}

// The lane-group CHUNK kernels (celerite_chunk_fwd_kernel / celerite_chunk_vjp_kernel) keep the S row of a record only at every
// lg_span-th cadence of a chunk -- a CHECKPOINT -- and the reverse kernel recomputes the rows in between (one fused multiply-add
// per entry and two all-gathers per cadence): the saved factorisation was 83 doubles per (draw, cadence) at J = 8, 123 at J = 10,
// written at 5.5 and read back at 4.8 TB/s -- both kernels sat on the HBM ceiling at 0.24-0.45 of their issue rate
// (profiles/r06_counters.json, legs j8 / j10).  The records keep their places (pieces 1 .. of the cadences in between are holes
// nobody touches; piece 0 -- (W, F) of every lane -- stays one contiguous run per cadence), so the sequential kernels, which
// write and read every S row of the draws they redo, share the layout unchanged.
// The span is a matter of registers: the reverse kernel holds span rows of J doubles (and span records) on top of its own 170-230,
// and what counts is staying at two waves per SIMD (256 registers): J = 10 with a span of 4 took 268 -- one wave -- and the step went
// from 7.5 to 8.7 ms where J = 8 (240: two waves, down from three) went from 4.04 to 3.59.
#ifndef EXO_LG_SPAN
#define EXO_LG_SPAN 0   // (> 0: that span for every width -- A/B builds)
#endif
template <int J>
constexpr int lg_span() { return EXO_LG_SPAN > 0 ? EXO_LG_SPAN : (J <= 9 ? 4 : (J <= 11 ? 3 : (J <= 14 ? 2 : 1))); }
// (W, F) of a record alone
template <int J>
__device__ __forceinline__ void store_record_wf(double* __restrict__ p, int64_t ps, double W, double F) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  if (record_piece(J) == 2) {
    const v2d x = {W, F};
    __builtin_nontemporal_store(x, reinterpret_cast<v2d*>(p));
  } else {
    __builtin_nontemporal_store(W, p);
    __builtin_nontemporal_store(F, p + ps);
  }
}
template <int J>
__device__ __forceinline__ void load_record_wf(const double* __restrict__ p, int64_t ps, double& W, double& F) {
  if (record_piece(J) == 2) {
    const double2 x = *reinterpret_cast<const double2*>(p);
    W = x.x; F = x.y;
  } else {
    W = p[0]; F = p[ps];
  }
}
// the S row of a record alone
template <int J>
__device__ __forceinline__ void load_record_s(const double* __restrict__ p, int64_t ps, double* S) {
  constexpr int R = 2 + J;
  if (record_piece(J) == 2) {
#pragma unroll
    for (int q = 1; q < R / 2; ++q) {
      const double2 x = *reinterpret_cast<const double2*>(p + q * ps);
      S[2 * q - 2] = x.x; S[2 * q - 1] = x.y;
    }
  } else {
#pragma unroll
    for (int q = 2; q < R; ++q) S[q - 2] = p[q * ps];
  }
}

}  // namespace
