// exo_celerite_dpp.hpp -- a draw on G adjacent lanes of a wave: the width of the group (Group<J>), the in-register lane
// exchanges (dpp_mov, group_get, xor_get), the all-gather of a group's values (EXO_GROUP_GATHER: DPP broadcasts or one
// trip through LDS) and the sum over a group (group_sum).  What the sequential and the lane-group kernels are written in.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "exo_celerite_core.hpp"
#include "exo_math.hpp"

namespace {

using namespace gp;

constexpr int kWave = 64;

// A draw is spread over G = next_pow2(J) adjacent lanes: lane j of the group owns
// state index j (row j of the symmetric J x J matrix S, W_j, F_j, U_j, V_j, P_j).
// The sequential chain per cadence then is: one row update (J FMAs), one row-times-
// vector (J FMAs), a log2(G)-step butterfly for the two dot products, one division --
// instead of the whole O(J^2) update on one lane.  A wave carries 64 / G draws.
template <int J>
struct Group {
  static constexpr int G = group_width(J);
};
// which state index and which draw a lane of these kernels has: blocks of one wave, 64 / G draws each.  The lanes past the last
// draw go through the motions on the last draw once more (the exchanges with them stay defined) and store nothing.
template <int G>
struct GroupLane {
  int j;
  int64_t draw;
  bool live_draw;
  __device__ __forceinline__ explicit GroupLane(int64_t n_draw) {
    j = threadIdx.x & (G - 1);
    const int64_t lane_draw = ((int64_t)blockIdx.x * kWave + threadIdx.x) / G;
    live_draw = lane_draw < n_draw;
    draw = live_draw ? lane_draw : n_draw - 1;
  }
};

// In-register lane exchange (DPP) -- an ds_bpermute-based __shfl costs ~100+ cycles of
// latency on the sequential chain; quad_perm / row_shl / row_shr moves cost a few.
// (bound_ctrl: a lane whose source lies outside its row reads 0 -- what `old` = 0 gave; with it the destination needs no
// zero written first: two moves fewer per exchanged double, a fifth of a butterfly step)
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
constexpr int kRowShl4 = 0x104, kRowShr4 = 0x114;  // lane i reads lane i+4 / i-4 (same row of 16)
constexpr int kRowShl8 = 0x108, kRowShr8 = 0x118;  // ... i+8 / i-8
constexpr int kRowMirror = 0x140, kRowHalfMirror = 0x141;   // lane i reads lane 15 - i of its row / lane 7 - i of its half row

// value held by the lane at distance 4 inside an aligned group of 8 (lane ^ 4)
__device__ __forceinline__ double xor4(double v) {
  const double up = dpp_mov<kRowShl4>(v), dn = dpp_mov<kRowShr4>(v);
  return (threadIdx.x & 4) ? dn : up;
}

// ... at distance 8 inside an aligned group (= DPP row) of 16 (lane ^ 8)
__device__ __forceinline__ double xor8(double v) {
  const double up = dpp_mov<kRowShl8>(v), dn = dpp_mov<kRowShr8>(v);
  return (threadIdx.x & 8) ? dn : up;
}

// value of `v` held by lane L of this lane's aligned group of G lanes
template <int G, int L>
__device__ __forceinline__ double group_get_c(double v) {
  if (G == 1) return v;
  if (G == 2) return dpp_mov<(L | (L << 2) | ((2 + L) << 4) | ((2 + L) << 6))>(v);
  constexpr int R = L & 3;
  const double q = dpp_mov<R * 0x55>(v);  // every quad broadcasts its own lane R
  if (G == 4) return q;
  // G >= 8: pick this quad's broadcast or the other quad's of the octet
  const double other = xor4(q);
  const double o8 = (((threadIdx.x >> 2) & 1) == ((L >> 2) & 1)) ? q : other;   // every octet broadcasts its own lane L & 7
  if (G == 8) return o8;
  // G == 16: this octet's or the other one's of the row
  const double other8 = xor8(o8);
  return (((threadIdx.x >> 3) & 1) == (L >> 3)) ? o8 : other8;
}

template <int G>
__device__ __forceinline__ double group_get(double v, int l) {
  switch (l) {  // l is a compile-time constant after unrolling; DPP controls are immediates
    case 0: return group_get_c<G, 0>(v);
    case 1: return group_get_c<G, (G > 1 ? 1 : 0)>(v);
    case 2: return group_get_c<G, (G > 2 ? 2 : 0)>(v);
    case 3: return group_get_c<G, (G > 2 ? 3 : 0)>(v);
    case 4: return group_get_c<G, (G > 4 ? 4 : 0)>(v);
    case 5: return group_get_c<G, (G > 4 ? 5 : 0)>(v);
    case 6: return group_get_c<G, (G > 4 ? 6 : 0)>(v);
    case 7: return group_get_c<G, (G > 4 ? 7 : 0)>(v);
    case 8: return group_get_c<G, (G > 8 ? 8 : 0)>(v);
    case 9: return group_get_c<G, (G > 8 ? 9 : 0)>(v);
    case 10: return group_get_c<G, (G > 8 ? 10 : 0)>(v);
    case 11: return group_get_c<G, (G > 8 ? 11 : 0)>(v);
    case 12: return group_get_c<G, (G > 8 ? 12 : 0)>(v);
    case 13: return group_get_c<G, (G > 8 ? 13 : 0)>(v);
    case 14: return group_get_c<G, (G > 8 ? 14 : 0)>(v);
    default: return group_get_c<G, (G > 8 ? 15 : 0)>(v);
  }
}

// integer flavour of group_get
template <int G>
__device__ __forceinline__ int group_get_int(int v, int l) {
  return __double2loint(group_get<G>(__hiloint2double(0, v), l));
}

// ALL-GATHER within a group: out[l] = the value `v` of lane l of this lane's group, l = 0 .. J - 1 (what the recurrences need
// three times per cadence: U, W and the propagators of every state index).  By DPP broadcasts a value costs ~10 vector
// instructions on a group of eight and ~20 on a row of sixteen (quad broadcast, xor-4 and xor-8 exchanges with their selects, twice
// for the two halves of a double): 200 instructions per gather at J = 10 -- most of what the lane-group kernels of the wide states
// issued (round 6: element kernel 4.3 ms of a 12.7 ms step).  Through LDS it is one ds_write_b64 of the wave's 64 values and J / 2
// ds_read_b128 per lane (the lanes of a group read the same addresses: broadcasts).  A block of these kernels is ONE wave, so the
// barriers below are waits on the LDS counter, not s_barrier round trips.  EXO_GATHER_LDS_MIN_G: from which group width on.
// Measured at the C5 shape, 128 chains (tools/ab_gp.py, same box, alternating): rows of sixteen (J = 10) 12.7 -> 9.5 ms; groups of
// eight too: J = 8 5.08 -> 4.66 ms, two chains redone by the sequential kernels (J = 6 on eight lanes) 182 -> 170 ms.  Pure data
// movement: results bit for bit.  Groups of four and two keep the DPP moves (a quad broadcast is one instruction).
#ifndef EXO_GATHER_LDS_MIN_G
#define EXO_GATHER_LDS_MIN_G 8
#endif
// EXO_GATHER_SYNC = 0: no barrier at all.  A block is one wave, and the LDS operations of ONE wave execute in the order they were
// issued: the reads see the write in front of them, and the next gather's write cannot overtake these reads.  The two
// __syncthreads() this had were each a wait for the LDS counter to drain to zero -- every gather a full write -> read round
// trip with nothing else in flight, 7-9 of them per cadence in the reverse kernel; without them the compiler waits only where
// a value is used, and consecutive gathers overlap.
#ifndef EXO_GATHER_SYNC
#define EXO_GATHER_SYNC 0
#endif
template <int G, int J>
__device__ __forceinline__ void group_gather_lds(double v, double (&out)[J]) {
  __shared__ double s_gather[kWave];
  s_gather[threadIdx.x] = v;
  if (EXO_GATHER_SYNC) __syncthreads(); else __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (the compiler keeps the order too; no instruction)
  const double* __restrict__ base = s_gather + (threadIdx.x & ~(G - 1));
#pragma unroll
  for (int l = 0; l < J; ++l) out[l] = base[l];
  if (EXO_GATHER_SYNC) __syncthreads(); else __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (the next gather overwrites the buffer)
}
// (narrower groups keep the DPP loop exactly as it stood)
#define EXO_GROUP_GATHER(v, out)                                   \
  do {                                                             \
    if constexpr (G >= EXO_GATHER_LDS_MIN_G) {                     \
      group_gather_lds<G, J>(v, out);                              \
    } else {                                                       \
      _Pragma("unroll") for (int l_ = 0; l_ < J; ++l_) (out)[l_] = group_get<G>(v, l_); \
    }                                                              \
  } while (0)

// butterfly partner lane ^ M within the group
template <int M>
__device__ __forceinline__ double xor_get(double v) {
  if (M == 1) return dpp_mov<0xB1>(v);  // quad_perm [1,0,3,2]
  if (M == 2) return dpp_mov<0x4E>(v);  // quad_perm [2,3,0,1]
  if (M == 4) return xor4(v);
  return xor8(v);
}

// sum over the G lanes of a group, result in every lane
// (after the two quad steps every lane of a quad holds the quad's sum, so the partner of the later steps may be ANY lane of the
// other quad / the other half row: the mirrored lane, one DPP move -- lane ^ 4 and lane ^ 8 take a shift each way and a select.
// The same two numbers are added: bit for bit the butterfly's sums.  Five of these per cadence in the reverse kernel.)
template <int G>
__device__ __forceinline__ double group_sum(double v) {
  if (G >= 2) v += xor_get<1>(v);
  if (G >= 4) v += xor_get<2>(v);
  if (G >= 8) v += dpp_mov<kRowHalfMirror>(v);
  if (G >= 16) v += dpp_mov<kRowMirror>(v);
  return v;
}

}  // namespace
