// exo_celerite_lane.hpp -- one lane per draw / per (draw, chunk): the kernels around the lane functions of
// exo_celerite_core.hpp, with the choice of a wave's term layout; the order in which their blocks take the chunks of a
// sparse model and the order of its draws; the sums over the chunks; dot_tril and predict; the partition of a batch by pair
// kind and the three J = 2 kernels that run the layout variants in one launch.
#pragma once
#include "exo_celerite_scan.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// One lane per draw / per (draw, chunk): thin wrappers over exo_celerite_core.hpp (the same
// functions the host harness of tests/ runs lane by lane).  Lanes of a wave are consecutive draws,
// the chunk is blockIdx.y: every access to the chunk workspace and to the checkpoints is coalesced.
// ---------------------------------------------------------------------------------------------
// Term layouts (exo_celerite_core.hpp, DeltaCoef): NR >= 0 -- the first NR state indices are real
// terms, the rest complex pairs -- is a compile-time constant of the kernel; NR = -1 decides per index
// at run time.  Every variant is a kernel of its own (its own register budget); a wave votes on the
// layout of its draws (layout_vote) and returns at once from the variants it did not vote for, so the
// host may launch several variants of one step when pair kinds are given per draw.
// J = 4 (two SHO terms, a RotationTerm): the all-complex layout as kernels OF ITS OWN (launched beside the run-time-layout ones;
// a wave runs the one it voted for).  Inside one kernel -- as J = 6, 8 have it -- the registers are those of the heavier
// run-time layout: forward 204 against 162 (two waves per SIMD against three), and element / reverse sit 14 / 24 registers above
// the 256 of TWO waves per SIMD, which they are held to here (EXO_J4_WAVES): a 1024-draw batch is 4096 waves -- four rounds of
// resident waves at one per SIMD, two at two.
#ifndef EXO_J4_SPLIT
#define EXO_J4_SPLIT 1
#endif
#ifndef EXO_J4_WAVES
#define EXO_J4_WAVES 2
#endif
constexpr bool split_layouts(int J) { return EXO_J4_SPLIT && J == 4; }
// (J <= 2: four waves per SIMD without the look-ahead load of the next block -- elem_lane's PREFETCH)
#ifndef EXO_ELEM_MIXED_WAVES
#define EXO_ELEM_MIXED_WAVES 4
#endif
// which chunk a block of the one-lane kernels works on.  Dense series: every wave costs the same, blocks in order.  SPARSE
// model: a wave is slow exactly while one of its 64 draws is inside a transit (+ 21 % per block: measured with every block
// forced onto either path), so the chunks that hold a transit are the long ones.  They are dealt FIRST (longest processing
// time first) and the short ones fill the tail of the launch: celerite_sparse_order_kernel writes the order.
// EXO_SPARSE_LPT=0: always in order.
#ifndef EXO_SPARSE_LPT
#define EXO_SPARSE_LPT 1
#endif
template <int SP>
__device__ __forceinline__ int chunk_of_block(const double* __restrict__ state, int64_t n, int64_t n_draw, int J, const ChunkGeom& cg) {
  const int y = (int)blockIdx.y;
  if (SP != 1 || !EXO_SPARSE_LPT) return y;
  return reinterpret_cast<const int32_t*>(state + chunk_ws(n, n_draw, J, cg).off_order())[y];
}
// One block: a chunk is LONG if a segment of one of a few sample draws (spread over the batch: with the draws sorted by
// transit time -- exo_sparse_model.row_of_draw -- the first, the last and those between span the transit times of all) reaches
// into it, widened by a block either side; long chunks first, each class in order of time (a stable partition).
constexpr int kOrderSamples = 8, kOrderSegs = 512;
__global__ __launch_bounds__(256) void celerite_sparse_order_kernel(SparseSegs sp, int64_t n, int64_t n_draw, ChunkGeom cg,
                                                                    int32_t* __restrict__ order) {
  __shared__ int s_long[1024 + 1];
  // the sample draws' segments, staged once: the searches below are dependent loads -- from global memory 8 x ~6 of them per
  // chunk made this kernel 43 us of the C3 step; from LDS ~8 (a draw with more than kOrderSegs segments is searched in place)
  __shared__ int s_lo[kOrderSamples][kOrderSegs], s_hi[kOrderSamples][kOrderSegs], s_n[kOrderSamples];
  {   // (32 threads per sample draw: the eight chains row -> count -> segments run side by side)
    static_assert(kOrderSamples * 32 == 256, "a group of 32 threads per sample");
    const int q = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t d = n_draw <= kOrderSamples ? (q < n_draw ? q : n_draw - 1) : (n_draw - 1) * q / (kOrderSamples - 1);
    const int64_t row = sp.row(d);
    const int32_t* sg = sp.seg + row * sp.seg_row;
    const int ns = sp.nseg[row];
    if (l == 0) s_n[q] = ns;
    if (ns <= kOrderSegs)
      for (int i = l; i < ns; i += 32) {
        s_lo[q][i] = sg[(int64_t)i * sp.seg_step];
        s_hi[q][i] = sg[(int64_t)i * sp.seg_step + sp.hi_at];
      }
  }
  __syncthreads();
  const int C = cg.C;
  for (int c0 = 0; c0 < C; c0 += 1024) {     // (plans hold at most 1024 chunks; written for any number)
    const int m = C - c0 < 1024 ? C - c0 : 1024;
    for (int i = threadIdx.x; i < m; i += 256) {
      const int c = c0 + i;
      const int64_t lo = (int64_t)c * cg.L - kCkptB, hi = ((int64_t)(c + 1) * cg.L < n ? (int64_t)(c + 1) * cg.L : n) + kCkptB;
      bool lng = false;
      for (int q = 0; q < kOrderSamples && !lng; ++q) {
        const int ns = s_n[q];
        int a = 0, b = ns;                      // the first segment that ends beyond lo
        if (ns <= kOrderSegs) {
          while (a < b) {
            const int mid = (a + b) >> 1;
            if (s_hi[q][mid] <= lo) a = mid + 1; else b = mid;
          }
          lng = a < ns && s_lo[q][a] < hi;
        } else {
          const int64_t d = n_draw <= kOrderSamples ? (q < n_draw ? q : n_draw - 1) : (n_draw - 1) * q / (kOrderSamples - 1);
          const int32_t* sg = sp.seg + sp.row(d) * sp.seg_row;
          while (a < b) {
            const int mid = (a + b) >> 1;
            if (sg[(int64_t)mid * sp.seg_step + sp.hi_at] <= lo) a = mid + 1; else b = mid;
          }
          lng = a < ns && sg[(int64_t)a * sp.seg_step] < hi;
        }
      }
      s_long[i] = lng ? 1 : 0;
    }
    __syncthreads();
    {   // stable partition, long chunks first: every thread four consecutive flags, an exclusive scan of the counts over the block
      __shared__ int s_cnt[256];
      const int i0 = threadIdx.x * 4;
      int mine = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) mine += (i0 + u < m) ? s_long[i0 + u] : 0;
      s_cnt[threadIdx.x] = mine;
      __syncthreads();
      for (int off = 1; off < 256; off <<= 1) {
        const int add = threadIdx.x >= off ? s_cnt[threadIdx.x - off] : 0;
        __syncthreads();
        s_cnt[threadIdx.x] += add;
        __syncthreads();
      }
      const int n_long = s_cnt[255];
      int at_long = c0 + s_cnt[threadIdx.x] - mine;            // long chunks before this thread's
      int at_short = c0 + n_long + (i0 < m ? i0 : m) - (s_cnt[threadIdx.x] - mine);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u < m) {
          if (s_long[i0 + u]) order[at_long++] = c0 + i0 + u; else order[at_short++] = c0 + i0 + u;
        }
    }
    __syncthreads();
  }
}
// the order of the draws of a sparse model by the spacing of their segments (exo_sparse_model_order)
constexpr int kOrderMaxDraws = EXO_SPARSE_ORDER_MAX_DRAWS;
__global__ __launch_bounds__(1024) void celerite_draw_order_kernel(SparseSegs sp, int64_t n_draw, int32_t* __restrict__ order) {
  __shared__ double s_key[kOrderMaxDraws];
  __shared__ int s_idx[kOrderMaxDraws];
  int M = 1;
  while (M < n_draw) M <<= 1;
  for (int i = threadIdx.x; i < M; i += 1024) {
    double key = INFINITY;
    if (i < n_draw) {
      const int32_t* sg = sp.seg + (int64_t)i * sp.seg_row;
      const int ns = sp.nseg[i];
      const double first = ns > 0 ? (double)sg[0] : 0.0;
      const double last = ns > 0 ? (double)sg[(int64_t)(ns - 1) * sp.seg_step] : 0.0;
      key = (last - first) / (double)(ns > 1 ? ns - 1 : 1) + 1e-9 * first;
    }
    s_key[i] = key;
    s_idx[i] = i;
  }
  __syncthreads();
  // (ranking every key against all others -- no barriers -- was tried for small batches: 45 us at 1024 draws against 23: the block
  // is one CU, 5 instructions x n_draw per key)
  if (M <= 1024) {
    // one element per thread, in registers: the steps inside a wave (partner = lane ^ j, j < 64: 45 of the 55 steps at 1024 draws)
    // are shuffles -- no LDS, no barrier -- and only the ten across waves go through LDS (23 -> 12 us)
    const int i = threadIdx.x;
    double key = i < M ? s_key[i] : INFINITY;
    int idx = i < M ? s_idx[i] : i;
    for (int k = 2; k <= M; k <<= 1)
      for (int j = k >> 1; j >= 1; j >>= 1) {
        double kp;
        int ip;
        if (j >= 64) {
          __syncthreads();
          if (i < M) { s_key[i] = key; s_idx[i] = idx; }
          __syncthreads();
          kp = i < M ? s_key[i ^ j] : INFINITY;
          ip = i < M ? s_idx[i ^ j] : i;
        } else {
          kp = __shfl_xor(key, j, 64);
          ip = __shfl_xor(idx, j, 64);
        }
        const bool lower = (i & j) == 0;                         // I am the lower index of the pair
        const bool mine_after = key > kp || (key == kp && idx > ip);
        const bool asc = (i & k) == 0;
        // the pair in ascending order puts the smaller at the lower index; descending the other way round
        const bool take = lower ? (mine_after == asc) : (mine_after != asc);
        if (take) { key = kp; idx = ip; }
      }
    if (i < n_draw) order[i] = idx;
    return;
  }
  for (int k = 2; k <= M; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int i = threadIdx.x; i < M; i += 1024) {
        const int p = i ^ j;
        if (p > i) {
          const double ka = s_key[i], kb = s_key[p];
          const int ia = s_idx[i], ib = s_idx[p];
          const bool a_after_b = ka > kb || (ka == kb && ia > ib);
          if (a_after_b == ((i & k) == 0)) { s_key[i] = kb; s_key[p] = ka; s_idx[i] = ib; s_idx[p] = ia; }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < n_draw; i += 1024) order[i] = s_idx[i];
}
// (A) the filtering element of every (draw, chunk)
template <int J, int NR, int SP>
__global__ __launch_bounds__(kWave, (J <= 2 ? EXO_ELEM_MIXED_WAVES : (split_layouts(J) && NR == 0 ? EXO_J4_WAVES : 1))) void celerite_elem_kernel(const double* __restrict__ t, Series rs,
                                                              const double* __restrict__ diag, int64_t n_diag, int64_t n,
                                                              Coefs cf, int64_t n_draw, double* __restrict__ state,
                                                              ChunkGeom cg, int64_t flag_at) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  const int vote = layout_vote<J>(cf, draw);
  if constexpr (J > 2 && NR == -1 && EXO_GP_WIDE_COMPLEX_LAYOUT && !split_layouts(J)) {   // a wave of all-complex draws takes the compile-time layout
    if (vote == 0) { elem_lane<J, 0, true, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, chunk_of_block<SP>(state, n, n_draw, J, cg), flag_at); return; }
  } else if (vote != NR) return;
  elem_lane<J, NR, (J > 2 || EXO_ELEM_MIXED_WAVES < 4), SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, chunk_of_block<SP>(state, n, n_draw, J, cg), flag_at);
}

// (B), (B'): the scans over the chunks are trees of compositions (celerite_tree_kernel, celerite_compose_lds_kernel above).
// (B') part 1: the adjoint elements, all chunks in parallel (chunk 0's entering adjoint is never needed)
template <int J>
__global__ __launch_bounds__(kWave) void celerite_badj_prep_kernel(const double* __restrict__ gloglike, int64_t n,
                                                                   int64_t n_draw, double* __restrict__ state,
                                                                   ChunkGeom cg, const int32_t* __restrict__ row) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  badj_prep_lane<J>(gloglike, n, n_draw, state, cg, draw, (int)blockIdx.y + 1, row);
}

// (C) / (C') with a checkpointed factorisation, J <= kLaneMaxJ
template <int J, int NR, int SP>
__global__ __launch_bounds__(kWave, (split_layouts(J) && NR == 0 ? 3 : 1)) void celerite_chunk1_fwd_kernel(const double* __restrict__ t, Series rs,
                                                                    const double* __restrict__ diag, int64_t n_diag,
                                                                    int64_t n, Coefs cf, int64_t n_draw,
                                                                    double* __restrict__ state, ChunkGeom cg) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  const int vote = layout_vote<J>(cf, draw);
  if constexpr (J > 2 && NR == -1 && EXO_GP_WIDE_COMPLEX_LAYOUT && !split_layouts(J)) {
    if (vote == 0) { chunk1_fwd_lane<J, 0, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, chunk_of_block<SP>(state, n, n_draw, J, cg), true); return; }
  } else if (vote != NR) return;
  chunk1_fwd_lane<J, NR, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, chunk_of_block<SP>(state, n, n_draw, J, cg), true);
}
// (two waves per SIMD asked for: the J = 2 complex-term variant sits at 254 + 4 registers otherwise -- one wave)
#ifndef EXO_VJP1_WAVES
#define EXO_VJP1_WAVES 2
#endif
#ifndef EXO_VJPP_WAVES
#define EXO_VJPP_WAVES 2
#endif
template <int J, int NR, int SP>
__global__ __launch_bounds__(kWave, (J < EXO_SPAN2_MIN_J ? EXO_VJP1_WAVES : (J <= 2 ? EXO_VJPP_WAVES : (split_layouts(J) && NR == 0 ? EXO_J4_WAVES : 1)))) void celerite_chunk1_vjp_kernel(const double* __restrict__ t, Series rs,
                                                                    const double* __restrict__ diag, int64_t n_diag,
                                                                    int64_t n, Coefs cf, int64_t n_draw,
                                                                    const double* __restrict__ gloglike,
                                                                    double* __restrict__ state, ChunkGeom cg,
                                                                    double* __restrict__ gresid, double* __restrict__ gdiag,
                                                                    double gsign) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  const int vote = layout_vote<J>(cf, draw);
  constexpr bool kBoth = J > 2 && NR == -1 && EXO_GP_WIDE_COMPLEX_LAYOUT && !split_layouts(J);   // (both layouts in this kernel)
  if (!kBoth && vote != NR) return;
  if constexpr (J >= EXO_SPAN2_MIN_J) {   // wide states: packed adjoint, two checkpoints per block, cotangent accumulators in LDS columns
    __shared__ double gacc[4 * J + 1][kWave];
    if constexpr (kBoth) {
      if (vote == 0) {
        chunkp_vjp_lane<J, 0, SP>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, gresid, gdiag, gsign, draw, chunk_of_block<SP>(state, n, n_draw, J, cg),
                              &gacc[0][threadIdx.x], kWave);
        return;
      }
    }
    chunkp_vjp_lane<J, NR, SP>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, gresid, gdiag, gsign, draw, chunk_of_block<SP>(state, n, n_draw, J, cg),
                           &gacc[0][threadIdx.x], kWave);
  } else
    chunk1_vjp_lane<J, NR, SP>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, gresid, gdiag, gsign, draw, chunk_of_block<SP>(state, n, n_draw, J, cg));
}

// (B') part 1 for those draws: the adjoint scan's inputs from the chunks' own reverse recurrences (chunk_adj_lane), written
// over the chunk's element where badj_prep_lane wrote its own -- launched between that kernel and the adjoint trees, which take
// them as they are.  A WAVE per (draw, chunk >= 1): the chunk's reverse sweep in eight pieces, a piece on a group of eight
// lanes (chunk_adj_lane's roles: the state adjoints, the J columns of X, R), the pieces' records multiplied back together
// through LDS (adj_combine_lane).  Nothing but latency -- 1.2 ms for a 127-cadence chunk on one lane at J = 6, 0.7 ms on eight
// lanes by roles, ~0.2 ms in eight pieces.  A block looks at its draws' flags and, almost always, leaves at once.
constexpr int kAdjDraws = 32;   // (8: 14 us of empty blocks for a clean batch of the C3 shape; 64: a batch of nothing but such draws 64 deep)
template <int J>
__global__ __launch_bounds__(kWave) void celerite_chunk_adj_kernel(const double* __restrict__ t, Series rs,
                                                                   const double* __restrict__ diag, int64_t n_diag, int64_t n,
                                                                   Coefs cf, int64_t n_draw, const double* __restrict__ gloglike,
                                                                   double* __restrict__ state, ChunkGeom cg) {
  static_assert(J + 2 <= 8, "roles 0 .. J + 1 on the eight lanes of a group");
  constexpr int kRec = adj_record_doubles<J>(), kPieces = kWave / 8;
  __shared__ double rec[kPieces * kRec];
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  // (a block looks at kAdjDraws consecutive draws: a batch of nothing but such draws works them kAdjDraws deep, a clean batch
  // pays (C - 1) n_draw / kAdjDraws empty blocks -- ~5 us at the C3 shape)
  const int64_t d0 = (int64_t)blockIdx.y * kAdjDraws, dl = d0 + threadIdx.x;
  const bool look = threadIdx.x < kAdjDraws && dl < n_draw;
  unsigned long long todo = __ballot(look && state[ws.off_flag() + (look ? dl : 0)] == kFlagRobust);
  const int c = 1 + (int)blockIdx.x, piece = (int)(threadIdx.x >> 3), role = (int)(threadIdx.x & 7);
  while (todo) {
    const int64_t draw = d0 + (__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    // (every lane has the same draw: the "vote" is that draw's layout -- the compile-time ones cost a quarter fewer instructions)
    if (role <= J + 1)
      with_layout<J>(cf, draw, [&](auto nr) {
        chunk_adj_lane<J, decltype(nr)::value, false>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, draw, c, role, piece,
                                                      kPieces, rec + piece * kRec, 1);
      });
    asm volatile("" ::: "memory");   // (one wave: its LDS operations execute in order; the compiler must keep them so)
    __builtin_amdgcn_wave_barrier();
    if (threadIdx.x == 0) adj_combine_lane<J>(rec, kRec, 1, kPieces, n, n_draw, state, cg, draw, c);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// sum over the wave in a fixed order (xor butterfly), result in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Sums over the chunks of [chunk][quantity][draw] arrays (the log-likelihood's partials, the coefficient cotangents'), the DRAWS
// ACROSS THE LANES: a row of 64 draws is 512 contiguous bytes.  (Rounds 2-4: a wave per (draw, quantity) with the chunks across its
// lanes -- every lane its own 64-B sector, 8 useful bytes of it: 52 + 20 us of the C3 step at a tenth of the bandwidth.)  Slice
// blockIdx.z of S adds the rows of chunks s, s + S, s + 2 S ... in order and leaves its partial sum in the slot of chunk s -- the
// first row it read; nobody else touches that row -- and the reader adds the S partials in order (slice_total).  S grows until
// the launch has ~2048 waves (chunk_sum_slices): a pure function of the plan, so a draw's sums do not depend on its neighbours.
__global__ __launch_bounds__(kWave) void celerite_chunk_slice_sum_kernel(double* __restrict__ arr, int K, int C, int S,
                                                                         int64_t n_draw) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  const int k = blockIdx.y, s0 = blockIdx.z;
  const int64_t step = (int64_t)S * K * n_draw;
  double* __restrict__ p = arr + ((int64_t)s0 * K + k) * n_draw + draw;
  const double* __restrict__ q = p;
  double v = 0.0;
  int c = s0;
  for (; c + 7 * S < C; c += 8 * S) {     // eight loads in flight, added in order
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = q[(int64_t)u * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += x[u];
    q += 8 * step;
  }
  for (; c < C; c += S) { v += *q; q += step; }
  *p = v;
}

// O(N) companions (exo_celerite_core.hpp): one lane per draw
template <int J>
__global__ __launch_bounds__(kWave) void celerite_dot_tril_kernel(const double* __restrict__ t,
                                                                  const double* __restrict__ diag, int64_t n_diag, int64_t n,
                                                                  Coefs cf, int64_t n_draw, const double* __restrict__ x,
                                                                  double* __restrict__ z) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  dot_tril_lane<J>(t, diag, n_diag, n, cf, x, z, draw);
}
template <int J>
__global__ __launch_bounds__(kWave) void celerite_predict_kernel(const double* __restrict__ t, int64_t n,
                                                                 const double* __restrict__ alpha, Coefs cf, int64_t n_draw,
                                                                 const double* __restrict__ tq, int64_t m,
                                                                 double* __restrict__ mu) {
  const int64_t draw = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (draw >= n_draw) return;
  predict_lane<J>(t, n, alpha, cf, tq, m, mu, draw);
}

// J = 2 with per-draw pair kinds: which draw a lane of the *_mixed_kernel launches works on.  A wave runs ONE layout, the one
// all its draws share, or the run-time layout (half again as many instructions) -- and the step waits for its slowest wave: a
// batch with 1 % of its draws on the other side of Q = 1/2 cost 1.84 x a clean one for the sake of ONE mixed wave.  So the
// lanes take the draws in an order that has no mixed wave: the complex-term draws, padded to whole waves, then the
// two-real-terms draws (a stable partition: neighbours stay neighbours, the [..][draw] arrays stay coalesced), written into the
// workspace by one small kernel per forward call (the reverse call finds it there).
__device__ __forceinline__ int64_t mixed_draw(const double* __restrict__ state, int64_t n, int64_t n_draw, const ChunkGeom& cg) {
  const ChunkWs ws = chunk_ws(n, n_draw, 2, cg);
  const int32_t* __restrict__ perm = reinterpret_cast<const int32_t*>(state + ws.off_perm());
  return perm[(int64_t)blockIdx.x * kWave + threadIdx.x];      // (the launches cover ws.perm_lanes() lanes)
}
__global__ __launch_bounds__(1024) void celerite_kind_partition_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ row,
                                                                       int64_t n_draw, int32_t* __restrict__ perm, int64_t lanes) {
  __shared__ int s_cnt[2][16];
  __shared__ int s_base[2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int64_t i = tid; i < lanes; i += 1024) perm[i] = -1;
  // the complex-term draws: how many
  int mine = 0;
  for (int64_t d = tid; d < n_draw; d += 1024) mine += kind[row ? row[d] : d] == 0 ? 1 : 0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
  if (lane == 0) s_cnt[0][wave] = mine;
  if (tid < 2) s_base[tid] = 0;
  __syncthreads();
  int c0 = 0;
  for (int w = 0; w < 16; ++w) c0 += s_cnt[0][w];
  const int64_t off1 = ((int64_t)c0 + 63) / 64 * 64;
  __syncthreads();
  for (int64_t d0 = 0; d0 < n_draw; d0 += 1024) {
    const int64_t d = d0 + tid;
    const int k = d < n_draw ? (kind[row ? row[d] : d] == 0 ? 0 : 1) : -1;
    const unsigned long long m0 = __ballot(k == 0), m1 = __ballot(k == 1), below = (1ull << lane) - 1ull;
    if (lane == 0) { s_cnt[0][wave] = __popcll(m0); s_cnt[1][wave] = __popcll(m1); }
    __syncthreads();
    if (k >= 0) {
      int pos = s_base[k] + __popcll((k == 0 ? m0 : m1) & below);
      for (int w = 0; w < wave; ++w) pos += s_cnt[k][w];
      perm[(k == 0 ? 0 : off1) + pos] = (int32_t)d;
    }
    __syncthreads();
    if (tid < 2) {
      int tot = 0;
      for (int w = 0; w < 16; ++w) tot += s_cnt[tid][w];
      s_base[tid] += tot;
    }
    __syncthreads();
  }
}

// J = 2 with per-draw pair kinds (a batch of SHO terms that straddles Q = 1/2): the three layout variants in ONE launch.
// blockIdx.z picks the variant; a wave runs the one it voted for and leaves the other two at once.  Launched one after the
// other (round 2), each variant cost its full single-wave latency however few waves took it: a batch with 1 % of its draws
// on the other side of Q = 1/2 paid twice the clean batch's time.  The layouts keep their own code (compile-time NR); the
// kernel's registers are those of the widest variant -- the same waves per SIMD as each alone (145 / 118 / 159, 113 / 100 /
// 124, 217 / 186 / 239 registers for element / forward / reverse).
template <int SP>
__global__ __launch_bounds__(kWave, EXO_ELEM_MIXED_WAVES) void celerite_elem_mixed_kernel(const double* __restrict__ t, Series rs,
                                                                    const double* __restrict__ diag, int64_t n_diag, int64_t n,
                                                                    Coefs cf, int64_t n_draw, double* __restrict__ state,
                                                                    ChunkGeom cg, int64_t flag_at) {
  const int64_t draw = mixed_draw(state, n, n_draw, cg);
  if (draw < 0) return;
  const int nr = layout_vote<2>(cf, draw);
  const int c = chunk_of_block<SP>(state, n, n_draw, 2, cg);
  if (blockIdx.z == 0) {
    if (nr == 0) elem_lane<2, 0, EXO_ELEM_MIXED_WAVES < 4, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, c, flag_at);
  } else {
    if (nr == 2) elem_lane<2, 2, EXO_ELEM_MIXED_WAVES < 4, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, c, flag_at);
  }   // (no wave is of mixed kinds: mixed_draw)
}
// (four waves per SIMD asked for: the three inlined layouts sit at 129 registers otherwise, and the plan offers four)
#ifndef EXO_FWD_MIXED_WAVES
#define EXO_FWD_MIXED_WAVES 4
#endif
template <int SP>
__global__ __launch_bounds__(kWave, EXO_FWD_MIXED_WAVES) void celerite_chunk1_fwd_mixed_kernel(const double* __restrict__ t, Series rs,
                                                                          const double* __restrict__ diag, int64_t n_diag,
                                                                          int64_t n, Coefs cf, int64_t n_draw,
                                                                          double* __restrict__ state, ChunkGeom cg) {
  const int64_t draw = mixed_draw(state, n, n_draw, cg);
  if (draw < 0) return;
  const int nr = layout_vote<2>(cf, draw);
  const int c = chunk_of_block<SP>(state, n, n_draw, 2, cg);
  if (blockIdx.z == 0) {
    if (nr == 0) chunk1_fwd_lane<2, 0, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, c, true);
  } else {
    if (nr == 2) chunk1_fwd_lane<2, 2, SP>(t, rs, diag, n_diag, n, cf, n_draw, state, cg, draw, c, true);
  }   // (no wave is of mixed kinds: mixed_draw)
}
template <int SP>
__global__ __launch_bounds__(kWave, EXO_VJP1_WAVES) void celerite_chunk1_vjp_mixed_kernel(
    const double* __restrict__ t, Series rs, const double* __restrict__ diag, int64_t n_diag, int64_t n, Coefs cf, int64_t n_draw,
    const double* __restrict__ gloglike, double* __restrict__ state, ChunkGeom cg, double* __restrict__ gresid,
    double* __restrict__ gdiag, double gsign) {
  static_assert(2 < EXO_SPAN2_MIN_J, "the mixed reverse kernel is the J = 2 register-resident form (chunk1_vjp_lane)");
  const int64_t draw = mixed_draw(state, n, n_draw, cg);
  if (draw < 0) return;
  const int nr = layout_vote<2>(cf, draw);
  const int c = chunk_of_block<SP>(state, n, n_draw, 2, cg);
  if (blockIdx.z == 0) {
    if (nr == 0) chunk1_vjp_lane<2, 0, SP>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, gresid, gdiag, gsign, draw, c);
  } else {
    if (nr == 2) chunk1_vjp_lane<2, 2, SP>(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, cg, gresid, gdiag, gsign, draw, c);
  }   // (no wave is of mixed kinds: mixed_draw)
}

}  // namespace
