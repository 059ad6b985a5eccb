// exo_predictive.hip -- quantiles along the strided axis of an (S, N) array of curves: the posterior bands of a model over a
// trace's draws (exoplanet_amd/predictive.py; exo_column_quantiles_f64).  No sort, no scratch, no atomics on floating-point
// numbers: selection by counting passes, the arithmetic of exo_predictive_core.hpp (shared with tests/predictive_harness.cpp).
//
// A workgroup of WAVES waves owns a tile of CW adjacent columns and ALL its rows.  A lane owns one column of the tile and a share
// of the rows: lane l of wave w reads column l % CW in the rows (w 64 + l) / CW, + RL, + 2 RL, ... with RL = WAVES 64 / CW rows
// per sweep.  CW = 64: a wave reads 512 contiguous bytes of one row per load; CW = 16 (few columns, many rows): 128 contiguous
// bytes of four rows.  A pass: every lane counts, for its rows, the values below its column's Q K trial values; the counts go
// to LDS as integers, and after a barrier every lane of the column adds up all RL shares and takes the same decision, so the
// search state is held redundantly by the lanes of a column and never communicated.  A pass settles B bits of the interval of
// keys (2^B - 1 trial values per quantile, bits_per_pass).  Passes per tile: one for the count, the minimum and the maximum
// key, ceil(ceil(log2(keys between them)) / B) for the widest column of the tile, one for the next order statistics where a
// position is fractional.  A grid of fewer workgroups than tiles walks the tiles (grid_for: how
// many tiles are in flight at once decides which cache serves the passes).  Layout, resources, times: DESIGN.md section 24.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_predictive_core.hpp"

namespace {

using namespace predictive;

static_assert(kMaxQ == EXO_QUANTILE_MAX_Q, "the header's constant is the core's");

constexpr int kWave = 64;

#ifndef EXO_PRED_TILE_BUDGET_MIB
#define EXO_PRED_TILE_BUDGET_MIB 192   // tiles in flight are kept below this many MiB where that leaves enough workgroups
#endif
#ifndef EXO_PRED_MIN_GRID
#define EXO_PRED_MIN_GRID 256          // ... but never fewer workgroups than this (one per compute unit)
#endif
#ifndef EXO_PRED_WIDE_TILES
#define EXO_PRED_WIDE_TILES 256        // 64-column tiles from this many on; below, 16-column tiles (four times as many)
#endif
#ifndef EXO_PRED_TALL_ROWS
#define EXO_PRED_TALL_ROWS 512         // 16 waves (8 for more than three quantiles) share a tile's rows from this many on; below, 4
#endif

struct Fractions {
  int64_t num[kMaxQ], den[kMaxQ];
};

// bytes of LDS per thread: a pass's Q counters; the first pass's count and two keys, and behind them the tile's two words (what
// the 24 is for); a (count, value) pair of the last pass
template <int Q>
constexpr int lds_per_thread() { return Q * 4 > 24 ? Q * 4 : 24; }   // (Q: counters per lane)

// bits of a column's key interval settled per pass: 2^B - 1 trial values per quantile, as many as the registers of a lane hold
// beside its loads in flight (16 waves: 128 registers) -- a pass waits for memory, not for its comparisons
template <int Q>
constexpr int bits_per_pass() { return Q == 1 ? 3 : Q <= 3 ? 2 : 1; }

template <int CW, int WAVES, int Q>
__global__ __launch_bounds__(WAVES* kWave) void column_quantiles_kernel(const double* __restrict__ x, int64_t n_rows, int64_t n_cols,
                                                                        int64_t row_stride, Fractions fr, int n_q, int64_t n_tiles,
                                                                        double* __restrict__ out, int32_t* __restrict__ n_valid) {
  constexpr int T = WAVES * kWave;   // threads
  constexpr int B = bits_per_pass<Q>(), K = (1 << B) - 1, QK = Q * K;
  constexpr int kUnroll = Q <= 3 ? 8 : 1;   // loads in flight per lane (Q = 16: the state of sixteen bisections fills the registers)
  constexpr int RL = T / CW;         // rows per sweep of the workgroup
  __shared__ __attribute__((aligned(8))) unsigned char lds[T * lds_per_thread<QK>()];
  int32_t* const sh_i = (int32_t*)lds;                       // [Q K or 1][T]
  uint64_t* const sh_k = (uint64_t*)(lds + 4 * T);           // [2][T] (behind one row of counts)
  double* const sh_d = (double*)(lds + 4 * T);               // [T]
  int32_t& tile_passes = *(int32_t*)(lds + 20 * T);          // (the first pass only)
  int32_t& tile_two = *(int32_t*)(lds + 20 * T + 4);
  const int t = threadIdx.x;
  const int cc = t % CW, rl = t / CW;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t col = tile * CW + cc;
    const bool live = col < n_cols;
    // (a lane past the last column reads the last column and writes nothing: the loops below stay uniform)
    const Column v{x + (live ? col : n_cols - 1), row_stride};

    // ---- pass 0: the count and the extreme keys
    Extent own = extent_empty();
#pragma unroll kUnroll
    for (int64_t i = rl; i < n_rows; i += RL) extent_add(own, v[i]);
    if (t == 0) tile_passes = 0, tile_two = 0;
    sh_i[t] = own.m;
    sh_k[t] = own.kmin;
    sh_k[T + t] = own.kmax;
    __syncthreads();
    Extent e = extent_empty();
#pragma unroll 4
    for (int j = 0; j < RL; ++j) extent_merge(e, sh_i[j * CW + cc], sh_k[j * CW + cc], sh_k[T + j * CW + cc]);
    Rank rank[Q];
    bool two = false;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      rank[q] = e.m ? rank_of(e.m, fr.num[q], fr.den[q]) : Rank{0, 0};
      two = two || rank[q].rem != 0;
    }
    Bisect<Q> s;
    bisect_begin<Q>(s, e, rank);
    // the widest column of the tile sets the number of passes (integers in LDS)
    if (rl == 0) {
      atomicMax(&tile_passes, passes_needed(e, B));
      if (two) atomicOr(&tile_two, 1);
    }
    __syncthreads();
    const int need = tile_passes;
    const bool any_two = tile_two != 0;
    __syncthreads();   // (the counters of the passes below reuse these bytes)

    // ---- the bisection: Q trial values and Q counters per lane, one sweep of the tile per pass
    for (int pass = 0; pass < need; ++pass) {
      double trial[QK];
      int32_t c[QK];
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < K; ++j) {
          trial[q * K + j] = bisect_trial<K>(s, q, j + 1);
          c[q * K + j] = 0;
        }
#pragma unroll kUnroll
      for (int64_t i = rl; i < n_rows; i += RL) {
        const double vi = v[i];
#pragma unroll
        for (int u = 0; u < QK; ++u) c[u] += (vi < trial[u]) ? 1 : 0;
      }
#pragma unroll
      for (int u = 0; u < QK; ++u) sh_i[u * T + t] = c[u];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        int32_t sum[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          sum[j] = 0;
#pragma unroll 4
          for (int r = 0; r < RL; ++r) sum[j] += sh_i[(q * K + j) * T + r * CW + cc];
        }
        bisect_decide<K>(s, q, sum);
      }
      __syncthreads();
    }

    // ---- the order statistic after each, where a position is fractional anywhere in the tile
    double a[Q], b[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) a[q] = b[q] = bisect_value<Q>(s, q);
    if (any_two) {
      Next nx[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) nx[q] = Next{0, INFINITY};
#pragma unroll kUnroll
      for (int64_t i = rl; i < n_rows; i += RL) {
        const double vi = v[i];
#pragma unroll
        for (int q = 0; q < Q; ++q) next_add(nx[q], vi, a[q]);
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        sh_i[t] = nx[q].c;
        sh_d[t] = nx[q].up;
        __syncthreads();
        Next all{0, INFINITY};
#pragma unroll 4
        for (int j = 0; j < RL; ++j) next_merge(all, sh_i[j * CW + cc], sh_d[j * CW + cc]);
        b[q] = next_value(all, s.k[q], a[q]);
        __syncthreads();
      }
    }
    if (live && rl == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (q < n_q) out[q * n_cols + col] = e.m ? interpolate(a[q], rank[q].rem ? b[q] : a[q], rank[q].rem, fr.den[q]) : NAN;
      if (n_valid) n_valid[col] = e.m;
    }
    // (every read of LDS above is followed by a barrier: the next tile may write at once)
  }
}

// workgroups for n_tiles tiles of tile_bytes each: all of them, unless that many tiles in flight outgrow the budget -- then as
// many as the budget holds, and at least EXO_PRED_MIN_GRID
int64_t grid_for(int64_t n_tiles, int64_t tile_bytes) {
  int64_t cap = ((int64_t)EXO_PRED_TILE_BUDGET_MIB << 20) / (tile_bytes > 0 ? tile_bytes : 1);
  if (cap < EXO_PRED_MIN_GRID) cap = EXO_PRED_MIN_GRID;
  if (cap > (int64_t(1) << 30)) cap = int64_t(1) << 30;
  return n_tiles < cap ? n_tiles : cap;
}

template <int CW, int WAVES, int Q>
void launch(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const Fractions& fr, int n_q, double* out,
            int32_t* n_valid, hipStream_t stream) {
  const int64_t n_tiles = (n_cols + CW - 1) / CW;
  const int64_t grid = grid_for(n_tiles, n_rows * CW * (int64_t)sizeof(double));
  hipLaunchKernelGGL((column_quantiles_kernel<CW, WAVES, Q>), dim3((unsigned)grid), dim3(WAVES * kWave), 0, stream, x, n_rows, n_cols,
                     row_stride, fr, n_q, n_tiles, out, n_valid);
}

template <int Q>
void launch_q(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const Fractions& fr, int n_q, double* out,
              int32_t* n_valid, hipStream_t stream) {
  const bool wide = (n_cols + 63) / 64 >= EXO_PRED_WIDE_TILES;
  const bool tall = n_rows >= EXO_PRED_TALL_ROWS;
  constexpr int W = Q <= 3 ? 16 : 8;   // (sixteen bisections need more than the 128 registers a lane of 16 waves has)
  if (wide && tall) launch<64, W, Q>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, stream);
  else if (wide) launch<64, 4, Q>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, stream);
  else if (tall) launch<16, W, Q>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, stream);
  else launch<16, 4, Q>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, stream);
}

}  // namespace

extern "C" {

int exo_column_quantiles_f64(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const int64_t* num,
                             const int64_t* den, int n_q, double* out, int32_t* n_valid, void* stream) {
  if (n_rows < 0 || n_cols < 0 || n_q < 0 || n_q > kMaxQ || n_rows >= (int64_t(1) << 31)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_cols == 0 || n_q == 0) return EXO_OK;
  if (row_stride < n_cols || !num || !den || !out || (n_rows > 0 && !x)) return EXO_ERR_INVALID_ARGUMENT;
  Fractions fr;
  for (int q = 0; q < kMaxQ; ++q) {
    const int p = q < n_q ? q : n_q - 1;     // (the unused slots of a kernel's Q repeat the last fraction)
    if (den[p] <= 0 || den[p] > 1000000000 || num[p] < 0 || num[p] > den[p]) return EXO_ERR_INVALID_ARGUMENT;
    fr.num[q] = num[p];
    fr.den[q] = den[p];
  }
  if (n_q == 1) launch_q<1>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, (hipStream_t)stream);
  else if (n_q <= 3) launch_q<3>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, (hipStream_t)stream);
  else launch_q<kMaxQ>(x, n_rows, n_cols, row_stride, fr, n_q, out, n_valid, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH;
}

}  // extern "C"
