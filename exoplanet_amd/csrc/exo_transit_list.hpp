// exo_transit_list.hpp -- the LIST PATH of the light-curve sweep (exo_transit.hip), whole: every cadence classified
// (transit_scan_kernel: conjunction windows, then the position-based classifier; per-wave work lists), the listed cadences
// solved densely (transit_heavy_kernel: eval_sample, per-block gradient partials), block partials -> gradients
// (transit_vjp_reduce_kernel); its launch geometry, workspace layout and launch helpers.
//   Work units: a (draw, run of tiles_per_block tiles of 512 consecutive cadences); a lane owns cadences (sub-exposures and
//   planets are register loops), so a wave is a run of consecutive cadences: transits are contiguous in time and whole waves
//   are in / out of transit except at the edges.
#pragma once
#include "exo_transit_sample.hpp"
#include "exo_transit_window.hpp"

namespace {
#ifndef EXO_TARGET_BLOCKS
#define EXO_TARGET_BLOCKS (256 * 16)
#endif
constexpr int kTargetBlocks = EXO_TARGET_BLOCKS;  // ~16 resident-or-queued blocks per CU: fills the chip, amortises
                                         // the per-block constant staging and gradient reduction
constexpr int kMaxMerge = 8;            // scan blocks per heavy block, at most

// ---------------------------------------------------------------------------
// Scan kernel: the classifier
// ---------------------------------------------------------------------------
// one (planet, sub-exposure) sample of the classifier:
//   0 = cannot overlap the disk,
//   1 = overlaps, and the small disk looks wholly inside the large one (b + r < 1),
//   2 = overlaps, may be on the limb.
// 1 versus 2 only orders the work list (limb cadences run the arc geometry of the solution
// vector, the others do not, and a wave votes on whether to enter it): a wrong guess costs
// time, never a result.
template <bool SECONDARY, bool FAST>
__device__ __forceinline__ int classify_sample(double tt, const PlanetConst& c) {
  if (FAST) {
    // conservative fp32 classification: only the phase is fp64 (see exo::orbit_pos_f32);
    // every accepted cadence is re-evaluated in fp64 by the heavy kernel.  The phase stays the plain product: its two
    // roundings (2.3e-16 |M| each, 7e-9 rad at |M| = 3e7) move the position by |d pos / d M| <= sqrt((1 + e) / (1 - e))
    // times that, in units of a -- 1e-7 at e = 0.99 -- against the 1.6e-3 a/R that the margin holds for the fp32 error.
    float cx, sx;
    exo::orbit_pos_f32((tt - c.tp) * c.n, c.ef, c.omf, c.sqf, &cx, &sx);
    const float x1 = c.cwf * cx - c.swf * sx;
    const float y1 = c.swf * cx + c.cwf * sx;
    const float Ys = c.cif * y1;
    const float Zs = c.zsf * y1;  // Z / (a/R)
    const bool vis = SECONDARY ? true : !(Zs <= c.zthrf);
    const float b2s = fmaf(x1, x1, Ys * Ys);
    return (vis && !(b2s >= c.thrf)) ? ((b2s < c.inthrf) ? 1 : 2) : 0;
  }
  // the exact classifier decides with the same phase as eval_sample
  const exo::KeplerHalf kh = exo::kepler_half(exo::mean_anomaly_reduced(tt, c.tp, c.n), c.e, c.se, c.pe);
  const double cx = kh.X * kh.X - kh.Y * kh.Y, sx = 2.0 * kh.X * kh.Y;
  const double x1 = c.cw * cx - c.sw * sx;  // position / (-a/R)
  const double y1 = c.sw * cx + c.cw * sx;
  const double Ys = c.ci * y1;
  const double Z = c.si * y1 * c.aor;       // = -sin(i) y1 (-a/R)
  const double b2 = (x1 * x1 + Ys * Ys) * c.aor * c.aor;
  const double lim = 1.0 + c.ror, lin = fmax(1.0 - c.ror, 0.0);
  const bool vis = SECONDARY ? true : !(Z <= 0.0);
  return (vis && !(b2 >= lim * lim)) ? ((b2 < lin * lin) ? 1 : 2) : 0;
}

// The scan kernel.  Two kinds of block share the launch (classify blocks first in the dispatch
// order, fill blocks after them), so that both kinds are resident together:
//   * fill blocks zero flux for their run of cadences -- a pure stream of 16-B stores
//     with nothing to wait for (the heavy kernel, ordered after this one on the stream,
//     overwrites the active cadences).  Stores and loads share one in-order counter on
//     gfx9, so a wave that alternates "load t, store 0" drains its stores every
//     iteration; giving the stores to waves that never load is what lets them run at
//     fill bandwidth;
//   * classify blocks read t (two cadences per lane, the next tile's pair prefetched),
//     decide which cadences can overlap the disk and append their offsets to per-wave
//     lists with ballot + mbcnt (no atomics).
// VEC2 (n_cad even and t 16-B aligned): a lane's two cadences are adjacent and t moves
// as 16-B loads; otherwise they are kBlock apart.
__device__ __forceinline__ void zero_fill(double* __restrict__ dst, int64_t n) {
  if (n <= 0) return;
  const int64_t head = (reinterpret_cast<uintptr_t>(dst) & 8) ? 1 : 0;
  if (threadIdx.x == 0 && head) dst[0] = 0.0;
  double2* __restrict__ d2 = reinterpret_cast<double2*>(dst + head);
  const int64_t n2 = (n - head) >> 1;
  int64_t k = threadIdx.x;
  // non-temporal: the zeros are not read again before they reach HBM, and keeping them out of
  // L2 leaves it to the heavy kernel that follows (measured: scan -21 us, heavy -10 us)
  typedef double v2d __attribute__((ext_vector_type(2)));
  v2d* __restrict__ q2 = reinterpret_cast<v2d*>(d2);
  const v2d z = {0.0, 0.0};
  for (; k < n2; k += kBlock) __builtin_nontemporal_store(z, q2 + k);
  if (threadIdx.x == 0 && ((n - head) & 1)) dst[n - 1] = 0.0;
}

constexpr int kScanDraws = 4;  // draws per classify block on the single-planet path

// ballot + mbcnt append of the active lanes' offsets to a per-wave list (no atomics).  The list
// is two-ended: kind 1 grows up from lst[0], kind 2 grows down from lst[cap - 1].
struct ListCount {
  int in, limb;
};
__device__ __forceinline__ void append_active(int kind, int off, int32_t* __restrict__ lst, int cap, ListCount& cnt) {
  const unsigned long long b1 = __ballot(kind == 1), b2 = __ballot(kind == 2);
  if (kind == 1) {
    const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b1, 0));
    lst[cnt.in + before] = off;
  } else if (kind == 2) {
    const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b2, 0));
    lst[cap - 1 - (cnt.limb + before)] = off;
  }
  cnt.in += __popcll(b1);
  cnt.limb += __popcll(b2);
}

// flags & kFlagGrouped: classify blocks take kScanDraws consecutive draws each (single planet,
// conjunction windows, one exposure time): t is loaded once per kScanDraws draws and the per-draw
// window constants sit in scalar registers.
constexpr uint32_t kFlagGrouped = 0x40000000u;

// (TTV: held to five waves per SIMD like the others -- four classify blocks per CU are resident
// at the start of a sweep, and the fifth slot is what lets fill blocks run beside them)
template <bool SECONDARY, bool FAST, bool VEC2, bool TTV = false>
__global__ __launch_bounds__(kBlock, (FAST && TTV) ? 5 : 1) void transit_scan_kernel(const double* __restrict__ t,
    int64_t n_cad, const double* __restrict__ texp, int64_t n_texp, const double* __restrict__ stencil_dt, int n_sub,
    const double* __restrict__ params, int n_planet, uint32_t flags, int tiles_per_block, int blocks_per_draw,
    int64_t n_draw, int64_t n_classify, double* __restrict__ flux, int32_t* __restrict__ counts, int32_t* __restrict__ list,
    const double* __restrict__ windows, Ttv ttv) {
  __shared__ Shared sh;
  // 1-D launch: classify blocks first (they feed the next kernel and should start early),
  // fill blocks after them; workgroups go to the 8 XCDs round-robin on the linear id, so both
  // kinds spread over all of them.
  int64_t work = blockIdx.x;
  if (work >= n_classify) {
    work -= n_classify;
    const int64_t draw = work / blocks_per_draw;
    const int bx = (int)(work - draw * blocks_per_draw);
    const int64_t lo = (int64_t)bx * tiles_per_block * kTile;
    const int64_t hi = lo + (int64_t)tiles_per_block * kTile;
    const int64_t npl = (flags & EXO_FLAG_PER_PLANET) ? n_planet : 1;
    zero_fill(flux + (draw * n_cad + lo) * npl, ((hi < n_cad ? hi : n_cad) - lo) * npl);
    return;
  }
  const bool grouped = flags & kFlagGrouped;
  const bool window = flags & EXO_FLAG_WINDOW;
  const bool stage1 = FAST || window;
  const int64_t unit = work / blocks_per_draw;  // draw, or group of kScanDraws draws
  const int bx = (int)(work - unit * blocks_per_draw);
  const int64_t draw = grouped ? unit * kScanDraws : unit;
  const int nd = grouped ? (int)((n_draw - draw) < kScanDraws ? (n_draw - draw) : kScanDraws) : 1;
  // TTV: this block's rows of the timing tables (its draw's planets, or its draws' single planets)
  // are copied to LDS when they fit: under the fill blocks' store stream a lookup that goes to
  // L2 waits microseconds, and a tile that crosses a bin boundary needs two in a row.
  constexpr int kTabMax = TTV ? 2048 : 1;
  __shared__ double s_tab[kTabMax];
  Ttv tl = ttv;                                                  // the tables as this block reads them
  int64_t row0 = grouped ? draw : draw * n_planet;               // table row of the block's first record
  if (TTV) {
    const int rows = grouped ? nd : n_planet, ne = ttv.n_edge;
    if (rows * (2 * ne + 1) <= kTabMax) {
      const double* __restrict__ src_e = ttv.edges + row0 * ne;
      const double* __restrict__ src_s = ttv.shift + row0 * (ne + 1);
      for (int q = threadIdx.x; q < rows * ne; q += kBlock) s_tab[q] = src_e[q];
      for (int q = threadIdx.x; q < rows * (ne + 1); q += kBlock) s_tab[rows * ne + q] = src_s[q];
      tl.edges = s_tab;
      tl.shift = s_tab + rows * ne;
      row0 = 0;
      __syncthreads();
    }
  }
  // grouped: the nd consecutive single-planet records are staged as if they were nd planets of one draw
  stage_constants(sh, params + (grouped ? draw * EXO_NPAR : 0), nullptr, stencil_dt, nullptr, n_sub,
                  grouped ? nd : n_planet, grouped ? 0 : draw, SECONDARY,
                  stage1 ? windows + (grouped ? kWin * draw : 0) : nullptr, TTV ? &tl : nullptr,
                  grouped ? row0 : row0 - draw * n_planet);
  // the windows are widened by the half-span of the exposure stencil; the reference widens its
  // contact windows by texp / 2 whatever the stencil (keplerian.py:765-769)
  const double span = window ? 0.5 : stencil_reach(sh.sdt, n_sub);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t blk_base = (int64_t)bx * tiles_per_block * kTile;
  const int64_t list_stride = (int64_t)tiles_per_block * 128;
  const int64_t wave_slot = ((int64_t)draw * blocks_per_draw + bx) * kWaves + wave;  // of the first draw
  const int64_t slot_stride = (int64_t)blocks_per_draw * kWaves;                    // draw to draw
  const int o0 = VEC2 ? 2 * (int)threadIdx.x : (int)threadIdx.x;
  const int o1 = o0 + (VEC2 ? 1 : kBlock);
  auto load_pair = [&](int tile, double& a, double& b) {
    const int64_t i0 = blk_base + tile * kTile + o0, i1 = blk_base + tile * kTile + o1;
    if (VEC2) {
      // n_cad even and i0 even: the pair is valid or invalid together
      const double2 v = (i0 < n_cad) ? *reinterpret_cast<const double2*>(t + i0) : double2{0.0, 0.0};
      a = v.x; b = v.y;
    } else {
      a = (i0 < n_cad) ? t[i0] : 0.0;
      b = (i1 < n_cad) ? t[i1] : 0.0;
    }
  };
  double nx0, nx1;
  load_pair(0, nx0, nx1);
  if (grouped) {
    // Common case per tile: 16 (draw, cadence) phase tests, five full-rate operations each, and
    // no lane near a conjunction.  Otherwise (transits are contiguous in time and aligned across
    // neighbouring draws, so this is ~5% of the tiles) a rolled loop over the draws runs the
    // position-based classifier on the candidates; the per-draw counts live in LDS there.
    __shared__ ListCount s_cnt[kWaves][kScanDraws];
    if (lane < kScanDraws) s_cnt[wave][lane] = ListCount{0, 0};
    const double te = n_texp ? texp[0] : 0.0;
    double nrev[kScanDraws], c0[kScanDraws], dmid[kScanDraws], lim0[kScanDraws], lim1[kScanDraws];
#pragma unroll
    for (int j = 0; j < kScanDraws; ++j) {
      const PlanetConst& c = sh.pc[j < nd ? j : 0];
      nrev[j] = uniform(c.nrev); c0[j] = uniform(c.c0); dmid[j] = uniform(c.dmid);
      const double widen = fabs(te) * span * fabs(c.nrev);
      lim0[j] = uniform(c.half[0] + widen);
      lim1[j] = SECONDARY ? uniform(c.half[1] + widen) : 0.0;
    }
    // TTV: each draw's current bin -- its edges and its shift -- rides along in scalar registers.
    // A tile whose cadences (and their exposures) all lie strictly inside that bin costs four
    // compares and a subtraction more than without timing tables; any other tile (a bin boundary
    // every few tiles; every tile if the times are not sorted) looks its cadences up one by one
    // and leaves the bin of its last cadence behind for the next tile.
    struct BinNow { double lo, hi, sh; };
    __shared__ BinNow s_now[kWaves][kScanDraws];
    double b_lo[kScanDraws], b_hi[kScanDraws], b_sh[kScanDraws];
#pragma unroll
    for (int j = 0; j < kScanDraws; ++j) {
      // no bin yet; draws past the end of the batch: one bin that holds everything
      b_lo[j] = j < nd ? __builtin_inf() : -__builtin_inf();
      b_hi[j] = -b_lo[j];
      b_sh[j] = 0.0;
    }
    // exposures reaching over an edge are looked at sample by sample (never under the caller's
    // windows: those warp the mid-exposure time only, like the reference's in_transit)
    const double hw = (TTV && !window) ? uniform(fma(fabs(te) * span, 1e-12, fabs(te) * span)) : 0.0;
    auto process = [&](int tile, double tv0, double tv1) {
      const double tv[2] = {tv0, tv1};
      unsigned cand = 0;
      unsigned redo = 0;   // TTV: draws whose cached bin does not hold the whole tile (wave-uniform)
#pragma unroll
      for (int j = 0; j < kScanDraws; ++j) {
        double sh_j = 0.0;
        if (TTV) {
          const bool inside = (tv0 - b_lo[j] > hw) && (b_hi[j] - tv0 > hw) && (tv1 - b_lo[j] > hw) && (b_hi[j] - tv1 > hw);
          if (__ballot(!inside) != 0) {
            redo |= 1u << j;
            continue;
          }
          sh_j = b_sh[j];
        }
#pragma unroll
        for (int v = 0; v < 2; ++v)
          cand |= near_conjunction<SECONDARY>(tv[v] - sh_j, nrev[j], c0[j], dmid[j], lim0[j], lim1[j]) ? (1u << (2 * j + v)) : 0u;
      }
      if (TTV && redo) {
#pragma unroll 1
        for (int j = 0; j < nd; ++j) {
          if (!((redo >> j) & 1u)) continue;
          const PlanetConst& c = sh.pc[j];
          const TtvRow row(tl, row0 + j);
          const double widen = fabs(te) * span * fabs(c.nrev);
          TtvRow::Hit hit[2];
          row.locate2(tv0, tv1, c.te0, c.tinv, c.tfin, hit[0], hit[1]);
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const bool mixed = !window && n_texp && (!(tv[v] - hit[v].lo > hw) || !(hit[v].hi - tv[v] > hw));
            const bool near = mixed || near_conjunction<SECONDARY>(tv[v] - hit[v].sh, c.nrev, c.c0, c.dmid,
                                                                   c.half[0] + widen, c.half[1] + widen);
            cand |= near ? (1u << (2 * j + v)) : 0u;
          }
          if (lane == 63) s_now[wave][j] = BinNow{hit[1].lo, hit[1].hi, hit[1].sh};
        }
        // (same wave wrote them: program order is enough)
#pragma unroll
        for (int j = 0; j < kScanDraws; ++j) {
          if (((redo >> j) & 1u) && j < nd) {
            const BinNow nb = s_now[wave][j];
            b_lo[j] = uniform(nb.lo); b_hi[j] = uniform(nb.hi); b_sh[j] = uniform(nb.sh);
          }
        }
      }
      // draws past the end of the batch
      cand &= (1u << (2 * nd)) - 1u;
      if (__ballot(cand != 0) == 0) return;
      const int off[2] = {tile * kTile + o0, tile * kTile + o1};
#pragma unroll 1
      for (int j = 0; j < nd; ++j) {
        int32_t* __restrict__ lst = list + (wave_slot + j * slot_stride) * list_stride;
        ListCount cnt = s_cnt[wave][j];
#pragma unroll 1
        for (int v = 0; v < 2; ++v) {
          int kind = 0;
          if ((cand >> (2 * j + v)) & 1u) {
            if (TTV) {
              const PlanetConst& c = sh.pc[j];
              const TtvRow row(tl, row0 + j);
              double e_lo, e_hi;
              const int kb = row.locate(tv[v], c.te0, c.tinv, c.tfin, e_lo, e_hi);
              const double shv = row.shift[kb];
              const bool mixed = !window && n_texp && (!(tv[v] - e_lo > hw) || !(e_hi - tv[v] > hw));
              for (int k = 0; k < n_sub; ++k) {
                const double tt = fma(te, sh.sdt[k], tv[v]);
                double shk = shv;
                if (mixed) shk = row.shift[row.neighbour(tt, kb, e_lo, e_hi)];
                kind = max(kind, classify_sample<SECONDARY, FAST>(tt - shk, c));
              }
            } else {
              for (int k = 0; k < n_sub; ++k)
                kind = max(kind, classify_sample<SECONDARY, FAST>(fma(te, sh.sdt[k], tv[v]), sh.pc[j]));
            }
            if (window) kind = max(kind, 1);  // the caller's window decides; the classifier only sorts
          }
          append_active((blk_base + off[v] < n_cad) ? kind : 0, off[v], lst, (int)list_stride, cnt);
        }
        if (lane == 0) s_cnt[wave][j] = cnt;
      }
    };
    // t runs kAhead tiles ahead of the tests (a block may be alone on its SIMD: no other wave
    // hides the load latency)
    constexpr int kAhead = 4;
    double ring[kAhead][2];
    ring[0][0] = nx0; ring[0][1] = nx1;
#pragma unroll
    for (int u = 1; u < kAhead; ++u) {
      ring[u][0] = ring[u][1] = 0.0;
      if (u < tiles_per_block) load_pair(u, ring[u][0], ring[u][1]);
    }
    for (int tile0 = 0; tile0 < tiles_per_block; tile0 += kAhead) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int tile = tile0 + u;
        if (tile < tiles_per_block) {
          const double a = ring[u][0], b = ring[u][1];
          if (tile + kAhead < tiles_per_block) load_pair(tile + kAhead, ring[u][0], ring[u][1]);
          process(tile, a, b);
        }
      }
    }
    if (lane < nd) {
      const ListCount cnt = s_cnt[wave][lane];
      counts[2 * (wave_slot + lane * slot_stride)] = cnt.in;
      counts[2 * (wave_slot + lane * slot_stride) + 1] = cnt.limb;
    }
    return;
  }
  int32_t* __restrict__ my_list = list + wave_slot * list_stride;
  ListCount cnt{0, 0};
  // TTV: per wave and planet, the bin of the wave's last cadence (edges, shift, number)
  struct GenBin { double lo, hi, sh; int k; };
  __shared__ GenBin s_gbin[kWaves][EXO_MAX_PLANETS];
  if (TTV && lane < n_planet) s_gbin[wave][lane] = GenBin{__builtin_inf(), -__builtin_inf(), 0.0, 0};   // no bin yet
  for (int tile = 0; tile < tiles_per_block; ++tile) {
    const double tv[2] = {nx0, nx1};
    if (tile + 1 < tiles_per_block) load_pair(tile + 1, nx0, nx1);
    const int off[2] = {tile * kTile + o0, tile * kTile + o1};
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int64_t i = blk_base + off[v];
      const bool valid = i < n_cad;
      const double te = (n_texp == 0) ? 0.0 : (n_texp == 1 ? texp[0] : (valid ? texp[i] : 0.0));
      int kind = 0;
      for (int p = 0; p < n_planet; ++p) {
        const PlanetConst& c = sh.pc[p];
        bool cand = true;
        if (TTV) {
          // the cadence in its own bin; an exposure that reaches into the next bin has
          // sub-exposures measured from another transit: no window argument covers those,
          // the classifier sees each of them (the caller's windows, like the reference's
          // in_transit, warp the mid-exposure time only)
          // The wave's last bin of this planet is tried first (LDS broadcast): times are usually
          // sorted, and a bin holds thousands of cadences.
          const TtvRow row(tl, row0 + p);
          const double hw = window ? 0.0 : fma(fabs(te) * span, 1e-12, fabs(te) * span);   // (the product was rounded)
          const GenBin nb = s_gbin[wave][p];
          double e_lo = nb.lo, e_hi = nb.hi, shv = nb.sh;
          int kb = nb.k;
          const bool inside = (tv[v] - e_lo > hw) && (e_hi - tv[v] > hw);
          if (__ballot(!inside) != 0) {
            kb = row.locate(tv[v], c.te0, c.tinv, c.tfin, e_lo, e_hi);
            shv = row.shift[kb];
            if (lane == 63) s_gbin[wave][p] = GenBin{e_lo, e_hi, shv, kb};
          }
          const double tw = tv[v] - shv;
          const bool mixed = !window && n_texp && (!(tv[v] - e_lo > hw) || !(e_hi - tv[v] > hw));
          if (stage1 && !mixed) {
            const double widen = fabs(te) * span * fabs(c.nrev);
            cand = near_conjunction<SECONDARY>(tw, c.nrev, c.c0, c.dmid, c.half[0] + widen, c.half[1] + widen);
          }
          if (cand) {
            int kp = window ? 1 : 0;
            for (int k = 0; k < n_sub; ++k) {
              const double tt = fma(te, sh.sdt[k], tv[v]);
              double shk = shv;
              if (mixed) shk = row.shift[row.neighbour(tt, kb, e_lo, e_hi)];
              kp = max(kp, classify_sample<SECONDARY, FAST>(tt - shk, c));
            }
            kind = max(kind, kp);
          }
          continue;
        }
        if (stage1) {
          const double widen = fabs(te) * span * fabs(c.nrev);
          cand = near_conjunction<SECONDARY>(tv[v], c.nrev, c.c0, c.dmid, c.half[0] + widen, c.half[1] + widen);
        }
        if (cand) {
          int kp = window ? 1 : 0;  // the caller's window decides; the classifier only sorts
          for (int k = 0; k < n_sub; ++k)
            kp = max(kp, classify_sample<SECONDARY, FAST>(fma(te, sh.sdt[k], tv[v]), c));
          kind = max(kind, kp);
        }
      }
      append_active(valid ? kind : 0, off[v], my_list, (int)list_stride, cnt);
    }
  }
  if (lane == 0) {
    counts[2 * wave_slot] = cnt.in;
    counts[2 * wave_slot + 1] = cnt.limb;
  }
}

// ---------------------------------------------------------------------------
// Heavy kernel: the cadences on the work lists of up to kMaxMerge scan blocks of one draw,
// concatenated ("inside" runs first, then "limb" runs) and processed densely, 256 at a time:
// Kepler solve in fp64, solution vector with its elliptic integrals, flux, and -- GRAD -- the
// reverse sweep into per-planet gradient slots that live in LDS columns for the whole block
// and are reduced once per planet in a fixed order (bit-reproducible).
// ---------------------------------------------------------------------------
// two waves per SIMD (<= 256 registers): measured 0.727 ms vs 0.776 ms per sweep at one wave
// (A/B via EXOPLANET_AMD_LIB), despite ~136 B/lane of scratch in the gradient variant
#ifndef EXO_HEAVY_MIN_WAVES
#define EXO_HEAVY_MIN_WAVES 2
#endif
template <bool GRAD, bool SECONDARY, bool TTV = false>
__global__ __launch_bounds__(kBlock, EXO_HEAVY_MIN_WAVES) void transit_heavy_kernel(const double* __restrict__ t,
    int64_t n_cad, const double* __restrict__ texp, int64_t n_texp, const double* __restrict__ stencil_dt,
    const double* __restrict__ stencil_w, int n_sub, const double* __restrict__ params, const double* __restrict__ ld,
    int n_planet, uint32_t flags, int tiles_per_block, int blocks_per_draw, int merge, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ list, const double* __restrict__ gflux, double* __restrict__ flux,
    double* __restrict__ partial, const double* __restrict__ windows, Ttv ttv) {
  __shared__ Shared sh;
  __shared__ int s_pre[2 * kWaves * kMaxMerge + 1];
  const int64_t draw = blockIdx.y;
  __shared__ BinCache s_bins;
  if (GRAD && TTV && threadIdx.x < kWaves * kBinSlots) (&s_bins.id[0][0])[threadIdx.x] = -1;
  // TTV: the draw's timing tables in LDS when they fit (a wave's 64 list entries often span two
  // transits of different planets: a lookup per planet and round; from LDS it costs a tenth)
  constexpr int kTabMax = TTV ? 2048 : 1;
  __shared__ double s_tab[kTabMax];
  Ttv tl = ttv;
  int64_t row0 = draw * n_planet;
  if (TTV && n_planet * (2 * ttv.n_edge + 1) <= kTabMax) {
    const int ne = ttv.n_edge;
    const double* __restrict__ src_e = ttv.edges + row0 * ne;
    const double* __restrict__ src_s = ttv.shift + row0 * (ne + 1);
    for (int q = threadIdx.x; q < n_planet * ne; q += kBlock) s_tab[q] = src_e[q];
    for (int q = threadIdx.x; q < n_planet * (ne + 1); q += kBlock) s_tab[n_planet * ne + q] = src_s[q];
    tl.edges = s_tab;
    tl.shift = s_tab + n_planet * ne;
    row0 = 0;
    __syncthreads();
  }
  stage_constants(sh, params, ld, stencil_dt, stencil_w, n_sub, n_planet, draw, SECONDARY, nullptr,
                  TTV ? &tl : nullptr, row0 - draw * n_planet);
  const bool per_planet = flags & EXO_FLAG_PER_PLANET;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // this block works through the lists of `nsub` consecutive scan blocks of its draw
  const int bx0 = blockIdx.x * merge;
  const int nsub = (blocks_per_draw - bx0 < merge) ? blocks_per_draw - bx0 : merge;
  const int cap = tiles_per_block * 128;
  // segment order: all "inside" runs (scan block by scan block, wave by wave), then all "limb" runs
  const int nseg = 2 * kWaves * nsub;
  if ((int)threadIdx.x < nseg) {
    const int sgm = threadIdx.x;
    const int kind = sgm / (kWaves * nsub), rem = sgm - kind * (kWaves * nsub);
    s_pre[sgm + 1] = counts[2 * (((int64_t)draw * blocks_per_draw + bx0) * kWaves + rem) + kind];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc_n = 0;
    s_pre[0] = 0;
    for (int sgm = 1; sgm <= nseg; ++sgm) {
      acc_n += s_pre[sgm];
      s_pre[sgm] = acc_n;
    }
  }
  __syncthreads();
  const int total = s_pre[nseg];
  const int ng_draw = n_planet * kNG + 7;
  double* __restrict__ pout = GRAD ? partial + ((int64_t)draw * gridDim.x + blockIdx.x) * ng_draw : nullptr;

  // slots [0, kNG): this planet's parameters; [kNG, kNG + 6): limb darkening; kNG + 6: sum(gflux * flux)
  __shared__ double lds_acc[kNG + 7][kBlock];
  const GradAcc acc{GRAD ? &lds_acc[0][threadIdx.x] : nullptr};
  if (GRAD) {
#pragma unroll
    for (int s = 0; s < kNG + 7; ++s) lds_acc[s][threadIdx.x] = 0.0;
  }
  // limb-darkening coefficients, scalar registers as well
  double cld[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) cld[k] = uniform((SECONDARY || k < 3) ? sh.c[k] : 0.0);
  // Several planets share one work list (a cadence is listed if ANY planet may overlap): a round
  // whose cadences are all away from planet p's conjunction windows is skipped for p on a wave
  // vote (the same five-operation test as the scan kernel's first stage), before any Kepler solve.
  const bool use_win = windows && n_planet > 1;
  double spanw = (flags & EXO_FLAG_WINDOW) ? 0.5 : 0.0;
  if (use_win && !(flags & EXO_FLAG_WINDOW))
    for (int k = 0; k < n_sub; ++k) spanw = fmax(spanw, fabs(sh.sdt[k]));
  // TTV: how far a sub-exposure can be from its cadence, in units of texp (stencil_reach, written out: see DESIGN.md 4)
  double reach = 0.0;
  if (TTV)
    for (int k = 0; k < n_sub; ++k) reach = fmax(reach, fabs(sh.sdt[k]));
  for (int p = 0; p < n_planet; ++p) {
    const PlanetS c(sh.pc[p]);
    const TtvRow row(tl, TTV ? row0 + p : 0);
    const TtvGrad tgrad{GRAD && TTV ? &lds_acc[0][threadIdx.x] : nullptr,
                        GRAD && TTV ? ttv.gshift + (draw * n_planet + p) * (int64_t)(ttv.n_edge + 1) : nullptr,
                        &s_bins};
    const double t_e0 = TTV ? uniform(sh.pc[p].te0) : 0.0, t_inv = TTV ? uniform(sh.pc[p].tinv) : 0.0;
    const int t_fin = TTV ? __builtin_amdgcn_readfirstlane(sh.pc[p].tfin) : 0;
    // the wave's current bin of this planet (scalar registers): list entries are consecutive
    // cadences, so a round usually stays in the bin of the one before
    double c_lo = __builtin_inf(), c_hi = -__builtin_inf(), c_sh = 0.0;
    int c_k = 0;
    double w_nrev = 0.0, w_c0 = 0.0, w_dmid = 0.0, w_h0 = 0.0, w_h1 = 0.0;
    if (use_win) {
      const double* wv = windows + kWin * (draw * n_planet + p);
      w_nrev = uniform(wv[0]); w_c0 = uniform(wv[1]); w_dmid = uniform(wv[2]);
      w_h0 = uniform(wv[3]); w_h1 = uniform(wv[4]);
    }
    if (GRAD && p > 0) {
#pragma unroll
      for (int s = 0; s < kNG; ++s) lds_acc[s][threadIdx.x] = 0.0;
    }
    // Two-deep software pipeline over the rounds: the list entry of round r + 2 and the cadence
    // data (t, texp, gflux) of round r + 1 are in flight while round r computes -- at two waves
    // per SIMD nothing else hides the two dependent loads (list -> t, gflux) of a round.
    auto list_index = [&](int jr, int64_t& base_cad) -> int {
      int sgm = 0;   // last segment whose start is <= jr (empty segments share a start: the search lands past them)
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) {
        const int q = sgm + step;
        if (q < nseg && jr >= s_pre[q]) sgm = q;
      }
      const int pos = jr - s_pre[sgm];
      const int kind = sgm / (kWaves * nsub), rem = sgm - kind * (kWaves * nsub);  // rem = sub * kWaves + wave
      const int64_t lbase = (((int64_t)draw * blocks_per_draw + bx0) * kWaves + rem) * (int64_t)cap;
      base_cad = (int64_t)(bx0 + rem / kWaves) * tiles_per_block * kTile;
      return list[lbase + (kind ? cap - 1 - pos : pos)];
    };
    struct Item { int64_t i; double tv, te, g; };
    auto load_item = [&](bool has_, int off_, int64_t base_) -> Item {
      Item it;
      it.i = has_ ? base_ + off_ : 0;
      it.tv = t[it.i];
      it.te = (n_texp == 0) ? 0.0 : (n_texp == 1 ? texp[0] : texp[it.i]);
      it.g = 0.0;
      if (GRAD && has_) it.g = per_planet ? gflux[(draw * n_cad + it.i) * n_planet + p] : gflux[draw * n_cad + it.i];
      return it;
    };
    int64_t base_n = 0, base_nn = 0;
    int off_n = 0, off_nn = 0;
    {
      const int j = threadIdx.x;
      if (j < total) off_n = list_index(j, base_n);
      if (j + kBlock < total) off_nn = list_index(j + kBlock, base_nn);
    }
    // (the gradient variant has no registers to spare for the data of a second round: it keeps
    // only the list entry one round ahead)
    constexpr bool kDeep = !GRAD;
    Item nxt{0, 0.0, 0.0, 0.0};
    if (kDeep) nxt = load_item((int)threadIdx.x < total, off_n, base_n);
    for (int j0 = 0; j0 < total; j0 += kBlock) {
      const int j = j0 + threadIdx.x;
      const bool has = j < total;
      Item cur;
      if (kDeep) {
        cur = nxt;
        // round r + 1's data (its list entry arrived a round ago), round r + 2's list entry
        if (j0 + kBlock < total) nxt = load_item(j + kBlock < total, off_nn, base_nn);
        if (j + 2 * kBlock < total) off_nn = list_index(j + 2 * kBlock, base_nn);
      } else {
        cur = load_item(has, off_n, base_n);
        off_n = off_nn; base_n = base_nn;
        if (j + 2 * kBlock < total) off_nn = list_index(j + 2 * kBlock, base_nn);
      }
      const int64_t i = cur.i;
      const double tv = cur.tv, te = cur.te;
      // TTV: the cadence's bin and shift; `mixed` = some sub-exposure may belong to another bin
      int kb = 0;
      double dsh = 0.0;
      bool mixed = false;
      if (TTV) {
        const double hw = fma(fabs(te) * reach, 1e-12, fabs(te) * reach);   // the product was rounded
        kb = c_k;
        dsh = c_sh;
        const bool inside = (tv - c_lo > hw) && (c_hi - tv > hw);
        const unsigned long long live = __ballot(has);
        if (__ballot(has && !inside) != 0) {
          double e_lo, e_hi;
          kb = row.locate(tv, t_e0, t_inv, t_fin, e_lo, e_hi);
          dsh = row.shift[kb];
          mixed = n_texp && (!(tv - e_lo > hw) || !(e_hi - tv > hw));
          // the last listed cadence of the wave leaves its bin behind
          const int last = 63 - __builtin_clzll(live);
          c_lo = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(e_lo), last),
                                  __builtin_amdgcn_readlane(__double2loint(e_lo), last));
          c_hi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(e_hi), last),
                                  __builtin_amdgcn_readlane(__double2loint(e_hi), last));
          c_sh = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(dsh), last),
                                  __builtin_amdgcn_readlane(__double2loint(dsh), last));
          c_k = __builtin_amdgcn_readlane(kb, last);
        }
      }
      if (use_win) {
        const double widen = fabs(te) * spanw * fabs(w_nrev);
        const bool near = has && ((mixed && !(flags & EXO_FLAG_WINDOW)) ||
                                  near_conjunction<SECONDARY>(tv - dsh, w_nrev, w_c0, w_dmid, w_h0 + widen, w_h1 + widen));
        if (!EXO_WAVE_ANY(near)) continue;   // the fill left this planet's flux at zero
      }
      const double g = cur.g;
      double f = 0.0;
      int kcur = kb;
      for (int k = 0; k < n_sub; ++k) {
        double tt = fma(te, sh.sdt[k], tv);
        if (TTV) {
          int ks = kb;
          double sh_k = dsh;
          if (mixed) {
            ks = row.bin(tt);
            sh_k = row.shift[ks];
          }
          if (GRAD && ks != kcur) {
            tgrad.flush_lane(kcur);
            kcur = ks;
          }
          tt -= sh_k;
        }
        const double gw = g * sh.sw[k];
        const double F = eval_sample<GRAD, SECONDARY>(tt, c, cld, gw, acc);
        f = fma(sh.sw[k], F, f);
        if (GRAD) acc.add(kNG + 6, gw * F);
      }
      if (GRAD && TTV) tgrad.flush_wave(kcur);
      if (flux && has) {
        if (per_planet) {
          flux[(draw * n_cad + i) * n_planet + p] = f;
        } else {
          double* dst = flux + draw * n_cad + i;
          *dst = (p == 0) ? f : (*dst + f);
        }
      }
    }
    if (GRAD && TTV) {
      tgrad.drain();
      // every sample's t_periastron term went through the bins; the planet's total is in G_PAD
      lds_acc[G_TP][threadIdx.x] = lds_acc[G_PAD][threadIdx.x];
      lds_acc[G_PAD][threadIdx.x] = 0.0;
    }
    if (GRAD) reduce_columns(lds_acc, sh.red, 0, kNG, pout + p * kNG);
  }
  if (GRAD) reduce_columns(lds_acc, sh.red, kNG, 7, pout + n_planet * kNG);
}

// Stage 2: one block per draw; thread s sums slot s over the blocks in order.
__global__ __launch_bounds__(kBlock) void transit_vjp_reduce_kernel(const double* __restrict__ partial, int nblk,
    int n_planet, bool secondary, double* __restrict__ gparams, double* __restrict__ gld, double* __restrict__ flux_dot) {
  partials_to_gradients(blockIdx.x, partial, nblk, n_planet, secondary, kBlock, gparams, gld, flux_dot,
                        [](int, double) {});
}

// blocks per draw and tiles per block: enough blocks to fill 256 CUs several
// times over, few enough that each block amortises its prologue / reduction
inline void transit_geometry(int64_t n_cad, int64_t n_draw, int* blocks_per_draw, int* tiles_per_block) {
  const int64_t n_tiles = (n_cad + kTile - 1) / kTile;
  int64_t bpd = (kTargetBlocks + n_draw - 1) / n_draw;
  if (bpd > n_tiles) bpd = n_tiles;
  if (bpd < 1) bpd = 1;
  const int64_t tpb = (n_tiles + bpd - 1) / bpd;
  bpd = (n_tiles + tpb - 1) / tpb;
  *blocks_per_draw = (int)bpd;
  *tiles_per_block = (int)tpb;
}

// heavy blocks take the lists of `merge` consecutive scan blocks: the per-block costs of the
// heavy kernel (constant staging, accumulator reduction, a half-empty last round) are paid
// kHeavyTargetBlocks times rather than kTargetBlocks times, while the scan kernel keeps its finer
// blocks
#ifndef EXO_HEAVY_TARGET_BLOCKS
#define EXO_HEAVY_TARGET_BLOCKS 1024
#endif
inline int heavy_merge(int64_t n_draw, int bpd) {
  int64_t m = (n_draw * bpd + EXO_HEAVY_TARGET_BLOCKS - 1) / EXO_HEAVY_TARGET_BLOCKS;
  if (m > kMaxMerge) m = kMaxMerge;
  if (m > bpd) m = bpd;
  return m < 1 ? 1 : (int)m;
}

// scratch layout shared by forward and reverse: [gradient partials][wave counts][wave lists]
struct Workspace {
  double* partial;
  double* windows;
  int32_t* counts;
  int32_t* list;
  int64_t bytes;
};

inline Workspace carve(void* base, int64_t n_draw, int bpd, int tpb, int n_planet) {
  Workspace w;
  const int64_t n_partial = n_draw * bpd * (int64_t)(n_planet * kNG + 7);
  const int64_t n_slots = n_draw * bpd * (int64_t)kWaves;
  const int64_t n_counts = 2 * n_slots;  // (inside, limb) per wave list
  const int64_t n_list = n_slots * (int64_t)tpb * 128;
  char* p = (char*)base;
  const int64_t n_win = kWin * n_draw * n_planet;
  w.partial = (double*)p;
  w.windows = w.partial + n_partial;
  w.counts = (int32_t*)(p + (n_partial + n_win) * 8);
  w.list = w.counts + ((n_counts + 1) & ~(int64_t)1);
  w.bytes = (n_partial + n_win) * 8 + (((n_counts + 1) & ~(int64_t)1) + n_list) * 4;
  return w;
}

constexpr uint32_t kFlagNoFlux = 0x80000000u;  // internal: scan kernel must not touch flux

// scan kernel launch on (secondary, exact fp64 classification requested) and the loads of t: VEC -- 16-B loads, pairs must
// not straddle the end (even n_cad) and t must be 16-B aligned.  The timing-variation path (TTV) has one variant: per-cadence
// table lookups dwarf the loads.
template <class... Args>
inline void launch_scan(uint32_t flags, bool has_ttv, dim3 grid, hipStream_t st, const double* t, int64_t n_cad, Args... args) {
  auto launch = [&](auto vec, auto ttv) {
    exo::with_flag(flags & EXO_FLAG_SECONDARY, [&](auto sec) {
      exo::with_flag(flags & EXO_FLAG_EXACT_SCAN, [&](auto exact) {
        hipLaunchKernelGGL((transit_scan_kernel<decltype(sec)::value, !decltype(exact)::value, decltype(vec)::value, decltype(ttv)::value>),
                           grid, dim3(kBlock), 0, st, t, n_cad, args...);
      });
    });
  };
  if (has_ttv) launch(std::false_type{}, std::true_type{});
  else if ((n_cad & 1) == 0 && (reinterpret_cast<uintptr_t>(t) & 15) == 0) launch(std::true_type{}, std::false_type{});
  else launch(std::false_type{}, std::false_type{});
}

// the windows of the scan kernel's first test: not needed when the caller asks for the exact
// fp64 scan of every cadence
inline void launch_windows(const double* params, int64_t n_draw, int n_planet, uint32_t flags, double* windows,
                           hipStream_t st) {
  if ((flags & EXO_FLAG_EXACT_SCAN) && !(flags & EXO_FLAG_WINDOW)) return;
  const int64_t n_rec = n_draw * n_planet;
  hipLaunchKernelGGL(transit_window_kernel, dim3((unsigned)((n_rec * kWinLanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     params, n_rec, flags, windows);
}

// scan kernel launch: classify blocks (one per draw and tile run, or one per kScanDraws draws on
// the single-planet path) followed by one fill block per draw and tile run
struct ScanPlan {
  uint32_t flags;      // caller's flags + internal ones
  int64_t n_classify;  // classify blocks
  dim3 grid;
};
inline ScanPlan scan_plan(uint32_t flags, int bpd, int64_t n_draw, int n_planet, int64_t n_texp, bool with_fill) {
  ScanPlan sp;
  const bool stage1 = (flags & EXO_FLAG_WINDOW) || !(flags & EXO_FLAG_EXACT_SCAN);
  const bool grouped = n_planet == 1 && n_texp <= 1 && stage1;
  sp.flags = (flags & 0x0fffffffu) | (grouped ? kFlagGrouped : 0u) | (with_fill ? 0u : kFlagNoFlux);
  sp.n_classify = (grouped ? (n_draw + kScanDraws - 1) / kScanDraws : n_draw) * bpd;
  sp.grid = dim3((unsigned)(sp.n_classify + (with_fill ? n_draw * bpd : 0)));
  return sp;
}

}  // namespace
