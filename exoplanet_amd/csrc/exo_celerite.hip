// exo_celerite.hip -- celerite (semiseparable) GP log-likelihood, value + VJP,
// batched over posterior draws / chains (gfx950, fp64 VALU, no MFMA).
//
// Replaces, for the reference's user-level model, what celerite2 does behind
//   GaussianProcess.compute() + GaussianProcess.log_likelihood(y)
// (celerite2 is a dependency of the reference, /root/reference/setup.py:36, but
// has no call site in its tree; the algorithm is the published one: Foreman-Mackey
// et al. 2017; Foreman-Mackey 2018):
//
//   factor:      S_n = (P P^T) o (S_{n-1} + d_{n-1} W_{n-1} W_{n-1}^T)
//                d_n = a_n - U_n S_n U_n^T ;  W_n = (V_n - S_n U_n) / d_n
//   solve_lower: F_n = P o (F_{n-1} + W_{n-1} z_{n-1}) ;  z_n = y_n - U_n . F_n
//   loglike    = -1/2 sum (z_n^2 / d_n + log d_n) - N/2 log 2 pi
//
// This file is the HOST side -- the launch plan of a call (gp_plan, celerite_fwd, celerite_vjp, celerite_adjoint_scan, the scan
// trees' launches), the second-stream fork of EXO_GP_PREPARE_ADJOINT and the extern "C" entries -- and the translation unit:
// the build's per-file compiler flags, tools/kres.py and tools/build_variant.sh go by its name.  The device code, one header
// per path, each including what it builds on (in this order):
//  * exo_celerite_dpp.hpp       a draw on G = next_pow2(J) adjacent lanes: DPP exchanges, the all-gather, the group's sum
//  * exo_celerite_state.hpp     the saved factorisation: addressing, the records' stores / loads, the S-row checkpoints
//  * exo_celerite_seq.hpp       SEQUENTIAL kernels (calls without a state buffer, short series, draws the time-parallel path
//    cannot take): parallelism over draws and, inside a draw, over the J state indices (lane j owns row j of S); U_n, V_n, P_n
//    come from a fully parallel pre-pass; the saved factorisation is laid out [quantity][cadence][draw x state index] and
//    read back through a software prefetch ring.
//  * exo_celerite_lanegroup.hpp TIME-PARALLEL, lane-group form (J >= 7): the series is cut into chunks whose entering states --
//    and, in reverse, their adjoints -- come from Kalman filtering elements and a short scan over the chunks, after which the
//    same recurrences run inside all chunks at once, a draw on G lanes (see its comment block "Time-parallel path").
//  * exo_celerite_scan.hpp      the scans over the chunks as trees of element compositions (with exo_celerite_group.hpp: items
//    on groups of eight lanes), and the ROBUST route's own scan of the entering states.
//  * exo_celerite_lane.hpp      TIME-PARALLEL, one lane per (draw, chunk) (J <= 6; the lane functions are exo_celerite_core.hpp,
//    which the host harnesses of tests/ compile too): every state index in the lane's registers -- no cross-lane traffic, none of
//    the G-fold duplicated scalar work -- and a CHECKPOINTED factorisation: the forward pass stores (F, S) every 4 cadences (10 B
//    per (draw, cadence) at J = 2 instead of 80), the reverse pass recomputes the cadences of a block from its checkpoint in
//    registers.  Draws too ill-conditioned for the scans' trees (a score up to 1e8) stay on this path by its ROBUST route:
//    Newton iterations on the chunks' entering states (celerite_robust_newton_kernel), the adjoint scan fed from the chunks' own
//    reverse recurrences (celerite_chunk_adj_kernel) -- docs/DESIGN_r1_r4.md 3.11.  Also: the wave's choice of a term layout, the
//    sparse model's chunk and draw orders, the sums over the chunks, dot_tril, predict.
// The library keeps no state between calls: how a series is cut is a pure function of the call's
// arguments (gp::chunk_plan), which the forward and the reverse call of a pair share.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <utility>

#include "../../include/exoplanet_amd.h"
#include "exo_celerite_lane.hpp"

namespace {

inline int launch_status() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

inline bool gp_args_ok(int64_t n, int64_t n_diag, int32_t n_real, int32_t n_complex, int64_t n_draw, int32_t n_chunks) {
  const int J = n_real + 2 * n_complex;
  return n >= 1 && n_draw >= 1 && n_real >= 0 && n_complex >= 0 && J >= 1 && J <= EXO_GP_MAX_J &&
         (n_diag == 1 || n_diag == n_draw) && n_chunks >= 0;
}

template <int V>
using IntK = std::integral_constant<int, V>;
// The state width as a compile-time constant: f(IntK<J>{}) for Lo <= J <= Hi; false (nothing called) outside that range.
// Every width of the range is instantiated, so a call site's range is the set of kernels it compiles.
template <int Lo, class F, int... I>
bool with_J_seq(int J, F&& f, std::integer_sequence<int, I...>) {
  return ((J == Lo + I ? (f(IntK<Lo + I>{}), true) : false) || ...);
}
template <int Lo, int Hi, class F>
bool with_J(int J, F&& f) {
  return with_J_seq<Lo>(J, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

#ifndef EXO_GP_MIXED_ONE_LAUNCH
#define EXO_GP_MIXED_ONE_LAUNCH 1
#endif
// The one-lane kernels' compile-time constants: f(J, NR, SP) -- IntK's -- for every layout variant NR the draws of a call may
// need (layout_vote), SP the series' kind (SeriesRowT: 1 a sparse model, 0 otherwise).  J = 1: one real term; J = 2: two real
// terms or one pair slot -- complex, or, with per-draw kinds, either: mixed(SP), the variants in one launch, or
// (EXO_GP_MIXED_ONE_LAUNCH = 0) f for all three one after the other (a wave returns at once from the variants it did not vote
// for); J > 2: run-time flags (J = 4 with no real term: a layout of its own too, split_layouts).  false: J > 8.
template <class F, class Mixed>
bool with_layouts(const Coefs& cf, const Series& rs, F&& f, Mixed&& mixed) {
  auto by_layout = [&](auto sp) {
    const int J = cf.J();
    if (J == 1) {
      f(IntK<1>{}, IntK<1>{}, sp);
    } else if (J == 2) {
      if (cf.n_real == 2) f(IntK<2>{}, IntK<2>{}, sp);
      else if (!cf.kind) f(IntK<2>{}, IntK<0>{}, sp);
      else if (EXO_GP_MIXED_ONE_LAUNCH) mixed(sp);
      else { f(IntK<2>{}, IntK<0>{}, sp); f(IntK<2>{}, IntK<2>{}, sp); f(IntK<2>{}, IntK<-1>{}, sp); }
    } else if (J == 4) {
      if (split_layouts(4) && cf.n_real == 0) f(IntK<4>{}, IntK<0>{}, sp);
      f(IntK<4>{}, IntK<-1>{}, sp);
    } else {
      return with_J<3, 8>(J, [&](auto jj) { f(jj, IntK<-1>{}, sp); });
    }
    return true;
  };
  return rs.sp.nseg ? by_layout(IntK<1>{}) : by_layout(IntK<0>{});
}
// the grid of a *_mixed_kernel launch (mixed): the complex-term draws are padded to whole waves (mixed_draw) -- a wave more than
// the draws fill -- and blockIdx.z is the layout variant
inline dim3 mixed_grid(const dim3& egrid) { return dim3(egrid.x + 1, egrid.y, 2); }
// the widest state of the one-lane tree kernel and of badj_prep: 8; every width when the LDS kernels for wide states are
// switched off (EXO_GP_WIDE_LDS = 0)
constexpr int kNarrowMaxJ = EXO_GP_WIDE_LDS ? kWideMinJ - 1 : EXO_GP_MAX_J;
// the SEQUENTIAL kernels (and the O(N) utilities) take state widths up to EXO_GP_MAX_J = 16 (a draw on a DPP row of 16 lanes
// above 8): celerite2, the reference's dependency (setup.py:36), has no limit, and two RotationTerms + an SHO term -- J = 10 --
// is an ordinary stellar-variability model.
static_assert(kLaneMaxJ <= 6, "the one-lane chunk kernels (chunk_adj: roles 0 .. J + 1 on a group of eight lanes) stop at 6");
static_assert(kLaneMaxJ >= 2, "with_layouts: compile-time layouts for J <= 2; J > 2 takes run-time flags");
// the scan trees on groups of eight lanes (celerite_tree_group_kernel): J = 3 .. 8
constexpr bool group_trees(int J) { return EXO_GP_GROUP_TREES && J >= 3 && J <= 8; }

}  // namespace

extern "C" {

int64_t exo_celerite_state_doubles(int64_t n, int64_t n_draw, int32_t n_real, int32_t n_complex, int32_t n_chunks) {
  const int64_t J = n_real + 2 * (int64_t)n_complex;
  if (n_chunks >= 0) n_chunks &= ~EXO_GP_PREPARE_ADJOINT;   // (the flag changes nothing in the workspace)
  if (n < 0 || n_draw < 0 || J < 1 || J > EXO_GP_MAX_J || n_chunks < 0) return -1;
  const int64_t base = seq_state_doubles(n, n_draw, (int)J);
  if (n == 0 || n_draw == 0) return base;
  const ChunkGeom cg = chunk_plan(n, n_draw, (int)J, n_chunks);
  if (cg.C <= 1) return base;
  return base + chunk_ws(n, n_draw, (int)J, cg).total();
}

// The number of chunks the plan takes by default -- for a caller who wants to pass it explicitly (the same value to
// exo_celerite_state_doubles and to both calls of a pair).  sparse != 0: the plan the SPARSE entries do best with -- twice as
// many chunks (of at least 32 cadences) as a dense series gets: the waves of a sparse launch are uneven (slow exactly while a
// draw is inside a transit), and with two rounds of them the short ones fill the tail (C3: 3.68 -> 3.59 ms).  1: sequential.
int32_t exo_celerite_default_chunks(int64_t n, int64_t n_draw, int32_t n_real, int32_t n_complex, int32_t sparse) {
  const int64_t J = n_real + 2 * (int64_t)n_complex;
  if (n < 0 || n_draw < 1 || J < 1 || J > EXO_GP_MAX_J) return 1;
  const ChunkGeom cg = chunk_plan(n, n_draw, (int)J, 0);
  if (cg.C <= 1 || !sparse || !cg.lane || J > 2) return cg.C;
  int64_t C = 2 * (int64_t)cg.C;
  if (C > n / 32) C = n / 32;
  return chunk_plan(n, n_draw, (int)J, (int32_t)(C < 2 ? 2 : C)).C;
}

// ---- the adjoint scan beside the forward chunk kernel (EXO_GP_PREPARE_ADJOINT, include/exoplanet_amd.h) -------------------------
// What the reverse call does before its chunk kernel -- adjoint elements (badj_prep), the robust route's own (chunk_adj), the
// scan (B') as a tree: 14-26 short launches, each an item's dependent latency, 0.13-0.17 ms at the C5 shape -- needs nothing of
// the forward chunk kernel: the elements and the entering states (B) are there before it starts, and the adjoint is LINEAR in
// the cotangent of the log-likelihood.  With the flag the forward call works it out for a cotangent of ONE, the scan on a second
// stream while the chunk kernel (one wave per SIMD at J >= 4, bound by its checkpoint stores) runs on the caller's, and the
// reverse chunk kernels scale the adjoint states by the draw's cotangent as they load them (ChunkGeom::prep; a cotangent of
// exactly 1 -- loglike.sum().backward() -- gives the bits of the serial order).  What goes where is decided by registers: a kernel
// that needs more than the forward chunk kernel's waves leave free on a SIMD (badj_prep 482, chunk_adj 512 at J = 6 against 280
// taken of 512) does not run beside it, it waits for it -- and everything queued behind it on its stream with it; those stay on the
// caller's stream, in front of the fork.  chunk_adj reads the forward checkpoints of the draws on the robust route, so those
// draws' recurrences run first and alone (ChunkGeom::which).  Inside a stream capture the second stream joins the capture
// through the two events, so a replayed graph carries the fork; eagerly they order the streams the same way.
#ifndef EXO_GP_SIDE_MAX_DEVICES
#define EXO_GP_SIDE_MAX_DEVICES 64
#endif
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
static SideStream* side_stream() {
  // one per host thread and device: an event recorded by two threads at once would order the wrong streams
  thread_local SideStream tl[EXO_GP_SIDE_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= EXO_GP_SIDE_MAX_DEVICES) return nullptr;
  SideStream& ss = tl[dev];
  if (!ss.s) {
    if (hipStreamCreateWithFlags(&ss.s, hipStreamNonBlocking) != hipSuccess) { ss.s = nullptr; (void)hipGetLastError(); return nullptr; }
    if (hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ss.join, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
  }
  return (ss.fork && ss.join) ? &ss : nullptr;
}
// the second stream, ordered behind everything issued on `st` so far; nullptr: none to be had
static SideStream* fork_side(hipStream_t st) {
  SideStream* q = side_stream();
  if (q && (hipEventRecord(q->fork, st) != hipSuccess || hipStreamWaitEvent(q->s, q->fork, 0) != hipSuccess)) {
    (void)hipGetLastError();
    q = nullptr;
  }
  return q;
}

extern "C++" {   // (templates: the entry points below are extern "C")
// a level of the scan trees on groups of eight lanes (J = 3 .. 8) -- also a level of the fine elements' pairwise composition
template <bool ADJ, bool DOWN>
static void launch_tree_group(const TreeOp& op, int J, int64_t n_draw, double* state, hipStream_t st) {
  const dim3 ggrid((unsigned)(((int64_t)op.n_item * n_draw + kScanBlock / 8 - 1) / (kScanBlock / 8)));
  with_J<3, 8>(J, [&](auto jj) {
    hipLaunchKernelGGL((celerite_tree_group_kernel<decltype(jj)::value, ADJ, DOWN>), ggrid, dim3(kScanBlock), 0, st, op, state);
  });
}

// The scan trees: (B) (ADJ = false: the entering states) and (B') (ADJ = true: the adjoint states, over positions
// p = C - 1 - chunk).  A launch per level (tree_scan); J <= 2 two levels per launch (tree_scan4); J = 3 .. 8 on groups of eight
// lanes, the top levels as one serial chain (tree_scan_top); J >= 9 a block per item, matrices in LDS (celerite_tree_wide_kernel).
// seed(): the caller's -- the initial state at ws.tree_state(ws.tree_top()).
template <bool ADJ, class Seed>
static void launch_scan_tree(const ChunkWs& ws, int J, int64_t n_draw, double* state, hipStream_t st, Seed&& seed) {
  const dim3 block(kWave);
  auto level = [&](const TreeOp& op, bool down) {
    exo::with_flag(down, [&](auto dn) {
      constexpr bool DOWN = decltype(dn)::value;
      const dim3 tgrid((unsigned)(((int64_t)op.n_item * n_draw + kWave - 1) / kWave));
      if (group_trees(J)) {
        launch_tree_group<ADJ, DOWN>(op, J, n_draw, state, st);
      } else if (EXO_GP_WIDE_LDS && J >= kWideMinJ) {
        hipLaunchKernelGGL((celerite_tree_wide_kernel<ADJ, DOWN>), dim3((unsigned)((int64_t)op.n_item * n_draw)), dim3(256), 0, st, op,
                           state);
      } else if (!ADJ && !DOWN && J >= 3 && J <= 8) {
        // composing two filtering elements keeps ~5 J x J matrices alive around the solve: one lane per
        // item spills 2 KB at J = 6 and crawls (76 us per level); a wave per item with the tiles in LDS
        hipLaunchKernelGGL(celerite_compose_lds_kernel, dim3((unsigned)(op.n_item * n_draw)), block, 0, st, op, state);
      } else {
        with_J<1, kNarrowMaxJ>(J, [&](auto jj) {
          hipLaunchKernelGGL((celerite_tree_kernel<decltype(jj)::value, ADJ, DOWN>), tgrid, block, 0, st, op, state);
        });
      }
    });
  };
  if (EXO_GP_TREE4 && J <= 2) {
    auto level_pair = [&](const TreeOp& a, const TreeOp& b, bool down) {
      const dim3 tgrid((unsigned)(((int64_t)b.n_item * n_draw + kWave - 1) / kWave));
      with_J<1, 2>(J, [&](auto jj) {
        exo::with_flag(down, [&](auto dn) {
          hipLaunchKernelGGL((celerite_tree4_kernel<decltype(jj)::value, ADJ, decltype(dn)::value>), tgrid, block, 0, st, a, b, state);
        });
      });
    };
    tree_scan4(ws, J, ADJ, level, level_pair, seed);
  } else {
    auto serial = [&](const TreeOp& op) {
      const dim3 sgrid((unsigned)((n_draw + kScanBlock / 8 - 1) / (kScanBlock / 8)));
      with_J<3, 8>(J, [&](auto jj) {
        hipLaunchKernelGGL((celerite_tree_serial_group_kernel<decltype(jj)::value, ADJ>), sgrid, dim3(kScanBlock), 0, st, op, state);
      });
    };
    tree_scan_top(ws, J, ADJ, group_trees(J) ? tree_serial_level(ws, J) : ws.tree_top(), level, seed, serial);
  }
}
}  // extern "C++"

// What celerite_fwd and celerite_vjp make of a call's arguments before anything is launched: the flag that rides on n_chunks
// taken off, the phases' origin set (cf), the argument and workspace checks, the chunk plan -- a pure function of the arguments,
// so both calls of a pair get the same one -- and the launch shapes.  out_ok: the call's own pointers are there.
struct GpPlan {
  int rc;          // EXO_OK, or what the call returns at once
  bool prep;       // EXO_GP_PREPARE_ADJOINT: the forward call runs the adjoint scan (celerite_adjoint_scan), the reverse call finds it done
  int J;
  ChunkGeom cg;    // (state == nullptr: none, a call without a state buffer runs the sequential kernel alone)
  dim3 block;      // one wave
  dim3 grid, per_draw;    // the draws on groups of G lanes (sequential and lane-group kernels) / one per lane
  dim3 cgrid, egrid;      // ... each by the chunks
  hipStream_t st;
};
static GpPlan gp_plan(const double* t, const Series& resid, const double* diag, int64_t n_diag, int64_t n, Coefs& cf, int64_t n_draw,
                      bool out_ok, const double* state, int64_t state_doubles, int32_t n_chunks, void* stream) {
  GpPlan pl{};
  pl.prep = n_chunks >= 0 && (n_chunks & EXO_GP_PREPARE_ADJOINT) != 0;   // (a flag riding on n_chunks: the same in both calls of a pair)
  if (pl.prep) n_chunks &= ~EXO_GP_PREPARE_ADJOINT;
  cf.origin = n > 0 ? t : nullptr;   // phases from the first time stamp (Coefs::origin)
  pl.rc = EXO_ERR_INVALID_ARGUMENT;
  if (!gp_args_ok(n, n_diag, cf.n_real, cf.n_complex, n_draw, n_chunks) || !t || !resid.y || !diag || !out_ok ||
      (cf.n_real > 0 && !cf.real) || (cf.n_complex > 0 && !cf.cplx))
    return pl;
  pl.rc = EXO_ERR_WORKSPACE;
  if (state && state_doubles < exo_celerite_state_doubles(n, n_draw, cf.n_real, cf.n_complex, n_chunks)) return pl;
  pl.rc = EXO_OK;
  pl.J = cf.J();
  const int64_t per_wave = kWave / group_width(pl.J);
  pl.block = dim3(kWave);
  pl.grid = dim3((unsigned)((n_draw + per_wave - 1) / per_wave));
  pl.per_draw = dim3((unsigned)((n_draw + kWave - 1) / kWave));
  if (state) pl.cg = chunk_plan(n, n_draw, pl.J, n_chunks);
  pl.cgrid = dim3(pl.grid.x, (unsigned)pl.cg.C);
  pl.egrid = dim3(pl.per_draw.x, (unsigned)pl.cg.C);
  pl.st = (hipStream_t)stream;
  return pl;
}

// gloglike == nullptr: for a cotangent of one (the forward call's; ChunkGeom::prep)
// parts: 1 = the adjoint elements (badj_prep, chunk_adj), 2 = the scan over them, 3 = both
static int celerite_adjoint_scan(const double* t, Series resid, const double* diag, int64_t n_diag, int64_t n, Coefs cf,
                                 int64_t n_draw, const double* gloglike, double* wstate, const ChunkGeom& cg, hipStream_t st,
                                 int parts = 3) {
  const int J = cf.J();
  const dim3 block(kWave);
  const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
  const dim3 per_draw((unsigned)((n_draw + kWave - 1) / kWave));
  if (parts & 1) {
    if (EXO_GP_WIDE_LDS && J >= kWideMinJ) {
      hipLaunchKernelGGL(celerite_badj_prep_wide_kernel, dim3((unsigned)n_draw, (unsigned)(cg.C - 1)), dim3(256), 0, st, gloglike, n,
                         n_draw, J, wstate, cg, cf.row);
    } else if (EXO_GP_GROUP_TREES && J >= EXO_GP_BADJ_GROUP_MIN_J && J <= 8) {
      const dim3 ggrid((unsigned)(((int64_t)(cg.C - 1) * n_draw + kScanBlock / 8 - 1) / (kScanBlock / 8)));
      with_J<3, 8>(J, [&](auto jj) {
        hipLaunchKernelGGL((celerite_badj_prep_group_kernel<decltype(jj)::value>), ggrid, dim3(kScanBlock), 0, st, gloglike, n, n_draw,
                           wstate, cg, cf.row);
      });
    } else if (!with_J<1, kNarrowMaxJ>(J, [&](auto jj) {
                 hipLaunchKernelGGL((celerite_badj_prep_kernel<decltype(jj)::value>), dim3(per_draw.x, (unsigned)(cg.C - 1)), block, 0,
                                    st, gloglike, n, n_draw, wstate, cg, cf.row);
               })) {
      return EXO_ERR_INVALID_ARGUMENT;
    }
    if (cg.lane) {
      // draws flagged kFlagRobust: those inputs once more, from the chunks' own reverse recurrences (chunk_adj_lane)
      with_J<1, kLaneMaxJ>(J, [&](auto jj) {
        hipLaunchKernelGGL((celerite_chunk_adj_kernel<decltype(jj)::value>),
                           dim3((unsigned)(cg.C - 1), (unsigned)((n_draw + kAdjDraws - 1) / kAdjDraws)), block, 0, st, t, resid, diag,
                           n_diag, n, cf, n_draw, gloglike, wstate, cg);
      });
    }
  }
  if (parts & 2) {
    // (B') as a tree over positions p = C - 1 - chunk: adjoint elements of chunks C - 1 .. 1, zero initial adjoint
    bool ok = true;
    launch_scan_tree<true>(ws, J, n_draw, wstate, st, [&]() {
      ok = exo::zero_fill_async(wstate + ws.tree_state(ws.tree_top()), (int64_t)ws.B() * n_draw, st);   // (never a memset node: exo_math.hpp)
    });
    if (!ok) return EXO_ERR_LAUNCH;
  }
  return launch_status();
}

static int celerite_fwd(const double* t, Series resid, const double* diag, int64_t n_diag, int64_t n, Coefs cf,
                        int64_t n_draw, double* loglike, double* state, int64_t state_doubles, int32_t n_chunks,
                        void* stream) {
  if (n_draw == 0) return EXO_OK;
  const GpPlan pl = gp_plan(t, resid, diag, n_diag, n, cf, n_draw, loglike != nullptr, state, state_doubles, n_chunks, stream);
  if (pl.rc != EXO_OK) return pl.rc;
  const int J = pl.J;
  hipStream_t st = pl.st;
  if (state) {
    const ChunkGeom cg = pl.cg;
    const double* only_flagged = nullptr;
    int n_slice = 0;
    if (cg.C <= 1) {
      const int64_t n_el = n * n_draw * J;
      hipLaunchKernelGGL(celerite_prep_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, st, t, n, cf, n_draw,
                         J, state);
      if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
    } else {
      // time-parallel path: flags (+ pre-pass for flagged draws), elements, entering states,
      // recurrences per chunk, sum of the partials
      const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
      if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
            hipLaunchKernelGGL((celerite_flag_kernel<decltype(jj)::value>), pl.per_draw, pl.block, 0, st, cf, n_draw, state + ws.off_flag());
          }))
        return EXO_ERR_INVALID_ARGUMENT;
#ifndef EXO_ELEM_LG_MIN_J
#define EXO_ELEM_LG_MIN_J 7
#endif
      // the elements are built at the finest level (ChunkGeom::fine: 2^fine times more, shorter chunks) and
      // composed pairwise up to the chunks the scans and the chunk kernels work on
      const ChunkGeom cge = cg.fine ? fine_geom(n, n_draw, J, cg, cg.fine) : cg;
      const int64_t flag_at = ws.off_flag();
      const dim3 egrid_f(pl.per_draw.x, (unsigned)cge.C), cgrid_f(pl.grid.x, (unsigned)cge.C);
      if (J == 2 && cf.n_real == 0 && cf.kind && EXO_GP_MIXED_ONE_LAUNCH)   // per-draw pair kinds: no wave of mixed kinds (mixed_draw)
        hipLaunchKernelGGL(celerite_kind_partition_kernel, dim3(1), dim3(1024), 0, st, cf.kind, cf.row, n_draw,
                           reinterpret_cast<int32_t*>(state + ws.off_perm()), ws.perm_lanes());
      if (resid.sp.nseg && cg.lane)   // sparse model: the order in which the one-lane kernels' blocks take the chunks (chunk_of_block)
        hipLaunchKernelGGL(celerite_sparse_order_kernel, dim3(1), dim3(256), 0, st, resid.sp, n, n_draw, cg,
                           reinterpret_cast<int32_t*>(state + ws.off_order()));
      if (J >= EXO_ELEM_LG_MIN_J) {   // the one-lane element kernel is as fast up to J = 6 and does not fit beyond
        if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
              hipLaunchKernelGGL((celerite_elem_lg_kernel<decltype(jj)::value>), cgrid_f, pl.block, 0, st, t, resid, diag, n_diag, n, cf,
                                 n_draw, state, cge, flag_at);
            }))
          return EXO_ERR_INVALID_ARGUMENT;
      } else if (!with_layouts(
                     cf, resid,
                     [&](auto jj, auto nr, auto sp) {
                       hipLaunchKernelGGL((celerite_elem_kernel<decltype(jj)::value, decltype(nr)::value, decltype(sp)::value>), egrid_f,
                                          pl.block, 0, st, t, resid, diag, n_diag, n, cf, n_draw, state, cge, flag_at);
                     },
                     [&](auto sp) {
                       hipLaunchKernelGGL(celerite_elem_mixed_kernel<decltype(sp)::value>, mixed_grid(egrid_f), pl.block, 0,
                                          st, t, resid, diag, n_diag, n, cf, n_draw, state, cge, flag_at);
                     })) {
        return EXO_ERR_INVALID_ARGUMENT;
      }
      for (int f = cg.fine; f >= 1; --f) {
        TreeOp op{};
        op.J = J; op.n_draw = n_draw;
        op.src_elem = ws.off_fine(f); op.src_n = op.src_len = cg.C << f;
        op.dst_elem = f > 1 ? ws.off_fine(f - 1) : ws.elem(0, 0, 0);
        op.n_item = cg.C << (f - 1);
        if (EXO_GP_FINE_GROUP && group_trees(J)) {
          // the scan trees' own item kernel (eight lanes per composition, 32 draws per block): the wave-per-composition LDS kernel
          // took 227 us for the 32 768 compositions of the C5 shape at J = 8, a level of the tree 26 us for 16 384
          launch_tree_group<false, false>(op, J, n_draw, state, st);
        } else {
          hipLaunchKernelGGL(celerite_compose_lds_kernel, dim3((unsigned)(op.n_item * n_draw)), pl.block, 0, st, op, state);
        }
      }
      // after the element kernel: it may flag more draws (measurement variance too small)
      hipLaunchKernelGGL(celerite_prep_flagged_kernel, dim3(8, (unsigned)n_draw), dim3(256), 0, st, t, n, cf, n_draw, J,
                         state, state + ws.off_flag());
      // (B) as a tree: compose up to one position, seed it with the initial state, apply back down
      launch_scan_tree<false>(ws, J, n_draw, state, st, [&]() {
        with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
          hipLaunchKernelGGL((celerite_scan_init_kernel<decltype(jj)::value>), pl.grid, pl.block, 0, st, t, cf, n_draw,
                             state + ws.tree_state(ws.tree_top()));
        });
      });
      // the recurrences per chunk -- and, with pl.prep, the adjoint scan for a cotangent of one, on a second stream where there
      // is one: `ss`, joined below on every way out of chunk_recurrences (an unjoined fork invalidates a stream capture)
      SideStream* ss = nullptr;
      auto chunk_recurrences = [&]() -> int {
        ChunkGeom fwd_cg = cg;   // (the draws of the one-lane launch: ChunkGeom::which)
        auto launch_fwd = [&]() {
          return with_layouts(
              cf, resid,
              [&](auto jj, auto nr, auto sp) {
                constexpr int JJ = decltype(jj)::value;
                hipLaunchKernelGGL((celerite_chunk1_fwd_kernel<(JJ <= kLaneMaxJ ? JJ : 1), decltype(nr)::value, decltype(sp)::value>),
                                   pl.egrid, pl.block, 0, st, t, resid, diag, n_diag, n, cf, n_draw, state, fwd_cg);
              },
              [&](auto sp) {
                hipLaunchKernelGGL(celerite_chunk1_fwd_mixed_kernel<decltype(sp)::value>, mixed_grid(pl.egrid), pl.block, 0, st, t,
                                   resid, diag, n_diag, n, cf, n_draw, state, fwd_cg);
              });
        };
        if (cg.lane) {
          // draws flagged kFlagRobust: their entering states once more -- Newton iterations from the trees' (J <= 2: the elements
          // applied one after the other)
          const dim3 rgrid((unsigned)(J >= 3 ? (n_draw + kWave / 8 - 1) / (kWave / 8) : pl.per_draw.x));
          if (EXO_GP_ROBUST_NEWTON && J >= 3) {
            with_J<3, kLaneMaxJ>(J, [&](auto jj) {
              hipLaunchKernelGGL((celerite_robust_newton_kernel<decltype(jj)::value>), dim3((unsigned)n_draw), dim3(kNewtonBlock), 0,
                                 st, n, cg, n_draw, state);
            });
          } else {
            with_J<1, kLaneMaxJ>(J, [&](auto jj) {
              hipLaunchKernelGGL((celerite_robust_scan_kernel<decltype(jj)::value>), rgrid, pl.block, 0, st, t, cf, n, cg, n_draw, state);
            });
          }
        }
        if (pl.prep) {
          // The adjoint elements first, on the caller's stream: badj_prep and chunk_adj take a SIMD's whole register file (482 /
          // 512 registers at J = 6; J = 7, 8: the lane-group badj_prep), so beside the forward chunk kernel -- a resident wave on
          // every SIMD -- they would only wait for it, the scan behind them.  chunk_adj reads the forward checkpoints of the draws
          // on the robust route: their recurrences run now (ChunkGeom::which = 1; no such draw: two launches that return at once),
          // everybody else's beside the scan.  J >= 9: badj_prep is a block per item, 81 registers: with the scan on the second
          // stream.
          const bool wide = EXO_GP_WIDE_LDS && J >= kWideMinJ;
          if (cg.lane) {
            fwd_cg.which = 1;
            if (!launch_fwd()) return EXO_ERR_INVALID_ARGUMENT;
            fwd_cg.which = 2;
          }
          if (!wide) {
            const int rc = celerite_adjoint_scan(t, resid, diag, n_diag, n, cf, n_draw, nullptr, state, cg, st, 1);
            if (rc != EXO_OK) return rc;
          }
          ss = fork_side(st);
          const int rc = celerite_adjoint_scan(t, resid, diag, n_diag, n, cf, n_draw, nullptr, state, cg, ss ? ss->s : st, wide ? 3 : 2);
          if (rc != EXO_OK) return rc;
        }
        if (cg.lane) return launch_fwd() ? EXO_OK : EXO_ERR_INVALID_ARGUMENT;
        const bool launched = with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
          hipLaunchKernelGGL((celerite_chunk_fwd_kernel<decltype(jj)::value>), pl.cgrid, pl.block, 0, st, t, resid, diag, n_diag, n, cf, n_draw,
                             state, cg);
        });
        return launched ? EXO_OK : EXO_ERR_INVALID_ARGUMENT;
      };
      const int rc = chunk_recurrences();
      // join: the sums below (and the caller) wait for the second stream.  (No second stream to be had: the scan went in line,
      // before the chunk kernel -- the reverse call expects it done.)
      const bool joined = !ss || (hipEventRecord(ss->join, ss->s) == hipSuccess && hipStreamWaitEvent(st, ss->join, 0) == hipSuccess);
      if (rc != EXO_OK) return rc;
      if (!joined) return EXO_ERR_LAUNCH;
      {
        const int S = chunk_sum_slices(cg.C, 3, n_draw, 16);   // (the last kernel's lanes add the S partials themselves)
        hipLaunchKernelGGL(celerite_chunk_slice_sum_kernel, dim3(pl.per_draw.x, 3, (unsigned)S), pl.block, 0, st, state + ws.off_part(), 3,
                           cg.C, S, n_draw);
        n_slice = S;   // (the sums' last step: the unflagged lanes of the sequential kernel below)
      }
      if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
      only_flagged = state + ws.off_flag();
    }
    if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
          hipLaunchKernelGGL((celerite_fwd_kernel<decltype(jj)::value, true>), pl.grid, pl.block, 0, st, t, resid, diag, n_diag, n, cf, n_draw,
                             loglike, state, only_flagged, cg, n_slice);
        }))
      return EXO_ERR_INVALID_ARGUMENT;
  } else if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
               hipLaunchKernelGGL((celerite_fwd_kernel<decltype(jj)::value, false>), pl.grid, pl.block, 0, st, t, resid, diag, n_diag, n, cf,
                                  n_draw, loglike, state, (const double*)nullptr, ChunkGeom{}, 0);
             })) {
    return EXO_ERR_INVALID_ARGUMENT;
  }
  return launch_status();
}

static int celerite_vjp(const double* t, Series resid, const double* diag, int64_t n_diag, int64_t n, Coefs cf,
                        int64_t n_draw, const double* gloglike, const double* state, int64_t state_doubles,
                        int32_t n_chunks, double* gresid, double gsign, double* gdiag, double* gdiag_sum,
                        double* gcoef_real, double* gcoef_complex, void* stream) {
  if (n_draw == 0) return EXO_OK;
  const bool out_ok = gloglike && state && gresid && (cf.n_real == 0 || gcoef_real) && (cf.n_complex == 0 || gcoef_complex);
  const GpPlan pl = gp_plan(t, resid, diag, n_diag, n, cf, n_draw, out_ok, state, state_doubles, n_chunks, stream);
  if (pl.rc != EXO_OK) return pl.rc;
  const int J = pl.J;
  hipStream_t st = pl.st;
  ChunkGeom cg = pl.cg;   // the same plan as the forward call's
  cg.prep = pl.prep ? 1 : 0;
  const double* only_flagged = nullptr;
  if (cg.C > 1) {
    double* wstate = const_cast<double*>(state);   // the chunk workspace lives behind the saved factorisation
    const ChunkWs ws = chunk_ws(n, n_draw, J, cg);
    if (!pl.prep) {   // (else the forward call ran the adjoint scan)
      const int rc = celerite_adjoint_scan(t, resid, diag, n_diag, n, cf, n_draw, gloglike, wstate, cg, st);
      if (rc != EXO_OK) return rc;
    }
    if (cg.lane) {
      if (!with_layouts(
              cf, resid,
              [&](auto jj, auto nr, auto sp) {
                constexpr int JJ = decltype(jj)::value;
                hipLaunchKernelGGL((celerite_chunk1_vjp_kernel<(JJ <= kLaneMaxJ ? JJ : 1), decltype(nr)::value, decltype(sp)::value>), pl.egrid,
                                   pl.block, 0, st, t, resid, diag, n_diag, n, cf, n_draw, gloglike, wstate, cg, gresid, gdiag, gsign);
              },
              [&](auto sp) {
                hipLaunchKernelGGL(celerite_chunk1_vjp_mixed_kernel<decltype(sp)::value>, mixed_grid(pl.egrid), pl.block, 0, st, t,
                                   resid, diag, n_diag, n, cf, n_draw, gloglike, wstate, cg, gresid, gdiag, gsign);
              }))
        return EXO_ERR_INVALID_ARGUMENT;
    } else if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
                 hipLaunchKernelGGL((celerite_chunk_vjp_kernel<decltype(jj)::value>), pl.cgrid, pl.block, 0, st, t, n, cf, n_draw, gloglike,
                                    wstate, cg, gresid, gdiag, gsign, resid);
               })) {
      return EXO_ERR_INVALID_ARGUMENT;
    }
    {
      const int K = 4 * J + 1, S = chunk_sum_slices(cg.C, K, n_draw);
      hipLaunchKernelGGL(celerite_chunk_slice_sum_kernel, dim3(pl.per_draw.x, (unsigned)K, (unsigned)S), pl.block, 0, st,
                         wstate + ws.off_gpart(), K, cg.C, S, n_draw);
      // (the S partial sums of the 4 J + 1 quantities once more, into chunk 0's slots: a lane of the last kernel would read
      // S rows per quantity one after the other -- 41 at the C5 shape)
      if (S > 1)
        hipLaunchKernelGGL(celerite_chunk_slice_sum_kernel, dim3(pl.per_draw.x, (unsigned)K, 1), pl.block, 0, st, wstate + ws.off_gpart(), K,
                           S, 1, n_draw);
      // (the combination into gcoef_*: the unflagged lanes of the sequential kernel below)
    }
    if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
    only_flagged = state + ws.off_flag();
  }
  if (!with_J<1, EXO_GP_MAX_J>(J, [&](auto jj) {
        hipLaunchKernelGGL((celerite_vjp_kernel<decltype(jj)::value>), pl.grid, pl.block, 0, st, t, diag, n_diag, n, cf, n_draw, gloglike,
                           state, gresid, gdiag, gdiag_sum, gcoef_real, gcoef_complex, only_flagged, gsign, resid, cg);
      }))
    return EXO_ERR_INVALID_ARGUMENT;
  return launch_status();
}

int exo_celerite_loglike_fwd_f64(const double* t, const double* resid, const double* diag, int64_t n_diag,
                                 int64_t n, const double* coef_real, int32_t n_real, const double* coef_complex,
                                 int32_t n_complex, const int32_t* pair_kind, int64_t n_draw, double* loglike,
                                 double* state, int64_t state_doubles, int32_t n_chunks, void* stream) {
  return celerite_fwd(t, Series{resid, nullptr, 0}, diag, n_diag, n, Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex},
                      n_draw, loglike, state, state_doubles, n_chunks, stream);
}

int exo_celerite_loglike_vjp_f64(const double* t, const double* resid, const double* diag, int64_t n_diag, int64_t n,
                                 const double* coef_real, int32_t n_real, const double* coef_complex,
                                 int32_t n_complex, const int32_t* pair_kind, int64_t n_draw, const double* gloglike,
                                 const double* state, int64_t state_doubles, int32_t n_chunks, double* gresid,
                                 double* gdiag, double* gdiag_sum, double* gcoef_real, double* gcoef_complex,
                                 void* stream) {
  return celerite_vjp(t, Series{resid, nullptr, 0}, diag, n_diag, n, Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex},
                      n_draw, gloglike, state, state_doubles, n_chunks, gresid, 1.0, gdiag, gdiag_sum, gcoef_real,
                      gcoef_complex, stream);
}

int exo_celerite_loglike_obs_fwd_f64(const double* t, const double* obs, const double* model, const double* diag,
                                     int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                     const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                     int64_t n_draw, double* loglike, double* state, int64_t state_doubles,
                                     int32_t n_chunks, void* stream) {
  if (n_draw > 0 && !obs) return EXO_ERR_INVALID_ARGUMENT;
  return celerite_fwd(t, Series{model, obs, 0}, diag, n_diag, n, Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex},
                      n_draw, loglike, state, state_doubles, n_chunks, stream);
}

int exo_celerite_loglike_obs_vjp_f64(const double* t, const double* obs, const double* model, const double* diag,
                                     int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                     const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                     int64_t n_draw, const double* gloglike, const double* state,
                                     int64_t state_doubles, int32_t n_chunks, double* gmodel, double* gdiag,
                                     double* gdiag_sum, double* gcoef_real, double* gcoef_complex, void* stream) {
  if (n_draw > 0 && !obs) return EXO_ERR_INVALID_ARGUMENT;
  return celerite_vjp(t, Series{model, obs, 0}, diag, n_diag, n, Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex},
                      n_draw, gloglike, state, state_doubles, n_chunks, gmodel, -1.0, gdiag, gdiag_sum, gcoef_real,
                      gcoef_complex, stream);
}

int exo_celerite_loglike_obs_fwd_cm_f64(const double* t, const double* obs, const double* model_cm, const double* diag,
                                        int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                        int64_t n_draw, double* loglike, double* state, int64_t state_doubles,
                                        int32_t n_chunks, void* stream) {
  if (n_draw > 0 && !obs) return EXO_ERR_INVALID_ARGUMENT;
  return celerite_fwd(t, Series{model_cm, obs, n_draw}, diag, n_diag, n,
                      Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex}, n_draw, loglike, state, state_doubles,
                      n_chunks, stream);
}

int exo_celerite_loglike_obs_vjp_cm_f64(const double* t, const double* obs, const double* model_cm, const double* diag,
                                        int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                        int64_t n_draw, const double* gloglike, const double* state,
                                        int64_t state_doubles, int32_t n_chunks, double* gmodel_cm, double* gdiag,
                                        double* gdiag_sum, double* gcoef_real, double* gcoef_complex, void* stream) {
  if (n_draw > 0 && !obs) return EXO_ERR_INVALID_ARGUMENT;
  return celerite_vjp(t, Series{model_cm, obs, n_draw}, diag, n_diag, n,
                      Coefs{coef_real, coef_complex, pair_kind, n_real, n_complex}, n_draw, gloglike, state, state_doubles,
                      n_chunks, gmodel_cm, -1.0, gdiag, gdiag_sum, gcoef_real, gcoef_complex, stream);
}

// the model as the light-curve sweep's SPARSE output (exo_sparse_model): segments of cadences + their values
static bool sparse_series(const exo_sparse_model* m, const double* obs, int64_t n, Series* out) {
  if (!m || !obs || !m->nseg || !m->seg || !m->off || !m->vals || m->seg_step < 1 || m->hi_at < 0 || m->hi_at >= m->seg_step ||
      m->seg_row < 0 || m->off_row < 0 || m->val_row < 0 || n > 0x7fffffff)
    return false;
  out->y = m->vals;
  out->obs = obs;
  out->cm = 0;
  out->sp.nseg = m->nseg; out->sp.seg = m->seg; out->sp.off = m->off;
  out->sp.seg_row = m->seg_row; out->sp.off_row = m->off_row; out->sp.val_row = m->val_row;
  out->sp.seg_step = m->seg_step; out->sp.hi_at = m->hi_at;
  out->sp.row_of_draw = m->row_of_draw;
  return true;
}

int exo_celerite_loglike_sparse_fwd_f64(const double* t, const double* obs, const exo_sparse_model* model, const double* diag,
                                        int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                        int64_t n_draw, double* loglike, double* state, int64_t state_doubles,
                                        int32_t n_chunks, void* stream) {
  if (n_draw == 0) return EXO_OK;
  Series rs{};
  if (!sparse_series(model, obs, n, &rs)) return EXO_ERR_INVALID_ARGUMENT;
  Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex};
  cf.row = model->row_of_draw;     // (every per-draw array of the call in the caller's order: Coefs::row)
  return celerite_fwd(t, rs, diag, n_diag, n, cf, n_draw, loglike, state, state_doubles, n_chunks, stream);
}

int exo_celerite_loglike_sparse_vjp_f64(const double* t, const double* obs, const exo_sparse_model* model, const double* diag,
                                        int64_t n_diag, int64_t n, const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                        int64_t n_draw, const double* gloglike, const double* state,
                                        int64_t state_doubles, int32_t n_chunks, double* gvals, double* gdiag,
                                        double* gdiag_sum, double* gcoef_real, double* gcoef_complex, void* stream) {
  if (n_draw == 0) return EXO_OK;
  Series rs{};
  if (!sparse_series(model, obs, n, &rs)) return EXO_ERR_INVALID_ARGUMENT;
  Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex};
  cf.row = model->row_of_draw;
  return celerite_vjp(t, rs, diag, n_diag, n, cf, n_draw, gloglike, state, state_doubles, n_chunks, gvals, -1.0, gdiag, gdiag_sum,
                      gcoef_real, gcoef_complex, stream);
}

// The order in which a sparse model's draws are best handed to the celerite kernels (exo_sparse_model.row_of_draw): ascending
// mean spacing of a draw's segments -- the period, in cadences: draws with neighbouring periods keep their transits together all
// along the series -- the start of the first segment breaking ties (draws with fewer than two segments: by that alone), then the
// draw's index.  One block: keys into LDS, a bitonic sort of (key, index) pairs.  Up to kOrderMaxDraws draws.
int exo_sparse_model_order(const exo_sparse_model* model, int64_t n_draw, int32_t* order, void* stream) {
  if (n_draw == 0) return EXO_OK;
  if (!model || !order || !model->nseg || !model->seg || model->seg_step < 1 || n_draw < 0 || n_draw > kOrderMaxDraws)
    return EXO_ERR_INVALID_ARGUMENT;
  SparseSegs sp{};
  sp.nseg = model->nseg; sp.seg = model->seg; sp.seg_row = model->seg_row; sp.seg_step = model->seg_step; sp.hi_at = model->hi_at;
  hipLaunchKernelGGL(celerite_draw_order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sp, n_draw, order);
  return launch_status();
}

int exo_celerite_dot_tril_f64(const double* t, const double* diag, int64_t n_diag, int64_t n, const double* coef_real,
                              int32_t n_real, const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                              int64_t n_draw, const double* x, double* z, void* stream) {
  if (n_draw == 0) return EXO_OK;
  if (!gp_args_ok(n, n_diag, n_real, n_complex, n_draw, 0) || !t || !diag || !x || !z || (n_real > 0 && !coef_real) ||
      (n_complex > 0 && !coef_complex))
    return EXO_ERR_INVALID_ARGUMENT;
  const Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex, n > 0 ? t : nullptr};
  const dim3 grid((unsigned)((n_draw + kWave - 1) / kWave)), block(kWave);
  if (!with_J<1, EXO_GP_MAX_J>(cf.J(), [&](auto jj) {
        hipLaunchKernelGGL((celerite_dot_tril_kernel<decltype(jj)::value>), grid, block, 0, (hipStream_t)stream, t, diag, n_diag, n, cf,
                           n_draw, x, z);
      }))
    return EXO_ERR_INVALID_ARGUMENT;
  return launch_status();
}

int exo_celerite_predict_f64(const double* t, int64_t n, const double* alpha, const double* coef_real, int32_t n_real,
                             const double* coef_complex, int32_t n_complex, const int32_t* pair_kind, int64_t n_draw,
                             const double* tq, int64_t m, double* mu, void* stream) {
  if (n_draw == 0 || m == 0) return EXO_OK;
  if (!gp_args_ok(n, 1, n_real, n_complex, n_draw, 0) || m < 0 || !t || !alpha || !tq || !mu ||
      (n_real > 0 && !coef_real) || (n_complex > 0 && !coef_complex))
    return EXO_ERR_INVALID_ARGUMENT;
  const Coefs cf{coef_real, coef_complex, pair_kind, n_real, n_complex, n > 0 ? t : nullptr};
  const dim3 grid((unsigned)((n_draw + kWave - 1) / kWave)), block(kWave);
  if (!with_J<1, EXO_GP_MAX_J>(cf.J(), [&](auto jj) {
        hipLaunchKernelGGL((celerite_predict_kernel<decltype(jj)::value>), grid, block, 0, (hipStream_t)stream, t, n, alpha, cf, n_draw,
                           tq, m, mu);
      }))
    return EXO_ERR_INVALID_ARGUMENT;
  return launch_status();
}

}  // extern "C"

