// exo_transit.hip -- the Kepler / limb-darkened light curve on the hot path (gfx950, wave64, fp64 VALU; no MFMA -- nothing
// here is a dense contraction): this file is the one translation unit and holds the HOST side -- the sweep request, the
// entry points' argument rules, the launches and the C ABI.  The kernels are in the headers beside it, one per path:
//   exo_transit_sample.hpp   what both paths' heavy work shares: constants, gradient slots, staged per-planet constants, timing
//                            tables, eval_sample (one sample: Kepler solve, solution vector, flux, reverse sweep), reduce_columns
//   exo_transit_window.hpp   conjunction windows of a record (window_lanes, transit_window_kernel) and the phase test
//   exo_transit_list.hpp     the list path
//   exo_transit_runs.hpp     the run-enumeration path
//   exo_transit_merge.hpp    the merged sparse model (sparse_merge_*_kernel)
//
// TWO paths through a sweep (runs_path() decides):
// * RUN ENUMERATION (sorted times, one exposure time -- or none -- for all cadences, no EXO_FLAG_EXACT_SCAN; timing tables
//   allowed when the sweep has transits only and no light delay): what every BASELINE config and every sampler leg takes.
//   A sweep (value, or value + VJP) is two launches, three when a draw is shared by several blocks:
//     enumerate   transit_enum_kernel<true>: windows and runs in one launch on the caller's word for sorted times; otherwise
//                 transit_window_kernel (+ sortedness blocks), then transit_enum_kernel<false> or transit_enum_ttv_kernel
//     runs        transit_runs_kernel: the solved cadences of the runs; a block that owns its draw (>= 512 draws) also finishes it
//     finish      transit_finish_kernel: block partials -> gparams / gld / sum(gflux flux); the runs' values to their cadences
//
// * LIST PATH (per-cadence exposure times, EXO_FLAG_EXACT_SCAN, timing tables together with occultations or light delay):
//   four launches, every cadence classified:
//     window      transit_window_kernel: per (draw, planet), where in mean anomaly an overlap is possible
//     scan        transit_scan_kernel: which cadences can overlap the disk -> per-wave work lists; fill blocks: flux = 0
//     heavy       transit_heavy_kernel: the listed cadences, dense: the same eval_sample; per-block gradient partials
//     reduce      transit_vjp_reduce_kernel: block partials -> gparams, gld, sum(gflux flux)
//
// Reference lines restated by the kernels (all under the reference's src/exoplanet):
//   orbits/keplerian.py:324-334   M = (t - t0 - tref) n ; kepler(M, e)
//   orbits/keplerian.py:400-409   r = a (1-e^2)/(1+e cos f) ; rotate
//   orbits/keplerian.py:303-314   omega rotation, inclination projection
//   orbits/keplerian.py:729-731,765-769   in-transit window test
//   light_curves/limb_dark.py:178-226     exposure stencil, b, los, s.c - 1, los > 0
//   light_curves/secondary_eclipse.py:45-70   flipped orbit + blend
//   orbits/ttv.py:158-187         bin edges / values, searchsorted, t - transit time of the bin (the TTV variants)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_contact.hpp"
#include "exo_math.hpp"
#include "exo_pack_core.hpp"
#include "exo_transit_list.hpp"
#include "exo_transit_merge.hpp"
#include "exo_transit_runs.hpp"
#include "exo_transit_sample.hpp"
#include "exo_transit_window.hpp"

namespace {

// (the reference's standalone Ops -- kepler, quad_solution_vector, contact_points -- are exo_ops.hip)
inline int launch_status() { return hipGetLastError() == hipSuccess ? EXO_OK : EXO_ERR_LAUNCH; }

// the fused likelihood (obs != nullptr): the misfit and its gradient instead of values
struct Chi2Args {
  const double* obs;
  const double* ivar;
  int64_t n_ivar;
  double* chi2;
  const NoiseIn* nz = nullptr;   // sampled mean / jitter: obs is the series y, ivar the VARIANCES
};

// lists per planet: its transits and, with EXO_FLAG_SECONDARY, its occultations
inline int events(uint32_t flags) { return (flags & EXO_FLAG_SECONDARY) ? 2 : 1; }

// ---- a sweep on the host ---------------------------------------------------------------------------------------------
// What every sweep entry is handed; an entry fills one from its arguments, and nothing below takes them one by one.
struct Sweep {
  const double* t = nullptr;
  int64_t n_cad = 0;
  const double* texp = nullptr;   // exposure times ([1] or [n_cad]; n_texp == 0: none) and their stencil of n_sub samples
  int64_t n_texp = 0;
  const double *stencil_dt = nullptr, *stencil_w = nullptr;
  int32_t n_sub = 1;
  const double *params = nullptr, *ld = nullptr;
  int64_t n_draw = 0;
  int32_t n_planet = 0;
  uint32_t flags = 0;
  Ttv ttv{};
  void* workspace = nullptr;
  int64_t workspace_bytes = 0;
  hipStream_t st = nullptr;
  bool has_ttv() const { return ttv.edges != nullptr; }
  bool secondary() const { return flags & EXO_FLAG_SECONDARY; }
  int n_ev() const { return events(flags); }
};
// What differs from call to call (nullptr: not asked for).
struct SweepOut {
  double *gparams = nullptr, *gld = nullptr, *flux_dot = nullptr;
  const double* gflux = nullptr;   // the cotangent of the dense flux: a gradient sweep
  double* flux = nullptr;          // dense values (of a gradient sweep: a by-product)
  double* jac = nullptr;           // value sweep that leaves every solved cadence's row of derivatives
  const double* gvals = nullptr;   // the cotangent in the VALUE layout of the sparse output instead of gflux
  bool reuse_runs = false;         // the workspace still holds the windows and runs of these very records: no enumeration
  const Chi2Args* chi2 = nullptr;
  // the records are not there yet -- `params` / `ld` are where the fused packing + enumeration launch will put them
  // (requires the fused launch: sorted times on the caller's word, no timing tables)
  const PackIn* pack = nullptr;
  void *ev_start = nullptr, *ev_stop = nullptr;   // events recorded around the sweep's launches
};

// ---- the entry points' argument rules, each written once: an entry calls the ones it has, in the order it has them ----
inline bool shape_ok(int64_t n_cad, int64_t n_draw, int32_t n_planet) {
  return n_cad >= 0 && n_draw >= 0 && n_planet >= 1 && n_planet <= EXO_MAX_PLANETS;
}
inline bool draws_ok(int64_t n_draw) { return n_draw <= 65535; }   // (a draw is a row of the grid)
inline bool sizes_ok(const Sweep& s) {
  return shape_ok(s.n_cad, s.n_draw, s.n_planet) && draws_ok(s.n_draw) && s.n_sub >= 1 && s.n_sub <= EXO_MAX_SUBEXP &&
         (s.n_texp == 0 || s.n_texp == 1 || s.n_texp == s.n_cad);
}
// every flag bit a sweep knows; anything else is a newer header talking to this library (ABI 10: refused, not ignored --
// a layout flag this build does not know would otherwise come back as a silently different array)
inline bool sweep_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)EXO_FLAG_SWEEP_ALL) == 0; }
// what the likelihood entries refuse, and what they refuse on top of it with timing tables; what the Jacobian pair refuses
constexpr uint32_t kLikelihoodRefuses = EXO_FLAG_PER_PLANET | EXO_FLAG_SPARSE | EXO_FLAG_EXACT_SCAN;
constexpr uint32_t kTimedLikelihoodRefuses = kLikelihoodRefuses | EXO_FLAG_SECONDARY | EXO_FLAG_LIGHT_DELAY;
constexpr uint32_t kJacRefuses = EXO_FLAG_PER_PLANET | EXO_FLAG_EXACT_SCAN | EXO_FLAG_LIGHT_DELAY;
inline bool layout_ok(const Sweep& s) { return !((s.flags & EXO_FLAG_CADENCE_MAJOR) && (s.flags & EXO_FLAG_PER_PLANET)); }
// exposure times come with their stencil
inline bool exposure_ok(const Sweep& s) { return s.n_texp <= 0 || (s.texp && s.stencil_dt && s.stencil_w); }
// timing tables: both of them, and where the shifts' cotangents go on a reverse sweep
inline bool ttv_ok(const Ttv& v, bool reverse) {
  return v.edges && v.shift && v.n_edge >= 1 && v.n_edge <= EXO_MAX_TTV_EDGES && (!reverse || v.gshift);
}
// what every gradient sweep needs: records in, their cotangents out, and times unless the series is empty
inline bool grad_ptrs_ok(const Sweep& s, const SweepOut& o) {
  return s.params && s.ld && o.gparams && o.gld && (s.n_cad <= 0 || s.t);
}
// which sweeps take the run-enumeration path (the list path keeps timing tables with occultations or light delay,
// per-cadence exposure times and the exact fp64 scan that the tests compare against)
inline bool runs_path(const Sweep& s) {
  if (s.has_ttv() && (s.flags & (EXO_FLAG_SECONDARY | EXO_FLAG_LIGHT_DELAY))) return false;
  return s.n_texp <= 1 && !(s.flags & EXO_FLAG_EXACT_SCAN);
}
inline bool grad_slots_fit(const Sweep& s) { return s.n_planet * kNG + 7 <= kBlock; }
// carve the run-enumeration workspace and say whether the caller's holds it
inline bool fit_runs(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet, RunWs* rw) {
  *rw = carve_runs(const_cast<void*>(workspace), n_cad, n_draw, n_planet);
  return workspace && workspace_bytes >= rw->bytes;
}
inline bool fit_runs(const Sweep& s, RunWs* rw) { return fit_runs(s.workspace, s.workspace_bytes, s.n_cad, s.n_draw, s.n_planet, rw); }
// no cadences: the gradients are zero
inline int zero_grads(const Sweep& s, const SweepOut& o) {
  if (!exo::zero_fill_async(o.gparams, (int64_t)(s.n_draw * s.n_planet * EXO_NPAR), s.st)) return EXO_ERR_LAUNCH;
  if (o.flux_dot && !exo::zero_fill_async(o.flux_dot, (int64_t)(s.n_draw), s.st)) return EXO_ERR_LAUNCH;
  return exo::zero_fill_async(o.gld, (int64_t)(s.n_draw * (s.secondary() ? 6 : 3)), s.st) ? EXO_OK : EXO_ERR_LAUNCH;
}
// the bins are accumulated into: start from zero
inline bool zero_gshift(const Sweep& s) {
  return exo::zero_fill_async(s.ttv.gshift, (int64_t)(s.n_draw * s.n_planet * (s.ttv.n_edge + 1)), s.st);
}

// ---- the launches of one sweep on the run-enumeration path -------------------------------------------------------------
template <bool G, bool SEC, bool LDELAY = false, bool CHI2 = false, bool TTV = false, bool JAC = false>
inline void launch_runs(const Sweep& s, const RunWs& w, const double* gflux, const double* gsparse, double* vals, int32_t* vcad,
                        double* fill, double* partial, const FinishArgs& fin, int64_t chi2_nw = 0) {
  hipLaunchKernelGGL((transit_runs_kernel<G, SEC, LDELAY, CHI2, TTV, JAC>), dim3((unsigned)w.hb, (unsigned)s.n_draw), dim3(kBlock), 0,
                     s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt, s.stencil_w, (int)s.n_sub, s.params, s.ld, (int)s.n_planet,
                     s.flags, s.n_ev(), w.rl, gflux, gsparse, vals, vcad, fill, partial, chi2_nw, s.ttv, fin);
}
// the sweeps without timing tables, Jacobian or fused likelihood: occultations and light delay as the flags say
template <bool G>
inline void launch_runs_plain(const Sweep& s, const RunWs& w, const double* gflux, const double* gsparse, double* vals,
                              int32_t* vcad, double* fill, double* partial, const FinishArgs& fin) {
  exo::with_flag(s.secondary(), [&](auto sec) {
    exo::with_flag(s.flags & EXO_FLAG_LIGHT_DELAY, [&](auto ldl) {
      launch_runs<G, decltype(sec)::value, decltype(ldl)::value>(s, w, gflux, gsparse, vals, vcad, fill, partial, fin);
    });
  });
}
// windows and runs of every (draw, planet, event) into the workspace
inline int enumerate_runs(const Sweep& s, const SweepOut& o, const RunWs& w) {
  // sorted times on the caller's word and no fence counters to clear: windows and runs in ONE launch
  const bool fused = (s.flags & EXO_FLAG_SORTED_TIMES) && !s.has_ttv();
  if (o.pack && (!fused || o.reuse_runs)) return EXO_ERR_INVALID_ARGUMENT;
  const int n_ev = s.n_ev();
  const dim3 lists((unsigned)(s.n_draw * s.n_planet * n_ev)), wave(64);
  if (o.reuse_runs) {
    // (nothing to launch)
  } else if (o.pack) {
    hipLaunchKernelGGL((transit_enum_kernel<true, true>), lists, wave, 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt,
                       (int)s.n_sub, s.flags, (const double*)nullptr, (const int32_t*)nullptr, 0, n_ev, w.rl, s.params, w.windows,
                       *o.pack);
  } else if (fused) {
    hipLaunchKernelGGL(transit_enum_kernel<true>, lists, wave, 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt, (int)s.n_sub,
                       s.flags, (const double*)nullptr, (const int32_t*)nullptr, 0, n_ev, w.rl, s.params, w.windows);
  } else {
    const int64_t n_rec = s.n_draw * s.n_planet;
    hipLaunchKernelGGL(transit_window_kernel, dim3((unsigned)((n_rec * kWinLanes + kBlock - 1) / kBlock + w.n_sorted)), dim3(kBlock), 0,
                       s.st, s.params, n_rec, s.flags, w.windows, s.t, s.n_cad, w.sorted, w.done, s.n_draw);
    if (s.has_ttv())
      hipLaunchKernelGGL(transit_enum_ttv_kernel, dim3((unsigned)n_rec), wave, 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt,
                         (int)s.n_sub, s.flags, w.windows, w.sorted, w.n_sorted, w.rl, s.ttv);
    else
      hipLaunchKernelGGL(transit_enum_kernel<false>, lists, wave, 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt, (int)s.n_sub,
                         s.flags, w.windows, w.sorted, w.n_sorted, n_ev, w.rl);
  }
  return launch_status();
}

// a draw that is one block's work is finished by that block (gradients from its partials, values to their cadences):
// no finish launch
// (not with a cadence-major flux: a draw's values land in lines other blocks zero-fill -- after the sweep, then)
inline bool own_block_finishes(const Sweep& s, const SweepOut& o, const RunWs& w) {
  return !((s.flags & EXO_FLAG_CADENCE_MAJOR) && o.flux) && w.hb == 1;
}
// what a finish launch is handed besides the request: the blocks' gradient partials (nullptr: none) and where a draw's
// "dot" slot goes; the values to scatter into a dense flux; the residual kernel's partial sums and where their total goes;
// the timing tables whose run cotangents are due
struct FinishIn {
  const double* partial;
  double* dot;
  const double* vals;
  double* fill;
  const double* chi2_part;
  int n_chi2_part;
  double* chi2;
  Ttv ttv;
};
inline int launch_finish(const Sweep& s, const SweepOut& o, const RunWs& w, const FinishIn& f) {
  const dim3 grid((unsigned)s.n_draw), block(s.n_draw <= 256 ? 1024 : kBlock);
  if (o.chi2 && o.chi2->nz)
    hipLaunchKernelGGL(transit_finish_noise_kernel, grid, block, 0, s.st, f.partial, w.hb, (int)s.n_planet, o.gparams, o.gld, f.dot,
                       s.n_cad, s.flags, s.n_ev(), w.rl, w.vcad, f.chi2_part, f.n_chi2_part, f.chi2, f.ttv, o.chi2->nz->out);
  else
    hipLaunchKernelGGL(transit_finish_kernel, grid, block, 0, s.st, f.partial, w.hb, (int)s.n_planet, s.secondary(), o.gparams, o.gld,
                       f.dot, s.n_cad, s.flags, s.n_ev(), w.rl, f.vals, w.vcad, f.fill, f.chi2_part, f.n_chi2_part, f.chi2, f.ttv);
  return launch_status();
}

// one planet, one sample per cadence: the cotangent of a cadence's flux needs nothing but that flux -- value and
// gradient in ONE evaluation per solved cadence (the misfit comes out of the "dot" slot of the partials)
inline bool single_pass(const Sweep& s) { return s.n_planet == 1 && !s.secondary() && s.n_sub == 1; }
inline int likelihood_single_pass(const Sweep& s, const SweepOut& o, const RunWs& w) {
  const Chi2Args& c = *o.chi2;
  const bool fold = own_block_finishes(s, o, w), ldelay = s.flags & EXO_FLAG_LIGHT_DELAY;
  const FinishArgs fin{o.gparams, o.gld, c.chi2, fold ? 1 : 0, w.done};
  // (c.nz: a sampled mean / jitter)
  const auto launch = [&](auto ldl, auto tv) {
    constexpr bool LDELAY = decltype(ldl)::value, TTV = decltype(tv)::value;
    if (c.nz)
      hipLaunchKernelGGL((transit_runs_kernel<true, false, LDELAY, true, TTV, false, true>), dim3((unsigned)w.hb, (unsigned)s.n_draw),
                         dim3(kBlock), 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt, s.stencil_w, (int)s.n_sub, s.params, s.ld,
                         (int)s.n_planet, s.flags, s.n_ev(), w.rl, c.obs, c.ivar, nullptr, nullptr, nullptr, w.partial, c.n_ivar,
                         s.ttv, fin, *c.nz);
    else
      launch_runs<true, false, LDELAY, true, TTV>(s, w, c.obs, c.ivar, nullptr, nullptr, nullptr, w.partial, fin, c.n_ivar);
  };
  if (s.has_ttv()) launch(std::false_type{}, std::true_type{});
  else if (ldelay) launch(std::true_type{}, std::false_type{});
  else launch(std::false_type{}, std::false_type{});
  if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
  if (fold) return EXO_OK;
  return launch_finish(s, o, w, FinishIn{w.partial, c.chi2, nullptr, nullptr, nullptr, 0, nullptr, s.ttv});
}

// value sweep into the sparse output, residuals + cotangents on it, gradient sweep reading them (gshift included)
inline int likelihood_three_sweeps(const Sweep& s, const SweepOut& o, const RunWs& w) {
  const Chi2Args& c = *o.chi2;
  const FinishArgs no_fin{nullptr, nullptr, nullptr, 0, nullptr};
  const dim3 grid(kResidualBlocks, (unsigned)s.n_draw), block(kBlock);
  if (s.has_ttv()) launch_runs<false, false, false, false, true>(s, w, nullptr, nullptr, w.vals, w.vcad, nullptr, nullptr, no_fin);
  else launch_runs_plain<false>(s, w, nullptr, nullptr, w.vals, w.vcad, nullptr, nullptr, no_fin);
  if (c.nz)
    hipLaunchKernelGGL(transit_residual_kernel<true>, grid, block, 0, s.st, s.n_cad, (int)s.n_planet, s.n_ev(), w.rl, w.vals, w.vcad,
                       c.obs, c.ivar, c.n_ivar, w.gvals, w.chi2_part, *c.nz);
  else
    hipLaunchKernelGGL(transit_residual_kernel<>, grid, block, 0, s.st, s.n_cad, (int)s.n_planet, s.n_ev(), w.rl, w.vals, w.vcad,
                       c.obs, c.ivar, c.n_ivar, w.gvals, w.chi2_part);
  if (s.has_ttv()) launch_runs<true, false, false, false, true>(s, w, nullptr, w.gvals, nullptr, nullptr, nullptr, w.partial, no_fin);
  else launch_runs_plain<true>(s, w, nullptr, w.gvals, nullptr, nullptr, nullptr, w.partial, no_fin);
  if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
  return launch_finish(s, o, w, FinishIn{w.partial, c.nz ? nullptr : o.flux_dot, nullptr, nullptr, w.chi2_part, kResidualBlocks,
                                         c.chi2, s.ttv});
}

// values, gradient (cotangent dense or in the sparse output's layout) or Jacobian
inline int plain_sweep(const Sweep& s, const SweepOut& o, const RunWs& w) {
  const bool sparse = s.flags & EXO_FLAG_SPARSE, grad = o.gflux != nullptr || o.gvals != nullptr;
  // the values are kept when somebody reads them: the dense output's last kernel, or the caller (sparse)
  double* vals = (o.flux || sparse) ? w.vals : nullptr;
  double* fill = sparse ? nullptr : o.flux;
  int32_t* vcad = fill ? w.vcad : nullptr;
  const bool fold = own_block_finishes(s, o, w);
  const FinishArgs fin{o.gparams, o.gld, o.flux_dot, fold ? 1 : 0, w.done};
  if (s.has_ttv()) {
    // (transits only, no light delay: runs_path)
    if (grad) launch_runs<true, false, false, false, true>(s, w, o.gflux, nullptr, vals, vcad, fill, w.partial, fin);
    else launch_runs<false, false, false, false, true>(s, w, nullptr, nullptr, vals, vcad, fill, nullptr, fin);
  } else if (o.gvals) {
    // (the values stay as the forward sweep left them: the GP's reverse pass has read them, nobody reads them again)
    launch_runs_plain<true>(s, w, nullptr, o.gvals, nullptr, nullptr, nullptr, w.partial, fin);
  } else if (grad) {
    launch_runs_plain<true>(s, w, o.gflux, nullptr, vals, vcad, fill, w.partial, fin);
  } else if (o.jac) {
    // value sweep that leaves every solved cadence's row of derivatives (transit_runs_kernel<.., JAC>; the cadence index
    // is written whatever the output: the contraction gathers the cotangent through it)
    exo::with_flag(s.secondary(), [&](auto sec) {
      launch_runs<true, decltype(sec)::value, false, false, false, true>(s, w, nullptr, nullptr, vals, w.vcad, fill, o.jac, fin);
    });
  } else {
    launch_runs_plain<false>(s, w, nullptr, nullptr, vals, vcad, fill, nullptr, fin);
  }
  if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
  if (!(grad || fill) || fold) return EXO_OK;
  return launch_finish(s, o, w, FinishIn{grad ? w.partial : nullptr, o.flux_dot, vals, fill, nullptr, kResidualBlocks, nullptr,
                                         grad ? s.ttv : Ttv{}});
}

// a sweep on the run-enumeration path, after the entry's checks: `w` is the caller's workspace, carved and large enough
inline int launch_runs_sweep(const Sweep& s, const SweepOut& o, const RunWs& w) {
  if (o.ev_start) (void)hipEventRecord((hipEvent_t)o.ev_start, s.st);
  int rc = enumerate_runs(s, o, w);
  if (rc == EXO_OK)
    rc = !o.chi2 ? plain_sweep(s, o, w) : (single_pass(s) ? likelihood_single_pass(s, o, w) : likelihood_three_sweeps(s, o, w));
  if (o.ev_stop) (void)hipEventRecord((hipEvent_t)o.ev_stop, s.st);
  return rc;
}

}  // namespace

extern "C" {

int32_t exo_abi_version(void) { return EXO_ABI_VERSION; }

int64_t exo_transit_flux_workspace_bytes(int64_t n_cad, int64_t n_draw, int32_t n_planet) {
  if (n_cad < 0 || n_draw < 0 || n_planet < 1) return -1;
  if (n_cad == 0 || n_draw == 0) return 0;
  int bpd, tpb;
  transit_geometry(n_cad, n_draw, &bpd, &tpb);
  const Workspace w = carve(nullptr, n_draw, bpd, tpb, n_planet);
  const RunWs r = carve_runs(nullptr, n_cad, n_draw, n_planet);
  return w.bytes > r.bytes ? w.bytes : r.bytes;
}

int exo_transit_flux_sparse_layout(int64_t n_cad, int64_t n_draw, int32_t n_planet, int64_t* out) {
  if (n_cad < 0 || n_draw < 0 || n_planet < 1 || !out) return EXO_ERR_INVALID_ARGUMENT;
  const RunWs r = carve_runs(nullptr, n_cad, n_draw, n_planet);
  out[0] = r.off_nrun; out[1] = r.off_runs; out[2] = r.off_pre_all; out[3] = r.off_vals; out[4] = r.rl.r_max;
  return EXO_OK;
}

int exo_transit_sparse_scatter_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                                   uint32_t flags, int32_t clear, double* flux, void* stream) {
  if (!shape_ok(n_cad, n_draw, n_planet) || !draws_ok(n_draw) || (flags & ~(uint32_t)EXO_FLAG_SECONDARY))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_cad == 0 || n_draw == 0) return EXO_OK;
  if (!flux) return EXO_ERR_INVALID_ARGUMENT;
  RunWs rw;
  if (!fit_runs(workspace, workspace_bytes, n_cad, n_draw, n_planet, &rw)) return EXO_ERR_WORKSPACE;
  exo::with_flag(clear, [&](auto clr) {
    hipLaunchKernelGGL(transit_scatter_runs_kernel<decltype(clr)::value>, dim3((unsigned)n_draw), dim3(kBlock), 0, (hipStream_t)stream,
                       rw.rl, rw.vals, n_cad, (int)n_planet, events(flags), flux);
  });
  return launch_status();
}

// A sweep after the entry points' own checks: the run-enumeration path where it applies (runs_path), else the list path --
// windows, scan, heavy kernel and, with a gradient (gflux != nullptr), the reduce kernel.  flux == nullptr: no values (the
// list path's scan skips the fill).
static int transit_sweep(const Sweep& s, const SweepOut& o) {
  if (!layout_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (runs_path(s)) {
    RunWs rw;
    if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
    return launch_runs_sweep(s, o, rw);
  }
  if (s.flags & (EXO_FLAG_SPARSE | EXO_FLAG_LIGHT_DELAY | EXO_FLAG_CADENCE_MAJOR)) return EXO_ERR_INVALID_ARGUMENT;   // run-enumeration path only
  int bpd, tpb;
  transit_geometry(s.n_cad, s.n_draw, &bpd, &tpb);
  const Workspace w = carve(s.workspace, s.n_draw, bpd, tpb, s.n_planet);
  if (!s.workspace || s.workspace_bytes < w.bytes) return EXO_ERR_WORKSPACE;
  const bool grad = o.gflux != nullptr;
  if (o.ev_start) (void)hipEventRecord((hipEvent_t)o.ev_start, s.st);
  launch_windows(s.params, s.n_draw, s.n_planet, s.flags, w.windows, s.st);
  const ScanPlan sp = scan_plan(s.flags, bpd, s.n_draw, s.n_planet, s.n_texp, o.flux != nullptr);
  launch_scan(s.flags, s.has_ttv(), sp.grid, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt, s.n_sub, s.params, s.n_planet,
              sp.flags, tpb, bpd, s.n_draw, sp.n_classify, o.flux, w.counts, w.list, w.windows, s.ttv);
  if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
  const int merge = heavy_merge(s.n_draw, bpd);
  const int nhb = (bpd + merge - 1) / merge;
  const double* hwin = ((s.flags & EXO_FLAG_EXACT_SCAN) && !(s.flags & EXO_FLAG_WINDOW)) ? nullptr : w.windows;
  exo::with_flag(grad, [&](auto g) {
    exo::with_flag(s.secondary(), [&](auto sec) {
      exo::with_flag(s.has_ttv(), [&](auto tv) {
        hipLaunchKernelGGL((transit_heavy_kernel<decltype(g)::value, decltype(sec)::value, decltype(tv)::value>),
                           dim3((unsigned)nhb, (unsigned)s.n_draw), dim3(kBlock), 0, s.st, s.t, s.n_cad, s.texp, s.n_texp, s.stencil_dt,
                           s.stencil_w, s.n_sub, s.params, s.ld, s.n_planet, s.flags, tpb, bpd, merge, w.counts, w.list, o.gflux,
                           o.flux, grad ? w.partial : nullptr, hwin, s.ttv);
      });
    });
  });
  if (grad) {
    if (launch_status() != EXO_OK) return EXO_ERR_LAUNCH;
    hipLaunchKernelGGL(transit_vjp_reduce_kernel, dim3((unsigned)s.n_draw), dim3(kBlock), 0, s.st, w.partial, nhb, s.n_planet,
                       s.secondary(), o.gparams, o.gld, o.flux_dot);
  }
  if (o.ev_stop) (void)hipEventRecord((hipEvent_t)o.ev_stop, s.st);
  return launch_status();
}

// forward sweep
static int transit_fwd(const Sweep& s, const SweepOut& o) {
  if (!sizes_ok(s) || !sweep_flags_ok(s.flags)) return EXO_ERR_INVALID_ARGUMENT;
  if (s.n_cad == 0 || s.n_draw == 0) return EXO_OK;
  if (!s.t || !s.params || !s.ld || (!o.flux && !(s.flags & EXO_FLAG_SPARSE)) || !exposure_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  return transit_sweep(s, o);
}

// value + VJP sweep (the forward value is a by-product: o.flux == nullptr, none)
static int transit_vjp(const Sweep& s, const SweepOut& o) {
  if (!sizes_ok(s) || !sweep_flags_ok(s.flags)) return EXO_ERR_INVALID_ARGUMENT;
  if (s.n_draw == 0) return EXO_OK;
  if (!grad_ptrs_ok(s, o) || (s.n_cad > 0 && !o.gflux) || !exposure_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (s.has_ttv() && !zero_gshift(s)) return EXO_ERR_LAUNCH;
  if (s.n_cad == 0) return zero_grads(s, o);
  if (!grad_slots_fit(s)) return EXO_ERR_INVALID_ARGUMENT;
  return transit_sweep(s, o);
}

int exo_transit_flux_fwd_ev_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                                uint32_t flags, double* flux, void* workspace, int64_t workspace_bytes,
                                void* stream, void* ev_start, void* ev_stop) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o;
  o.flux = flux; o.ev_start = ev_start; o.ev_stop = ev_stop;
  return transit_fwd(s, o);
}

int exo_transit_flux_fwd_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                             const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                             const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, double* flux, void* workspace, int64_t workspace_bytes, void* stream) {
  return exo_transit_flux_fwd_ev_f64(t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw,
                                     n_planet, flags, flux, workspace, workspace_bytes, stream, nullptr, nullptr);
}

int exo_transit_flux_ttv_fwd_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                 const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                 const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                                 uint32_t flags, const double* ttv_edges, const double* ttv_shift, int32_t n_edge,
                                 double* flux, void* workspace, int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags,
                Ttv{ttv_edges, ttv_shift, nullptr, n_edge}, workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o;
  o.flux = flux;
  if (!ttv_ok(s.ttv, false)) return EXO_ERR_INVALID_ARGUMENT;
  return transit_fwd(s, o);
}

int exo_transit_flux_vjp_ev_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                                uint32_t flags, const double* gflux, double* flux_out, double* gparams,
                                double* gld, double* flux_dot, void* workspace, int64_t workspace_bytes,
                                void* stream, void* ev_start, void* ev_stop) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o{gparams, gld, flux_dot, gflux, flux_out};
  o.ev_start = ev_start; o.ev_stop = ev_stop;
  return transit_vjp(s, o);
}

int exo_transit_flux_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                             const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                             const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, const double* gflux, double* flux_out, double* gparams,
                             double* gld, double* flux_dot, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  return exo_transit_flux_vjp_ev_f64(t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw,
                                     n_planet, flags, gflux, flux_out, gparams, gld, flux_dot, workspace,
                                     workspace_bytes, stream, nullptr, nullptr);
}

int exo_transit_flux_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                 const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                 const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                                 uint32_t flags, const double* ttv_edges, const double* ttv_shift, int32_t n_edge,
                                 const double* gflux, double* flux_out, double* gparams, double* gld,
                                 double* gshift, double* flux_dot, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags,
                Ttv{ttv_edges, ttv_shift, gshift, n_edge}, workspace, workspace_bytes, (hipStream_t)stream};
  const SweepOut o{gparams, gld, flux_dot, gflux, flux_out};
  if (!ttv_ok(s.ttv, true)) return EXO_ERR_INVALID_ARGUMENT;
  return transit_vjp(s, o);
}

int64_t exo_transit_flux_jac_doubles(int64_t n_cad, int64_t n_draw, int32_t n_planet) {
  if (!shape_ok(n_cad, n_draw, n_planet)) return -1;
  return (int64_t)kJac * n_cad * n_draw * n_planet;
}

int exo_transit_flux_fwd_jac_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                 const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                 int64_t n_draw, int32_t n_planet, uint32_t flags, double* flux, double* jac,
                                 int64_t jac_doubles, void* workspace, int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o;
  o.flux = flux; o.jac = jac;
  if (!sizes_ok(s) || !sweep_flags_ok(flags) || (flags & kJacRefuses)) return EXO_ERR_INVALID_ARGUMENT;
  if (!runs_path(s)) return EXO_ERR_INVALID_ARGUMENT;   // one exposure time (or none) for all cadences
  if (n_cad == 0 || n_draw == 0) return EXO_OK;
  if (!t || !params || !ld || (!flux && !(flags & EXO_FLAG_SPARSE)) || !jac || !exposure_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (jac_doubles < exo_transit_flux_jac_doubles(n_cad, n_draw, n_planet)) return EXO_ERR_WORKSPACE;
  RunWs rw;
  if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
  return launch_runs_sweep(s, o, rw);
}

int exo_transit_flux_jac_vjp_f64(const double* gflux, int64_t n_cad, int64_t n_draw, int32_t n_planet, uint32_t flags,
                                 const double* jac, void* workspace, int64_t workspace_bytes, double* gparams, double* gld,
                                 double* flux_dot, void* stream) {
  Sweep s;   // (no series: the forward call's workspace holds the runs, values and cadence index)
  s.n_cad = n_cad; s.n_draw = n_draw; s.n_planet = n_planet; s.flags = flags;
  s.workspace = workspace; s.workspace_bytes = workspace_bytes; s.st = (hipStream_t)stream;
  const SweepOut o{gparams, gld, flux_dot};
  if (!shape_ok(n_cad, n_draw, n_planet) || !draws_ok(n_draw) || !sweep_flags_ok(flags) || (flags & kJacRefuses))
    return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!gparams || !gld || (n_cad > 0 && (!gflux || !jac))) return EXO_ERR_INVALID_ARGUMENT;
  if (n_cad == 0) return zero_grads(s, o);
  RunWs rw;
  if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
  hipLaunchKernelGGL(transit_jac_vjp_kernel, dim3((unsigned)rw.hb, (unsigned)n_draw), dim3(kBlock), 0, s.st, n_cad, (int)n_planet,
                     s.n_ev(), flags, rw.rl, rw.vals, rw.vcad, jac, gflux, n_draw, rw.partial);
  hipLaunchKernelGGL(transit_finish_kernel, dim3((unsigned)n_draw), dim3(kBlock), 0, s.st, rw.partial, rw.hb, (int)n_planet,
                     s.secondary(), gparams, gld, flux_dot, n_cad, flags & ~(uint32_t)(EXO_FLAG_CADENCE_MAJOR | EXO_FLAG_SPARSE), s.n_ev(),
                     rw.rl, nullptr, nullptr, nullptr, nullptr, 0, nullptr, Ttv{});
  return launch_status();
}

// columns in (as exo_pack_records_cols_f64), records + sweep + (optionally) column cotangents out
int exo_transit_flux_cols_vjp_f64(const double* const* cols, const int64_t* draw_stride, const int64_t* planet_stride,
                                  const double* defaults, const double* const* ld_cols, const int64_t* ld_draw_stride,
                                  uint32_t pack_flags, const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                  const double* stencil_dt, const double* stencil_w, int32_t n_sub, int64_t n_draw,
                                  int32_t n_planet, uint32_t flags, const double* gflux, double* flux_out, double* params,
                                  double* ld, double* gparams, double* gld, double* flux_dot, int32_t fold,
                                  const double* gscale, double* const* gcols, double* const* gld_cols, void* workspace,
                                  int64_t workspace_bytes, void* stream, void* ev_start, void* ev_stop) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o{gparams, gld, flux_dot, gflux, flux_out};
  o.ev_start = ev_start; o.ev_stop = ev_stop;
  if (!sizes_ok(s) || !sweep_flags_ok(flags)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_draw == 0) return EXO_OK;
  if (!cols || !draw_stride || !planet_stride || !defaults || !ld_cols || !ld_draw_stride || !grad_ptrs_ok(s, o) ||
      (fold && (!gcols || !gld_cols)) || (n_cad > 0 && !gflux) || !exposure_ok(s))
    return EXO_ERR_INVALID_ARGUMENT;
  if (!grad_slots_fit(s) || !layout_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (((pack_flags ^ flags) & EXO_FLAG_SECONDARY) != 0) return EXO_ERR_INVALID_ARGUMENT;   // (one answer to "occultations?")
  // the launches fuse when the sweep is a run-enumeration sweep on sorted times (the caller's word: EXO_FLAG_SORTED_TIMES); anything
  // else is the three calls one after the other -- same results
  const bool fused = n_cad > 0 && runs_path(s) && (flags & EXO_FLAG_SORTED_TIMES);
  PackIn pk{};
  int rc;
  if (!fused) {
    rc = exo_pack_records_cols_f64(cols, draw_stride, planet_stride, defaults, ld_cols, ld_draw_stride, n_draw, n_planet,
                                   pack_flags, params, ld, stream);
    if (rc != EXO_OK) return rc;
    rc = transit_vjp(s, o);
  } else {
    const int nld = (pack_flags & EXO_FLAG_SECONDARY) ? 4 : 2;
    for (int k = 0; k < EXO_NIN; ++k) {
      pk.src.ptr[k] = cols[k]; pk.src.ds[k] = draw_stride[k]; pk.src.ps[k] = planet_stride[k]; pk.src.def[k] = defaults[k];
    }
    for (int k = 0; k < 4; ++k) {
      pk.src.ldp[k] = k < nld ? ld_cols[k] : nullptr;
      pk.src.lds[k] = k < nld ? ld_draw_stride[k] : 0;
      if (k < nld && !ld_cols[k]) return EXO_ERR_INVALID_ARGUMENT;
    }
    pk.flags = pack_flags; pk.n_planet = n_planet; pk.params = params; pk.ld = ld;
    RunWs rw;
    if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
    o.pack = &pk;
    rc = launch_runs_sweep(s, o, rw);
  }
  if (rc != EXO_OK || !fold) return rc;
  return exo_pack_records_cols_vjp_f64(cols, draw_stride, planet_stride, defaults, ld_cols, ld_draw_stride, n_draw, n_planet,
                                       pack_flags, gparams, gld, gscale, gcols, gld_cols, stream);
}

int exo_transit_flux_vjp_sparse_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                    const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                    int64_t n_draw, int32_t n_planet, uint32_t flags, const double* gvals, double* gparams,
                                    double* gld, double* flux_dot, void* workspace, int64_t workspace_bytes, int32_t reuse_runs,
                                    void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  SweepOut o{gparams, gld, flux_dot};
  o.gvals = gvals; o.reuse_runs = reuse_runs != 0;
  if (!sizes_ok(s) || !sweep_flags_ok(flags)) return EXO_ERR_INVALID_ARGUMENT;
  if (!(flags & EXO_FLAG_SPARSE) || (flags & (EXO_FLAG_PER_PLANET | EXO_FLAG_CADENCE_MAJOR | EXO_FLAG_EXACT_SCAN)))
    return EXO_ERR_INVALID_ARGUMENT;
  if (!runs_path(s)) return EXO_ERR_INVALID_ARGUMENT;   // one exposure time (or none) for all cadences
  if (n_draw == 0) return EXO_OK;
  if (!grad_ptrs_ok(s, o) || (n_cad > 0 && !gvals) || !exposure_ok(s) || !grad_slots_fit(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (n_cad == 0) return zero_grads(s, o);
  RunWs rw;
  if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
  return launch_runs_sweep(s, o, rw);
}

int exo_transit_flux_sparse_model(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                                  uint32_t flags, exo_sparse_model* out) {
  if (!shape_ok(n_cad, n_draw, n_planet) || !out || n_cad > 0x7fffffff) return EXO_ERR_INVALID_ARGUMENT;
  const int n_ev = events(flags);
  // one list per draw: the runs ARE the segments (several lists -- planets, occultations -- need the merged form)
  if (n_planet * n_ev != 1) return EXO_ERR_INVALID_ARGUMENT;
  RunWs rw;
  if (!fit_runs(workspace, workspace_bytes, n_cad, n_draw, n_planet, &rw)) return EXO_ERR_WORKSPACE;
  // (lists are packed with stride n_ev -- list = (draw * n_planet + planet) * n_ev + event -- so with one list per draw
  // consecutive draws are consecutive rows, although the workspace is SIZED for two lists per record)
  out->nseg = rw.rl.nrun;
  out->seg = reinterpret_cast<const int32_t*>(rw.rl.runs);
  out->off = rw.rl.pre_all;
  out->vals = rw.vals;
  out->seg_step = 4; out->hi_at = 3;
  out->seg_row = (int64_t)n_planet * n_ev * rw.rl.r_max * 4;
  out->off_row = (int64_t)n_planet * n_ev * (rw.rl.r_max + 1);
  out->val_row = (int64_t)n_planet * n_cad;
  out->row_of_draw = nullptr;
  return EXO_OK;
}

// ---- the MERGED sparse model (round 6): several lists per draw -- planets, occultations -- as one ascending list of disjoint
// segments with the SUM of the lists' values: what exo_transit_flux_sparse_model refuses.  See include/exoplanet_amd.h.
int64_t exo_sparse_merge_workspace_bytes(int64_t n_cad, int64_t n_draw, int32_t n_planet) {
  if (!shape_ok(n_cad, n_draw, n_planet)) return -1;
  return carve_merge(nullptr, n_cad, n_draw, n_planet).bytes;
}

int exo_sparse_merge_layout(int64_t n_cad, int64_t n_draw, int32_t n_planet, int64_t* out) {
  if (!shape_ok(n_cad, n_draw, n_planet) || !out) return EXO_ERR_INVALID_ARGUMENT;
  const MergeWs m = carve_merge(nullptr, n_cad, n_draw, n_planet);
  out[0] = m.off_nseg; out[1] = m.off_seg; out[2] = m.off_off; out[3] = m.off_vals; out[4] = m.cap_seg;
  return EXO_OK;
}

static int merge_args(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                      uint32_t flags, const void* merge_ws, int64_t merge_ws_bytes, RunWs* rw, MergeWs* m) {
  if (!shape_ok(n_cad, n_draw, n_planet) || n_cad >= ((int64_t)1 << 31) || !draws_ok(n_draw) || (flags & ~(uint32_t)EXO_FLAG_SECONDARY))
    return EXO_ERR_INVALID_ARGUMENT;
  *m = carve_merge(const_cast<void*>(merge_ws), n_cad, n_draw, n_planet);
  if (!fit_runs(workspace, workspace_bytes, n_cad, n_draw, n_planet, rw) || !merge_ws || merge_ws_bytes < m->bytes)
    return EXO_ERR_WORKSPACE;
  return EXO_OK;
}

static void describe_merged(const MergeWs& m, int64_t n_cad, exo_sparse_model* out) {
  out->nseg = m.nseg;
  out->seg = m.seg;
  out->off = m.off;
  out->vals = m.vals;
  out->seg_step = 2; out->hi_at = 1;
  out->seg_row = (int64_t)m.cap_seg * 2;
  out->off_row = (int64_t)m.cap_seg + 1;
  out->val_row = n_cad;
  out->row_of_draw = nullptr;
}

int exo_sparse_model_merged(const void* merge_ws, int64_t merge_ws_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                            exo_sparse_model* out) {
  if (!shape_ok(n_cad, n_draw, n_planet) || !out) return EXO_ERR_INVALID_ARGUMENT;
  const MergeWs m = carve_merge(const_cast<void*>(merge_ws), n_cad, n_draw, n_planet);
  if (!merge_ws || merge_ws_bytes < m.bytes) return EXO_ERR_WORKSPACE;
  describe_merged(m, n_cad, out);
  return EXO_OK;
}

int exo_sparse_model_merge_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                               uint32_t flags, void* merge_ws, int64_t merge_ws_bytes, exo_sparse_model* out, void* stream) {
  RunWs rw;
  MergeWs m;
  const int rc = merge_args(workspace, workspace_bytes, n_cad, n_draw, n_planet, flags, merge_ws, merge_ws_bytes, &rw, &m);
  if (rc != EXO_OK) return rc;
  if (out) describe_merged(m, n_cad, out);
  if (n_cad == 0 || n_draw == 0) return EXO_OK;
  const int n_ev = events(flags);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sparse_merge_segments_kernel, dim3((unsigned)n_draw), dim3(kBlock), 0, st, rw.rl, (int)n_planet, n_ev, n_cad, m);
  hipLaunchKernelGGL(sparse_merge_values_kernel, dim3((unsigned)merge_blocks_per_draw(n_draw), (unsigned)n_draw), dim3(kBlock), 0, st,
                     rw.rl, rw.vals, (int)n_planet, n_ev, n_cad, m);
  return launch_status();
}

int exo_sparse_model_merge_vjp_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                                   uint32_t flags, const void* merge_ws, int64_t merge_ws_bytes, const double* gmvals,
                                   double* gvals, void* stream) {
  RunWs rw;
  MergeWs m;
  const int rc = merge_args(workspace, workspace_bytes, n_cad, n_draw, n_planet, flags, merge_ws, merge_ws_bytes, &rw, &m);
  if (rc != EXO_OK) return rc;
  if (n_cad == 0 || n_draw == 0) return EXO_OK;
  if (!gmvals || !gvals) return EXO_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sparse_merge_vjp_kernel, dim3((unsigned)merge_blocks_per_draw(n_draw), (unsigned)n_draw), dim3(kBlock), 0,
                     (hipStream_t)stream, rw.rl, (int)n_planet, events(flags), n_cad, m, gmvals, gvals);
  return launch_status();
}

// The four likelihood entries: each checks the extents and pointers of its own arrays (nothing is read when there are no
// draws) and its timing tables, then the rules they share -- `refuses` is the flag set that entry cannot take.
static bool chi2_args_ok(const Sweep& s, const Chi2Args& c) {
  if (c.n_ivar != 1 && c.n_ivar != s.n_cad) return false;
  return s.n_draw == 0 || s.n_cad <= 0 || (c.obs && c.ivar);
}
// (a sampled mean and a jitter: c.obs is the series y, c.ivar the variances)
static bool noise_args_ok(const Sweep& s, const Chi2Args& c) {
  const NoiseIn& nz = *c.nz;
  if ((c.n_ivar != 1 && c.n_ivar != s.n_cad) || (nz.n_mean != 1 && nz.n_mean != s.n_draw) ||
      (nz.n_jit != 0 && nz.n_jit != 1 && nz.n_jit != s.n_draw))
    return false;
  if (s.n_draw == 0) return true;
  return c.ivar && nz.mean && nz.out.gmean && nz.out.gjit2 && (s.n_cad == 0 || c.obs) && (nz.n_jit == 0 || nz.jit2);
}
static int likelihood(const Sweep& s, const Chi2Args& c, uint32_t refuses, double* gparams, double* gld) {
  SweepOut o{gparams, gld};
  o.chi2 = &c;
  if (!sizes_ok(s) || !sweep_flags_ok(s.flags) || (s.flags & refuses)) return EXO_ERR_INVALID_ARGUMENT;
  if (s.n_draw == 0) return EXO_OK;
  if (!grad_ptrs_ok(s, o) || !c.chi2 || !exposure_ok(s)) return EXO_ERR_INVALID_ARGUMENT;
  if (!runs_path(s)) return EXO_ERR_INVALID_ARGUMENT;   // one exposure time (or none) for all cadences
  RunWs rw;
  if (!fit_runs(s, &rw)) return EXO_ERR_WORKSPACE;
  if (s.has_ttv() && !zero_gshift(s)) return EXO_ERR_LAUNCH;
  return launch_runs_sweep(s, o, rw);
}

int exo_transit_chi2_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                             const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                             int64_t n_draw, int32_t n_planet, uint32_t flags, const double* obs, const double* ivar,
                             int64_t n_ivar, double* chi2, double* gparams, double* gld, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  const Chi2Args c2{obs, ivar, n_ivar, chi2};
  if (!chi2_args_ok(s, c2)) return EXO_ERR_INVALID_ARGUMENT;
  return likelihood(s, c2, kLikelihoodRefuses, gparams, gld);
}

int exo_transit_chi2_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                 const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                 int64_t n_draw, int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                 const double* ttv_shift, int32_t n_edge, const double* obs, const double* ivar,
                                 int64_t n_ivar, double* chi2, double* gparams, double* gld, double* gshift, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags,
                Ttv{ttv_edges, ttv_shift, gshift, n_edge}, workspace, workspace_bytes, (hipStream_t)stream};
  const Chi2Args c2{obs, ivar, n_ivar, chi2};
  if (n_cad < 1 || !chi2_args_ok(s, c2) || !ttv_ok(s.ttv, true)) return EXO_ERR_INVALID_ARGUMENT;
  return likelihood(s, c2, kTimedLikelihoodRefuses, gparams, gld);
}

int exo_transit_noise_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                              const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                              int64_t n_draw, int32_t n_planet, uint32_t flags, const double* y, const double* var,
                              int64_t n_var, const double* mean, int64_t n_mean, const double* jit2, int64_t n_jit,
                              double* chi2, double* gmean, double* gjit2, double* gparams, double* gld, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags, Ttv{},
                workspace, workspace_bytes, (hipStream_t)stream};
  const NoiseIn nz{mean, jit2, n_mean, n_jit, NoiseOut{gmean, gjit2}};
  const Chi2Args c2{y, var, n_var, chi2, &nz};
  if (!noise_args_ok(s, c2)) return EXO_ERR_INVALID_ARGUMENT;
  return likelihood(s, c2, kLikelihoodRefuses, gparams, gld);
}

int exo_transit_noise_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                  const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                  int64_t n_draw, int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                  const double* ttv_shift, int32_t n_edge, const double* y, const double* var, int64_t n_var,
                                  const double* mean, int64_t n_mean, const double* jit2, int64_t n_jit, double* chi2,
                                  double* gmean, double* gjit2, double* gparams, double* gld, double* gshift, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  const Sweep s{t, n_cad, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, n_draw, n_planet, flags,
                Ttv{ttv_edges, ttv_shift, gshift, n_edge}, workspace, workspace_bytes, (hipStream_t)stream};
  const NoiseIn nz{mean, jit2, n_mean, n_jit, NoiseOut{gmean, gjit2}};
  const Chi2Args c2{y, var, n_var, chi2, &nz};
  if (n_cad < 1 || !noise_args_ok(s, c2) || !ttv_ok(s.ttv, true)) return EXO_ERR_INVALID_ARGUMENT;
  return likelihood(s, c2, kTimedLikelihoodRefuses, gparams, gld);
}

}  // extern "C"
