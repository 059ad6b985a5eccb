/* exoplanet_amd.h -- C ABI of libexoplanet_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-leapfrog-step log-likelihood hot path of
 * exoplanet-dev/exoplanet.  Every entry point replaces one third-party Op that
 * the reference reaches through `exoplanet.compat.ops`
 * (/root/reference/src/exoplanet/compat.py:27,56) or through celerite2, or one
 * block of elementwise PyTensor graph between those Ops.  The binding a
 * maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM), float64, C-contiguous (the column-form packing entry points take
 *     HOST arrays of device pointers and say so); ordinary hipMalloc memory (coarse-grained): the summed flux of
 *     several planets and the cotangents of timing shifts are accumulated with the hardware's fp64 atomics, which
 *     fine-grained / host-mapped allocations do not offer;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     calls are asynchronous and stream-ordered, nothing is allocated inside;
 *   - return value: 0 = launched, EXO_ERR_* otherwise (no exceptions cross the
 *     boundary); numeric failure is in-band (NaN in -> NaN out, `flag` words);
 *   - the library keeps no global state (no caches, no environment reads): re-entrant,
 *     one process per GPU.
 */
#ifndef EXOPLANET_AMD_H
#define EXOPLANET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXO_OK 0
#define EXO_ERR_INVALID_ARGUMENT 1
#define EXO_ERR_LAUNCH 2
#define EXO_ERR_WORKSPACE 3

/* ABI version, bumped whenever a signature, a layout or the set of flags below changes.
 * 10: EXO_FLAG_CADENCE_MAJOR, EXO_FLAG_SORTED_TIMES, the *_cm_f64 entry points, exo_transit_flux_fwd_jac_f64 / _jac_vjp_f64,
 *     exo_transit_sparse_scatter_f64, exo_sho_coefficients_multi_*; a larger exo_celerite_state_doubles (the lane order of
 *     batches of mixed pair kinds lives in the state: forward and reverse call must be the same build); flag bits a build
 *     does not know are EXO_ERR_INVALID_ARGUMENT.
 * 11: the sparse model -- exo_sparse_model, exo_transit_flux_sparse_model, exo_transit_flux_vjp_sparse_f64,
 *     exo_celerite_loglike_sparse_{fwd,vjp}_f64, exo_celerite_default_chunks; EXO_FLAG_SPARSE accepted by the Jacobian pair;
 *     exo_transit_flux_cols_vjp_f64; EXO_GP_MAX_J 16; a larger exo_transit_flux_workspace_bytes.
 * 12: exo_sparse_model.row_of_draw covers EVERY per-draw array of a sparse celerite call (coefficients, pair kinds, per-draw diag,
 *     loglike, gloglike, the cotangents written back: all in the caller's order, nothing to permute); exo_sparse_model_order.
 * 13: the MERGED sparse model -- exo_sparse_merge_workspace_bytes, exo_sparse_merge_layout, exo_sparse_model_merge_f64,
 *     exo_sparse_model_merged, exo_sparse_model_merge_vjp_f64: several lists per draw (planets, occultations) as one.
 * 14: EXO_GP_PREPARE_ADJOINT, a flag or-ed into n_chunks of a celerite pair (the adjoint scan beside the forward chunk kernel).
 * 15: the predictive variance -- exo_celerite_predict_var_work_doubles, exo_celerite_predict_var_f64.
 * 16: period search -- exo_bls_workspace_bytes, exo_bls_power_f64, exo_lomb_scargle_power_f64.
 * 17: priors and constrained parameters -- exo_prior_block, EXO_PRIOR_*, exo_prior_transform_f64 / _vjp_f64.
 * 18: the white-noise likelihood with a sampled mean and jitter -- exo_transit_noise_vjp_f64, exo_transit_noise_ttv_vjp_f64,
 *     exo_white_noise_terms_f64, exo_white_noise_workspace_bytes; a slightly larger exo_transit_flux_workspace_bytes.
 * 19: the radial-velocity likelihood -- exo_rv_loglike_vjp_f64, EXO_RV_MAX_TREND, EXO_RV_MAX_INST.
 * 20: the solve -- exo_celerite_solve_work_doubles, exo_celerite_solve_f64.
 * 21: the astrometric likelihood -- exo_astrometry_loglike_vjp_f64.  (Entry points added since, no new number because no
 *     caller breaks: exo_tls_power_f64; exo_location_windows_f64, exo_running_location_f64, EXO_LOCATION_*;
 *     exo_timing_windows_f64, exo_transit_timing_f64, EXO_TIMING_*; exo_running_trend_f64, EXO_TREND_MAX_WINDOW;
 *     exo_keplerian_workspace_bytes, exo_keplerian_power_f64, EXO_KEP_*; exo_astrometric_workspace_bytes,
 *     exo_astrometric_power_f64, EXO_AST_NCOEF; exo_column_quantiles_f64, EXO_QUANTILE_MAX_Q;
 *     exo_column_psis_f64, EXO_PSIS_MAX_TAIL; exo_keplerian_max_workspace_bytes, exo_keplerian_max_f64;
 *     exo_metric_apply_f64, exo_metric_accumulate_f64, exo_metric_update_f64, EXO_METRIC_*;
 *     exo_laplace_points_f64, exo_laplace_factor_f64, EXO_LAPLACE_*.) */
#define EXO_ABI_VERSION 21
int32_t exo_abi_version(void);

/* ---------------------------------------------------------------------------
 * ops.kepler(M, ecc) -> (sinf, cosf)
 * replaces exoplanet_core's Kepler Op; reference call sites
 *   src/exoplanet/orbits/keplerian.py:333  (ecc pre-broadcast to M's shape)
 *   src/exoplanet/orbits/keplerian.py:818
 * ecc outside [0,1) -> NaN (docstring keplerian.py:58).
 * ------------------------------------------------------------------------- */
int exo_kepler_f64(const double* M, const double* ecc, double* sinf, double* cosf,
                   int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * ops.quad_solution_vector(b, r) -> s[..., 3]   (+ ds/db, ds/dr, nullable)
 * replaces exoplanet_core's quad_solution_vector Op; reference call site
 *   src/exoplanet/light_curves/limb_dark.py:24
 * Takes |b| (tests/light_curves_test.py:24-27 feed b < 0); dsdb carries sign(b).
 * s, dsdb, dsdr are [n][3].  Pass dsdb = dsdr = NULL for value only.
 * ------------------------------------------------------------------------- */
int exo_quad_solution_vector_f64(const double* b, const double* r, double* s,
                                 double* dsdb, double* dsdr, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * ops.contact_points(a, e, cosw, sinw, cosi, sini, L) -> (M_left, M_right, flag)
 * replaces exoplanet_core's contact_points Op; reference call site
 *   src/exoplanet/orbits/keplerian.py:744-753
 * flag != 0 means "no contact found"; the caller then evaluates every cadence
 * (keplerian.py:771-775).
 * ------------------------------------------------------------------------- */
int exo_contact_points_f64(const double* a, const double* e, const double* cosw,
                           const double* sinw, const double* cosi, const double* sini,
                           const double* L, double* M_left, double* M_right,
                           int32_t* flag, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * Fused transit flux: everything between the time array and the flux array of
 *   LimbDarkLightCurve.get_light_curve   (src/exoplanet/light_curves/limb_dark.py:99-232)
 *   KeplerianOrbit._get_true_anomaly / _get_position / _rotate_vector
 *                                        (src/exoplanet/orbits/keplerian.py:283-334,380-409)
 *   KeplerianOrbit.in_transit mask       (keplerian.py:729-731,765-769)
 *   SecondaryEclipseLightCurve blend     (src/exoplanet/light_curves/secondary_eclipse.py:45-70)
 * for `n_draw` independent parameter sets (posterior draws / chains) at once.
 *
 * Per-(draw, planet) parameter record, EXO_NPAR doubles, all lengths in units
 * of the stellar radius (the O(P) algebra that produces them stays on the host
 * side, in autograd):
 * ------------------------------------------------------------------------- */
#define EXO_NPAR 20
#define EXO_P_N 0       /* mean motion 2 pi / period            keplerian.py:146     */
#define EXO_P_TP 1      /* t_periastron = t0 - M0/n             keplerian.py:277     */
#define EXO_P_ECC 2     /* eccentricity (0 for ecc=None)                              */
#define EXO_P_COSW 3    /* cos(omega)   (1 for ecc=None)        keplerian.py:303-308 */
#define EXO_P_SINW 4    /* sin(omega)   (0 for ecc=None)                              */
#define EXO_P_COSI 5    /* cos(incl)                            keplerian.py:227,312 */
#define EXO_P_SINI 6    /* sin(incl)  (only its sign is used: los > 0 test)          */
#define EXO_P_AOR 7     /* a / R_star                                                 */
#define EXO_P_ROR 8     /* r_planet / R_star                                          */
#define EXO_P_T0 9      /* reference transit time (window phase) keplerian.py:731    */
#define EXO_P_PERIOD 10 /* period                                                     */
#define EXO_P_TS 11     /* first contact  - t0 (<= 0), without texp keplerian.py:755-762 */
#define EXO_P_TE 12     /* fourth contact - t0 (>= 0)                                 */
#define EXO_P_FRATIO 13 /* secondary: sbr * ror^2                secondary_eclipse.py:68 */
#define EXO_P_TS2 14    /* secondary-eclipse window start - t0 (may exceed +-P/2)    */
#define EXO_P_TE2 15    /* secondary-eclipse window end   - t0                        */
#define EXO_P_CLIGHT 16 /* speed of light in stellar radii per day (constants.py:36 / R_star): only read
                           with EXO_FLAG_LIGHT_DELAY                                  */
/* slots 17 .. 19: reserved, written as 0 by the packing kernel, not read */

/* flags */
#define EXO_FLAG_PER_PLANET 1u /* flux is [n_draw][n_cad][n_planet] instead of summed [n_draw][n_cad] */
#define EXO_FLAG_WINDOW 2u     /* skip cadences outside [TS,TE] (+- texp/2): use_in_transit semantics */
#define EXO_FLAG_SECONDARY 4u  /* also evaluate the occultation of the planet; ld is [n_draw][6]      */
/* 8u is EXO_PACK_CIRCULAR (record packing only) */
#define EXO_FLAG_EXACT_SCAN 16u /* classify cadences with the fp64 Kepler solve instead of the conservative
                                   fp32 pre-filter.  Results are identical either way (accepted cadences are
                                   always evaluated in fp64); the flag exists to measure / verify that.      */

#define EXO_FLAG_SPARSE 32u     /* run-enumeration sweeps only (sorted t, scalar or no texp, no timing tables, no
                                   EXO_FLAG_EXACT_SCAN; EXO_ERR_INVALID_ARGUMENT otherwise): the flux array is NOT
                                   touched (pass NULL); the output is the runs of cadences in which a planet can
                                   overlap the disk and a compact value array, both inside `workspace`
                                   (exo_transit_flux_sparse_layout); every other cadence has flux exactly 0.  */

#define EXO_FLAG_LIGHT_DELAY 64u /* light-travel delay (keplerian.py:411-470, _get_retarded_position with z0 = 0):
                                   a body is seen where it was at t - delay, the delay from its line-of-sight
                                   position, velocity and acceleration at t; a second Kepler solve per sample, in
                                   the same kernel.  Needs slot EXO_P_CLIGHT and the VALUE of EXO_P_SINI (both get
                                   cotangents then).  Run-enumeration sweeps only (see EXO_FLAG_SPARSE).        */

#define EXO_FLAG_CADENCE_MAJOR 128u /* the dense SUMMED flux arrays of the call -- flux (out), gflux (in) -- are
                                      [n_cad][n_draw] instead of [n_draw][n_cad]: the layout the celerite kernels read
                                      with every wave's accesses contiguous (exo_celerite_loglike_obs_*_cm_f64).
                                      Run-enumeration sweeps only (see EXO_FLAG_SPARSE); not with
                                      EXO_FLAG_PER_PLANET (EXO_ERR_INVALID_ARGUMENT).                            */

#define EXO_FLAG_SORTED_TIMES 256u /* the caller has CHECKED that t is non-decreasing (the sweep otherwise checks it on
                                     the device, every call, in a launch of its own before the searches): windows and runs
                                     then come out of one launch.  The word is taken for NEIGHBOURING cadences only: the
                                     launch still looks at 65 evenly spaced cadences, and a series that does not ascend
                                     through them (a NaN included) is swept cadence by cadence, as without the flag.
                                     Disorder finer than that under this flag gives undefined results; without the flag
                                     unsorted times are merely slow (every cadence solved).  A flag is part of a captured
                                     launch: it must hold for whatever the time buffer contains at every replay.       */

/* a sweep called with a flag bit outside this set returns EXO_ERR_INVALID_ARGUMENT */
#define EXO_FLAG_SWEEP_ALL (EXO_FLAG_PER_PLANET | EXO_FLAG_WINDOW | EXO_FLAG_SECONDARY | EXO_FLAG_EXACT_SCAN | \
                            EXO_FLAG_SPARSE | EXO_FLAG_LIGHT_DELAY | EXO_FLAG_CADENCE_MAJOR | EXO_FLAG_SORTED_TIMES)

#define EXO_MAX_PLANETS 16
#define EXO_MAX_SUBEXP 63

/* Forward.
 *   t          [n_cad]                  shared by all draws
 *   texp       NULL (n_texp = 0), scalar (n_texp = 1) or per cadence (n_texp = n_cad)
 *   stencil_dt [n_sub], stencil_w [n_sub]   exposure stencil in units of texp
 *                                       (limb_dark.py:181-197); n_sub = 1 if no texp
 *   params     [n_draw][n_planet][EXO_NPAR]
 *   ld         [n_draw][3] Green's-basis coefficients c of get_cl (limb_dark.py:11-18),
 *              or [n_draw][6] = primary c then secondary c with EXO_FLAG_SECONDARY
 *   flux       out, see EXO_FLAG_PER_PLANET
 *   workspace  exo_transit_flux_workspace_bytes() bytes of scratch                 */
int exo_transit_flux_fwd_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                             const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                             const double* params, const double* ld, int64_t n_draw,
                             int32_t n_planet, uint32_t flags, double* flux, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* Bytes of scratch the fused entry points need (active-cadence lists of the scan
 * kernel + the deterministic two-stage gradient reduction).                     */
int64_t exo_transit_flux_workspace_bytes(int64_t n_cad, int64_t n_draw, int32_t n_planet);

/* Where the sparse output of an EXO_FLAG_SPARSE sweep lives inside `workspace` (same n_cad, n_draw,
 * n_planet as the sweep).  out[0..4] = byte offsets of nrun, runs, pre_all, vals, and r_max:
 *   list = (draw * n_planet + planet) * n_ev + event   (n_ev = 2 with EXO_FLAG_SECONDARY: 0 transits,
 *                                                       1 occultations; else n_ev = 1)
 *   nrun    int32 [n_list]                 windows of the list that reach into the series
 *   runs    int32 [n_list][r_max][4]       (lo, a, b, hi): cadences [lo, hi) of window k
 *   pre_all int32 [n_list][r_max + 1]      exclusive prefix sums of hi - lo
 *   vals    double [n_draw][n_planet][n_cad]  flux of cadence i of window k of (draw, planet):
 *           vals[draw][planet][(event ? pre_all[list of event 0][nrun] : 0) + pre_all[list][k] + i - lo]
 * (per planet, EXO_FLAG_PER_PLANET or not).  If t is not sorted, or a window cannot be bounded, the
 * list is the whole series cut into a few runs.                                                   */
int exo_transit_flux_sparse_layout(int64_t n_cad, int64_t n_draw, int32_t n_planet, int64_t* out);

/* The sparse output as a MODEL for the celerite entries (exo_celerite_loglike_sparse_*_f64, which see for the layout): segments
 * of cadences + their values, per draw.  exo_transit_flux_sparse_model fills the descriptor with pointers into `workspace`
 * (that of an EXO_FLAG_SPARSE sweep with the same n_cad, n_draw, n_planet; flags: EXO_FLAG_SECONDARY as the sweep had it).
 * One list per draw (one planet, no occultations): the runs are the segments.  Otherwise EXO_ERR_INVALID_ARGUMENT -- callers
 * merge the lists first (exo_sparse_model_merge_f64 below) or keep the dense model.                                                                                      */
typedef struct exo_sparse_model {
  const int32_t* nseg;
  const int32_t* seg;
  const int32_t* off;
  const double* vals;
  int64_t seg_row, off_row, val_row;
  int32_t seg_step, hi_at;
  const int32_t* row_of_draw;   /* NULL, or [n_draw], a permutation: the ORDER in which the celerite kernels take the draws -- their
                                   draw d (a lane; 64 consecutive ones a wave) is row row_of_draw[d] of nseg / seg / off / vals / gvals
                                   AND of every other per-draw array of the call: coefficients, pair kinds, a per-draw diag, loglike,
                                   gloglike, gcoef_*, gdiag, gdiag_sum.  All arrays stay in the caller's order; nothing is permuted
                                   (ABI 12; ABI 11 applied it to the model alone).  Why: a wave pays for a transit while ANY of its 64
                                   draws is inside one; taking the draws sorted by transit timing (exo_sparse_model_order) keeps a
                                   wave's transits together -- C3: 3.6 -> 3.3 ms of GP kernels.  exo_transit_flux_sparse_model sets it
                                   to NULL.                                                                                     */
} exo_sparse_model;
int exo_transit_flux_sparse_model(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw,
                                  int32_t n_planet, uint32_t flags, exo_sparse_model* out);
/* The MERGED model (ABI 13): what exo_transit_flux_sparse_model refuses.  A draw with several lists -- n_planet planets, and with
 * EXO_FLAG_SECONDARY a transit and an occultation list each -- becomes ONE ascending list of disjoint segments: the union of
 * the lists' runs, a cadence's value the SUM of the values the lists hold for it (the reference sums the planets per cadence,
 * limb_dark.py:228-230; a planet's transit and occultation never share a cadence, secondary_eclipse.py:67-70).  It lives in a
 * caller-owned `merge_ws` (exo_sparse_merge_workspace_bytes; layout: exo_sparse_merge_layout out[0..4] = byte offsets of
 * nseg int32 [n_draw], seg int32 [n_draw][cap][2] = (lo, hi), off int32 [n_draw][cap + 1], vals double [n_draw][n_cad], and cap):
 *   exo_sparse_model_merge_f64       two launches on `stream` (segments: a block per draw, every run ranked among the draw's
 *                                    runs by binary search, a prefix-maximum scan of the run ends; values: a thread per merged
 *                                    cadence); `workspace` = the EXO_FLAG_SPARSE sweep's, same n_cad / n_draw / n_planet / flags;
 *                                    fills `out` (may be NULL)
 *   exo_sparse_model_merged          the descriptor alone (no launch): for the reverse call
 *   exo_sparse_model_merge_vjp_f64   gvals (the sweep's value layout: what exo_transit_flux_vjp_sparse_f64 takes) from gmvals
 *                                    [n_draw][n_cad], the cotangent the celerite reverse entry wrote for the merged values
 * n_cad < 2^31, n_draw <= 65535.  Deterministic (no atomics): a merged value is summed in list order.                        */
int64_t exo_sparse_merge_workspace_bytes(int64_t n_cad, int64_t n_draw, int32_t n_planet);
int exo_sparse_merge_layout(int64_t n_cad, int64_t n_draw, int32_t n_planet, int64_t* out);
int exo_sparse_model_merge_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                               uint32_t flags, void* merge_ws, int64_t merge_ws_bytes, exo_sparse_model* out, void* stream);
int exo_sparse_model_merged(const void* merge_ws, int64_t merge_ws_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                            exo_sparse_model* out);
int exo_sparse_model_merge_vjp_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                                   uint32_t flags, const void* merge_ws, int64_t merge_ws_bytes, const double* gmvals,
                                   double* gvals, void* stream);
/* order [n_draw] (device, int32): the draws of `model` (its rows 0 .. n_draw - 1; row_of_draw ignored) by ascending mean spacing of
 * their segments -- the period, in cadences: neighbouring periods keep their transits together all along the series -- ties by the
 * start of the first segment, then by index: what to pass as row_of_draw.  One launch, no host synchronisation.  n_draw <=
 * EXO_SPARSE_ORDER_MAX_DRAWS (EXO_ERR_INVALID_ARGUMENT beyond: sort on the host side, or pass NULL).                          */
#define EXO_SPARSE_ORDER_MAX_DRAWS 4096
int exo_sparse_model_order(const exo_sparse_model* model, int64_t n_draw, int32_t* order, void* stream);
/* Reverse sweep for a cotangent given in the VALUE layout of the sparse output -- gvals [n_draw][n_planet][n_cad], gvals of
 * (draw, planet) at the positions of that planet's values: what exo_celerite_loglike_sparse_vjp_f64 writes -- instead of a
 * dense gflux.  flags must carry EXO_FLAG_SPARSE (and whatever the forward sweep carried); otherwise as
 * exo_transit_flux_vjp_f64 without flux_out.  reuse_runs != 0: `workspace` is the forward sweep's, untouched since, for these
 * very t / params (the windows and runs in it are reused: no enumeration launch).                                       */
int exo_transit_flux_vjp_sparse_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                    const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                    const double* params, const double* ld, int64_t n_draw, int32_t n_planet,
                                    uint32_t flags, const double* gvals, double* gparams, double* gld, double* flux_dot,
                                    void* workspace, int64_t workspace_bytes, int32_t reuse_runs, void* stream);

/* A light curve whose cotangent is not known yet (the mean of a GP: limb_dark.py:99-232 feeding celerite2's
 * log_likelihood; the cotangent is the GP's gradient with respect to its mean): the forward sweep and, once the cotangent
 * exists, its VJP WITHOUT a second sweep.  exo_transit_flux_fwd_jac_f64 is exo_transit_flux_fwd_f64 (same arguments, same flux,
 * bit for bit) that also leaves, for every solved cadence, the sixteen derivatives of its flux -- ten record slots, six
 * limb-darkening coefficients -- in `jac` (exo_transit_flux_jac_doubles(n_cad, n_draw, n_planet) doubles, caller-owned);
 * exo_transit_flux_jac_vjp_f64 contracts them with the cotangent (rows or EXO_FLAG_CADENCE_MAJOR, as the flux was) into what
 * exo_transit_flux_vjp_f64 returns.  `workspace` of the second call is the forward call's, untouched in between (it holds
 * the runs, the values and their cadences).  Run-enumeration sweeps (see EXO_FLAG_SPARSE) of the summed flux, without timing
 * tables, EXO_FLAG_LIGHT_DELAY or EXO_FLAG_PER_PLANET: EXO_ERR_INVALID_ARGUMENT otherwise -- callers keep
 * the two-sweep route for those.  With EXO_FLAG_SPARSE (both calls): flux may be NULL and is not written, and gflux is
 * the cotangent in the value layout (see exo_transit_flux_vjp_sparse_f64).  Worth it when a cadence is several samples (an exposure stencil: each of them a Kepler
 * solve, the row still sixteen doubles); bit-reproducible.                                                              */
int64_t exo_transit_flux_jac_doubles(int64_t n_cad, int64_t n_draw, int32_t n_planet);
int exo_transit_flux_fwd_jac_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                 const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                 int64_t n_draw, int32_t n_planet, uint32_t flags, double* flux, double* jac,
                                 int64_t jac_doubles, void* workspace, int64_t workspace_bytes, void* stream);
int exo_transit_flux_jac_vjp_f64(const double* gflux, int64_t n_cad, int64_t n_draw, int32_t n_planet, uint32_t flags,
                                 const double* jac, void* workspace, int64_t workspace_bytes, double* gparams, double* gld,
                                 double* flux_dot, void* stream);

/* White-noise Gaussian likelihood of ONE observed series against the light curves of n_draw parameter sets, value and
 * gradient, without a dense flux array -- what a sampler step needs when there is no correlated-noise model (the
 * reference's `pm.Normal("obs", mu=light_curve, sigma=yerr, observed=y)`, docs/tutorials: the (draw, cadence) arrays of
 * flux, residual and their cotangents never exist).  With f[d][n] the summed flux of draw d (exactly 0 outside the runs
 * of the sparse output, see EXO_FLAG_SPARSE), w_n = ivar[n_ivar == 1 ? 0 : n]:
 *   chi2[d]   = sum over the cadences n solved for draw d of  w_n ((f[d][n] - obs[n])^2 - obs[n]^2)
 *             = sum_n w_n (f[d][n] - obs[n])^2  -  sum_n w_n obs[n]^2      (the second sum is the caller's constant)
 *   gparams, gld = d chi2[d] / d (params, ld)
 * One planet without occultation or exposure stencil: ONE evaluation per solved cadence (the cotangent 2 w (f - obs) is
 * formed inside it).  Otherwise three sweeps' worth of launches in one call: values into the sparse output, residuals and
 * cotangents on it (a draw's planets may transit at once: every value sees the draw's total flux at its cadence),
 * gradient sweep.  Sorted t, one
 * exposure time (or none), no timing tables (EXO_ERR_INVALID_ARGUMENT otherwise); flags: EXO_FLAG_SECONDARY,
 * EXO_FLAG_WINDOW, EXO_FLAG_LIGHT_DELAY.  Bit-reproducible.                                                          */
int exo_transit_chi2_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                             const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                             int64_t n_draw, int32_t n_planet, uint32_t flags, const double* obs, const double* ivar,
                             int64_t n_ivar, double* chi2, double* gparams, double* gld, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* The same likelihood for an orbit with transit-timing variations (tables as for exo_transit_flux_ttv_vjp_f64, which
 * see; transits only, no light delay: EXO_FLAG_WINDOW is the one flag), plus
 *   gshift [n_draw][n_planet][n_edge + 1] = d chi2[d] / d ttv_shift
 * -- the gradient of a timing fit (TTVOrbit with `ttvs` or `transit_times` as parameters: ttv.py:71-156) without a
 * (draw, cadence) array.  n_cad >= 1.  One planet and no exposure stencil: one evaluation per solved cadence. */
int exo_transit_chi2_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                 const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                 int64_t n_draw, int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                 const double* ttv_shift, int32_t n_edge, const double* obs, const double* ivar,
                                 int64_t n_ivar, double* chi2, double* gparams, double* gld, double* gshift, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* The same likelihood with a PER-DRAW mean and a PER-DRAW jitter added in quadrature -- the reference's
 * `pm.Normal("obs", mu=mean + light_curve, sigma=sqrt(yerr**2 + exp(2 * log_jitter)), observed=y)` with `mean` and
 * `log_jitter` sampled.  With v_n = var[n_var == 1 ? 0 : n] (yerr^2), mean_d = mean[n_mean == 1 ? 0 : d],
 * s2_d = n_jit == 0 ? 0 : jit2[n_jit == 1 ? 0 : d] (jitter^2), w_dn = 1 / (v_n + s2_d), r_dn = y[n] - mean_d, and the sums
 * over the cadences n solved for draw d:
 *   chi2[d]  = sum w_dn (f[d][n]^2 - 2 f[d][n] r_dn)           (= exo_transit_chi2_vjp_f64 with obs = r_d, ivar = w_d)
 *   gmean[d] = sum w_dn f[d][n]                                 (d chi2 / d mean_d = 2 gmean[d])
 *   gjit2[d] = sum w_dn^2 (f[d][n]^2 - 2 f[d][n] r_dn)          (d chi2 / d s2_d = -gjit2[d])
 *   gparams, gld = d chi2[d] / d (params, ld)                   (cotangent 2 w_dn (f - r_dn) per solved cadence)
 * The sums over ALL cadences that complete the likelihood are exo_white_noise_terms_f64.  n_var: 1 or n_cad; n_mean: 1 or
 * n_draw; n_jit: 0, 1 or n_draw (EXO_ERR_INVALID_ARGUMENT otherwise).  Routes, flags, workspace and the other argument
 * checks are those of exo_transit_chi2_vjp_f64; the two extra sums ride the same block partials in the same fixed order:
 * bit-reproducible, no floating-point atomics. */
int exo_transit_noise_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                              const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                              int64_t n_draw, int32_t n_planet, uint32_t flags, const double* y, const double* var,
                              int64_t n_var, const double* mean, int64_t n_mean, const double* jit2, int64_t n_jit,
                              double* chi2, double* gmean, double* gjit2, double* gparams, double* gld, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* ... and with timing tables: exo_transit_chi2_ttv_vjp_f64 (which see for the tables, the flags and gshift) with the
 * data arguments and the two extra sums of exo_transit_noise_vjp_f64. */
int exo_transit_noise_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp, const double* stencil_dt,
                                  const double* stencil_w, int32_t n_sub, const double* params, const double* ld,
                                  int64_t n_draw, int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                  const double* ttv_shift, int32_t n_edge, const double* y, const double* var, int64_t n_var,
                                  const double* mean, int64_t n_mean, const double* jit2, int64_t n_jit, double* chi2,
                                  double* gmean, double* gjit2, double* gparams, double* gld, double* gshift, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* The data side of that likelihood: for every draw the sums over ALL n_cad cadences (notation as above)
 *   terms[0][d] = Q   = sum w_dn r_dn^2         terms[1][d] = Lam = sum log(v_n + s2_d)
 *   terms[2][d] = G   = sum w_dn r_dn           terms[3][d] = H   = sum w_dn^2 r_dn^2        terms[4][d] = A = sum w_dn
 * (terms is [5][n_draw]), so that
 *   loglike_d = -(Q + chi2 + Lam) / 2 - n_cad / 2 log(2 pi),   d / d mean_d = G - gmean,   d / d s2_d = (H + gjit2 - A) / 2.
 * Three regimes, chosen from n_var, n_mean and n_jit alone:
 *   n_jit == 0 or n_var == 1: the weight separates, w_dn = u_n x (a factor of the draw).  Per-series sums of the series
 *     CENTRED on its weighted mean (series[0..7]: ybar, sum u, sum u y', sum u y'^2, sum u^2, sum u^2 y', sum u^2 y'^2,
 *     sum log v; y' = y - ybar) are taken in one launch unless series_ready != 0 says that `series` still holds them for
 *     this (y, var) -- they are data -- and every draw is O(1) work from them.  Centring keeps Q a sum of non-negative terms.
 *   otherwise (per-cadence variances AND a jitter): one pass over (draw, cadence), no array of that size; Lam as the
 *     logarithm of a running product of mantissas with a summed exponent.  workspace: exo_white_noise_workspace_bytes.
 * `series` ([8], device) may be null in the second regime; `workspace` in the first.  Every sum in a fixed order:
 * bit-reproducible, and a draw's terms do not depend on the batch it is in.  n_draw == 0: nothing to do. */
int64_t exo_white_noise_workspace_bytes(int64_t n_cad, int64_t n_draw);
int exo_white_noise_terms_f64(const double* y, const double* var, int64_t n_cad, int64_t n_var, const double* mean,
                              int64_t n_mean, const double* jit2, int64_t n_jit, int64_t n_draw, double* series,
                              int32_t series_ready, double* terms, void* workspace, int64_t workspace_bytes, void* stream);

/* Diagnostic for the scan kernel's conservative fp32 cadence classifier: the fp32
 * estimate of (cos E - e, sqrt(1-e^2) sin E) for mean anomaly M (fp64 phase) and
 * eccentricity ecc, widened back to double.  The classifier's safety margin assumes
 * |error| <= 8e-4; tests/test_gpu_scan_filter.py checks that here.                 */
int exo_selftest_orbit_pos_f32(const double* M, const double* ecc, double* cx, double* sx, int64_t n,
                               void* stream);

/* Profiling hook shared by the fused entry points below: if `ev_start` /
 * `ev_stop` (hipEvent_t passed as void*, may be NULL) are given, they are
 * recorded on `stream` immediately before the first / after the last kernel of the
 * sweep (scan + heavy [+ reduce]; the small memset of the gradient buffer stays
 * outside), so a caller can time the kernels alone without a profiler attached. */
int exo_transit_flux_fwd_ev_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                const double* params, const double* ld, int64_t n_draw,
                                int32_t n_planet, uint32_t flags, double* flux, void* workspace,
                                int64_t workspace_bytes, void* stream, void* ev_start, void* ev_stop);

/* Reverse (recompute-forward): given gflux (same shape as flux) accumulate
 *   gparams [n_draw][n_planet][EXO_NPAR]  (slots T0, PERIOD, TS.. are 0; SINI, CLIGHT too without EXO_FLAG_LIGHT_DELAY)
 *   gld     [n_draw][3 or 6]
 * and, if flux_out != NULL, also write the forward value in the same pass
 * (value + gradient in one sweep over t: 24 B per (draw, cadence)); if
 * flux_dot != NULL, flux_dot[n_draw] receives sum_n gflux * flux per draw (the
 * scalar whose gradient gparams / gld are).                                    */
int exo_transit_flux_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                             const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                             const double* params, const double* ld, int64_t n_draw,
                             int32_t n_planet, uint32_t flags, const double* gflux,
                             double* flux_out, double* gparams, double* gld, double* flux_dot,
                             void* workspace, int64_t workspace_bytes, void* stream);
int exo_transit_flux_vjp_ev_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                const double* params, const double* ld, int64_t n_draw,
                                int32_t n_planet, uint32_t flags, const double* gflux,
                                double* flux_out, double* gparams, double* gld, double* flux_dot,
                                void* workspace, int64_t workspace_bytes, void* stream, void* ev_start,
                                void* ev_stop);

/* The whole user-level step of a standard-parameterisation orbit in one call (round 5): the constructor's COLUMNS in -- as
 * exo_pack_records_cols_f64, which see below: cols / draw_stride / planet_stride / defaults / ld_cols / ld_draw_stride are HOST
 * arrays of device pointers, strides and defaults; pack_flags: EXO_PACK_CIRCULAR, EXO_FLAG_WINDOW, EXO_FLAG_SECONDARY (as in
 * flags) -- the records (params, ld: written, the caller's buffers), the value + VJP sweep of exo_transit_flux_vjp_f64 (flux_out
 * nullable or, with EXO_FLAG_SPARSE, unused; gparams, gld, flux_dot out), and, fold != 0, the packing VJP behind it:
 *   gcols[k] [n_draw][n_planet], gld_cols[k] [n_draw]  (HOST arrays of device pointers, NULL entry = not wanted)
 *                = gscale[d] (or 1, gscale == NULL) x d sum_n gflux flux / d column
 * On a run-enumeration sweep with EXO_FLAG_SORTED_TIMES the packing rides on the windows + enumeration launch (every list's wave
 * packs its own record: no packing launch in front); the packing VJP is a launch of its own behind the sweep (folded into the
 * sweep's last kernel it was measured slower: one thread's serial chain at the tail of every block).  Anything else runs the three
 * calls one after the other: same results, bit for bit.  ev_start / ev_stop as exo_transit_flux_vjp_ev_f64.  Reference:
 * keplerian.py:75-281 + limb_dark.py:99-232 and their gradients, one likelihood-gradient evaluation of a sampler.      */
int exo_transit_flux_cols_vjp_f64(const double* const* cols, const int64_t* draw_stride, const int64_t* planet_stride,
                                  const double* defaults, const double* const* ld_cols, const int64_t* ld_draw_stride,
                                  uint32_t pack_flags, const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                  const double* stencil_dt, const double* stencil_w, int32_t n_sub, int64_t n_draw,
                                  int32_t n_planet, uint32_t flags, const double* gflux, double* flux_out, double* params,
                                  double* ld, double* gparams, double* gld, double* flux_dot, int32_t fold,
                                  const double* gscale, double* const* gcols, double* const* gld_cols, void* workspace,
                                  int64_t workspace_bytes, void* stream, void* ev_start, void* ev_stop);

/* ---------------------------------------------------------------------------
 * The same two sweeps for an orbit with transit-timing variations
 *   TTVOrbit._get_model_dt / _warp_times   (src/exoplanet/orbits/ttv.py:158-187)
 * Every time -- cadence or sub-exposure -- is measured from its nearest labelled
 * transit before it reaches the orbit: planet p of draw d has
 *   ttv_edges [n_draw][n_planet][n_edge]      ascending bin edges (ttv.py:158-166:
 *                                             midpoints between consecutive transit times,
 *                                             closed by half a period either side); rows
 *                                             with fewer edges are padded with +inf
 *   ttv_shift [n_draw][n_planet][n_edge + 1]  per bin k = #{edges < t} (searchsorted,
 *                                             ttv.py:171-172): transit time of the bin
 *                                             (ttv.py:167-170) MINUS the record's t0
 * and a time t acts as t - ttv_shift[k(t)]: mean anomaly (t - shift - TP) N, window
 * phase t - shift - T0.  The reverse sweep adds
 *   gshift    [n_draw][n_planet][n_edge + 1]  d sum(gflux * flux) / d ttv_shift
 * Sorted times, one exposure time (or none), no occultations: the windows are enumerated per
 * timing bin (run-enumeration sweep; EXO_FLAG_SPARSE is accepted), and gshift is summed run by
 * run in a fixed order -- bit-reproducible -- unless a transit lies across a bin edge (that
 * list's samples look their bins up one by one).  Otherwise, and for such lists: hardware fp64
 * atomics, one per wave and cadence run -- the last bits of gshift depend on scheduling;
 * everything else is as reproducible as without timing variations.
 * EXO_FLAG_WINDOW: the caller's windows are tested on the warped mid-exposure time
 * (keplerian.py:729-731 with ttv.py:181-187).
 * ------------------------------------------------------------------------- */
#define EXO_MAX_TTV_EDGES 65536
int exo_transit_flux_ttv_fwd_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                 const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                 const double* params, const double* ld, int64_t n_draw,
                                 int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                 const double* ttv_shift, int32_t n_edge, double* flux,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int exo_transit_flux_ttv_vjp_f64(const double* t, int64_t n_cad, const double* texp, int64_t n_texp,
                                 const double* stencil_dt, const double* stencil_w, int32_t n_sub,
                                 const double* params, const double* ld, int64_t n_draw,
                                 int32_t n_planet, uint32_t flags, const double* ttv_edges,
                                 const double* ttv_shift, int32_t n_edge, const double* gflux,
                                 double* flux_out, double* gparams, double* gld, double* gshift,
                                 double* flux_dot, void* workspace, int64_t workspace_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * Stellar reflex radial velocity from the same Kepler solve
 *   KeplerianOrbit.get_radial_velocity   (src/exoplanet/orbits/keplerian.py:633-677)
 * for n_draw parameter sets:   rv[d][n][p] = AMP (COSW cos f - SINW sin f + ECC COSW),
 * f the true anomaly at mean anomaly (t_n - TP) N.  Per-(draw, planet) record, EXO_RV_NPAR
 * doubles; AMP is the caller's K (keplerian.py:660-669; ECC = 0, COSW = 1, SINW = 0 for a
 * circular orbit, :658-659) or, for the mass-based form (:671-676, with :572-578 and :283-322),
 * conv sin(incl) K0 m_planet.  rv / grv are [n_draw][n_cad][n_planet] (the reference returns
 * one column per planet); gparams [n_draw][n_planet][EXO_RV_NPAR].
 * ------------------------------------------------------------------------- */
#define EXO_RV_NPAR 6
#define EXO_RV_N 0     /* mean motion                      */
#define EXO_RV_TP 1    /* t_periastron                     */
#define EXO_RV_ECC 2   /* eccentricity (NaN result outside [0, 1)) */
#define EXO_RV_COSW 3
#define EXO_RV_SINW 4
#define EXO_RV_AMP 5   /* semi-amplitude                   */
int exo_radial_velocity_fwd_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw,
                                int32_t n_planet, double* rv, void* stream);
int exo_radial_velocity_vjp_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw,
                                int32_t n_planet, const double* grv, double* gparams, void* stream);

/* ---------------------------------------------------------------------------
 * Gaussian log-likelihood of an observed radial-velocity series, value and every gradient in ONE launch -- the tutorials'
 *   rv_model = zero_point + orbit.get_radial_velocity(t, K=semiamp) [+ trend];  sigma = sqrt(rv_err**2 + exp(2 log_jitter));
 *   pm.Normal("obs", mu=rv_model, sigma=sigma, observed=rv_obs)
 * for n_draw parameter sets.  With g(t; rec) = COSW (cos f + ECC) - SINW sin f of the records above:
 *   m[d][n]  = sum_p AMP[d][p] g(t_n; rec[d][p]) + sum_{k < n_trend} trend[d][k] tau_n^k + offset[d][inst_n]
 *   s2[d][n] = var[n_var == 1 ? 0 : n] + jit2[d][inst_n],    w = 1 / s2,    rho = w (rv_n - m)
 *   loglike[d]    = -1/2 sum_n (w (rv_n - m)^2 + log s2) - n_cad / 2 log(2 pi)
 *   gparams[d][p] = d loglike / d rec[d][p]      (EXO_RV_NPAR doubles: the reverse pass of the radial velocity with cotangent rho)
 *   gtrend[d][k]  = sum_n rho tau_n^k
 *   goffset[d][i] = sum over the epochs of instrument i of rho
 *   gjit2[d][i]   = 1/2 sum over the epochs of instrument i of (rho^2 - w)
 * t [n_cad] are the epochs the orbit is evaluated at; tau [n_cad] = t - t_ref is formed by the caller (the kernel subtracts no
 * large numbers; may be null when n_trend <= 1).  inst: int32 [n_cad], the instrument of every epoch, in [0, n_inst) (an index
 * outside gives NaN in every draw; may be null when n_inst == 1).  rv [n_cad]; var [n_var], n_var = 1 or n_cad.  params
 * [n_draw][n_planet][EXO_RV_NPAR], n_planet <= EXO_MAX_PLANETS.  trend [n_draw][n_trend], 0 <= n_trend <= EXO_RV_MAX_TREND,
 * powers increasing.  offset, jit2 [n_draw][n_inst], 1 <= n_inst <= EXO_RV_MAX_INST; either may be null (zero).  A null
 * gradient output is not written.  An instrument without epochs gets gradients of exactly 0; ECC outside [0, 1) gives NaN in
 * that draw only.  No workspace: one workgroup per draw, whose width depends on n_cad alone, every sum in a fixed order
 * (bit-reproducible, and a draw's results do not depend on the batch it is in).  n_draw == 0: EXO_OK, nothing launched.
 * ------------------------------------------------------------------------- */
#define EXO_RV_MAX_TREND 4
#define EXO_RV_MAX_INST 8
int exo_rv_loglike_vjp_f64(const double* t, const double* tau, const int32_t* inst, const double* rv, const double* var,
                           int64_t n_cad, int64_t n_var, const double* params, int64_t n_draw, int32_t n_planet,
                           const double* trend, int32_t n_trend, const double* offset, const double* jit2, int32_t n_inst,
                           double* loglike, double* gparams, double* gtrend, double* goffset, double* gjit2, void* stream);

/* ---------------------------------------------------------------------------
 * Position / velocity vectors in the observer frame from the same solve.  Replaces, for n_draw parameter sets, the
 * sub-graph behind
 *   KeplerianOrbit.get_{star,planet,relative}_position   (src/exoplanet/orbits/keplerian.py:472-542 -> :380-409)
 *   KeplerianOrbit.get_{star,planet,relative}_velocity   (keplerian.py:580-631 -> :572-578)
 *   KeplerianOrbit.get_relative_angles                   (keplerian.py:544-570: rho, theta from X, Y)
 *   KeplerianOrbit.get_{star,planet,relative}_acceleration   (keplerian.py:679-706)
 * In the orbital plane  position (flags = 0): (u, v) = (1 - e^2) / (1 + e cos f) (cos f, sin f);  flags =
 * EXO_OV_VELOCITY: (u, v) = (-sin f, cos f + e);  flags = EXO_OV_ACCELERATION: (u, v) = -(1 + e cos f)^2 / (1 - e^2)
 * (cos f, sin f);  then _rotate_vector (keplerian.py:283-322) and the amplitude:
 *   x1 = COSW u - SINW v, y1 = SINW u + COSW v;  x2 = x1, y2 = COSI y1, Z = -SINI y1;
 *   X = COSO x2 - SINO y2, Y = SINO x2 + COSO y2;   out[d][n][p] = AMP (X, Y, Z)
 * AMP: a_star / a_planet / -a (times parallax au_per_R_sun, keplerian.py:404-406) for positions, K0 m for velocities,
 * (K0 m)^2 / a for accelerations;
 * COSO = 1, SINO = 0 when the orbit has no Omega; ECC = 0, COSW = 1, SINW = 0 when circular.
 * out / gout [n_draw][n_cad][n_planet][3]; params / gparams [n_draw][n_planet][EXO_OV_NPAR].
 * ------------------------------------------------------------------------- */
#define EXO_OV_NPAR 10
#define EXO_OV_N 0
#define EXO_OV_TP 1
#define EXO_OV_ECC 2    /* NaN result outside [0, 1) */
#define EXO_OV_COSW 3
#define EXO_OV_SINW 4
#define EXO_OV_COSI 5
#define EXO_OV_SINI 6
#define EXO_OV_AMP 7
#define EXO_OV_COSO 8
#define EXO_OV_SINO 9
#define EXO_OV_VELOCITY 1u
#define EXO_OV_ACCELERATION 2u
int exo_orbit_vector_fwd_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, double* out, void* stream);
int exo_orbit_vector_vjp_f64(const double* t, int64_t n_cad, const double* params, int64_t n_draw, int32_t n_planet,
                             uint32_t flags, const double* gout, double* gparams, void* stream);

/* ---------------------------------------------------------------------------
 * Gaussian log-likelihood of an observed astrometric series -- separation rho_n and position angle theta_n of ONE companion
 * at the epochs t_n, with independent errors -- value and every gradient in ONE launch: the tutorial's
 *   rho_model, theta_model = orbit.get_relative_angles(t, parallax);
 *   pm.Normal("rho_obs", mu=rho_model, sd=sqrt(rho_err**2 + exp(2 log_rho_s)), observed=rho_data)
 *   theta_diff = arctan2(sin(theta_model - theta_data), cos(theta_model - theta_data))      (the wrap across the branch cut)
 *   pm.Normal("theta_obs", mu=theta_diff, sd=sqrt(theta_err**2 + exp(2 log_theta_s)), observed=0)
 * for n_draw parameter sets.  rec[d] is an EXO_OV_* record (above) and (X, Y) = AMP R (u, v) the sky-plane position of the
 * position mode (flags = 0) at t_n:
 *   rho_m   = sqrt(X^2 + Y^2)
 *   delta   = atan2(Y c_n - X s_n,  X c_n + Y s_n)          (c_n, s_n) = (cos, sin) theta_n
 *           = atan2(sin(theta_m - theta_n), cos(theta_m - theta_n)),  theta_m = atan2(Y, X), in (-pi, pi]: theta_m is never
 *             formed, the data's cos / sin are formed once by the caller, and theta_n may be given in any 2 pi convention
 *   s2r = var_rho[n_var_rho == 1 ? 0 : n] + jit2_rho[d]        wr = 1 / s2r     r = rho_n - rho_m     kappa  = wr r
 *   s2t = var_theta[n_var_theta == 1 ? 0 : n] + jit2_theta[d]  wt = 1 / s2t                           lambda = -wt delta
 *   loglike[d]     = -1/2 sum_n (wr r^2 + log s2r + wt delta^2 + log s2t) - n_cad log(2 pi)
 *   gparams[d]     = d loglike / d rec[d]      (EXO_OV_NPAR doubles: the reverse pass of the position with the cotangents
 *                    d loglike / d (X, Y, Z) = (kappa X / rho_m - lambda Y / rho_m^2, kappa Y / rho_m + lambda X / rho_m^2, 0))
 *   gjit2_rho[d]   = 1/2 sum_n (kappa^2 - wr)
 *   gjit2_theta[d] = 1/2 sum_n (lambda^2 - wt)
 * t, rho, cos_theta, sin_theta [n_cad]; var_rho [n_var_rho], var_theta [n_var_theta], each count 1 or n_cad.  params
 * [n_draw][EXO_OV_NPAR]: one companion per call (AMP = -a, times parallax au_per_R_sun for arcseconds; COSO = 1, SINO = 0
 * without an Omega; ECC = 0, COSW = 1, SINW = 0 when circular).  jit2_rho, jit2_theta [n_draw]; either may be null (zero).
 * loglike [n_draw]; gparams [n_draw][EXO_OV_NPAR], gjit2_rho, gjit2_theta [n_draw]: a null gradient output is not written,
 * and without gparams the reverse arithmetic is skipped.  ECC outside [0, 1) gives NaN in that draw only; so does a model
 * separation of exactly 0 (no direction).  No workspace: one workgroup per draw, whose width depends on n_cad alone, every sum
 * in a fixed order (bit-reproducible, and a draw's results do not depend on the batch it is in).  Sizes are checked first,
 * then the required pointers, before any launch; n_draw == 0: EXO_OK, nothing launched.  n_cad == 0 with n_draw > 0 (n_var_*
 * = 1; the series' pointers are not read and may be null): the sums are empty -- loglike = 0 and every gradient output that is
 * passed is written as 0.  A gradient output of a jitter may be passed where that jit2 is null: it is the derivative at zero.
 * ------------------------------------------------------------------------- */
int exo_astrometry_loglike_vjp_f64(const double* t, const double* rho, const double* cos_theta, const double* sin_theta,
                                   const double* var_rho, int64_t n_var_rho, const double* var_theta, int64_t n_var_theta,
                                   int64_t n_cad, const double* params, int64_t n_draw, const double* jit2_rho,
                                   const double* jit2_theta, double* loglike, double* gparams, double* gjit2_rho,
                                   double* gjit2_theta, void* stream);

/* ---------------------------------------------------------------------------
 * celerite GP log-likelihood, value + VJP, for n_draw independent (kernel,
 * residual) pairs.  Replaces what celerite2 (a dependency of the reference,
 * /root/reference/setup.py:36; the user's model calls it, the reference tree
 * itself has no call site) does behind
 *     gp = GaussianProcess(kernel, t=t, diag=diag);  gp.log_likelihood(y - model)
 * i.e. celerite2's `factor` + `solve_lower` + `norm` Ops and their reverse Ops.
 *
 *   t            [n]               sorted, shared by all draws
 *   resid        [n_draw][n]       y - mean model, per draw
 *   diag         [n_diag][n]       white-noise variance (yerr^2 + jitter); n_diag = 1 (shared) or n_draw
 *   coef_real    [n_draw][n_real][2]     (a, c)        of celerite2 Term.get_coefficients()
 *   coef_complex [n_draw][n_complex][4]  (a, b, c, d)  -- a "pair slot": two state indices
 *   pair_kind    NULL, or [n_draw][n_complex] int32: 0 = the slot is a complex term (a, b, c, d);
 *                1 = the slot holds TWO REAL terms (a1, c1, a2, c2).  An SHO term is one complex
 *                term for Q >= 1/2 and two real ones for Q < 1/2 (celerite2 terms.SHOTerm): with
 *                the kind per draw a batch of draws may straddle Q = 1/2 with a static state width
 *   J = n_real + 2 n_complex <= EXO_GP_MAX_J
 *   loglike      [n_draw]          out; -inf if the matrix is not positive definite
 *   state        NULL (value only, sequential recurrences) or exo_celerite_state_doubles() doubles,
 *                16-byte aligned: what the reverse pass re-reads.  Opaque to the caller: whatever
 *                wrote it (this library, this ABI version, the same n_chunks) must read it back
 *   n_chunks     how the series is cut for the time-parallel recurrences: 0 = the library's plan,
 *                1 = sequential recurrences, > 1 = that many chunks (tuning / tests).  The three
 *                calls of a pair -- exo_celerite_state_doubles, forward, reverse -- must be given
 *                the same value (and n, n_draw, n_real, n_complex): the plan is a pure function of
 *                them, the library keeps NO state between calls (EXO_ERR_WORKSPACE if state_doubles
 *                is smaller than exo_celerite_state_doubles() of the same arguments).
 *                EXO_GP_PREPARE_ADJOINT may be or-ed into it (ABI 14), again in every call of the pair: the FORWARD call then
 *                also runs everything of the reverse pass that does not need the cotangent -- the adjoint elements of the
 *                chunks and the scan over them, a dozen or two short, latency-bound launches -- for a cotangent of one, on a
 *                stream of the library's own BESIDE the forward chunk kernel (forked from and joined back into `stream` by
 *                events, so it is legal inside a stream capture and a replayed graph keeps the fork), and the REVERSE call
 *                starts at its chunk kernel, scaling by the actual cotangent (the adjoint is linear in it; a cotangent of
 *                exactly 1 gives the bits of the unflagged pair).  For callers that know the reverse call will follow (a
 *                sampler's value-and-gradient step) -- and that have MEASURED it: the scan's kernels are bound by memory
 *                latency, and beside a chunk kernel that saturates HBM with its checkpoint stores they slow down by about
 *                what the overlap hides (C5 -2 %, J = 10 -3 %; C3 +2.5 %): the Python host side leaves
 *                it off.  A forward call with the flag and no reverse call after it has only done work nobody reads.
 *
 * With a state buffer and n >= 64 the recurrences run in parallel over TIME (docs/DESIGN_r1_r4.md 3.5): the
 * series is cut into chunks, chunk "filtering elements" and a short per-draw scan over them give
 * the recurrence state entering every chunk (and, in the reverse pass, its adjoint), and the
 * ordinary recurrences then run inside all chunks at once.  J <= 6: one lane per (draw, chunk) and
 * a CHECKPOINTED factorisation -- the forward pass stores the recurrence state every 4 cadences (J <= 2) or every 2
 * (J = 3 .. 6), the reverse pass recomputes the cadences in between (which is why it takes the series again);
 * J > 6: a draw on 8 (J = 7, 8) or 16 lanes, (d, z, W, F) of every cadence saved and the S rows at every 2nd to 4th.
 * Same results as the
 * sequential recurrences (1e-14 relative in loglike); draws whose terms do not admit the filter
 * form (a <= 0 or |b d| > a c for some term) or are ill-conditioned are redone by the sequential
 * kernels on the device.
 * ------------------------------------------------------------------------- */
#define EXO_GP_PREPARE_ADJOINT 0x40000000   /* or-ed into n_chunks: see above */
#define EXO_GP_MAX_J 16   /* every state width takes the time-parallel path (1 .. 6: one lane per (draw, chunk); 7, 8: a draw on 8 lanes; 9 .. 16,
                             round 6: on a DPP row of 16 lanes, the scans on 256-thread blocks); the sequential recurrences are the
                             fallback for flagged draws and for series too short to cut */
int64_t exo_celerite_state_doubles(int64_t n, int64_t n_draw, int32_t n_real, int32_t n_complex,
                                   int32_t n_chunks);
/* the number of chunks the default plan (n_chunks = 0) cuts the series into, for callers that pass it explicitly; sparse != 0:
 * what the sparse entries (exo_celerite_loglike_sparse_*_f64) do best with -- twice as many for J <= 2 (their waves are uneven: two
 * rounds of them balance).  1 = sequential recurrences.                                                               */
int32_t exo_celerite_default_chunks(int64_t n, int64_t n_draw, int32_t n_real, int32_t n_complex, int32_t sparse);
int exo_celerite_loglike_fwd_f64(const double* t, const double* resid, const double* diag, int64_t n_diag,
                                 int64_t n, const double* coef_real, int32_t n_real,
                                 const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                 int64_t n_draw, double* loglike, double* state, int64_t state_doubles,
                                 int32_t n_chunks, void* stream);
/* Reverse: given gloglike [n_draw], the series again and the saved state, write
 *   gresid [n_draw][n], gdiag [n_draw][n] (nullable), gdiag_sum [n_draw] (nullable,
 *   = sum_n d loglike / d diag_n, the cotangent of a scalar jitter),
 *   gcoef_real [n_draw][n_real][2], gcoef_complex [n_draw][n_complex][4] (a pair slot of kind 1
 *   receives the cotangents of (a1, c1, a2, c2)).                                  */
int exo_celerite_loglike_vjp_f64(const double* t, const double* resid, const double* diag, int64_t n_diag,
                                 int64_t n, const double* coef_real, int32_t n_real,
                                 const double* coef_complex, int32_t n_complex, const int32_t* pair_kind,
                                 int64_t n_draw, const double* gloglike, const double* state,
                                 int64_t state_doubles, int32_t n_chunks, double* gresid, double* gdiag,
                                 double* gdiag_sum, double* gcoef_real, double* gcoef_complex, void* stream);

/* The same pair for the usual case of one observed series against a per-draw model:
 *   resid[d][n] = obs[n] - model[d][n]
 * is formed inside the kernels (obs [n], model [n_draw][n]), and the reverse entry returns
 * gmodel = d loglike / d model = -(d loglike / d resid): neither the residual nor the sign
 * flip of its cotangent exists as an array.  Everything else as above; a state buffer
 * written by one pair must be read back by the same pair.                                */
int exo_celerite_loglike_obs_fwd_f64(const double* t, const double* obs, const double* model,
                                     const double* diag, int64_t n_diag, int64_t n,
                                     const double* coef_real, int32_t n_real,
                                     const double* coef_complex, int32_t n_complex,
                                     const int32_t* pair_kind, int64_t n_draw, double* loglike,
                                     double* state, int64_t state_doubles, int32_t n_chunks, void* stream);
int exo_celerite_loglike_obs_vjp_f64(const double* t, const double* obs, const double* model,
                                     const double* diag, int64_t n_diag, int64_t n,
                                     const double* coef_real, int32_t n_real,
                                     const double* coef_complex, int32_t n_complex,
                                     const int32_t* pair_kind, int64_t n_draw, const double* gloglike,
                                     const double* state, int64_t state_doubles, int32_t n_chunks,
                                     double* gmodel, double* gdiag, double* gdiag_sum, double* gcoef_real,
                                     double* gcoef_complex, void* stream);

/* The obs pair with the model (and, from the reverse entry, its cotangent) CADENCE-MAJOR:
 *   model_cm [n][n_draw], gmodel_cm [n][n_draw]
 * -- the layout the light-curve sweep writes under EXO_FLAG_CADENCE_MAJOR.  A lane of the kernels is a
 * draw: with the draws innermost every access of a wave to the series is 512 contiguous bytes instead of 64
 * pieces of 64 rows (C3, 1024 draws x 150 000 cadences: forward chunk kernel 0.86 -> 0.64 ms, reverse
 * 2.02 -> 1.54 ms).  diag / gdiag stay [n_diag][n] / [n_draw][n].  Same arithmetic, same results.     */
int exo_celerite_loglike_obs_fwd_cm_f64(const double* t, const double* obs, const double* model_cm,
                                        const double* diag, int64_t n_diag, int64_t n,
                                        const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex,
                                        const int32_t* pair_kind, int64_t n_draw, double* loglike,
                                        double* state, int64_t state_doubles, int32_t n_chunks, void* stream);
int exo_celerite_loglike_obs_vjp_cm_f64(const double* t, const double* obs, const double* model_cm,
                                        const double* diag, int64_t n_diag, int64_t n,
                                        const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex,
                                        const int32_t* pair_kind, int64_t n_draw, const double* gloglike,
                                        const double* state, int64_t state_doubles, int32_t n_chunks,
                                        double* gmodel_cm, double* gdiag, double* gdiag_sum, double* gcoef_real,
                                        double* gcoef_complex, void* stream);

/* The obs pair with the model SPARSE (round 5): a transit light curve is zero at ~97 % of the cadences, and as the mean of
 * a GP (limb_dark.py:99-232 feeding celerite2's log_likelihood) it used to cross HBM as a dense (draw, cadence) array five
 * times per value + gradient -- written, scattered, read by three kernels -- and its cotangent, of which the light curve's
 * reverse pass reads the same 3 %, twice more.  Here the model is what the EXO_FLAG_SPARSE sweep produces: per draw a few
 * SEGMENTS of cadences, ascending and disjoint, and the values of exactly those cadences:
 *   segment k of draw d   cadences [lo, hi),  lo = seg[d * seg_row + k * seg_step],  hi = seg[d * seg_row + k * seg_step + hi_at],
 *                         k < nseg[d]
 *   model[d][n]           vals[d * val_row + off[d * off_row + k] + (n - lo)]  for lo <= n < hi,  0 outside every segment
 * and the reverse entry writes gvals = d loglike / d vals at the same positions (nothing elsewhere: positions of `gvals` that
 * no segment covers are left as they were).  exo_transit_flux_sparse_model() fills the descriptor from a sweep's workspace.
 * n < 2^31.  Same arithmetic as the dense entries on the same model: same log-likelihood, bit for bit.                 */
int exo_celerite_loglike_sparse_fwd_f64(const double* t, const double* obs, const exo_sparse_model* model,
                                        const double* diag, int64_t n_diag, int64_t n,
                                        const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex,
                                        const int32_t* pair_kind, int64_t n_draw, double* loglike,
                                        double* state, int64_t state_doubles, int32_t n_chunks, void* stream);
int exo_celerite_loglike_sparse_vjp_f64(const double* t, const double* obs, const exo_sparse_model* model,
                                        const double* diag, int64_t n_diag, int64_t n,
                                        const double* coef_real, int32_t n_real,
                                        const double* coef_complex, int32_t n_complex,
                                        const int32_t* pair_kind, int64_t n_draw, const double* gloglike,
                                        const double* state, int64_t state_doubles, int32_t n_chunks,
                                        double* gvals, double* gdiag, double* gdiag_sum, double* gcoef_real,
                                        double* gcoef_complex, void* stream);

/* ---------------------------------------------------------------------------
 * O(N) companions of the likelihood (celerite2's GaussianProcess.dot_tril and the kernel product of
 * GaussianProcess.predict; the reference's docs pair it with celerite2: docs/index.rst:14,48-49):
 *   dot_tril: z[d] = L x[d] with K + diag = L L^T (prior samples: x ~ N(0, I));  NaN from the first
 *             cadence at which the matrix is not positive definite
 *   predict:  mu[d][m] = sum_n k(|tq[m] - t[n]|) alpha[d][n], t and tq sorted, in O(N + M) by one
 *             forward and one backward sweep -- the conditional mean at new times is this with
 *             alpha = (K + diag)^-1 (y - mean) = -d loglike / d resid
 * Sequential in time, one lane per draw: utilities, not part of the per-step path.  Coefficients,
 * pair kinds and diag as for exo_celerite_loglike_fwd_f64.
 * ------------------------------------------------------------------------- */
int exo_celerite_dot_tril_f64(const double* t, const double* diag, int64_t n_diag, int64_t n,
                              const double* coef_real, int32_t n_real, const double* coef_complex,
                              int32_t n_complex, const int32_t* pair_kind, int64_t n_draw, const double* x,
                              double* z, void* stream);
int exo_celerite_predict_f64(const double* t, int64_t n, const double* alpha, const double* coef_real,
                             int32_t n_real, const double* coef_complex, int32_t n_complex,
                             const int32_t* pair_kind, int64_t n_draw, const double* tq, int64_t m,
                             double* mu, void* stream);

/* ---------------------------------------------------------------------------
 * Predictive variance (ABI 15; celerite2's GaussianProcess.predict(return_var=True), optionally of a
 * component of the kernel):
 *   var[d][q] = k2(0) - k2(tq[q], t) (K + diag)^-1 k2(t, tq[q])
 * k2: the kernel restricted to the terms whose slot_mask entry is nonzero -- slot_mask (int32) holds one
 * entry per real slot, then one per pair slot (a pair slot of kind 1 holds two real terms, selected
 * together); NULL: every term, k2 = k.  K + diag always uses every term.  The latent process: no
 * white noise at the query times.  t [n] and tq [m] sorted; var [n_draw][m].  Coefficients, pair
 * kinds and diag as for exo_celerite_loglike_fwd_f64 (n >= 1).
 * One lane per draw, O((n + m) J^2), sequential in time.  With A = K + diag = L diag(d) L^T, S_i the
 * state entering cadence i and E(tau) = diag(exp(-c tau)):
 *   forward:   d_i = diag_i + sum a - U_i^T S_i U_i,  W_i = (V_i - S_i U_i) / d_i,
 *              S+_i = S_i + d_i W_i W_i^T,  S_(i+1) = E(t_(i+1) - t_i) S+_i E(t_(i+1) - t_i)
 *   backward:  B_n = 0,  X = E(t_(i+1) - t_i) B_(i+1) E(t_(i+1) - t_i)  (0 at the last cadence),
 *              B_i = U_i U_i^T / d_i + (I - W_i U_i^T)^T X (I - W_i U_i^T)
 *   query t* after the last cadence k with t_k <= t* (k = -1: none), U*, V* of the predicted terms only:
 *              S* = E(t* - t_k) S+_k E(t* - t_k) (0 for k = -1),  r* = V* - S* U*,
 *              B* = E(t_(k+1) - t*) B_(k+1) E(t_(k+1) - t*) (0 for k = n - 1),
 *              var = k2(0) - U*^T S* U* - r*^T B* r*
 * work: device scratch of exo_celerite_predict_var_work_doubles(n, m, n_real, n_complex, n_draw) =
 * (n + m) (J + 1) n_draw doubles (J = n_real + 2 n_complex), laid out [row][quantity][draw]; its content
 * before the call does not matter (EXO_ERR_WORKSPACE: too small).  A draw whose factorisation meets
 * d <= 0 (the matrix is not positive definite) gets NaN at every query time, as dot_tril does.
 * ------------------------------------------------------------------------- */
int64_t exo_celerite_predict_var_work_doubles(int64_t n, int64_t m, int32_t n_real, int32_t n_complex, int64_t n_draw);
int exo_celerite_predict_var_f64(const double* t, const double* diag, int64_t n_diag, int64_t n,
                                 const double* coef_real, int32_t n_real, const double* coef_complex,
                                 int32_t n_complex, const int32_t* pair_kind, const int32_t* slot_mask,
                                 int64_t n_draw, const double* tq, int64_t m, double* var, double* work,
                                 int64_t work_doubles, void* stream);

/* ---------------------------------------------------------------------------
 * The solve (ABI 20; celerite2's GaussianProcess.apply_inverse):  alpha[d] = (K + diag)^-1 y[d]  by the
 * published recurrences -- the factorisation with the lower sweep beside it, z / d, the upper sweep --
 * one lane per draw, sequential in time, O(n J^2).  Its backward error max |A alpha - y| / max |y| is
 * that of the sequential algorithm, which the reverse pass of the likelihood (the same vector as minus
 * the gradient with respect to y) does not reach on every input.  t [n] sorted; y, alpha [n_draw][n],
 * not the same array.  Coefficients, pair kinds and diag as for exo_celerite_loglike_fwd_f64 (n >= 1).
 * work: device scratch of exo_celerite_solve_work_doubles(n, n_real, n_complex, n_draw) = n J n_draw
 * doubles, laid out [cadence][j][draw]; its content before the call does not matter (EXO_ERR_WORKSPACE:
 * too small).  A draw whose factorisation meets d <= 0 gets NaN everywhere.
 * ------------------------------------------------------------------------- */
int64_t exo_celerite_solve_work_doubles(int64_t n, int32_t n_real, int32_t n_complex, int64_t n_draw);
int exo_celerite_solve_f64(const double* t, const double* diag, int64_t n_diag, int64_t n, const double* coef_real,
                           int32_t n_real, const double* coef_complex, int32_t n_complex,
                           const int32_t* pair_kind, int64_t n_draw, const double* y, double* alpha,
                           double* work, int64_t work_doubles, void* stream);

/* ---------------------------------------------------------------------------
 * Record packing: the O(planets) algebra of KeplerianOrbit.__init__
 * (src/exoplanet/orbits/keplerian.py:133-281,849-934), get_cl
 * (src/exoplanet/light_curves/limb_dark.py:11-18), the in-transit windows
 * (keplerian.py:733-763) and the secondary flux ratio
 * (src/exoplanet/light_curves/secondary_eclipse.py:67-68) for the standard
 * transit parameterisation, as one kernel + one reverse kernel (in the
 * reference, and in torch, this is ~170 launch-bound elementwise nodes).
 *
 *   orbit_in  [n_draw][n_planet][EXO_NIN]   see EXO_IN_* (R_sun, M_sun, days)
 *   ld_in     [n_draw][2] = (u1, u2), or [n_draw][4] with EXO_FLAG_SECONDARY
 *   flags     EXO_PACK_CIRCULAR (ecc=None: e = 0, omega unused, keplerian.py:182-185),
 *             EXO_FLAG_WINDOW (fill TS/TE[, TS2/TE2]; else +-inf), EXO_FLAG_SECONDARY
 *   params    out [n_draw][n_planet][EXO_NPAR];  ld out [n_draw][3|6]
 * ------------------------------------------------------------------------- */
#define EXO_NIN 10
#define EXO_IN_PERIOD 0
#define EXO_IN_T0 1
#define EXO_IN_B 2
#define EXO_IN_ECC 3
#define EXO_IN_OMEGA 4
#define EXO_IN_R 5
#define EXO_IN_MSTAR 6
#define EXO_IN_RSTAR 7
#define EXO_IN_MPLANET 8
#define EXO_IN_SBR 9
#define EXO_PACK_CIRCULAR 8u
int exo_pack_records_f64(const double* orbit_in, const double* ld_in, int64_t n_draw, int32_t n_planet,
                         uint32_t flags, double* params, double* ld, void* stream);
/* Reverse: cotangents of params / ld -> cotangents of orbit_in / ld_in (window and
 * T0 / PERIOD slots carry no gradient: they only select cadences).              */
int exo_pack_records_vjp_f64(const double* orbit_in, const double* ld_in, int64_t n_draw,
                             int32_t n_planet, uint32_t flags, const double* gparams,
                             const double* gld, double* gorbit_in, double* gld_in, void* stream);
/* Column form of the two calls above, for callers whose parameters are separate arrays (one tensor per
 * constructor argument of KeplerianOrbit): no packing pass in front, no unpacking pass behind.
 *   cols, draw_stride, planet_stride, defaults   HOST arrays of EXO_NIN entries: input k of (draw, planet) is
 *       cols[k][draw * draw_stride[k] + planet * planet_stride[k]]  (device memory; stride 0 = broadcast), or
 *       defaults[k] where cols[k] is NULL (the reference's constructor defaults: m_star = r_star = 1, m_planet = 0)
 *   ld_cols, ld_draw_stride   HOST arrays of 2 (u1, u2) or, with EXO_FLAG_SECONDARY, 4 device pointers / strides
 * Reverse: gscale (optional, [n_draw]) multiplies the record cotangents as they are read -- the chain rule through
 * a per-draw scalar such as L[d] = sum_n gbar[d][n] flux[d][n] without a pass of its own; gcols[k] / gld_cols[k]
 * (HOST arrays; NULL entry = not wanted) receive the cotangents DENSELY, [n_draw][n_planet] / [n_draw] doubles each:
 * the caller sums over whatever it broadcast.                                                                  */
int exo_pack_records_cols_f64(const double* const* cols, const int64_t* draw_stride, const int64_t* planet_stride,
                              const double* defaults, const double* const* ld_cols, const int64_t* ld_draw_stride,
                              int64_t n_draw, int32_t n_planet, uint32_t flags, double* params, double* ld,
                              void* stream);
int exo_pack_records_cols_vjp_f64(const double* const* cols, const int64_t* draw_stride, const int64_t* planet_stride,
                                  const double* defaults, const double* const* ld_cols, const int64_t* ld_draw_stride,
                                  int64_t n_draw, int32_t n_planet, uint32_t flags, const double* gparams,
                                  const double* gld, const double* gscale, double* const* gcols,
                                  double* const* gld_cols, void* stream);

/* The No-U-Turn sampler's tree building for a batch of chains (exoplanet_amd/sampling.py: NUTS; the reference hands
 * its models to PyMC's NUTS, docs/tutorials/data-and-models.md:289) on (chains, parameters) arrays that stay on the
 * device.  A transition grows every chain's trajectory by doublings; per doubling
 *   phase 2: every chain draws its direction, the sub-tree starts at that end of its trajectory;
 *   per leaf, phase 0: half kick and drift of the sub-tree's moving end into the scratch rows qn, ph (the caller then
 *            evaluates log-density and gradient at qn into lpn, gn), phase 1: second half kick, energy error,
 *            divergence, multinomial candidate, momentum sums, checkpoint write / generalised turning checks, which
 *            chains go on (the leaf index is kept on the device: a captured leaf needs nothing from the host);
 *   phase 3: a valid sub-tree joins the trajectory (proposal, new end, sums, weights, the trajectory's turning check).
 * ptrs: HOST array of 40 device pointers -- sub-tree: qe, pe, ge [D][n]; eps [D]; on [D] (bytes); H0, logw [D]; psum,
 * sq, sg [D][n]; slp [D]; turn, div [D] (bytes); acc, accn [D]; ckp, cks [n_slot][D][n]; then mass, qn, ph, gn [D][n];
 * lpn [D]; trajectory: ql, pl, gl, qr, pr, gr, tsum [D][n]; logW [D]; propq, propg [D][n]; proplp [D]; active,
 * diverged, going [D] (bytes); depth [D]; eps_abs [D]; R [2 + leaves][D] (uniform random numbers of the doubling: row 0
 * directions, row 1 the merge, row 2 + k leaf k); leaf (int32 [1]).                                               */
int exo_nuts_f64(const void* const* ptrs, int64_t n_chain, int32_t n_param, int32_t n_slot, double max_energy_error,
                 int32_t phase, void* stream);

/* Batched L-BFGS with a backtracking Armijo line search (exoplanet_amd/optimize.py: LBFGS -- the reference climbs to the
 * posterior mode with pmx.optimize before it samples, docs/tutorials/data-and-models.md:287-296) on (chains, parameters)
 * arrays that stay on the device: every chain minimises f = -logp on its own, all in lockstep.  The caller evaluates logp
 * and its gradient at the trial points xt into lpt, gt; then
 *   phase 0 (after the evaluation at the starting points, xt == x): status 4 for a chain whose value or gradient is not
 *            finite, 1 for one that is converged already, else the first direction -g, the first step, the first trial point;
 *   phase 1 (after every later evaluation): accept (history pair, or no history at all if s.y <= eps y.y; move; stop with status 1
 *            when max |g_i| <= gtol or 2 when f_prev - f <= ftol max(|f_prev|, |f|, 1) for n_hist accepted steps in a
 *            row; else the two-loop direction, its first scaling per column, and the next trial point) or reject (half the step; after max_linesearch in a row drop the history and restart
 *            along -g, or stop if there was none: status 3, or 2 right after a small decrease).  A chain with a status other than 0 is left as it is.
 * The rules in full: DESIGN.md section 15.  ptrs: HOST array of 22 device pointers -- x, g, xt, gt, d, free [D][n] (gt:
 * in, the gradient of logp at xt; out, -gt * free; free: 0 / 1, a column with 0 never moves); hs, hy [n_hist][n][D] and
 * hsy, coef [n_hist][D] (the kernels' own: pairs, s.y, workspace); logp, lpt, alpha, gamma, grad_max [D]; status,
 * n_iter, n_eval, m, head, n_rej, n_small (int32 [D]).  Phase 0 initialises everything but x, xt, gt, lpt, free and the
 * history's content.  EXO_ERR_INVALID_ARGUMENT: a null table or entry, n_chain < 0, n_param < 1, n_hist outside
 * 1 .. EXO_LBFGS_MAX_HISTORY, max_linesearch < 1, a phase other than 0 or 1.  n_chain == 0: EXO_OK, nothing launched
 * (sizes are checked first).  One launch, nothing else enqueued.  (Added without a new ABI number: no caller breaks.)  */
#define EXO_LBFGS_MAX_HISTORY 32
int exo_lbfgs_f64(const void* const* ptrs, int64_t n_chain, int32_t n_param, int32_t n_hist, int32_t max_linesearch, double c1,
                  double gtol, double ftol, int32_t phase, void* stream);

/* Timing tables of a TTVOrbit whose transits are all labelled and given as offsets `ttvs` from the linear ephemeris
 * (orbits/ttv.py:99-170): transit k of planet p of a draw at tt_k = t0 + period k + ttv_k, k < n_transit[p];
 *   edges [n_draw][n_planet][n_edge]      tt_0 - period/2, midpoints of neighbours, tt_last + period/2, then +inf
 *                                         (ttv.py:158-166); n_edge = max_p n_transit[p] + 1
 *   shift [n_draw][n_planet][n_edge + 1]  bin j -> transit max(0, min(j - 1, n - 1)) (ttv.py:167-170): period k + ttv_k
 * -- the tables the exo_transit_*_ttv_* entry points take.  period, t0: device arrays read at
 * [draw * draw_stride + planet * planet_stride] (strides in elements, 0 = broadcast); ttv, ttv_draw_stride, n_transit:
 * HOST arrays [n_planet] of device pointers (row of a draw: n_transit[p] contiguous doubles), draw strides, counts.
 * Reverse: gshift -> gttv[p] [n_draw][n_transit[p]] and gperiod [n_draw][n_planet], dense, either may be NULL (per
 * planet for gttv); the edges carry no gradient (searchsorted, ttv.py:174) and t0 none through the tables.       */
int exo_ttv_tables_f64(const double* period, int64_t period_draw_stride, int64_t period_planet_stride, const double* t0,
                       int64_t t0_draw_stride, int64_t t0_planet_stride, const double* const* ttv,
                       const int64_t* ttv_draw_stride, const int32_t* n_transit, int64_t n_draw, int32_t n_planet,
                       int32_t n_edge, double* edges, double* shift, void* stream);
int exo_ttv_tables_vjp_f64(const double* period, int64_t period_draw_stride, int64_t period_planet_stride, const double* t0,
                           int64_t t0_draw_stride, int64_t t0_planet_stride, const double* const* ttv,
                           const int64_t* ttv_draw_stride, const int32_t* n_transit, int64_t n_draw, int32_t n_planet,
                           int32_t n_edge, const double* gshift, double* const* gttv, double* gperiod, void* stream);

/* ---------------------------------------------------------------------------
 * celerite2's SHOTerm -> the pair slot of the GP entry points above (one slot per term and draw, two state indices):
 * the term's parameters in any of celerite2's parameterisations -- amplitude S0 or (EXO_SHO_SIGMA) sigma, frequency w0
 * or (EXO_SHO_RHO) the undamped period rho, damping Q or (EXO_SHO_TAU) tau -- to coef[n][4] and kind[n]:
 *   Q >= 1/2: kind 0, one complex term (a, b, c, d) = (S0 w0 Q, a / f, w0 / 2Q, c f),  f = sqrt(max(4 Q^2 - 1, eps))
 *   Q <  1/2: kind 1, two real terms (a1, c1, a2, c2) = (a (1 + 1/f) / 2, c (1 - f), a (1 - 1/f) / 2, c (1 + f)),
 *             f = sqrt(max(1 - 4 Q^2, eps))
 * decided per element on the device (a batch may straddle Q = 1/2).  One launch, and one for the reverse
 * (gcoef[n][4] -> gamp, gfreq, gdamp[n]); in the reference this algebra is celerite2's Python, in torch ~35 kernels.
 * ------------------------------------------------------------------------- */
#define EXO_SHO_SIGMA 1u
#define EXO_SHO_RHO 2u
#define EXO_SHO_TAU 4u
int exo_sho_coefficients_f64(const double* amp, const double* freq, const double* damp, uint32_t flags, double eps,
                             int64_t n, double* coef, int32_t* kind, void* stream);
int exo_sho_coefficients_vjp_f64(const double* amp, const double* freq, const double* damp, uint32_t flags, double eps,
                                 int64_t n, const double* gcoef, double* gamp, double* gfreq, double* gdamp,
                                 void* stream);

/* A dense flux array KEPT ACROSS STEPS (the dense light curve a sampler asks LimbDarkLightCurve.get_light_curve for at every step:
 * src/exoplanet/light_curves/limb_dark.py:163-170, 228-230).  `workspace` holds the sparse output of an EXO_FLAG_SPARSE sweep (same n_cad, n_draw,
 * n_planet; flags: EXO_FLAG_SECONDARY as in that sweep, nothing else).  clear == 0: the summed flux of the cadences in its runs
 * is written into flux[n_draw][n_cad] (planets in order: the bits of the dense sweep), every other entry left alone;
 * clear != 0: those entries are zeroed.  A caller that keeps `flux` and `workspace` from step to step -- zero-initialised
 * both before the first -- calls: scatter(clear) -> sparse sweep -> scatter(write), and holds, after every step, the dense
 * array the dense sweep would have produced, for the price of the sparse one (no fill of every cadence: 1.2 GB at the
 * headline shape).  The library keeps no state: the promise that `flux` is zero outside the runs of `workspace` is the
 * caller's. */
int exo_transit_sparse_scatter_f64(const void* workspace, int64_t workspace_bytes, int64_t n_cad, int64_t n_draw, int32_t n_planet,
                                   uint32_t flags, int32_t clear, double* flux, void* stream);

/* A SUM of SHO terms (celerite2's terms.TermSum, term_1 + term_2 + ...; celerite2 is a dependency of the reference,
 * /root/reference/setup.py:36, its terms are what the reference's GP models are built from), all of it in one launch each way: term k reads its own
 * amp[k], freq[k], damp[k] (host arrays of n_terms <= EXO_SHO_MAX_TERMS device pointers to n doubles each) under its own
 * flags[k], and owns slot k of coef[n][n_terms][4] and kind[n][n_terms] -- the pair-slot arrays the celerite entry points
 * take (no concatenation; the reverse reads gcoef[n][n_terms][4] in place and writes every term's gamp / gfreq / gdamp[n]). */
#define EXO_SHO_MAX_TERMS 8
int exo_sho_coefficients_multi_f64(const double* const* amp, const double* const* freq, const double* const* damp,
                                   const uint32_t* flags, int32_t n_terms, double eps, int64_t n, double* coef, int32_t* kind,
                                   void* stream);
int exo_sho_coefficients_multi_vjp_f64(const double* const* amp, const double* const* freq, const double* const* damp,
                                       const uint32_t* flags, int32_t n_terms, double eps, int64_t n, const double* gcoef,
                                       double* const* gamp, double* const* gfreq, double* const* gdamp, void* stream);

/* ---------------------------------------------------------------------------
 * Period search (exoplanet_amd/estimators.py; definitions: DESIGN.md section 9).  n_series series y[n_series][n] on one time
 * axis t[n] (any order); yerr: n_yerr = 0 (none, unit weights), 1 (one row for every series) or n_series rows.  Kernels
 * on the caller's stream only; `workspace` (device, 8-byte aligned) carries everything between them.
 *
 * Box least squares, the binned method: bins of width delta = min(durations) / oversample over the folded time, boxes of
 * duration_bins[k] bins (HOST array, n_duration <= EXO_BLS_MAX_DURATIONS entries >= 1, round(duration / delta) taken by the
 * caller), every start.  periods[n_period] on the device; min_bins and max_bins bound ceil(p / delta) + oversample over them
 * (computed by the caller with the same fp64 division): a period's histogram lives in LDS up to 3835 bins and in a slab of
 * the workspace above that.  out[7][n_series][n_period]: power, depth, depth_err, depth_snr, log_likelihood, duration,
 * transit_time at the first maximiser of the objective; no admissible box: -inf, then NaN.  The bin sums are fp64 atomic
 * adds: their last bits may differ from run to run.
 *
 * Lomb-Scargle: the exact floating-mean periodogram, "psd" normalisation, power[n_series][n_frequency] =
 * (chi2_0 - chi2(f)) / 2.  Its workspace: exo_bls_workspace_bytes(n, n_series, 0, 0).
 * ------------------------------------------------------------------------- */
#define EXO_BLS_MAX_DURATIONS 16
#define EXO_BLS_LIKELIHOOD 0
#define EXO_BLS_SNR 1
int64_t exo_bls_workspace_bytes(int64_t n, int64_t n_series, int64_t n_period, int64_t max_bins);
int exo_bls_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                      const double* periods, int64_t n_period, int64_t min_bins, int64_t max_bins, const int32_t* duration_bins,
                      int32_t n_duration, double delta, int32_t oversample, int32_t objective, double* out, void* workspace,
                      int64_t workspace_bytes, void* stream);
int exo_lomb_scargle_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                               const double* frequencies, int64_t n_frequency, double* power, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* Transit least squares on the same bins (definition: DESIGN.md section 18): the box of duration k is replaced by a template
 * g_k[0 .. duration_bins[k] - 1], and the level c and the depth of the model "c - depth g_k inside the window, c outside" are
 * fitted jointly by weighted least squares; log_likelihood is half the drop in chi-squared against a constant, exactly.
 * The arguments of exo_bls_power_f64, the same out[7][n_series][n_period] and the same workspace
 * (exo_bls_workspace_bytes), plus templates: ONE flat table on the device, finite values (the caller's promise), and
 * template_offsets: HOST array of n_duration + 1 entries, template k at templates[template_offsets[k] ..
 * template_offsets[k + 1] - 1].  EXO_ERR_INVALID_ARGUMENT, before any launch: what exo_bls_power_f64 rejects, a null table or
 * null offsets, template_offsets[0] < 0, template_offsets[k + 1] - template_offsets[k] != duration_bins[k], a table that
 * ends beyond EXO_TLS_MAX_TEMPLATE entries (64 KiB).  With every template entry 1 the depth, its error and its signal to
 * noise are the box search's.  (Added without a new ABI number: no caller breaks.) */
#define EXO_TLS_MAX_TEMPLATE 8192
int exo_tls_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                      const double* periods, int64_t n_period, int64_t min_bins, int64_t max_bins, const int32_t* duration_bins,
                      int32_t n_duration, double delta, int32_t oversample, int32_t objective, const double* templates,
                      const int32_t* template_offsets, double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Detrending before the search (exoplanet_amd/estimators.py: location_plan, running_location, flatten, sde; definition:
 * DESIGN.md section 19): the running median, median absolute deviation and Tukey biweight location of n_series series
 * y[n_series][n] over time windows on one axis t[n], finite and non-decreasing (the caller's promise).  Kernels only, on
 * the caller's stream; no atomics: results are bitwise reproducible, and a row of a batch is bitwise the single call.
 *
 * exo_location_windows_f64 -- the windows.  Cadence i opens a new segment when t[i] - t[i-1] > break_tolerance (> 0;
 * INFINITY: one segment).  lo[i], hi[i]: the first and the last cadence j of i's segment with t[j] >= t[i] - half_window and
 * t[j] <= t[i] + half_window, each bound ONE fp64 operation; edge[i] = 1 where t[i] is closer than edge_cutoff to its segment's
 * first or last time (t[i] - t_first < edge_cutoff or t_last - t[i] < edge_cutoff), else 0; *widest = max(hi - lo + 1), one
 * device int32.  EXO_ERR_INVALID_ARGUMENT, before any launch: a null pointer, n < 1, half_window negative or NaN,
 * break_tolerance not > 0, edge_cutoff negative or NaN.
 *
 * exo_running_location_f64 -- the filter.  exclude: n_exclude = 0 (none), 1 (one row for every series) or n_series rows of n
 * bytes, non-zero: the cadence is left out of every window (it still gets a value).  lo, hi: from the call above; edge:
 * from it, or NULL (no cadence is cut).  max_window: at least the widest window, the `widest` of the call above read back by
 * the caller; the workgroup's LDS is sized by it, 8 (256 + 2 max_window - 2) bytes, which bounds it by
 * EXO_LOCATION_MAX_WINDOW = 8192 cadences (a 1 d window at 20 s cadence is 4320; 133 104 of the 163 840 bytes of a CU).  A cadence
 * whose window is wider than max_window gets NaN, never a wrong value (and so may cadences of its 256-cadence tile: their
 * shared span is cut to the size promised); no index leaves [0, n) or the staged span whatever lo and hi hold.
 * trend[n_series][n]: method EXO_LOCATION_MEDIAN: the median of the window's participating values (the mean of the two
 * middle ones for an even count); EXO_LOCATION_BIWEIGHT: exactly n_iter steps of the biweight location with tuning constant
 * cval from the median, scaled by the MAD (the median where the MAD is 0).  scale[n_series][n], or NULL: the MAD, unscaled.
 * No participating value, or edge[i]: NaN in both.  EXO_ERR_INVALID_ARGUMENT, before any launch: a null y, lo, hi or trend,
 * n < 1, n_series < 1, cval <= 0 (or NaN), n_iter < 0, an unknown method, max_window outside [1, EXO_LOCATION_MAX_WINDOW],
 * n_exclude other than 0, 1 or n_series, or rows promised and a null exclude.  (Added without a new ABI number: no caller
 * breaks.) */
#define EXO_LOCATION_MEDIAN 0
#define EXO_LOCATION_BIWEIGHT 1
#define EXO_LOCATION_MAX_WINDOW 8192
int exo_location_windows_f64(const double* t, int64_t n, double half_window, double break_tolerance, double edge_cutoff,
                             int32_t* lo, int32_t* hi, uint8_t* edge, int32_t* widest, void* stream);
int exo_running_location_f64(const double* y, const uint8_t* exclude, int64_t n_exclude, int64_t n, int64_t n_series,
                             const int32_t* lo, const int32_t* hi, const uint8_t* edge, int32_t max_window, int32_t method,
                             double cval, int32_t n_iter, double* trend, double* scale, void* stream);

/* ---------------------------------------------------------------------------
 * The robust local-polynomial trend (exoplanet_amd/estimators.py: running_location and flatten with order = 1 or 2;
 * definition: DESIGN.md section 21): over the windows of exo_location_windows_f64, Tukey-biweight M-estimation of a
 * polynomial of degree `order` in time, evaluated at the cadence's own time -- what the location above is for degree 0,
 * without its bias next to a segment's end and at an extremum.  One kernel on the caller's stream; no atomics, no
 * workspace: results are bitwise reproducible, and a row of a batch is bitwise the single call.
 *
 * exo_running_trend_f64 -- t[n]: the axis the windows were made for; y, exclude, n_exclude, lo, hi, edge (or NULL): as for
 * exo_running_location_f64.  max_window: at least the widest window; the workgroup stages the values AND the times of its
 * 256-cadence tile's span, 16 (256 + 2 max_window - 2) bytes of LDS, which bounds it by EXO_TREND_MAX_WINDOW = 4096 cadences
 * (135 136 of the 163 840 bytes of a CU).  A cadence whose window is wider than max_window or does not hold the cadence
 * itself gets NaN, never a wrong value; no index leaves [0, n) or the staged span whatever lo and hi hold.
 * trend[n_series][n]: from the window's median, scaled by its MAD, exactly n_iter weighted least-squares steps of a
 * polynomial of degree min(order, distinct times of the window - 1) in x = (t - t[i]) / max(t[hi[i]] - t[i], t[i] - t[lo[i]]);
 * then `rescale` times: the median absolute residual as the new scale and n_iter more steps; the value at x = 0.  The median
 * where the MAD or the window's extent is 0; a stage stops where the weights sum to 0 or a pivot of the moment matrix is at
 * most 1e-10 of that sum.  scale[n_series][n], or NULL: the scale of the last stage run (the MAD where none ran).  No
 * participating value, or edge[i]: NaN in both.  EXO_ERR_INVALID_ARGUMENT, before any launch: a null t, y, lo, hi or
 * trend, n < 1, n_series < 1, an order other than 1 or 2, cval <= 0 (or NaN), n_iter < 0, rescale < 0, max_window outside
 * [1, EXO_TREND_MAX_WINDOW], n_exclude other than 0, 1 or n_series, or rows promised and a null exclude.  (Added without a
 * new ABI number: no caller breaks.) */
#define EXO_TREND_MAX_WINDOW 4096
int exo_running_trend_f64(const double* t, const double* y, const uint8_t* exclude, int64_t n_exclude, int64_t n, int64_t n_series,
                          const int32_t* lo, const int32_t* hi, const uint8_t* edge, int32_t max_window, int32_t order, double cval,
                          int32_t n_iter, int32_t rescale, double* trend, double* scale, void* stream);

/* ---------------------------------------------------------------------------
 * Per-transit times and depths (exoplanet_amd/estimators.py: timing_plan, transit_times, ttv_estimator; definition:
 * DESIGN.md section 20, restated in numpy by tests/timing_oracle.py): around every transit of a linear ephemeris a template
 * is slid over a grid of trial shifts of the mid-time; at every shift the level and the depth of "c - depth g" are fitted to
 * the cadences of the transit's window by weighted least squares, and the maximum of the log-likelihood gain over a
 * constant is refined by the parabola through its three samples.  Kernels only, on the caller's stream; no atomics, no
 * workspace: every output is bitwise reproducible, and a row of a batch is bitwise the single call.
 *
 * exo_timing_windows_f64 -- the windows, one thread per epoch.  epochs[n_transit]: device int64, the transit numbers n_k.
 * linear_time[k] <- T_k = t0 + period n_k (one multiplication, one addition).  lo[k], hi[k] <- the first and the last cadence i
 * of t[n] (finite, non-decreasing: the caller's promise) with -window / 2 <= t_i - T_k <= window / 2, the difference ONE
 * fp64 operation; a window without a cadence has hi = lo - 1.  *widest <- max(hi - lo + 1), one device int32.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: a null pointer, n < 1, n_transit < 1, period or window not positive (or NaN),
 * t0 not finite.
 *
 * exo_transit_timing_f64 -- the fit, one workgroup per (transit, series) of y[n_series][n].  ivar: the weights 1 / yerr^2,
 * n_ivar = 0 (NULL: unit weights), 1 (one row for every series) or n_series rows of n; a weight of 0 takes the cadence out.
 * linear_time, lo, hi: from the call above; max_window: at least its `widest`, read back by the caller -- the workgroup's
 * LDS is sized by it, 8 (3 max_window + n_template + n_shift) + 5120 bytes, which gives the three caps below (144 392 of the
 * 163 840 bytes of a CU with all three reached).  A window wider than max_window gives an invalid transit, never a wrong
 * value, and no index leaves [0, n) whatever lo and hi hold.  duration: first to fourth contact; the trial shifts are
 * delta_j = -max_shift + j (2 max_shift / (n_shift - 1)), j = 0 .. n_shift - 1, n_shift odd; window: the one the windows
 * were made with (it is only checked here).  tmpl[n_template]: the template's samples at the bin centres
 * (2 q + 1) / n_template - 1, finite; between them it is linear, beyond the outermost linear to 0 at -1 and +1.
 * depth: n_depth = 0 (NULL: the depth is fitted), 1 or n_series values it is held at.  min_in_transit >= 1.
 * out[7][n_series][n_transit]: transit_time, shift, time_err, depth, depth_err, log_likelihood, depth_snr;
 * iout[4][n_series][n_transit] (int32): n_window (hi - lo + 1, whatever the weights), n_in (at the maximum), valid, at_edge;
 * curve[n_series][n_transit][n_shift] or NULL: the log-likelihood gain of every shift, -inf where (k, j) is not
 * admissible.  An invalid transit: NaN in out, n_in = 0, at_edge = 0.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: a null t, y, linear_time, lo, hi, tmpl, out or iout; n < 1, n_series < 1 (or
 * > 65535), n_transit < 1; n_shift even, < 3 or > EXO_TIMING_MAX_SHIFTS; duration, window not positive (or NaN); max_shift
 * negative (or NaN); window < duration + 2 max_shift; max_window outside [1, EXO_TIMING_MAX_WINDOW]; n_template outside
 * [1, EXO_TIMING_MAX_TEMPLATE]; min_in_transit < 1; n_ivar other than 0, 1 or n_series, n_depth likewise, or rows promised
 * and a null pointer.  (Added without a new ABI number: no caller breaks.) */
#define EXO_TIMING_MAX_WINDOW 4096
#define EXO_TIMING_MAX_TEMPLATE 1024
#define EXO_TIMING_MAX_SHIFTS 4097
int exo_timing_windows_f64(const double* t, int64_t n, const int64_t* epochs, int64_t n_transit, double period, double t0,
                           double window, double* linear_time, int32_t* lo, int32_t* hi, int32_t* widest, void* stream);
int exo_transit_timing_f64(const double* t, const double* y, const double* ivar, int64_t n_ivar, int64_t n, int64_t n_series,
                           const double* linear_time, const int32_t* lo, const int32_t* hi, int64_t n_transit,
                           int32_t max_window, double duration, double max_shift, int32_t n_shift, double window,
                           const double* tmpl, int32_t n_template, const double* depth, int64_t n_depth,
                           int32_t min_in_transit, double* out, int32_t* iout, double* curve, void* stream);

/* ---------------------------------------------------------------------------
 * The Keplerian periodogram of radial velocities (exoplanet_amd/estimators.py: keplerian_power, keplerian_estimator;
 * definition, kernel and measurements: DESIGN.md section 22).  For every frequency f and every series of y[n_series][n] at the
 * epochs t[n]: the maximum over the candidates (e_j, phi_k = k / n_phase) of
 *     power = (chi2_0 - chi2) / 2,    chi2 = min over (c, A, B) of sum w (y - c_inst - A cos nu - B sin nu)^2,
 * nu the true anomaly at mean anomaly 2 pi (f (t - t_min) - phi_k) and eccentricity e_j, one free constant per instrument,
 * chi2_0 the same with A = B = 0.  This is the package's radial-velocity model with A = K cos w, B = -K sin w,
 * c_inst = zero_point_inst + e A and t_periastron = t_min + phi_k / f.  Candidates are numbered j * n_phase + k; where
 * e_j == 0 only k = 0 is one; the lowest number wins among equal powers.
 *
 * The epochs are given SORTED BY INSTRUMENT: instrument k owns the epochs segment_offsets[k] .. segment_offsets[k + 1] - 1 of
 * t, y and yerr, with 0 = segment_offsets[0] < ... < segment_offsets[n_instrument] = n.  Inside a segment any order.
 * yerr: n_yerr = 0 (NULL: unit weights), 1 (one row for every series) or n_series rows of n; w = 1 / yerr^2.
 * segment_offsets and ecc are HOST arrays (they travel by value in the kernel arguments); everything else lives on the
 * device.  power[n_series][n_frequency]; candidate[n_series][n_frequency] (int32); coef[n_series][n_frequency][2 + n_instrument]
 * = A, B and the constants c_k.  A (frequency, series) at which no candidate has a power that compares (NaN input): power
 * -inf, candidate -1, coef NaN.  workspace: exo_keplerian_workspace_bytes(n, n_series) bytes (-1: invalid sizes), written
 * by a preparation kernel (t - t_min, w, w y and every segment's sum w and sum w y) and read by the search.  Every sum has a
 * fixed order: the outputs are bitwise reproducible, and a row of a batch is bitwise the single call.
 * n_frequency == 0: EXO_OK, nothing launched.  EXO_ERR_INVALID_ARGUMENT, before any launch: a null t, y, segment_offsets,
 * frequencies, ecc, power, candidate, coef or workspace; n < 1, n_series < 1 (or > 65535); n_yerr other than 0, 1 or
 * n_series, or rows promised and a null pointer; n_instrument outside [1, EXO_KEP_MAX_INSTRUMENTS]; offsets that do not tile
 * 0 .. n with a non-empty segment each; n_ecc outside [1, EXO_KEP_MAX_ECC]; n_phase outside [1, EXO_KEP_MAX_PHASES]; an e
 * outside [0, 1) (or NaN).  EXO_ERR_WORKSPACE: workspace_bytes too small.  (Added without a new ABI number: no caller breaks.) */
#define EXO_KEP_MAX_INSTRUMENTS 8
#define EXO_KEP_MAX_ECC 64
#define EXO_KEP_MAX_PHASES 4096
int64_t exo_keplerian_workspace_bytes(int64_t n, int64_t n_series);
int exo_keplerian_power_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                            const int32_t* segment_offsets, int32_t n_instrument, const double* frequencies, int64_t n_frequency,
                            const double* ecc, int32_t n_ecc, int32_t n_phase, double* power, int32_t* candidate, double* coef,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The highest peak of that periodogram for every series, without the periodogram (exoplanet_amd/estimators.py:
 * keplerian_max_power, false_alarm): what the resamplings behind a false-alarm probability need.  The
 * arguments are those of exo_keplerian_power_f64; the series are searched in groups that share every solve of Kepler's
 * equation (the true anomaly depends on the epoch, the frequency and the candidate alone), in blocks of
 * frequencies_per_block consecutive frequencies (0: the host chooses; the results do not depend on it).  Per series:
 * max_power[n_series], the largest power over the grid -- bit for bit the largest entry of exo_keplerian_power_f64's row --,
 * frequency_index[n_series] (int32) the lowest index at which it is reached, candidate[n_series] (int32) the winning
 * candidate there.  A series without a finite power (NaN input, or n_frequency == 0): -inf, -1, -1.  workspace:
 * exo_keplerian_max_workspace_bytes(n, n_series, n_frequency, frequencies_per_block) bytes (-1: invalid sizes), pure
 * arithmetic; every slot of it that is read is written by a kernel first.  Nothing but kernels is enqueued, no atomics: the
 * outputs are bitwise reproducible, and a row of a batch is bitwise the single call.  EXO_ERR_INVALID_ARGUMENT, before any
 * launch: what exo_keplerian_power_f64 rejects, a null output, frequencies_per_block < 0.  EXO_ERR_WORKSPACE: workspace_bytes
 * too small.  (Added without a new ABI number: no caller breaks.) */
int64_t exo_keplerian_max_workspace_bytes(int64_t n, int64_t n_series, int64_t n_frequency, int32_t frequencies_per_block);
int exo_keplerian_max_f64(const double* t, const double* y, const double* yerr, int64_t n_yerr, int64_t n, int64_t n_series,
                          const int32_t* segment_offsets, int32_t n_instrument, const double* frequencies, int64_t n_frequency,
                          const double* ecc, int32_t n_ecc, int32_t n_phase, int32_t frequencies_per_block, double* max_power,
                          int32_t* frequency_index, int32_t* candidate, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The astrometric orbit search on the Thiele-Innes constants (exoplanet_amd/estimators.py: astrometric_power,
 * astrometric_estimator; definition, kernel and measurements: DESIGN.md section 23).  For every frequency f and every series
 * of separations rho[n_series][n] and position angles theta[n_series][n] at the epochs t[n]: the maximum over the candidates
 * (e_j, phi_k = k / n_phase) of the Keplerian periodogram's grid of
 *     power = (chi2_0 - chi2) / 2,    chi2 = min over (TA, TB, TF, TG) of sum r^T P r,
 *     r = (rho cos theta - TA xi - TF eta, rho sin theta - TB xi - TG eta),   xi = cos E - e,  eta = sqrt(1 - e^2) sin E,
 *     P = (c, s)(c, s)^T / rho_err^2 + (-s, c)(-s, c)^T / (rho theta_err)^2,  (c, s) = (cos, sin) theta,
 * E the eccentric anomaly at the mean anomaly 2 pi (f (t - t_min) - phi_k), chi2_0 = sum (x, y) P (x, y)^T.  A candidate whose
 * normal matrix, scaled to a unit diagonal, has a squared Cholesky pivot below 1e-12 (or a non-positive diagonal) is none at
 * that frequency.  Equal powers: the lowest candidate number j * n_phase + k wins.
 * ecc is a HOST array (it travels by value in the kernel arguments); everything else lives on the device.  rho_err and
 * theta_err: n_rho_err / n_theta_err rows of n, 1 (shared by the series) or n_series.  power[n_series][n_frequency];
 * candidate[n_series][n_frequency] (int32); coef[n_series][n_frequency][EXO_AST_NCOEF] = TA, TB, TF, TG, a_angular, incl,
 * omega, Omega, t_periastron = t_min + phi_k / f, chi2 -- the elements in the convention of KeplerianOrbit (amplitude
 * -a_angular), Omega in [0, pi), omega in (-pi, pi].  A (frequency, series) with no candidate: power 0, candidate -1, coef NaN.
 * workspace: exo_astrometric_workspace_bytes(n, n_series) bytes (-1: invalid sizes), written by a preparation kernel and read
 * by the search.  Every sum has a fixed order: the outputs are bitwise reproducible, and a row of a batch is bitwise the
 * single call.  n_frequency == 0: EXO_OK, nothing launched.  EXO_ERR_INVALID_ARGUMENT, before any launch: a null pointer;
 * n < 1, n_series < 1 (or > 65535); n_rho_err or n_theta_err other than 1 or n_series; n_frequency < 0; n_ecc outside
 * [1, EXO_KEP_MAX_ECC]; n_phase outside [1, EXO_KEP_MAX_PHASES]; an e outside [0, 1) (or NaN).  EXO_ERR_WORKSPACE:
 * workspace_bytes too small.  (Added without a new ABI number: no caller breaks.) */
#define EXO_AST_NCOEF 10
int64_t exo_astrometric_workspace_bytes(int64_t n, int64_t n_series);
int exo_astrometric_power_f64(const double* t, const double* rho, const double* rho_err, int64_t n_rho_err, const double* theta,
                              const double* theta_err, int64_t n_theta_err, int64_t n, int64_t n_series, const double* frequencies,
                              int64_t n_frequency, const double* ecc, int32_t n_ecc, int32_t n_phase, double* power,
                              int32_t* candidate, double* coef, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Priors and constrained parameters (exoplanet_amd/distributions.py; definitions and measurements: DESIGN.md section 10).
 * One unconstrained array z[n_chain][n_free] -- the flat array the samplers integrate -- becomes the constrained, named
 * parameters of a model and the log prior density of every chain INCLUDING the log-Jacobians of the transforms, in one
 * kernel; the reverse is one kernel too.  s(z) = 1 / (1 + exp(-z)), L(z) = log s(z) + log s(-z).
 *
 *   kind                 free coordinates        constrained value(s)                          contribution to the log prior
 *   NORMAL               z                       x = z                                         -((x-mu)/sd)^2/2 - log sd - log(2 pi)/2
 *   LOGNORMAL            z                       x = exp z                                     the normal log-density of z
 *   UNIFORM              z                       x = lo + (hi-lo) s(z)                         L(z)
 *   ANGLE                z1, z2                  theta = atan2(z1, z2)                         -(z1^2+z2^2)/2 - log 2pi [+ reg log(z1^2+z2^2)]
 *   UNIT_DISK            z1, z2                  x = s(z1) - s(-z1), y = (s(z2) - s(-z2)) w    L(z1) + L(z2) + log(w),  w = 2 sqrt(s(z1) s(-z1))
 *   QUAD_LIMB_DARK       z1, z2                  u1 = 2 sqrt(s(z1)) s(z2),                     L(z1) + L(z2)
 *                                                u2 = sqrt(s(z1)) (s(-z2) - s(z2))
 *   IMPACT_PARAMETER     z                       b = s(z) (1 + ror)                            L(z)
 *   KIPPING13            z                       e = lo + (hi-lo) s(z)                         log Beta(e; alpha, beta) - log(I_hi - I_lo) + log(hi-lo) + L(z)
 *   VANEYLEN19           z                       e = lo + (hi-lo) s(z)                         L(z) + logaddexp(log(1-f) + halfnormal(e; sg), log f + Rayleigh(e; sr))
 *   KIPPING13_HYPER      za, zb, z               alpha = exp za, beta = exp zb, e = s(z)       the Beta log-density of every e + L(z), the hyperpriors
 *   VANEYLEN19_HYPER     zg, zr, zf, z           sg = exp zg, sr = exp zr, f = s(zf), e        as VANEYLEN19, the hyperpriors
 *
 * A block has `count` elements.  Its free coordinates start at column `offset` of z: the hyperparameters first (one each,
 * shared by the elements), then z1 of every element, then z2 of every element.  Its values go to consecutive entries of
 * the output pointer list, the first at index `out`: one array [n_chain][count] per value (NORMAL .. VANEYLEN19: one;
 * UNIT_DISK, QUAD_LIMB_DARK: two), then one array [n_chain] per hyperparameter.  p[]:
 *   NORMAL, LOGNORMAL: mu, sd.  UNIFORM: lo, hi.  ANGLE: reg (flags & 1: regularised).  IMPACT_PARAMETER: ror, used when
 *   link < 0; link >= 0 names an EARLIER block of kind NORMAL, LOGNORMAL or UNIFORM with `count` elements or one, whose
 *   value is ror (and receives db/dror in the reverse pass).  KIPPING13: alpha, beta, lo, hi, c with c = -log B(alpha, beta)
 *   [- log(I_hi - I_lo) + log(hi - lo) when flags & 1: bounded], computed by the caller.  VANEYLEN19: sg, sr, f, lo, hi.
 *   KIPPING13_HYPER: alpha_mu, alpha_sd, beta_mu, beta_sd (truncated normals, lower bound 0; log-Jacobian za, zb).
 *   VANEYLEN19_HYPER: sg_mu, sg_sd, sr_mu, sr_sd, f_mu, f_sd, lo, hi (sg, sr as above; f a normal truncated to [0, 1]).
 *
 * table: HOST array of n_block <= EXO_PRIOR_MAX_BLOCKS blocks; theta: HOST array of the device output pointers (at most
 * EXO_PRIOR_MAX_OUTPUTS, every one required); both travel by value in the kernel arguments.  log_prior[n_chain].  The
 * reverse recomputes from z; gtheta: HOST array of the cotangents of the outputs, a null entry standing for zero;
 * glog_prior[n_chain] or null; gz[n_chain][n_free]: every element is written (coordinates no block covers: zero).
 * A lane is a chain and sums its log prior in a register: results do not depend on the launch geometry.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: negative sizes, null pointers, an unknown kind, a block outside z or
 * overlapping its predecessor, a link that points forward or to itself.  n_chain == 0: EXO_OK, nothing launched.
 * ------------------------------------------------------------------------- */
#define EXO_PRIOR_MAX_BLOCKS 32
#define EXO_PRIOR_MAX_OUTPUTS 48
#define EXO_PRIOR_NORMAL 0
#define EXO_PRIOR_LOGNORMAL 1
#define EXO_PRIOR_UNIFORM 2
#define EXO_PRIOR_ANGLE 3
#define EXO_PRIOR_UNIT_DISK 4
#define EXO_PRIOR_QUAD_LIMB_DARK 5
#define EXO_PRIOR_IMPACT_PARAMETER 6
#define EXO_PRIOR_KIPPING13 7
#define EXO_PRIOR_VANEYLEN19 8
#define EXO_PRIOR_KIPPING13_HYPER 9
#define EXO_PRIOR_VANEYLEN19_HYPER 10
#define EXO_PRIOR_N_KINDS 11
typedef struct exo_prior_block {
  int32_t kind, offset, count, link, out, flags;
  double p[8];
} exo_prior_block;
int exo_prior_transform_f64(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                            double* const* theta, double* log_prior, void* stream);
int exo_prior_transform_vjp_f64(const double* z, int64_t n_chain, int32_t n_free, const exo_prior_block* table, int32_t n_block,
                                const double* const* gtheta, const double* glog_prior, double* gz, void* stream);

/* -------------------------------------------------------------------------
 * Rank-normalised split diagnostics of a batch of chains (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021): R-hat, bulk /
 * tail / mean effective sample sizes, the Monte-Carlo standard error of the mean, moments and quantiles, per parameter
 * (exoplanet_amd/diagnostics.py states every quantity in torch).  A call handles n_param parameters;
 * after splitting each chain into its first and last halves a parameter is n_half = 2 chains half-chains of n_len draws,
 * S = n_half n_len values, held pooled as [n_len][n_half] (half-chains innermost).  The caller sorts -- nothing else:
 *   1. sorted, perm = sort of x [n_param][S]; sorted_full [n_param][n_full] = sort of ALL draws of a parameter (the same
 *      array when no middle draw was dropped);
 *   2. exo_diag_prepare_f64: folded [n_param][S] = |x - median|; sets [n_param][EXO_DIAG_SETS][S]: the tail indicators
 *      1[x <= q05], 1[x <= q95] (sets 2, 3) and x minus a pivot (set 4); moments [n_param][EXO_DIAG_MOMENTS]
 *      = mean, sd (ddof 1), q05, q50, q95 (linear interpolation), not-finite, constant, the pivot;
 *   3. exo_diag_rank_f64 with (sorted, perm) into set 0 and with the sort of `folded` into set 1: average ranks (ties share the
 *      mean of their ranks), z = Phi^-1((r - 3/8) / (S + 1/4)), scattered through perm (int64, values outside 0 .. S - 1
 *      are skipped);
 *   4. for block = 0, 1, ...: exo_diag_autocov_f64 (lags block EXO_DIAG_LAG_BLOCK .. + EXO_DIAG_LAG_BLOCK - 1 of every set
 *      that is not done) then exo_diag_finish_f64 with the same block (rho_t, Geyer's initial positive sequence, and -- once a
 *      set's sequence has ended -- the monotone sequence, tau, the effective sample size, done[set] = 1); blocks in order,
 *      until every done [n_param EXO_DIAG_SETS] (int32, zeroed by the caller) is 1: after ceil(n_len / EXO_DIAG_LAG_BLOCK)
 *      blocks at the latest;
 *   5. exo_diag_finish_f64 with block = -1: out [n_param][EXO_DIAG_OUT] = mean, sd, q05, q50, q95, mcse_mean, ess_bulk,
 *      ess_tail, ess_mean, r_hat, max_t of the bulk / lower tail / upper tail / mean sequences, R-hat of z and of folded z.
 * A parameter with a value that is not finite: NaN everywhere (max_t -1); a constant one: ESS = S, R-hat NaN.
 * workspace: exo_diag_workspace_bytes(n_param, n_half, n_len) bytes, the same array in every call of steps 4 and 5; -1 for
 * sizes that cannot be.  EXO_ERR_INVALID_ARGUMENT, before any launch: negative sizes, n_len < 2, an odd n_half, n_param
 * EXO_DIAG_SETS > 65535, n_full < S, a set other than 0 or 1, a block outside the series, a null pointer;
 * EXO_ERR_WORKSPACE: too small.  n_param == 0 or n_half == 0: EXO_OK, nothing launched (sizes are checked first).
 * Kernels only; every sum in a fixed order, no atomics: bit-reproducible.  (Added without a new ABI number: no caller
 * breaks.)
 * ------------------------------------------------------------------------- */
#define EXO_DIAG_LAG_BLOCK 16
#define EXO_DIAG_SETS 5
#define EXO_DIAG_MOMENTS 8
#define EXO_DIAG_OUT 16
int64_t exo_diag_workspace_bytes(int64_t n_param, int64_t n_half, int64_t n_len);
int exo_diag_prepare_f64(const double* x, const double* sorted, const double* sorted_full, int64_t n_full, int64_t n_param,
                         int64_t n_half, int64_t n_len, double* folded, double* sets, double* moments, void* stream);
int exo_diag_rank_f64(const double* sorted, const int64_t* perm, int64_t n_param, int64_t n_half, int64_t n_len, int32_t set,
                      double* sets, void* stream);
int exo_diag_autocov_f64(const double* sets, int64_t n_param, int64_t n_half, int64_t n_len, int64_t block, const int32_t* done,
                         void* workspace, int64_t workspace_bytes, void* stream);
int exo_diag_finish_f64(int64_t n_param, int64_t n_half, int64_t n_len, int64_t block, const double* moments, double* out,
                        int32_t* done, void* workspace, int64_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Quantiles along the strided axis of an array of curves: the posterior bands of a model over a trace's draws
 * (exoplanet_amd/predictive.py).  x: n_rows rows of n_cols doubles, row_stride >= n_cols doubles apart
 * (the last axis contiguous), on the device.  For every column and every q < n_q (1 .. EXO_QUANTILE_MAX_Q), with the
 * fraction num[q] / den[q] (HOST arrays, read before the launch; 0 <= num <= den, 1 <= den <= 1e9):
 *   the m values of the column that are not NaN take part; m = 0: NaN.  Position (m - 1) num / den = lo + rem / den in whole
 *   numbers; rem = 0: x_(lo), the lo-th smallest, untouched; otherwise x_(lo) + (rem / den) (x_(lo+1) - x_(lo)), these four
 *   operations in this order, none fused.  An order statistic is a NUMBER: a zero of either sign is +0.
 * out [n_q][n_cols]; n_valid [n_cols] (int32, or NULL) = m.  Selection by counting passes over the column: no sort, no
 * workspace, no atomics on floating-point numbers; kernels only, no host synchronisation, bit-reproducible, capturable.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: negative sizes, n_rows >= 2^31, n_q > EXO_QUANTILE_MAX_Q, row_stride < n_cols,
 * a null x (with n_rows > 0), num, den or out, den <= 0 or > 1e9, num outside [0, den].  n_cols == 0 or n_q == 0: EXO_OK,
 * nothing launched (sizes are checked first).  n_rows == 0: NaN and m = 0 everywhere.  (Added without a new ABI number: no
 * caller breaks.)
 * ------------------------------------------------------------------------- */
#define EXO_QUANTILE_MAX_Q 16
int exo_column_quantiles_f64(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, const int64_t* num,
                             const int64_t* den, int n_q, double* out, int32_t* n_valid, void* stream);

/* -------------------------------------------------------------------------
 * PSIS-LOO and WAIC per column of an array of pointwise log-likelihoods (exoplanet_amd/comparison.py).
 * x: n_rows draws of n_cols observations, row_stride >= n_cols doubles apart (the last axis contiguous), on the device.  For
 * every column l_s, with M = n_tail_max (1 .. EXO_PSIS_MAX_TAIL; the caller's ceil(min(S / 5, 3 sqrt(S / reff)))):
 *   a NaN or an infinity in the column, or n_rows == 0: NaN in every floating output, n_tail = 0.  Otherwise x_s = l_min - l_s,
 *   the cut-off c = max(x_(max(S-M-1, 0)), log(DBL_MIN)), the tail {x_s > c} of n <= M values; n <= 4: k = +inf, nothing is
 *   smoothed; otherwise the generalised-Pareto fit of Zhang & Stephens (2009) to exp(x) - exp(c) of the tail ascending, with
 *   the prior of ArviZ's _gpdfit, gives k and sigma, and a finite k replaces the j-th tail value by
 *   min(log(sigma expm1(-k log1p(-p_j)) / k + exp(c)), 0), p_j = (j + 0.5) / n.  With the smoothed x':
 *   out_elpd = logsumexp_s(x'_s + l_s) - logsumexp_s(x'_s); out_k = k; out_lppd = logsumexp_s(l_s) - log S; out_var = the
 *   variance of l_s over the draws with divisor S, about the mean; out_n_tail = n.  Each [n_cols].
 * One kernel: selection by counting passes for the cut-off, the tail gathered, sorted and fitted in LDS; no workspace, no
 * atomics on floating-point numbers, no host synchronisation; bit-reproducible, capturable.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: negative sizes, n_rows >= 2^31, n_tail_max outside 1 .. EXO_PSIS_MAX_TAIL,
 * row_stride < n_cols, a null x (with n_rows > 0) or a null output.  n_cols == 0: EXO_OK, nothing launched (sizes are checked
 * first).  (Added without a new ABI number: no caller breaks.)
 * ------------------------------------------------------------------------- */
#define EXO_PSIS_MAX_TAIL 1024
int exo_column_psis_f64(const double* x, int64_t n_rows, int64_t n_cols, int64_t row_stride, int32_t n_tail_max, double* out_elpd,
                        double* out_k, double* out_lppd, double* out_var, int32_t* out_n_tail, void* stream);

/* -------------------------------------------------------------------------
 * The dense metric of HMC / NUTS (exoplanet_amd/sampling.py, set_metric and adapt_mass="dense"): a
 * covariance Sigma = L L^T, L lower triangular, and a centre c; the samplers run at unit masses in x, q = c + L x.
 * chol: row-major (n, n), only the lower triangle is read; n <= EXO_METRIC_MAX_N.  Rows are contiguous, (n_row, n).  Every sum
 * has the one order stated here and no product is fused with an addition, so a result is bitwise reproducible and bitwise
 * that of the host build of csrc/exo_metric_core.hpp.  No atomics, no workspace, no host synchronisation; capturable.
 *
 * exo_metric_apply_f64, per row, `out` may be `in`:
 *   EXO_METRIC_FORWARD     out_i = c_i + sum_{j <= i} L_ij in_j, the sum from its first product on, j ascending, c_i last;
 *   EXO_METRIC_TRANSPOSED  out_j = sum_{i >= j} in_i L_ij, i ascending (center is not read and may be null);
 *   EXO_METRIC_SOLVE       L out = in - c by forward substitution: ((in_i - c_i) - L_i0 out_0 - ...) / L_ii, j ascending.
 * exo_metric_accumulate_f64: with dq = q - shift, row d ascending, every row whose n elements are all finite adds dq_i into
 *   sum1[i] and dq_i dq_j into sum2[i * n + j], j <= i (the upper triangle is not touched), each running sum taking the rows
 *   in their order; the number of rows kept is added to *count.
 * exo_metric_update_f64, one workgroup: N = *count; m_i = shift_i + sum1_i / N; S_ij = (sum2_ij - sum1_i sum1_j / N) / (N - 1);
 *   Sigma = N / (N + 5) S + 1e-3 (5 / (N + 5)) diag(S) (Stan's shrinkage, relative to each variance); the Cholesky factor, entry (i, j) = Sigma_ij less
 *   L_ik L_jk for k ascending, divided by L_jj off the diagonal, the square root on it.  On success cov (symmetric), chol
 *   (upper part zero) and center = m are written and *status = EXO_METRIC_STATUS_OK.  N < 2 (TOO_FEW), a non-finite m, Sigma
 *   or pivot (NOT_FINITE), a pivot <= 0 (NOT_POSITIVE): NOTHING but *status is written -- the previous metric stays in force.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: negative sizes, n outside 1 .. EXO_METRIC_MAX_N, an unknown mode, a null
 * pointer.  n_row == 0: EXO_OK, nothing launched (sizes are checked first).  (Added without a new ABI number: no caller breaks.)
 * ------------------------------------------------------------------------- */
#define EXO_METRIC_MAX_N 64
#define EXO_METRIC_FORWARD 0
#define EXO_METRIC_TRANSPOSED 1
#define EXO_METRIC_SOLVE 2
#define EXO_METRIC_STATUS_OK 0
#define EXO_METRIC_STATUS_TOO_FEW 1
#define EXO_METRIC_STATUS_NOT_FINITE 2
#define EXO_METRIC_STATUS_NOT_POSITIVE 3
int exo_metric_apply_f64(const double* chol, const double* center, const double* in, double* out, int64_t n_row, int32_t n,
                         int32_t mode, void* stream);
int exo_metric_accumulate_f64(const double* q, int64_t n_row, int32_t n, const double* shift, double* sum1, double* sum2,
                              int64_t* count, void* stream);
int exo_metric_update_f64(const double* sum1, const double* sum2, const int64_t* count, const double* shift, int32_t n,
                          double* cov, double* chol, double* center, int32_t* status, void* stream);

/* -------------------------------------------------------------------------
 * The Laplace approximation at the chains' modes (exoplanet_amd/laplace.py; the definition is
 * tests/laplace_oracle.py): the Hessian of f = -logp by central differences of the batched gradient, and from it, per chain,
 * the covariance H^-1 and the Laplace log-evidence.  x: (n_chain, n) positions; free_index: m ascending int32 indices into a
 * row, on the device, the same for every chain; order: 2 or 4; n and m at most EXO_LAPLACE_MAX_N.  Every sum has one stated
 * order and no product is fused with an addition, so a result is bitwise reproducible and bitwise that of the host build of
 * csrc/exo_laplace_core.hpp.  No atomics, no workspace, no host synchronisation; capturable.
 *
 * exo_laplace_points_f64: points (n_chain, order m, n), dx (n_chain, order m).  Row r = s m + k is x with coordinate
 *   free_index[k] moved by +h_k (s = 0), -h_k (1), +2 h_k (2), -2 h_k (3); dx[r] is the REALISED offset fl(fl(x + off) - x).
 *   h_k = eps^(1/3) scale_k, scale (n), or (n_chain, n) with scale_per_chain != 0, or null: max(|x|, 1); with hess (n_chain, m,
 *   m; a previous pass's) h_k = delta / sqrt(hess_kk) where that and hess_kk are finite and positive.
 * exo_laplace_factor_f64, one wave per chain: grad (n_chain, order m, n), the gradient of logp at the points.
 *   A1_ik = -(g_{k}[F_i] - g_{m+k}[F_i]) / (dx_k - dx_{m+k}), A2 from the rows 2m + k, 3m + k; A = A1 (order 2) or
 *   (4 A1 - A2) / 3; hess = (A + A^T) / 2 (n_chain, m, m); asymmetry = max_{i>k} |A_ik - A_ki| / sqrt(|H_ii H_kk|); fd_error =
 *   max_{i>=k} |H1_ik - H2_ik| / sqrt(|H_ii H_kk|) (NaN at order 2).  s_i = 1 / sqrt(H_ii), C = S H S with a unit diagonal
 *   = R R^T; logdet = sum log H_ii + 2 sum log R_ii; cov = S (R^-1)^T R^-1 S (n_chain, m, m), sd_i = sqrt(cov_ii);
 *   log_evidence = logp + (m / 2) log(2 pi) - logdet / 2.  status: EXO_LAPLACE_STATUS_NOT_FINITE -- a non-finite offset or free
 *   gradient entry, dx_+ - dx_- == 0, a non-finite H_ii --, EXO_LAPLACE_STATUS_NOT_POSITIVE -- an H_ii <= 0 or a pivot of C at
 *   or below m eps --: hess, asymmetry and fd_error are written, everything else of that chain is NaN.
 * EXO_ERR_INVALID_ARGUMENT, before any launch: n_chain < 0, m < 1, m > n, n or m above EXO_LAPLACE_MAX_N, order outside
 * {2, 4}, hess with delta <= 0, a null pointer (scale and hess may be null).  n_chain == 0: EXO_OK, nothing launched (sizes
 * are checked first).  (Added without a new ABI number: no caller breaks.)
 * ------------------------------------------------------------------------- */
#define EXO_LAPLACE_MAX_N 64
#define EXO_LAPLACE_STATUS_OK 0
#define EXO_LAPLACE_STATUS_NOT_FINITE 1
#define EXO_LAPLACE_STATUS_NOT_POSITIVE 2
int exo_laplace_points_f64(const double* x, int64_t n_chain, int32_t n, const int32_t* free_index, int32_t m, const double* scale,
                           int32_t scale_per_chain, const double* hess, double delta, int32_t order, double* points, double* dx,
                           void* stream);
int exo_laplace_factor_f64(const double* grad, const double* dx, const double* logp, int64_t n_chain, int32_t n,
                           const int32_t* free_index, int32_t m, int32_t order, double* hess, double* cov, double* sd, double* logdet,
                           double* log_evidence, double* asymmetry, double* fd_error, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXOPLANET_AMD_H */
