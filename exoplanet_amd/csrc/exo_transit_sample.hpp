// exo_transit_sample.hpp -- what the two paths of the light-curve sweep (exo_transit.hip) share in their heavy work: the block
// geometry and the compact gradient slots, the per-(draw, planet) constants staged in LDS and pinned to scalar registers, the
// timing tables, ONE (cadence, sub-exposure, planet) sample -- eval_sample: Kepler solve, solution vector, flux, reverse
// sweep into LDS gradient columns -- and the fixed-order reduction of those columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/exoplanet_amd.h"
#include "exo_math.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 2 * kBlock;         // cadences per tile: two per lane
constexpr int kNG = 12;                 // compact gradient slots per planet
constexpr int kWin = 7;                 // doubles per record written by transit_window_kernel
// compact slot order
enum { G_N = 0, G_TP, G_ECC, G_COSW, G_SINW, G_COSI, G_AOR, G_ROR, G_FR, G_PAD, G_SINI, G_CL };   // (SINI, CL: light delay only)
constexpr double kCLight = 37231.66360672704;   // R_sun / day (orbits/constants.py:36)

// Per-(draw, planet) constants derived once per block and staged in LDS.
struct PlanetConst {
  double n, tp, e, se, pe, sq1me2, cw, sw, ci, si, aor, ror, iror;
  double t0, period, iperiod, ts, te, fr, ts2, te2, isq1me2;
  double clr;   // speed of light, stellar radii per day (light delay)
  // fp32 copies for the conservative classifier of the scan kernel
  float ef, omf, sqf, cwf, swf, cif, zsf, thrf, zthrf, inthrf;
  // conjunction windows of the scan kernel's first test (see transit_window_kernel)
  double nrev, c0, dmid, half[2];
  // timing tables: first edge, bins per unit time, number of finite edges (see TtvRow::locate)
  double te0, tinv;
  int tfin;
};

struct Shared {
  PlanetConst pc[EXO_MAX_PLANETS];
  double c[6];
  double sdt[EXO_MAX_SUBEXP + 1];
  double sw[EXO_MAX_SUBEXP + 1];
  double red[16][16];  // reduce_columns: up to 16 slots x 16 partial sums
};

// ---------------------------------------------------------------------------
// Transit-timing variations (reference: orbits/ttv.py:158-187).  Every time is measured from its
// nearest labelled transit: planet p of a draw has n_edge bin edges (ascending, padded with +inf)
// and n_edge + 1 shifts; a time t falls in bin k = #{edges < t} (searchsorted, left) and is
// warped to t - shift[k] before anything else happens to it (shift[k] = transit time k - the
// record's t0; the mean anomaly and the window phase are then those of the unperturbed orbit).
// ---------------------------------------------------------------------------
struct Ttv {
  const double* edges = nullptr;   // [n_draw][n_planet][n_edge]; nullptr: no timing tables
  const double* shift = nullptr;   // [n_draw][n_planet][n_edge + 1]
  double* gshift = nullptr;        // [n_draw][n_planet][n_edge + 1], reverse sweep only
  int n_edge = 0;
};

// one planet's table
struct TtvRow {
  const double* __restrict__ edges;
  const double* __restrict__ shift;
  int n_edge;
  __device__ __forceinline__ TtvRow(const Ttv& tv, int64_t rec)
      : edges(tv.edges + rec * tv.n_edge), shift(tv.shift + rec * (tv.n_edge + 1)), n_edge(tv.n_edge) {}
  // #{edges < t}: lower bound, branch-free steps (NaN t -> 0)
  __device__ __forceinline__ int bin(double t) const {
    int lo = 0, len = n_edge;
    while (len > 0) {
      const int half = len >> 1;
      const bool lt = edges[lo + half] < t;
      lo = lt ? lo + half + 1 : lo;
      len = lt ? len - half - 1 : half;
    }
    return lo;
  }
  // The same bin from a guess: labelled transits are nearly evenly spaced, so bin ~ 1 + (t - e0) *
  // inv; the two edges around the guess confirm it (two independent loads instead of a chain of
  // log2(n_edge) dependent ones), anything else falls back to the search.  lo / hi: the edges of
  // the bin (-inf / +inf at the ends).
  __device__ __forceinline__ int locate(double t, double e0, double inv, int n_fin, double& lo, double& hi) const {
    const double x = (t - e0) * inv;
    int g = (x > 0.0) ? ((x < (double)n_fin) ? (int)x + 1 : n_fin) : 0;
    lo = edges[g > 0 ? g - 1 : 0];
    hi = edges[g < n_edge ? g : n_edge - 1];
    if (!((g == 0 || lo < t) && (g == n_edge || !(hi < t)))) {
      g = bin(t);
      lo = edges[g > 0 ? g - 1 : 0];
      hi = edges[g < n_edge ? g : n_edge - 1];
    }
    lo = g > 0 ? lo : -__builtin_inf();
    hi = g < n_edge ? hi : __builtin_inf();
    return g;
  }
  // bin of a sub-exposure time tt of a cadence in bin k = (lo, hi]: k or, for an exposure that
  // reaches over an edge, a neighbour (one confirming load; anything else is searched for)
  __device__ __forceinline__ int neighbour(double tt, int k, double lo, double hi) const {
    if (!(tt > lo)) {          // lo is -inf for k = 0: never taken there
      k -= 1;
      if (k > 0 && !(edges[k - 1] < tt)) k = bin(tt);
    } else if (tt > hi) {      // hi is +inf for k = n_edge
      k += 1;
      if (k < n_edge && edges[k] < tt) k = bin(tt);
    }
    return k;
  }
  // Two times at once, shifts included: all six loads of the two guesses are issued before
  // anything is checked (one memory latency for the pair instead of four in a row).
  struct Hit { int k; double lo, hi, sh; };
  __device__ __forceinline__ int guess(double t, double e0, double inv, int n_fin) const {
    const double x = (t - e0) * inv;
    return (x > 0.0) ? ((x < (double)n_fin) ? (int)x + 1 : n_fin) : 0;
  }
  __device__ __forceinline__ void settle(Hit& h, double t) const {
    if (!((h.k == 0 || h.lo < t) && (h.k == n_edge || !(h.hi < t)))) {
      h.k = bin(t);
      h.lo = edges[h.k > 0 ? h.k - 1 : 0];
      h.hi = edges[h.k < n_edge ? h.k : n_edge - 1];
      h.sh = shift[h.k];
    }
    h.lo = h.k > 0 ? h.lo : -__builtin_inf();
    h.hi = h.k < n_edge ? h.hi : __builtin_inf();
  }
  __device__ __forceinline__ void locate2(double ta, double tb, double e0, double inv, int n_fin, Hit& a, Hit& b) const {
    a.k = guess(ta, e0, inv, n_fin);
    b.k = guess(tb, e0, inv, n_fin);
    a.lo = edges[a.k > 0 ? a.k - 1 : 0]; a.hi = edges[a.k < n_edge ? a.k : n_edge - 1]; a.sh = shift[a.k];
    b.lo = edges[b.k > 0 ? b.k - 1 : 0]; b.hi = edges[b.k < n_edge ? b.k : n_edge - 1]; b.sh = shift[b.k];
    settle(a, ta);
    settle(b, tb);
  }
};

__device__ __forceinline__ void stage_constants(Shared& sh, const double* __restrict__ params, const double* __restrict__ ld,
    const double* __restrict__ stencil_dt, const double* __restrict__ stencil_w, int n_sub, int n_planet, int64_t draw,
    bool secondary, const double* __restrict__ windows = nullptr, const Ttv* ttv = nullptr, int64_t ttv_first = 0) {
  const int tid = threadIdx.x;
  if (tid < n_planet) {
    const double* p = params + (draw * n_planet + tid) * EXO_NPAR;
    PlanetConst& c = sh.pc[tid];
    const double e = p[EXO_P_ECC];
    // e outside [0,1) -> NaN everywhere (docstring keplerian.py:58)
    const bool ok = (e >= 0.0) && (e < 1.0);
    c.n = p[EXO_P_N]; c.tp = p[EXO_P_TP]; c.e = e;
    c.se = ok ? sqrt(1.0 - e) : __builtin_nan("");
    c.pe = sqrt(1.0 + e);
    c.sq1me2 = c.se * c.pe;
    c.isq1me2 = 1.0 / c.sq1me2;
    c.cw = p[EXO_P_COSW]; c.sw = p[EXO_P_SINW];
    c.ci = p[EXO_P_COSI]; c.si = p[EXO_P_SINI];
    c.aor = p[EXO_P_AOR]; c.ror = p[EXO_P_ROR]; c.iror = 1.0 / p[EXO_P_ROR];
    c.t0 = p[EXO_P_T0]; c.period = p[EXO_P_PERIOD]; c.iperiod = 1.0 / p[EXO_P_PERIOD];
    c.ts = p[EXO_P_TS]; c.te = p[EXO_P_TE];
    c.fr = p[EXO_P_FRATIO]; c.ts2 = p[EXO_P_TS2]; c.te2 = p[EXO_P_TE2];
    c.clr = p[EXO_P_CLIGHT];
    // classifier: accept if (x^2 + y^2) (a/R)^2 < (1 + ror + margin)^2 with the fp32 position error
    // bound of exo::orbit_pos_f32 folded into the margin (never a false negative)
    const double margin = 2e-3 + c.aor * 1.6e-3;   // 2x the 8e-4 bound of exo::orbit_pos_f32
    const double lim = (1.0 + c.ror + margin) / c.aor;
    c.ef = (float)e; c.omf = (float)(1.0 - e); c.sqf = (float)c.sq1me2;
    c.cwf = (float)c.cw; c.swf = (float)c.sw; c.cif = (float)c.ci;
    c.zsf = (float)c.si;
    c.thrf = (float)(lim * lim) * 1.00001f;
    c.zthrf = (float)(-margin / c.aor);
    const double lin = fmax(1.0 - c.ror - margin, 0.0) / c.aor;
    c.inthrf = (float)(lin * lin);
    if (windows) {
      const double* wv = windows + kWin * (draw * n_planet + tid);
      c.nrev = wv[0]; c.c0 = wv[1]; c.dmid = wv[2]; c.half[0] = wv[3]; c.half[1] = wv[4];
    }
    if (ttv) {
      const TtvRow row(*ttv, ttv_first + draw * n_planet + tid);
      const int nf = row.bin(__builtin_inf());   // the padding is +inf
      c.tfin = nf;
      c.te0 = row.edges[0];
      const double width = nf > 1 ? row.edges[nf - 1] - row.edges[0] : 0.0;
      c.tinv = width > 0.0 ? (double)(nf - 1) / width : 0.0;
    }
  }
  const int nld = secondary ? 6 : 3;
  if (ld && tid >= 64 && tid < 64 + nld) sh.c[tid - 64] = ld[draw * nld + (tid - 64)];
  if (tid >= 128 && tid < 128 + n_sub) {
    sh.sdt[tid - 128] = stencil_dt ? stencil_dt[tid - 128] : 0.0;
    sh.sw[tid - 128] = stencil_w ? stencil_w[tid - 128] : 1.0;
  }
  __syncthreads();
}

// a wave-uniform double pinned to scalar registers
__device__ __forceinline__ double uniform(double x) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  return __hiloint2double(hi, lo);
}

// The heavy kernel's view of one planet: the constants eval_sample touches, pinned to scalar
// registers (they are the same for every lane; read from LDS they would sit in ~50 vector
// registers for the whole block, next to the elliptic-integral code that needs them all).
struct PlanetS {
  double n, tp, e, se, pe, sq1me2, isq1me2, cw, sw, ci, si, aor, ror, iror, fr, clr;
  __device__ __forceinline__ explicit PlanetS(const PlanetConst& c)
      : n(uniform(c.n)), tp(uniform(c.tp)), e(uniform(c.e)), se(uniform(c.se)), pe(uniform(c.pe)),
        sq1me2(uniform(c.sq1me2)), isq1me2(uniform(c.isq1me2)), cw(uniform(c.cw)), sw(uniform(c.sw)),
        ci(uniform(c.ci)), si(uniform(c.si)), aor(uniform(c.aor)), ror(uniform(c.ror)), iror(uniform(c.iror)),
        fr(uniform(c.fr)), clr(uniform(c.clr)) {}
};

// Gradient accumulators of the heavy kernel live in LDS, one column per thread
// ([slot][thread]: consecutive threads hit consecutive banks).  They are touched only
// by samples that overlap the disk, and keeping 17 doubles out of the register file is
// what lets two waves share a SIMD next to the elliptic-integral code.
// `add` is the LDS's own fp64 adder (ds_add_f64, no return value): one instruction, nothing to wait for -- as a
// read-modify-write in the wave (ds_read, wait ~100 cycles, v_add, ds_write) the dozen accumulations of a sample cost
// the kernel more stalled cycles than the arithmetic of its Kepler solve.  A column belongs to one thread and the LDS
// executes a wave's operations in order: the sums are those of the sequential loop, bit for bit, run after run.
struct GradAcc {
  double* col;  // &lds[0][threadIdx.x]
  __device__ __forceinline__ void add(int slot, double v) const {
    __hip_atomic_fetch_add(col + slot * kBlock, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
};

// One (cadence, sub-exposure, planet) sample.  Returns the flux contribution F
// and, if GRAD, adds gw * dF/d(theta) into the LDS accumulator columns.
// LDELAY (EXO_FLAG_LIGHT_DELAY; keplerian.py:411-470 with z0 = 0): the body is seen where it was at
// tt - D.  With the relative orbit's line-of-sight position z, velocity vz and acceleration az at tt
// (a first Kepler solve; a -> -a, r = a (1 - e cos E), vz = n a sin i (e cos w + cos(w + f)) / sqrt(1 -
// e^2), az = -n^2 z / (1 - e cos E)^3) the reference's
//     D = (c / az) ((1 + vz / c) - sqrt((1 + vz / c)^2 - 2 az (z0 - z) / c^2)),   (z0 - z) / (c + vz) if |az| < 1e-10
// is evaluated in the algebraically identical form  D = 2 q / (c (w + s)),  q = z0 - z, w = 1 + vz / c,
// s = sqrt(w^2 - 2 az q / c^2): no cancellation, and the small-az branch is its limit.  An occultation
// is the transit of the flipped orbit (keplerian.py:779-804), whose relative position, velocity and
// acceleration are the negatives: sigma = -1 below.  The reverse sweep takes the cotangent of the
// retarded time (-n Mbar of the second solve) back through D and the first solve by hand.
// CHI2 (one planet, no occultation, no exposure stencil: the sample IS the cadence's flux): `gw` carries the observed
// value and c2w its weight on the way in; the cotangent of F is formed once F is known, 2 w (F - obs), so the value
// and the gradient of a white-noise misfit take ONE evaluation per cadence.
template <bool GRAD, bool SECONDARY, bool LDELAY = false, bool CHI2 = false>
__device__ __forceinline__ double eval_sample(double tt, const PlanetS& c, const double* cld,
                                              double gw, const GradAcc& acc, double c2w = 0.0) {
  // saved by the delay computation for its reverse sweep
  double ld_cx = 0, ld_sx = 0, ld_den = 0, ld_z = 0, ld_vz = 0, ld_az = 0, ld_w = 0, ld_s = 0, ld_D = 0, ld_sig = 1, ld_t = tt;
  if (LDELAY) {
    const exo::KeplerHalf k1 = exo::kepler_half(exo::mean_anomaly_reduced(tt, c.tp, c.n), c.e, c.se, c.pe);
    const double X2 = k1.X * k1.X, Y2 = k1.Y * k1.Y;
    ld_cx = X2 - Y2; ld_sx = 2.0 * k1.X * k1.Y; ld_den = X2 + Y2;
    const double y1 = -c.aor * (c.sw * ld_cx + c.cw * ld_sx);
    ld_z = -c.si * y1;
    const double iden = exo::fast_div(1.0, ld_den);
    const double cwf = (c.cw * ld_cx - c.sw * ld_sx) * iden;
    ld_vz = -c.n * c.aor * c.isq1me2 * c.si * (c.e * c.cw + cwf);
    ld_az = -c.n * c.n * ld_z * iden * iden * iden;
    ld_sig = (SECONDARY && ld_z < 0.0) ? -1.0 : 1.0;   // behind the star: the flipped orbit's delay
    const double q = -ld_sig * ld_z, ic = exo::fast_div(1.0, c.clr);
    ld_w = fma(ld_sig * ld_vz, ic, 1.0);
    ld_s = sqrt(fma(-2.0 * ld_sig * ld_az * q, ic * ic, ld_w * ld_w));
    ld_D = 2.0 * q * ic / (ld_w + ld_s);
    tt -= ld_D;
  }
  // not (tt - c.tp) * c.n: with BJD-sized times and t_periastron = O(1) the plain product's two roundings are 3e-9 rad,
  // which every gradient slot then carries in its ninth digit (tests/golden/lightcurve_mp.npz, bjd_times_tp_03)
  const double M = exo::mean_anomaly_reduced(tt, c.tp, c.n);
  const exo::KeplerHalf kh = exo::kepler_half(M, c.e, c.se, c.pe);
  const double X2 = kh.X * kh.X, Y2 = kh.Y * kh.Y;
  const double cx = X2 - Y2;            // (1 - e cos E) cos f = cos E - e
  const double sx = 2.0 * kh.X * kh.Y;  // (1 - e cos E) sin f = sqrt(1-e^2) sin E
  const double den = X2 + Y2;           // 1 - e cos E, without the cancellation at e -> 1
  // position relative to the star in units of R_star; the reference passes a = -self.a
  // (keplerian.py:540) and r = a (1-e^2)/(1+e cos f) = a (1 - e cos E)
  const double xo = -c.aor * cx, yo = -c.aor * sx;
  const double x1 = c.cw * xo - c.sw * yo;
  const double y1 = c.sw * xo + c.cw * yo;
  const double Ys = c.ci * y1;
  const double Z = -c.si * y1;
  const double b2 = x1 * x1 + Ys * Ys;
  const double lim = 1.0 + c.ror;
  const bool front = !(Z <= 0.0);  // NaN counts as in front so that NaN parameters propagate
  const bool behind = SECONDARY && (Z < 0.0);
  // NaN parameters must propagate: treat NaN b2 as active
  const bool act = (front || behind) && !(b2 >= lim * lim);
  if (!EXO_WAVE_ANY(act)) return 0.0;
  double ib;  // 1 / b, for the reverse sweep
  double b = exo::fast_sqrt_rs(b2, &ib);
  if (!(b2 > 0.0)) {  // centre of the disk (no direction: zero gradient through b), or NaN
    b = (b2 == 0.0) ? 0.0 : b2;
    ib = 0.0;
  }
  // transit: (b, ror) on the star; occultation: star of radius 1/ror passes in
  // front of the planet, in units of the planet radius (secondary_eclipse.py:56-58)
  const bool occ = SECONDARY && behind;
  const double bq = occ ? b * c.iror : b;
  const double rq = occ ? c.iror : c.ror;
  exo::SV sv;
  exo::quad_sv<GRAD>(act ? bq : 2.0 + rq, rq, sv);
  const double* cc = occ ? cld + 3 : cld;
  const double Fq = fma(sv.s0, cc[0], fma(sv.s1, cc[1], sv.s2 * cc[2])) - 1.0;
  double F;
  double wq = 1.0;  // dF/dFq
  if (SECONDARY) {
    const double inv = exo::fast_div(1.0, 1.0 + c.fr);
    wq = occ ? c.fr * inv : inv;
    F = act ? Fq * wq : 0.0;
  } else {
    F = act ? Fq : 0.0;
  }
  if (CHI2) gw = 2.0 * c2w * (F - gw);
  if (GRAD) {
    if (act) {
      const double gq = gw * wq;
      // limb-darkening coefficients
      const int o = occ ? 3 : 0;
      acc.add(kNG + o + 0, gq * sv.s0);
      acc.add(kNG + o + 1, gq * sv.s1);
      acc.add(kNG + o + 2, gq * sv.s2);
      double bbar_q = gq * fma(sv.db0, cc[0], fma(sv.db1, cc[1], sv.db2 * cc[2]));
      double rbar_q = gq * fma(sv.dr0, cc[0], fma(sv.dr1, cc[1], sv.dr2 * cc[2]));
      double bbar, rorbar;
      if (occ) {
        // bq = b / ror, rq = 1 / ror ; F = fr Fq / (1 + fr)
        bbar = bbar_q * c.iror;
        rorbar = -(bbar_q * b + rbar_q) * c.iror * c.iror;
        acc.add(G_FR, gw * Fq * (1.0 / ((1.0 + c.fr) * (1.0 + c.fr))));
      } else {
        bbar = bbar_q;
        rorbar = rbar_q;
        if (SECONDARY) acc.add(G_FR, -gw * Fq * (1.0 / ((1.0 + c.fr) * (1.0 + c.fr))));
      }
      acc.add(G_ROR, rorbar);
      const double x1bar = bbar * x1 * ib;
      const double Ysbar = bbar * Ys * ib;
      const double y1bar = Ysbar * c.ci;
      acc.add(G_COSI, Ysbar * y1);
      const double xobar = c.cw * x1bar + c.sw * y1bar;
      const double yobar = -c.sw * x1bar + c.cw * y1bar;
      acc.add(G_COSW, x1bar * xo + y1bar * yo);
      acc.add(G_SINW, -x1bar * yo + y1bar * xo);
      acc.add(G_AOR, -(xobar * cx + yobar * sx));
      const double cxbar = -c.aor * xobar, sxbar = -c.aor * yobar;
      // cx = cos E - e, sx = sqrt(1-e^2) sin E ; dE/dM = 1/den, dE/de = sin E/den
      // sin E, cos E back from (cx, sx) rather than from the half angles: two values live across the
      // solution vector instead of six
      const double sinE = sx * c.isq1me2;
      const double cosE = cx + c.e;
      const double iden = exo::fast_div(1.0, den);
      const double Ebar = fma(-sinE, cxbar, c.sq1me2 * cosE * sxbar);
      const double Mbar = Ebar * iden;
      acc.add(G_ECC, Mbar * sinE - cxbar - c.e * sinE * c.isq1me2 * sxbar);
      // d M / d n = t - tp: fl(tt - c.tp) is the leading part of mean_anomaly_reduced's split, good to one rounding
      // (relative 1e-16 of this term), so the cotangent needs no tail
      acc.add(G_N, Mbar * (tt - c.tp));
      acc.add(G_TP, -Mbar * c.n);
      if (LDELAY) {
        // tt = t_obs - D: Dbar = -(d / d tt) = -n Mbar; back through D = 2 q / (c (w + s))
        const double cl = c.clr, ic = 1.0 / cl;
        const double q = -ld_sig * ld_z, u = ld_w + ld_s;
        const double Dbar = -Mbar * c.n;
        double qbar = Dbar * 2.0 * ic / u;
        double clbar = -Dbar * ld_D * ic;
        const double ubar = -Dbar * ld_D / u;
        // s = sqrt(w^2 - 2 sig az q / c^2)
        const double discbar = ubar / (2.0 * ld_s);
        double wbar = ubar + discbar * 2.0 * ld_w;
        const double azbar = discbar * (-2.0 * ld_sig * q * ic * ic);
        qbar += discbar * (-2.0 * ld_sig * ld_az * ic * ic);
        clbar += discbar * (4.0 * ld_sig * ld_az * q * ic * ic * ic);
        // w = 1 + sig vz / c
        const double vzbar = wbar * ld_sig * ic;
        clbar -= wbar * ld_sig * ld_vz * ic * ic;
        acc.add(G_CL, clbar);
        // q = -sig z ;  az = -n^2 z / den^3
        const double id1 = 1.0 / ld_den, id3 = id1 * id1 * id1;
        double zbar = -ld_sig * qbar - azbar * c.n * c.n * id3;
        double nbar = -azbar * 2.0 * c.n * ld_z * id3;
        double denbar = azbar * 3.0 * c.n * c.n * ld_z * id3 * id1;
        // vz = vamp si P, vamp = -n a / sqrt(1 - e^2), P = e cw + cwf
        const double cwf = (c.cw * ld_cx - c.sw * ld_sx) * id1, Pq = c.e * c.cw + cwf;
        const double vamp = -c.n * c.aor * c.isq1me2;
        const double vampbar = vzbar * c.si * Pq, Pbar = vzbar * vamp * c.si;
        double sibar = vzbar * vamp * Pq;
        nbar += vampbar * (-c.aor * c.isq1me2);
        double aorbar = vampbar * (-c.n * c.isq1me2);
        // d(1/sqrt(1-e^2))/de = e / (1-e^2)^(3/2)
        double ebar = vampbar * (-c.n * c.aor) * c.e * c.isq1me2 * c.isq1me2 * c.isq1me2 + Pbar * c.cw;
        double cwbar = Pbar * c.e, swbar = 0.0;
        // cwf = (cw cx - sw sx) / den
        const double Nbar = Pbar * id1;
        denbar -= Pbar * cwf * id1;
        cwbar += Nbar * ld_cx; swbar -= Nbar * ld_sx;
        double cxbar1 = Nbar * c.cw, sxbar1 = -Nbar * c.sw;
        // z = -si y1 ;  y1 = -a (sw cx + cw sx)
        const double y1 = -c.aor * (c.sw * ld_cx + c.cw * ld_sx);
        sibar -= zbar * y1;
        const double y1bar = -zbar * c.si;
        aorbar -= y1bar * (c.sw * ld_cx + c.cw * ld_sx);
        swbar -= y1bar * c.aor * ld_cx; cwbar -= y1bar * c.aor * ld_sx;
        cxbar1 -= y1bar * c.aor * c.sw; sxbar1 -= y1bar * c.aor * c.cw;
        // first solve: cx = cos E - e, sx = sqrt(1-e^2) sin E, den = 1 - e cos E
        const double sinE1 = ld_sx * c.isq1me2, cosE1 = ld_cx + c.e;
        const double Ebar1 = -cxbar1 * sinE1 + sxbar1 * c.sq1me2 * cosE1 + denbar * c.e * sinE1;
        ebar += -cxbar1 - sxbar1 * c.e * c.isq1me2 * sinE1 - denbar * cosE1;
        const double Mbar1 = Ebar1 * id1;
        ebar += Mbar1 * sinE1;
        nbar += Mbar1 * (ld_t - c.tp);
        acc.add(G_TP, -Mbar1 * c.n);
        acc.add(G_N, nbar);
        acc.add(G_ECC, ebar);
        acc.add(G_COSW, cwbar);
        acc.add(G_SINW, swbar);
        acc.add(G_AOR, aorbar);
        acc.add(G_SINI, sibar);
      }
    }
  }
  return F;
}

// sum over the wave, valid in lane 63: row_shr 1/2/4/8 inside the rows of 16, then row_bcast 15 / 31
// (in-register DPP moves; a ds_bpermute butterfly costs an LDS round trip per step)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
  return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_last(double v) {
  v = dpp_add<0x111, 0xf>(v);
  v = dpp_add<0x112, 0xf>(v);
  v = dpp_add<0x114, 0xf>(v);
  v = dpp_add<0x118, 0xf>(v);
  v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}

// Reverse sweep of the warp: d L / d shift[k] is the sum over the samples of bin k of their
// d L / d t_periastron (both enter as t - shift - tp).  eval_sample leaves that sum in the lane's
// G_TP column; after every cadence it is moved to the bin and to the G_PAD column, which ends up
// holding the planet's total.  Each wave keeps kBinSlots bins in LDS (direct-mapped on the bin
// number: a block works through a run of consecutive cadences, i.e. a few transits; one lane per
// wave touches them, so plain loads and stores -- LDS fp64 atomics measured 100 us slower per
// sweep) and sends them to the output table with one hardware fp64 atomic each when the planet is
// done; a bin that finds its slot taken goes to the table directly.  The table is the one place
// where the summation order -- and with it the last bits -- depends on scheduling.
constexpr int kBinSlots = 16;
struct BinCache {
  double sum[kWaves][kBinSlots];
  int id[kWaves][kBinSlots];
};
struct TtvGrad {
  double* __restrict__ col;   // &lds_acc[0][threadIdx.x]
  double* __restrict__ grow;  // gshift row of this (draw, planet)
  BinCache* cache;
  __device__ __forceinline__ double take() const {
    const double d = col[G_TP * kBlock];
    col[G_TP * kBlock] = 0.0;
    col[G_PAD * kBlock] += d;
    return d;
  }
  // one lane on its own (its bin changed in the middle of an exposure)
  __device__ __forceinline__ void flush_lane(int k) const {
    const double d = take();
    if (d != 0.0) unsafeAtomicAdd(grow + k, d);
  }
  // The whole wave, after a cadence.  A wave holds 64 consecutive list entries, i.e. cadences of
  // one transit or of two neighbouring ones: one pass per distinct bin, each a wave sum and one
  // addition by the last lane.
  __device__ __forceinline__ void flush_wave(int k) const {
    const double d = take();
    unsigned long long todo = __ballot(d != 0.0);
    while (todo) {
      const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      const int k0 = __builtin_amdgcn_readlane(k, first);
      const bool mine = k == k0;
      const double sum = wave_sum_last(mine ? d : 0.0);
      todo &= ~__ballot(mine);
      // (wave number through a scalar register: an address built from threadIdx.x is kept by the
      // compiler across the whole loop -- in scratch, and a scratch reload waits for every load
      // in flight, the prefetched list entries included)
      const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), slot = k0 & (kBinSlots - 1);
      if ((threadIdx.x & 63) == 63) {
        const int owner = cache->id[w][slot];
        if (owner == k0) {
          cache->sum[w][slot] += sum;
        } else if (owner < 0) {
          cache->id[w][slot] = k0;
          cache->sum[w][slot] = sum;
        } else {
          unsafeAtomicAdd(grow + k0, sum);
        }
      }
    }
  }
  // Run-enumeration path, a list whose runs carry their bins: the wave's sums go to its own row of a [wave][run]
  // table in LDS (q = the lane's run within the batch; a wave holds cadences of one or two runs)
  __device__ __forceinline__ void flush_runs(int q, double* __restrict__ tab, int row_len) const {
    const double d = take();
    unsigned long long todo = __ballot(d != 0.0);
    while (todo) {
      const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      const int q0 = __builtin_amdgcn_readlane(q, first);
      const bool mine = q == q0;
      const double sum = wave_sum_last(mine ? d : 0.0);
      todo &= ~__ballot(mine);
      const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      if ((threadIdx.x & 63) == 63) tab[w * row_len + q0] += sum;
    }
  }
  // block-wide, between planets: bins -> output table
  __device__ __forceinline__ void drain() const {
    __syncthreads();
    if (threadIdx.x < kWaves * kBinSlots) {
      const int k = (&cache->id[0][0])[threadIdx.x];
      if (k >= 0) unsafeAtomicAdd(grow + k, (&cache->sum[0][0])[threadIdx.x]);
      (&cache->id[0][0])[threadIdx.x] = -1;
    }
    __syncthreads();
  }
};

// Sum the kBlock per-thread columns of accumulator slots [first, first + n) and write the n
// totals to out[0..n).  Two passes through LDS in a fixed order (bit-reproducible): thread
// (slot, c) adds the 16 columns c, c + 16, ..., then one thread per slot adds the 16 partials.
// A shuffle tree per slot costs 17 x 6 dependent cross-lane hops per block and was the bulk of
// the heavy kernel's per-block overhead.
__device__ __forceinline__ void reduce_columns(double (*acc)[kBlock], double (*red)[16], int first, int n,
    double* __restrict__ out) {
  __syncthreads();
  const int s = threadIdx.x >> 4, c = threadIdx.x & 15;
  if (s < n) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < kBlock / 16; ++i) v += acc[first + s][c + 16 * i];
    red[s][c] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < n) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) v += red[threadIdx.x][i];
    out[threadIdx.x] = v;
  }
  __syncthreads();
}

// Block partials -> gradients of one draw, by the `nthr` threads of one block (the list path's reduce kernel; finish_draw
// of the run-enumeration path).  A block's partials are n_planet x kNG compact slots, then the seven per-draw ones: limb
// darkening (three, or six with occultations) and sum(gflux * flux).  Record slots that carry no gradient (T0, PERIOD, the
// windows, the reserved ones) read 0; thread s sums slot s over the draw's nblk blocks IN BLOCK ORDER and stores it where
// it belongs.  `extra(k, v)`: called by the thread that summed per-draw slot k with its sum -- the sampled-mean / jitter
// likelihood keeps two sums of its own in the free slots 3 and 4.
// (No restrict on `partial`: transit_runs_kernel calls this on what it wrote itself.)
template <class Extra>
__device__ __forceinline__ void partials_to_gradients(int64_t draw, const double* partial, int nblk, int n_planet,
                                                      bool secondary, int nthr, double* gparams, double* gld,
                                                      double* flux_dot, Extra extra) {
  const int ng_draw = n_planet * kNG + 7;
  const int s = threadIdx.x;
  for (int q = s; q < n_planet * EXO_NPAR; q += nthr) {
    const int p = q / EXO_NPAR, slot = q % EXO_NPAR;
    const bool carried = slot == EXO_P_N || slot == EXO_P_TP || slot == EXO_P_ECC || slot == EXO_P_COSW ||
                         slot == EXO_P_SINW || slot == EXO_P_COSI || slot == EXO_P_AOR || slot == EXO_P_ROR ||
                         slot == EXO_P_FRATIO || slot == EXO_P_SINI || slot == EXO_P_CLIGHT;
    if (!carried) gparams[(draw * n_planet + p) * EXO_NPAR + slot] = 0.0;
  }
  if (s < ng_draw) {
    const double* src = partial + draw * nblk * (int64_t)ng_draw + s;
    double v = 0.0;
    for (int b = 0; b < nblk; ++b) v += src[(int64_t)b * ng_draw];
    if (s < n_planet * kNG) {
      const int p = s / kNG, k = s % kNG;
      // compact slot -> EXO_P_* slot
      const int map[kNG] = {EXO_P_N, EXO_P_TP, EXO_P_ECC, EXO_P_COSW, EXO_P_SINW,
                            EXO_P_COSI, EXO_P_AOR, EXO_P_ROR, EXO_P_FRATIO, -1, EXO_P_SINI, EXO_P_CLIGHT};
      if (map[k] >= 0) gparams[(draw * n_planet + p) * EXO_NPAR + map[k]] = v;
    } else {
      const int k = s - n_planet * kNG;
      const int nld = secondary ? 6 : 3;
      if (k < nld) gld[draw * nld + k] = v;
      if (k == 6 && flux_dot) flux_dot[draw] = v;
      extra(k, v);
    }
  }
}

// how far a sub-exposure can be from its cadence, in units of the exposure time: max |stencil_dt|
__device__ __forceinline__ double stencil_reach(const double* sdt, int n_sub) {
  double reach = 0.0;
  for (int k = 0; k < n_sub; ++k) reach = fmax(reach, fabs(sdt[k]));
  return reach;
}

}  // namespace
