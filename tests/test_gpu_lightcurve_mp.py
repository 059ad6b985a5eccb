"""GPU: the light-curve kernels of exo_transit.hip (its headers exo_transit_*.hpp: both paths and eval_sample), forward and reverse, against the multiprecision fixture
tests/golden/lightcurve_mp.npz (tools/make_lightcurve_golden.py) -- every route to the fixture, none merely to another
route: autograd on the two-sweep and on the Jacobian route, the one-sweep value + VJP (rows, cadence-major cotangent, exact
scan), transit_flux_dot, transit_chi2, the fused white-noise likelihood with a per-draw mean and jitter, the sparse sweep and
the sparse / merged model back to dense, contact windows, light delay, timing-variation tables with the cotangent of the
shift table, and a series made only of out-of-transit times.

The series of a unit is its t_in interleaved with its t_out and tiled to 600 cadences: three blocks of 256, the last ragged,
in-transit cadences in every block; as it comes (unsorted: every cadence is solved) or in time order (the run-enumeration
sweeps).  Three draws of the same record carry three different cotangents.  Tolerances: tests/lightcurve_mp_cases.py; the
unit of a VJP is the float64 oracle's own error on the same series and cotangent.  Every check prints its figures first.

(unit, route) pairs a route cannot express, by the route's documented rule (include/exoplanet_amd.h), are listed in
``inexpressible`` below and counted: at most 10 % of all pairs.
The two light-delay units have no oracle unit (oracle.numpy_port has no record-level light delay): their VJPs, sin i and
c / R_star included, are held at the floor 1e-13 alone.
User level: ops.pack_records (values and VJP, also at e = 1 - 1e-8 and 1 - 1e-6), the column route
(ops.orbit_flux_value_and_grad, ops.orbit_flux_dot) and the public KeplerianOrbit + LimbDarkLightCurve /
SecondaryEclipseLightCurve with backward(), against the fixture's jac_user / jac_cu (mpmath.diff of the constructor's algebra)."""
import numpy as np
import pytest
import torch

import lightcurve_mp_cases as K
from oracle import numpy_port as P

pytestmark = pytest.mark.gpu

N, D = 600, 3
UNITS = K.units()
IDS = [u[0] for u in UNITS]
ROUTES = ("autograd", "autograd_sorted", "autograd_jac", "vjp_cadence_major", "vjp_exact_scan", "flux_dot", "per_planet",
          "window", "sparse_sweep", "sparse_model", "chi2", "white_noise", "vouched_sorted", "pack", "cols_grad", "cols_dot",
          "public")
USER_ROUTES = ("pack", "cols_grad", "cols_dot", "public")


def inexpressible(unit, route):
    """why this route cannot carry this unit (None: it can)"""
    if route == "autograd_jac" and not unit.stencil:
        return "the Jacobian route starts at two samples per cadence (ops._JAC_MIN_SUB)"
    if unit.light_delay and route in ("vjp_exact_scan", "sparse_model"):
        return "light delay: run-enumeration sweeps only, no sparse mean (include/exoplanet_amd.h, ops.sparse_mean_supported)"
    if unit.light_delay and route == "window":
        return "light delay with use_in_transit=True is refused by get_light_curve"
    if unit.ttv is not None and route == "sparse_model":
        return "transit_flux_sparse_model takes no timing tables"
    if route in USER_ROUTES and unit.user is None:
        return "the entry is given by t_periastron: no (period, t0, b, ecc, omega, ...) call reproduces its record"
    if route in USER_ROUTES[1:] and unit.ttv is not None:
        return "the column route and KeplerianOrbit take no timing tables (TTVOrbit builds its own from transit times)"
    return None


def _units_for(route):
    g = K.load()
    keep = [u for u in UNITS if inexpressible(K.Unit(g, *u), route) is None]
    return dict(argnames="label,idx", argvalues=keep, ids=[u[0] for u in keep])


def test_inexpressible_pairs_are_few():
    """(needs no GPU: tests/test_lightcurve_mp_host.py runs it with the CPU suite as well)"""
    pairs = [(label, r) for label, idx in UNITS for r in ROUTES]
    g = K.load()
    out = [(label, r) for label, idx in UNITS for r in ROUTES if inexpressible(K.Unit(g, label, idx), r)]
    print("inexpressible pairs:", len(out), "of", len(pairs), out)
    assert len(out) <= 0.1 * len(pairs)


@pytest.fixture(scope="module")
def g():
    return K.load()


def T(a, dev, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev).requires_grad_(grad)


def inputs(unit, dev, grad=True, rec=None):
    """(params, ld, keyword arguments: the exposure stencil and the timing tables -- kw["ttv"][1] is the shift leaf)"""
    rec = unit.rec if rec is None else rec
    pt = T(np.repeat(rec, D, axis=0), dev, grad)
    ct = T(np.repeat(unit.c, D, axis=0), dev, grad)
    kw = {}
    if unit.stencil:
        kw = dict(texp=T([unit.stencil["texp"]], dev), stencil_dt=T(unit.stencil["stencil_dt"], dev),
                  stencil_w=T(unit.stencil["stencil_w"], dev))
    if unit.ttv is not None:
        kw["ttv"] = (T(np.repeat(unit.ttv[0], D, axis=0), dev), T(np.repeat(unit.ttv[1], D, axis=0), dev, grad))
    return pt, ct, kw


def leaves(pt, ct, kw):
    return (pt, ct) + ((kw["ttv"][1],) if "ttv" in kw else ())


def base_flags(unit):
    from exoplanet_amd import ops

    return (ops.FLAG_SECONDARY if unit.secondary else 0) | (ops.FLAG_LIGHT_DELAY if unit.light_delay else 0)


def judge(unit, route, t, pick, go, flux, gp, gl, per_planet=False, extra=None, gs=None):
    """flux [D, n(, P)] (or None), gp [D, P, NPAR], gl [D, nld] for cotangents go [D, n(, P)] against the fixture.
    ``extra`` [D, P, 9] / [D, nld]: what the route's own cotangent adds to the allowance (chi2, white noise).
    ``gs`` [D, 1, 3]: the cotangent of the shift table of a unit with timing variations."""
    gp, gl = np.asarray(gp.cpu() if torch.is_tensor(gp) else gp), np.asarray(gl.cpu() if torch.is_tensor(gl) else gl)
    if unit.ttv is not None and unit.grad:
        assert gs is not None, "a unit with timing tables must have its shift cotangent checked"
        gs = np.asarray(gs.cpu() if torch.is_tensor(gs) else gs)
    want_f, J, Jc = unit.expected(pick)
    tol_sum, tol_pp = unit.flux_tol(t, J)
    line = {}
    if flux is not None:
        want = want_f if per_planet else want_f.sum(axis=1)
        err = np.abs(flux - want[None])
        line["flux_error_over_tol"] = err / (tol_pp if per_planet else tol_sum)[None]
        out = pick < 0
        zero_ok = bool(np.all(flux[:, out] == 0.0))
    bad = []
    if unit.grad and gp is not None:
        slots = K.grad_slots(unit.light_delay)
        other = [k for k in range(P.NPAR) if k not in slots]
        exact0 = bool(np.all(gp[..., other] == 0.0))
        line.update(unit=0.0, vjp_error=0.0, vjp_error_over_tol=0.0)
        for d in range(D):
            wr, dr, wc, dc, zr, zc = K.want_vjp(unit, pick, go[d])
            ora = K.oracle_vjp(unit, t, go[d], per_planet=per_planet)
            if ora is None:          # (light delay: no oracle at record level, the floor alone)
                ur, uc = np.zeros_like(wr), np.zeros_like(wc)
            else:
                ur, uc = np.abs(ora[1] - wr) / dr, np.abs(ora[2] - wc) / dc
            tr, tc = K.vjp_tol(ur), K.vjp_tol(uc)
            if extra is not None:
                tr, tc = tr + extra[0][d] / dr, tc + extra[1][d] / dc
            rr, rc = np.abs(gp[d][:, slots] - wr) / dr, np.abs(gl[d] - wc) / dc
            line["unit"] = max(line["unit"], ur.max(), uc.max())
            line["vjp_error"] = max(line["vjp_error"], rr.max(), rc.max())
            line["vjp_error_over_tol"] = max(line["vjp_error_over_tol"], (rr / tr).max(), (rc / tc).max())
            if not (np.all(rr <= tr) and np.all(rc <= tc)):
                bad.append(("vjp", d, (rr / tr).tolist(), (rc / tc).tolist()))
            if not (np.all(gp[d][:, slots][zr] == 0.0) and np.all(gl[d][zc] == 0.0)):
                bad.append(("a slot with an identically zero Jacobian is not exactly 0", d))
            if unit.ttv is not None:
                g1 = go[d] if go[d].ndim == 1 else go[d][:, 0]
                ws, ds, zs = K.want_gshift(unit, t, pick, g1)
                us = np.abs(ora[3] - ws) / ds
                ts_ = K.vjp_tol(us) + (0.0 if extra is None else extra[2][d] / ds)
                rs = np.abs(gs[d, 0] - ws) / ds
                line["shift_vjp_error_over_tol"] = max(line.get("shift_vjp_error_over_tol", 0.0), (rs / ts_).max())
                if not (np.all(rs <= ts_) and np.all(gs[d, 0][zs] == 0.0)):
                    bad.append(("shift cotangent", d, (rs / ts_).tolist()))
        if not exact0:
            bad.append(("a slot that carries no gradient is not exactly 0",))
    K.report(f"{unit.label} / {route}", **line)
    if flux is not None:
        assert np.all(line["flux_error_over_tol"] <= 1.0), (unit.label, route, float(np.max(line["flux_error_over_tol"])))
        assert zero_ok, (unit.label, route, "flux at t_out is not exactly 0")
    assert not bad, (unit.label, route, bad[:3])


def cot(unit, route, n, per_planet=False):
    return K.cotangent(unit.label, route, (D, n, unit.P) if per_planet else (D, n))


# ------------------------------------------------------------------------------------------------------------------------
# autograd: two sweeps (unsorted and sorted series), the Jacobian route
# ------------------------------------------------------------------------------------------------------------------------
def _autograd(dev, unit, route, order, jac, flags=0, per_planet=False, rec=None):
    from exoplanet_amd import ops

    t, pick = unit.series(N, order)
    go = cot(unit, route, N, per_planet)
    pt, ct, kw = inputs(unit, dev, rec=rec)
    flags |= base_flags(unit) | (ops.FLAG_PER_PLANET if per_planet else 0)
    ops._JAC_ROUTE[0] = jac
    try:
        before = ops._JAC_CALLS[0]
        flux = ops.transit_flux(T(t, dev), pt, ct, flags=flags, **kw)
        assert (ops._JAC_CALLS[0] - before) == (1 if jac else 0)        # (the route under test is the one that ran)
        gp, gl, *gs = torch.autograd.grad(flux, leaves(pt, ct, kw), grad_outputs=T(go, dev))
    finally:
        ops._JAC_ROUTE[0] = True
    judge(unit, route, t, pick, go, flux.detach().cpu().numpy(), gp, gl, per_planet, gs=gs[0] if gs else None)


@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_autograd_two_sweeps(label, idx, dev, g):
    unit = K.Unit(g, label, idx)
    _autograd(dev, unit, "autograd", "interleaved", False)
    _autograd(dev, unit, "autograd_sorted", "sorted", False)
    _autograd(dev, unit, "per_planet", "sorted", False, per_planet=True)


@pytest.mark.parametrize("label,idx", [u for u in UNITS if "stencil" in u[0]], ids=[i for i in IDS if "stencil" in i])
def test_autograd_jacobian_route(label, idx, dev, g):
    unit = K.Unit(g, label, idx)
    assert inexpressible(unit, "autograd_jac") is None
    _autograd(dev, unit, "autograd_jac", "sorted", True)


def windowed(unit):
    """the unit's record with contact windows, as tests/test_gpu_transit.py::make_record(window=True) fills them"""
    rec = unit.rec.copy()
    r = rec[0]
    n, aor, ror, period = r[:, P.P_N], r[:, P.P_AOR], r[:, P.P_ROR], r[:, P.P_PERIOD]
    Ml, Mr, flag = P.contact_points(aor, r[:, P.P_ECC], r[:, P.P_COSW], r[:, P.P_SINW], r[:, P.P_COSI], r[:, P.P_SINI], 1 + ror)
    assert np.all(flag == 0)
    M0 = (r[:, P.P_T0] - r[:, P.P_TP]) * n
    hp = 0.5 * period
    ts = np.mod((Ml - M0) / n + hp, period) - hp
    te = np.mod((Mr - M0) / n + hp, period) - hp
    r[:, P.P_TS] = np.where(ts > 0, ts - period, ts)
    r[:, P.P_TE] = np.where(te < 0, te + period, te)
    return rec


@pytest.mark.parametrize(**_units_for("window"))
def test_contact_windows(label, idx, dev, g):
    """FLAG_WINDOW with the windows of make_record(window=True): the same flux and gradients (transits; an occultation
    keeps its +-inf window)"""
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    _autograd(dev, unit, "window", "sorted", False, flags=ops.FLAG_WINDOW, rec=windowed(unit))


# ------------------------------------------------------------------------------------------------------------------------
# one sweep: value + VJP, the dot product
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_value_and_vjp_and_dot(label, idx, dev, g):
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    pt, ct, kw = inputs(unit, dev, grad=False)
    # cotangent as [cadence][draw] (FLAG_CADENCE_MAJOR), sorted series
    t, pick = unit.series(N, "sorted")
    go = cot(unit, "vjp_cadence_major", N)
    gcm = T(go.T, dev).t()
    assert ops.is_cadence_major(gcm)
    flux, gp, gl, *gs = ops.transit_flux_value_and_vjp(T(t, dev), pt, ct, gcm, flags=base_flags(unit) | ops.FLAG_CADENCE_MAJOR, **kw)
    judge(unit, "vjp_cadence_major", t, pick, go, flux.cpu().numpy(), gp, gl, gs=gs[0] if gs else None)
    # exact scan, the series as it comes
    if not inexpressible(unit, "vjp_exact_scan"):
        t, pick = unit.series(N)
        go = cot(unit, "vjp_exact_scan", N)
        flux, gp, gl, *gs = ops.transit_flux_value_and_vjp(T(t, dev), pt, ct, T(go, dev),
                                                           flags=base_flags(unit) | ops.FLAG_EXACT_SCAN, **kw)
        judge(unit, "vjp_exact_scan", t, pick, go, flux.cpu().numpy(), gp, gl, gs=gs[0] if gs else None)
    # L = sum g f, differentiated
    t, pick = unit.series(N, "sorted")
    go = cot(unit, "flux_dot", N)
    pt, ct, kw = inputs(unit, dev)
    flux, L = ops.transit_flux_dot(T(t, dev), pt, ct, T(go, dev), flags=base_flags(unit), **kw)
    gp, gl, *gs = torch.autograd.grad(L.sum(), leaves(pt, ct, kw))
    judge(unit, "flux_dot", t, pick, go, flux.cpu().numpy(), gp, gl, gs=gs[0] if gs else None)
    want_f = unit.expected(pick)[0].sum(axis=1)
    tol_sum = unit.flux_tol(t, unit.expected(pick)[1])[0]
    Lw = (go.astype(np.longdouble) * want_f[None]).sum(axis=1)
    Ltol = (np.abs(go) * tol_sum[None]).sum(axis=1) + 16 * K.EPS * (np.abs(go) * np.abs(want_f)[None]).sum(axis=1)
    K.report(f"{label} / flux_dot L", error_over_tol=np.abs(L.detach().cpu().numpy() - Lw.astype(np.float64)) / Ltol)
    assert np.all(np.abs(L.detach().cpu().numpy() - Lw.astype(np.float64)) <= Ltol)


# ------------------------------------------------------------------------------------------------------------------------
# sparse
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_sparse_sweep(label, idx, dev, g):
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    pt, ct, kw = inputs(unit, dev, grad=False)
    go = cot(unit, "sparse_sweep", N)
    sp, gp, gl, dot, *gs = ops.transit_flux_sparse(T(t, dev), pt, ct, T(go, dev), flags=base_flags(unit), **kw)
    judge(unit, "sparse_sweep", t, pick, go, sp.to_dense(), gp, gl, gs=gs[0] if gs else None)


@pytest.mark.parametrize(**_units_for("sparse_model"))
def test_sparse_model_to_dense(label, idx, dev, g):
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    # the sparse model (one list per draw: the sweep's runs, or the merged form) back to dense, differentiated
    go = cot(unit, "sparse_model", N)
    pt, ct, kw = inputs(unit, dev)
    lc = ops.transit_flux_sparse_model(T(t, dev), pt, ct, flags=base_flags(unit), **kw)
    assert isinstance(lc, ops.MergedSparseLightCurve) == (unit.P > 1 or unit.secondary)
    dense = lc.dense()
    gp, gl = torch.autograd.grad(dense, (pt, ct), grad_outputs=T(go, dev))
    judge(unit, "sparse_model", t, pick, go, dense.detach().cpu().numpy(), gp, gl)


# ------------------------------------------------------------------------------------------------------------------------
# likelihoods: expected value and gradient from the fixture's F and J combined in np.longdouble
# ------------------------------------------------------------------------------------------------------------------------
def _noise_data(unit, route, want_f):
    rng = np.random.default_rng(K.seed(unit.label, route + "/data"))
    obs = want_f + 1e-2 * rng.normal(size=want_f.size)          # (|f - obs| ~ 1e-2 >> the flux allowance: see _extra)
    yerr = 1e-2 * rng.uniform(0.5, 2.0, size=want_f.size)
    return obs, yerr, rng


def _extra(unit, t, w2, tol_sum, J, Jc):
    """what the allowance of F adds to a VJP whose cotangent 2 w (F - obs) is formed from F: sum_n |2 w_n| tol_n |J_n|;
    w2 [D, n]"""
    out = (np.einsum("dn,npk->dpk", np.abs(w2) * tol_sum[None], np.abs(J)),
           np.einsum("dn,npk->dk", np.abs(w2) * tol_sum[None], np.abs(Jc)))
    if unit.ttv is not None:
        bins = np.searchsorted(unit.ttv[0][0, 0], t)
        term = np.abs(w2) * tol_sum[None] * np.abs(J[:, 0, K.COL_TP])[None]
        out += (np.stack([term[:, bins == k].sum(axis=1) for k in range(3)], axis=1),)
    return out


@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_chi2(label, idx, dev, g):
    """chi2[d] = sum_n w_n ((F_n - obs_n)^2 - obs_n^2) = sum_n w_n (F_n^2 - 2 F_n obs_n) (include/exoplanet_amd.h: the misfit
    relative to an empty light curve): |error| <= sum_n w_n 2 |F_n - obs_n| tol_n (the flux allowance carried through) +
    16 EPS sum_n w_n (|F_n| + |obs_n|)^2 (the roundings of the terms, in either form, and of their sum); the gradient is the
    VJP with g_n = 2 w_n (F_n - obs_n), allowed the usual max(16 unit, 1e-13) plus sum_n 2 w_n tol_n |J_n|"""
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    Fpp, J, Jc = unit.expected(pick)
    F = Fpp.sum(axis=1)
    tol_sum = unit.flux_tol(t, J)[0]
    obs, yerr, _ = _noise_data(unit, "chi2", F)
    w = 1.0 / yerr ** 2
    L = np.longdouble
    want = (w.astype(L) * ((F.astype(L) - obs) ** 2 - obs.astype(L) ** 2)).sum()
    tol = (w * 2 * np.abs(F - obs) * tol_sum).sum() + 16 * K.EPS * (w * (np.abs(F) + np.abs(obs)) ** 2).sum()
    gcot = np.repeat((2 * w * (F - obs))[None], D, axis=0)
    pt, ct, kw = inputs(unit, dev)
    chi2 = ops.transit_chi2(T(t, dev), pt, ct, T(obs, dev), T(w, dev), flags=base_flags(unit), **kw)
    gp, gl, *gs = torch.autograd.grad(chi2.sum(), leaves(pt, ct, kw))
    err = np.abs(chi2.detach().cpu().numpy() - float(want))
    K.report(f"{label} / chi2 value", error_over_tol=err / tol, relative_error=err / abs(float(want)))
    assert np.all(err <= tol)
    judge(unit, "chi2", t, pick, gcot, None, gp, gl, gs=gs[0] if gs else None,
          extra=_extra(unit, t, np.repeat((2 * w)[None], D, axis=0), tol_sum, J, Jc))


@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_white_noise_fused(label, idx, dev, g):
    """ll_d = -1/2 sum_n ((y_n - m_d - F_n)^2 / s_dn + log(2 pi s_dn)), s_dn = yerr_n^2 + jitter_d^2, with a per-draw mean and
    jitter (the fused route, ops.sampled_noise): value, d/d mean, d/d jitter, and the VJP of the record and c with
    g_dn = (y_n - m_d - F_n) / s_dn.  The library forms them relative to an empty light curve (include/exoplanet_amd.h:
    with r = y - m, w = 1 / s: ll = -(sum w r^2 + sum w (F^2 - 2 F r) + sum log(2 pi s)) / 2, d/d mean = sum w r - sum w F,
    d/d s = (sum w^2 r^2 + sum w^2 (F^2 - 2 F r) - sum w) / 2), so the allowance is 16 EPS times the sum of the absolute
    values of THOSE terms, plus the flux allowance carried through"""
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    Fpp, J, Jc = unit.expected(pick)
    F = Fpp.sum(axis=1)
    tol_sum = unit.flux_tol(t, J)[0]
    y, yerr, rng = _noise_data(unit, "white_noise", F)
    mean = rng.normal(size=D) * 3e-3
    jit = rng.uniform(0.3e-2, 1e-2, size=D)
    L = np.longdouble
    s = (yerr.astype(L) ** 2)[None] + (jit.astype(L) ** 2)[:, None]
    res = y.astype(L)[None] - mean.astype(L)[:, None] - F.astype(L)[None]
    terms = res ** 2 / s + np.log(2 * np.pi * s)
    want = -0.5 * terms.sum(axis=1)
    gres = (res / s).astype(np.float64)                                     # d ll / d F_n = d ll / d mean
    want_gm = (res / s).sum(axis=1)
    jterms = (res ** 2 / s ** 2 - 1 / s) * jit.astype(L)[:, None]
    want_gj = jterms.sum(axis=1)
    carried = (np.abs(gres) * tol_sum[None]).sum(axis=1)
    s64 = s.astype(np.float64)
    size = np.abs(y[None] - mean[:, None]) + np.abs(F)[None]                      # |r| + |F|
    tol_v = 16 * K.EPS * (size ** 2 / s64 + np.abs(np.log(2 * np.pi * s64))).sum(axis=1) / 2 + carried
    tol_m = 16 * K.EPS * (size / s64).sum(axis=1) + (tol_sum[None] / s64).sum(axis=1)
    tol_j = (16 * K.EPS * (size ** 2 / s64 ** 2 + 1 / s64).sum(axis=1)
             + (2 * np.abs(res / s ** 2).astype(np.float64) * tol_sum[None]).sum(axis=1)) * jit
    pt, ct, kw = inputs(unit, dev)
    mt, jt = T(mean, dev, True), T(jit, dev, True)
    assert ops.sampled_noise(mt, jt)
    ll = ops.white_noise_loglike(T(t, dev), pt, ct, T(y, dev), T(yerr, dev), mean=mt, jitter=jt, flags=base_flags(unit), **kw)
    gp, gl, gm, gj, *gs = torch.autograd.grad(ll.sum(), (pt, ct, mt, jt) + leaves(pt, ct, kw)[2:])
    figures = dict(value=np.abs(ll.detach().cpu().numpy() - want.astype(np.float64)) / tol_v,
                   d_mean=np.abs(gm.cpu().numpy() - want_gm.astype(np.float64)) / tol_m,
                   d_jitter=np.abs(gj.cpu().numpy() - want_gj.astype(np.float64)) / tol_j)
    K.report(f"{label} / white_noise error over tol", **figures)
    for k, v in figures.items():
        assert np.all(v <= 1.0), (label, k, v)
    judge(unit, "white_noise", t, pick, gres, None, gp, gl, gs=gs[0] if gs else None,
          extra=_extra(unit, t, 1 / s.astype(np.float64), tol_sum, J, Jc))


# ------------------------------------------------------------------------------------------------------------------------
# nothing but out-of-transit times
# ------------------------------------------------------------------------------------------------------------------------
def test_out_of_transit_series_is_exactly_zero(dev, g):
    """t_out tiled to 600 cadences through the two-sweep route (as it comes and sorted), the Jacobian route and the sparse
    sweep: flux and every cotangent exactly 0"""
    from exoplanet_amd import ops

    for label, idx in UNITS:
        unit = K.Unit(g, label, idx)
        t, pick = unit.series(N, "out")
        go = cot(unit, "out", N)
        for order in ("as it comes", "sorted"):
            tt = np.sort(t) if order == "sorted" else t
            for jac in ([False, True] if unit.stencil else [False]):
                pt, ct, kw = inputs(unit, dev)
                ops._JAC_ROUTE[0] = jac
                try:
                    flux = ops.transit_flux(T(tt, dev), pt, ct, flags=base_flags(unit), **kw)
                    grads = torch.autograd.grad(flux, leaves(pt, ct, kw), grad_outputs=T(go, dev))
                finally:
                    ops._JAC_ROUTE[0] = True
                assert bool((flux == 0).all()) and all(bool((x == 0).all()) for x in grads), (label, order, jac)
        pt, ct, kw = inputs(unit, dev, grad=False)
        sp, *rest = ops.transit_flux_sparse(T(np.sort(t), dev), pt, ct, T(go, dev), flags=base_flags(unit), **kw)
        assert np.all(sp.to_dense() == 0) and all(bool((x == 0).all()) for x in rest), label


# ------------------------------------------------------------------------------------------------------------------------
# FLAG_SORTED_TIMES on the caller's word (ops.vouch_sorted)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,idx", UNITS, ids=IDS)
def test_vouched_sorted_series(label, idx, dev, g):
    """the time-ordered series vouched for with ops.vouch_sorted: the sweeps carry FLAG_SORTED_TIMES (windows and runs in
    one launch) on the caller's word; autograd and the one-sweep value + VJP with the flag also passed explicitly"""
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    tt = ops.vouch_sorted(T(t, dev))
    try:
        assert ops._sorted_flag(tt) == ops.FLAG_SORTED_TIMES
        go = cot(unit, "vouched_sorted", N)
        pt, ct, kw = inputs(unit, dev)
        flux = ops.transit_flux(tt, pt, ct, flags=base_flags(unit) | ops.FLAG_SORTED_TIMES, **kw)
        gp, gl, *gs = torch.autograd.grad(flux, leaves(pt, ct, kw), grad_outputs=T(go, dev))
        judge(unit, "vouched_sorted autograd", t, pick, go, flux.detach().cpu().numpy(), gp, gl, gs=gs[0] if gs else None)
        pt, ct, kw = inputs(unit, dev, grad=False)
        flux, gp, gl, *gs = ops.transit_flux_value_and_vjp(tt, pt, ct, T(go, dev), flags=base_flags(unit) | ops.FLAG_SORTED_TIMES, **kw)
        judge(unit, "vouched_sorted value+vjp", t, pick, go, flux.cpu().numpy(), gp, gl, gs=gs[0] if gs else None)
    finally:
        ops.release_sorted(tt)


# ------------------------------------------------------------------------------------------------------------------------
# user level
# ------------------------------------------------------------------------------------------------------------------------
def pack_flags(unit):
    from exoplanet_amd import ops

    return (K.EXO_PACK_CIRCULAR if unit.user["circular"] else 0) | (ops.FLAG_SECONDARY if unit.secondary else 0)


def _check_pack(dev, label, inp, u, rec11, c, jac, jac_cu, flags, light_delay):
    """ops.pack_records on inp [1, P, 10], u [1, 2|4]: the record's slots against rec11 [P, 11] (pack_value_tol), c (8 EPS of
    the component), and the VJP of a seeded cotangent on those slots against jac [P, 11, 10] / jac_cu: no float64 oracle of
    the packing's reverse pass exists, so the floor alone, 1e-13 of sum |g_s d slot_s / d input|; exact zeros where the
    Jacobian is identically 0"""
    from exoplanet_amd import ops

    oi, ui = T(np.repeat(inp, D, axis=0), dev, True), T(np.repeat(u, D, axis=0), dev, True)
    params, ld = ops.pack_records(oi, ui, flags=flags)
    got = params.detach().cpu().numpy()[0][:, list(K.REC_COLS)]
    want = rec11.copy()
    want[:, 10] = float(P.c_light) / inp[0, :, 7]                    # (packed for every record, read only with light delay)
    tol = K.pack_value_tol(want, inp[0])
    ratio = np.abs(got - want) / np.where(tol > 0, tol, 1.0)
    rc = np.abs(ld.detach().cpu().numpy()[0] - c) / (8 * K.EPS * np.abs(c))
    assert np.array_equal(params.detach().cpu().numpy()[0][:, [P.P_T0, P.P_PERIOD]], inp[0][:, [1, 0]])
    grec = K.cotangent(label, "pack", (D, inp.shape[1], 11))
    if not light_delay:
        grec[..., 9:] = 0.0                                           # (sin i and c / R_star carry cotangents with light delay only)
    gc = K.cotangent(label, "pack/c", (D, c.size))
    full = np.zeros((D, inp.shape[1], P.NPAR))
    full[..., list(K.REC_COLS)] = grec
    go, gu = torch.autograd.grad([params, ld], [oi, ui], grad_outputs=[T(full, dev), T(gc, dev)])
    go, gu = go.cpu().numpy(), gu.cpu().numpy()
    worst = 0.0
    bad = []
    for d in range(D):
        w, den, z, wu, du, zu = K.want_user_vjp(grec[d], gc[d], jac, jac_cu)
        r, ru = np.abs(go[d] - w) / den, np.abs(gu[d] - wu[:gu.shape[1]]) / du[:gu.shape[1]]
        worst = max(worst, r.max(), ru.max())
        if not (np.all(r <= K.VJP_FLOOR) and np.all(ru <= K.VJP_FLOOR)):
            bad.append((d, (r / K.VJP_FLOOR).tolist(), (ru / K.VJP_FLOOR).tolist()))
        if not (np.all(go[d][z] == 0.0) and np.all(gu[d][zu[:gu.shape[1]]] == 0.0)):
            bad.append((d, "an input with an identically zero Jacobian is not exactly 0"))
    K.report(f"{label} / pack", value_error_over_tol=ratio, c_error_over_tol=rc, vjp_error=worst, vjp_error_over_floor=worst / K.VJP_FLOOR)
    assert np.all(np.abs(got - want) <= tol), (label, ratio.max(axis=0))
    assert np.all(rc <= 1.0)
    assert not bad, (label, bad[:2])


@pytest.mark.parametrize(**_units_for("pack"))
def test_pack_records(label, idx, dev, g):
    unit = K.Unit(g, label, idx)
    rec11 = unit.rec[0][:, list(K.REC_COLS)]
    _check_pack(dev, label, unit.user["inp"], unit.user["u"], rec11, unit.c[0], unit.user["jac"], unit.user["jac_cu"],
                pack_flags(unit), unit.light_delay)


def test_pack_records_near_parabolic(dev, g):
    """e = 1 - 1e-8 and 1 - 1e-6, where a rounded e * e would put 1e-8 / 1e-10 into 1 - e^2 and so into cos i and the whole
    d / d e row.  (The header forms (1 - e)(1 + e); a compiler that contracts 1 - e * e into one fma gets the same digits, so
    this test holds the result, not the spelling.)"""
    for k in range(g["pk_in"].shape[0]):
        _check_pack_orbit(dev, f"near_parabolic_{k}", g["pk_in"][k][None, None], g["pk_u"][k][None], g["pk_rec"][k][None],
                          g["pk_jac"][k][None])


def _check_pack_orbit(dev, label, inp, u, rec11, jac):
    """the orbit half of _check_pack (the limb darkening of these entries is not in the fixture)"""
    from exoplanet_amd import ops

    oi, ui = T(np.repeat(inp, D, axis=0), dev, True), T(np.repeat(u, D, axis=0), dev)
    params, ld = ops.pack_records(oi, ui, flags=0)
    got = params.detach().cpu().numpy()[0][:, list(K.REC_COLS)]
    tol = K.pack_value_tol(rec11, inp[0])
    ratio = np.abs(got - rec11) / np.where(tol > 0, tol, 1.0)
    grec = K.cotangent(label, "pack", (D, 1, 11))
    grec[..., 9:] = 0.0
    full = np.zeros((D, 1, P.NPAR))
    full[..., list(K.REC_COLS)] = grec
    (go,) = torch.autograd.grad(params, oi, grad_outputs=T(full, dev))
    go = go.cpu().numpy()
    worst = 0.0
    for d in range(D):
        w, den, z, _, _, _ = K.want_user_vjp(grec[d], np.zeros(3), jac, np.zeros((6, 4)))
        worst = max(worst, (np.abs(go[d] - w) / den).max())
        assert np.all(go[d][z] == 0.0), (label, "an input with an identically zero Jacobian is not exactly 0")
    K.report(f"{label} / pack", e=inp[0, 0, 3], value_error_over_tol=ratio, vjp_error=worst, vjp_error_over_floor=worst / K.VJP_FLOOR)
    assert np.all(np.abs(got - rec11) <= tol), (label, ratio)
    assert worst <= K.VJP_FLOOR, (label, worst)


def _user_expectation(unit, t, pick, go, per_planet=False):
    """per draw: (wanted d / d inputs [P, 10], allowance [P, 10], wanted d / d u, allowance) of a user-level route: the
    fixture's record-level VJP carried through jac_user / jac_cu; allowance = what the record-level VJP is allowed,
    max(16 unit, 1e-13) of its terms, plus the oracle's sensitivity of that VJP to the roundings of the device's own packed
    record (lightcurve_mp_cases.record_sensitivity), both carried through |jac_user|, plus the floor on the chain's own sum"""
    ns = 11 if unit.light_delay else 9
    J, Jcu = unit.user["jac"][:, :ns, :], unit.user["jac_cu"]
    wr, dr, wc, dc, _, _ = K.want_vjp(unit, pick, go)
    ora = K.oracle_vjp(unit, t, go, per_planet=per_planet)
    if ora is None:          # (light delay: no oracle unit at record level, the floor alone -- as in judge())
        ur, uc = np.zeros_like(wr), np.zeros_like(wc)
    else:
        ur, uc = np.abs(ora[1] - wr) / dr, np.abs(ora[2] - wc) / dc
    sr, sc = K.record_sensitivity(unit, t, go, per_planet)
    if unit.light_delay:
        # sin i and c / R_star carry g . dF/dt times d delay / d slot: as sensitive to the record's roundings as the
        # t_periastron column, which is g . dF/dt too -- the same fraction of their own terms
        sr = np.concatenate([sr, dr[:, 9:] * (sr[:, 1:2] / dr[:, 1:2])], axis=1)
    ar, ac = K.vjp_tol(ur) * dr * (np.abs(wr) > 0) + sr, K.vjp_tol(uc) * dc * (np.abs(wc) > 0) + sc
    want = np.einsum("ps,psk->pk", wr, J)
    den = np.einsum("ps,psk->pk", dr * (np.abs(wr) > 0), np.abs(J))
    tol = np.einsum("ps,psk->pk", ar, np.abs(J)) + K.VJP_FLOOR * den
    n = wc.size
    wu = wc @ Jcu[:n]
    tu = ac @ np.abs(Jcu[:n]) + K.VJP_FLOOR * ((dc * (np.abs(wc) > 0)) @ np.abs(Jcu[:n]))
    return want, tol, wu, tu


def _user_flux_tol(unit, t, J):
    rec11 = unit.rec[0][:, list(K.REC_COLS)]
    ns = J.shape[2]                                   # (9, or 11 with light delay: sin i and c / R_star too)
    slot_tol = K.pack_value_tol(rec11, unit.user["inp"][0])[:, :ns]
    return unit.flux_tol(t, J)[1] + np.einsum("ps,nps->np", slot_tol, np.abs(J))


def _cols(unit, dev, grad):
    inp, u = unit.user["inp"][0], unit.user["u"][0]                 # [P, 10], [2 | 4]
    cols = [T(np.repeat(inp[None, :, k], D, axis=0), dev, grad) for k in range(10)]
    if unit.user["circular"]:
        cols[3] = cols[4] = None
    if not unit.secondary:
        cols[9] = None
    lcols = [T(np.full(D, v), dev, grad) for v in u]
    return cols, lcols


def _judge_user(unit, route, t, pick, go, flux, gcols, glcols):
    """flux [D, n] and the gradients per orbit column [D, P] (None: no such column) / per limb-darkening column [D]"""
    want_f, J, _ = unit.expected(pick)
    ftol = _user_flux_tol(unit, t, J).sum(axis=1)
    rf = np.abs(flux - want_f.sum(axis=1)[None]) / ftol[None]
    worst = worst_u = 0.0
    bad = []
    if unit.grad:
        for d in range(flux.shape[0]):
            want, tol, wu, tu = _user_expectation(unit, t, pick, go[d])
            for k, gk in enumerate(gcols):
                if gk is None:
                    continue
                r = np.abs(gk[d] - want[:, k]) / np.where(tol[:, k] > 0, tol[:, k], 1.0)
                r = np.where((tol[:, k] == 0) & (gk[d] == want[:, k]), 0.0, r)
                worst = max(worst, r.max())
                if not np.all(np.abs(gk[d] - want[:, k]) <= tol[:, k]):
                    bad.append((K.USER_NAMES[k], d, r.tolist()))
            for k, gk in enumerate(glcols):
                r = abs(gk[d] - wu[k]) / (tu[k] if tu[k] > 0 else 1.0)
                worst_u = max(worst_u, r)
                if not abs(gk[d] - wu[k]) <= tu[k]:
                    bad.append((f"u{k}", d, r))
    K.report(f"{unit.label} / {route}", flux_error_over_tol=rf, user_vjp_error_over_tol=worst, u_vjp_error_over_tol=worst_u)
    assert np.all(rf <= 1.0), (unit.label, route, float(rf.max()))
    assert np.all(flux[:, pick < 0] == 0.0)
    assert not bad, (unit.label, route, bad[:4])


@pytest.mark.parametrize(**_units_for("cols_grad"))
def test_column_route(label, idx, dev, g):
    """ops.orbit_flux_value_and_grad and ops.orbit_flux_dot: the records are packed inside the sweep, the gradients come back
    per input column"""
    from exoplanet_amd import ops

    unit = K.Unit(g, label, idx)
    t, pick = unit.series(N, "sorted")
    _, _, kw = inputs(unit, dev, grad=False)
    go = cot(unit, "cols_grad", N)
    cols, lcols = _cols(unit, dev, False)
    flux, L, gcols, glcols = ops.orbit_flux_value_and_grad(T(t, dev), T(go, dev), cols, lcols, flags=base_flags(unit),
                                                           pack_flags=pack_flags(unit), **kw)
    _judge_user(unit, "cols_grad", t, pick, go, flux.cpu().numpy(), [None if x is None else x.cpu().numpy() for x in gcols],
                [x.cpu().numpy() for x in glcols])
    go = cot(unit, "cols_dot", N)
    cols, lcols = _cols(unit, dev, True)
    flux, L = ops.orbit_flux_dot(T(t, dev), T(go, dev), cols, lcols, flags=base_flags(unit), pack_flags=pack_flags(unit), **kw)
    leaf = [c for c in cols if c is not None] + lcols
    grads = list(torch.autograd.grad(L.sum(), leaf))
    gcols = [None if c is None else grads.pop(0).cpu().numpy() for c in cols]
    _judge_user(unit, "cols_dot", t, pick, go, flux.cpu().numpy(), gcols, [x.cpu().numpy() for x in grads])


@pytest.mark.parametrize(**_units_for("public"))
def test_public_classes(label, idx, dev, g):
    """KeplerianOrbit(period, t0, b, ecc, omega, m_star, r_star, m_planet) + LimbDarkLightCurve(u1, u2).get_light_curve /
    SecondaryEclipseLightCurve, total flux, backward() to every leaf (one draw)"""
    import exoplanet_amd as xo

    unit = K.Unit(g, label, idx)
    s = K.SYSTEMS[idx[0]]
    t, pick = unit.series(N, "sorted")
    go = K.cotangent(label, "public", (1, N))
    inp, u = unit.user["inp"][0], unit.user["u"][0]
    names = ["period", "t0", "b", "ecc", "omega", "r", "m_star", "r_star", "m_planet", "sbr"]
    S = lambda v: torch.tensor(float(v), dtype=torch.float64, device=dev, requires_grad=True)  # noqa: E731
    leaf = {n: T(inp[:, k], dev, True) for k, n in enumerate(names)}
    leaf["m_star"], leaf["r_star"] = S(inp[0, 6]), S(inp[0, 7])
    kw = {n: leaf[n] for n in ("period", "t0", "b", "m_star", "r_star", "m_planet")}
    if not unit.user["circular"]:
        kw.update(ecc=leaf["ecc"], omega=leaf["omega"])
    orbit = xo.KeplerianOrbit(**kw)
    ul = [S(v) for v in u]
    if unit.secondary:
        sbr = S(inp[0, 9])
        lc = xo.SecondaryEclipseLightCurve((ul[0], ul[1]), (ul[2], ul[3]), sbr)
    else:
        lc = xo.LimbDarkLightCurve(ul[0], ul[1])
    ekw = dict(texp=s["stencil"][0], oversample=s["stencil"][1], order=s["stencil"][2]) if s["stencil"] else {}
    if unit.light_delay:
        ekw["light_delay"] = True
    flux = lc.get_light_curve(orbit=orbit, r=leaf["r"], t=T(t, dev), total=True, **ekw)
    flux = flux.reshape(1, N)
    flux.backward(T(go, dev))
    gcols = []
    for k, n in enumerate(names):
        x = sbr if (n == "sbr" and unit.secondary) else leaf[n]
        if x.grad is None:
            # only a leaf that was never handed over may come back without a gradient
            assert (n in ("ecc", "omega") and unit.user["circular"]) or (n == "sbr" and not unit.secondary), (label, n)
            gcols.append(None)
            continue
        gr = x.grad.cpu().numpy()
        if n in ("m_star", "r_star", "sbr"):
            gcols.append(None)            # (one leaf shared by the planets: checked below as the sum over the planets)
            leaf[n + "_grad"] = float(gr)
        else:
            gcols.append(gr.reshape(1, -1))
    _judge_user(unit, "public", t, pick, go, flux.detach().cpu().numpy(), gcols, [x.grad.cpu().numpy().reshape(1) for x in ul])
    if unit.grad:
        want, tol, _, _ = _user_expectation(unit, t, pick, go[0])
        for n, k in (("m_star", 6), ("r_star", 7)) + ((("sbr", 9),) if unit.secondary else ()):
            got = leaf[n + "_grad"]
            assert abs(got - want[:, k].sum()) <= tol[:, k].sum(), (label, n, got, want[:, k].sum(), tol[:, k].sum())
