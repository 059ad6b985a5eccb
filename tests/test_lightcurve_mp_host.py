"""CPU: the light-curve oracle (oracle.numpy_port.transit_flux / transit_flux_vjp and the C port's transit) against the
multiprecision fixture tests/golden/lightcurve_mp.npz (tools/make_lightcurve_golden.py): flux and the derivative to every
gradient slot of the record and to the limb-darkening vector, at e up to 0.995, omega = +-fl(pi/2), 0, fl(pi), b = 0 exactly and beside it, grazing, r / R up to 1.2, three planets of one star summed and per planet,
occultations, the three exposure stencils, three transits with timing variations (and the cotangent of the shift table),
BJD-sized times with t_periastron beside them and at 0.3; the light-delay entries through numpy_port's classes, flux only
(the oracle has no record-level light delay: their gradients are held on the GPU alone, at the floor).
Tolerances: tests/lightcurve_mp_cases.py (derived there).  Every test prints its figures before it asserts.

User level: numpy_port.KeplerianOrbit + get_cl from the table's inputs against the fixture's record and c, the flux of
numpy_port's classes from those inputs, and the port's record-level VJP carried through the fixture's jac_user / jac_cu.
The cap on inexpressible (unit, route) pairs of tests/test_gpu_lightcurve_mp.py is asserted here too."""
import numpy as np
import pytest

import lightcurve_mp_cases as K
from oracle import c_port as C
from oracle import numpy_port as P

UNITS = K.units()


@pytest.fixture(scope="module")
def g():
    return K.load()


def _eval(impl, unit, t, go, per_planet):
    """(flux [n(, P)], gparams [P, 9], gld [nld]) of one implementation on the unit's record"""
    if impl == "numpy":
        return K.oracle_vjp(unit, t, go, per_planet=per_planet)
    if unit.ttv is not None:
        fl, gp, gl, gs = C.transit_ttv(t, unit.rec, unit.c, unit.ttv, go[None], per_planet=per_planet, **unit.stencil)
        return fl[0], gp[0][:, K.grad_slots()], gl[0], gs[0, 0]
    fl, gp, gl = C.transit(t, unit.rec, unit.c, go[None], per_planet=per_planet, secondary=unit.secondary, **unit.stencil)
    return fl[0], gp[0][:, K.grad_slots()], gl[0]


RECORD_UNITS = [u for u in UNITS if not K.SYSTEMS[u[1][0]]["light_delay"]]
DELAY_UNITS = [u for u in UNITS if K.SYSTEMS[u[1][0]]["light_delay"]]


def test_table_and_fixture_agree(g):
    assert g["rec"].shape == (len(K.SYSTEMS), P.NPAR) and g["t_in"].shape == (len(K.SYSTEMS), K.N_IN)
    assert K.SLOT_NAMES == tuple(n for n in ("n", "tp", "ecc", "cosw", "sinw", "cosi", "aor", "ror", "fratio"))
    assert K.grad_slots() == [P.P_N, P.P_TP, P.P_ECC, P.P_COSW, P.P_SINW, P.P_COSI, P.P_AOR, P.P_ROR, P.P_FRATIO]
    for i, s in enumerate(K.SYSTEMS):
        assert bool(g["grad"][i]) == s["grad"] and bool(g["secondary"][i]) == (s["sbr"] is not None)
        assert g["flux"][i].min() < -1e-4
        assert abs(g["rec"][i, P.P_COSI]) < 1
    assert all(s["grad"] for s in K.SYSTEMS)          # (every entry carries its Jacobian, e = 0.995 included)
    assert len(DELAY_UNITS) == 2 and sum(1 for s in K.SYSTEMS if s["ttv"]) == 1


@pytest.mark.parametrize("impl", ["numpy", "c"])
@pytest.mark.parametrize("label,idx", RECORD_UNITS, ids=[u[0] for u in RECORD_UNITS])
def test_flux_and_vjp(impl, label, idx, g):
    """t_in followed by t_out, per planet and (for a group) summed: flux per cadence, exact zeros at t_out, and the VJP per
    (planet, slot) and per component of c; the condition on the inputs (unit <= UNIT_CEILING) for every gradient system"""
    unit = K.Unit(g, label, idx)
    t = np.concatenate([unit.t_in, unit.t_out])
    pick = np.concatenate([np.arange(K.N_IN), np.full(K.N_OUT, -1)])
    want_f, J, Jc = unit.expected(pick)
    tol_sum, tol_pp = unit.flux_tol(t, J)
    for per_planet in ([True, False] if unit.P > 1 else [True]):
        route = "host/per_planet" if per_planet else "host/summed"
        go = K.cotangent(label, route, (t.size, unit.P) if per_planet else (t.size,))
        fl, gp, gl, *gs = _eval(impl, unit, t, go, per_planet)
        err = np.abs(fl - (want_f if per_planet else want_f.sum(axis=1)))
        ratio = err / (tol_pp if per_planet else tol_sum)
        K.report(f"flux[{impl}] {label} {route}", worst_error=err, worst_error_over_tol=ratio)
        assert np.all(ratio <= 1.0), (label, float(ratio.max()))
        assert np.all(fl[K.N_IN:] == 0.0)
        if not unit.grad:
            continue
        _, ugp, ugl, *ugs = K.oracle_vjp(unit, t, go, per_planet=per_planet)
        wr, dr, wc, dc, zr, zc = K.want_vjp(unit, pick, go)
        unit_r, unit_c = np.abs(ugp - wr) / dr, np.abs(ugl - wc) / dc
        rr, rc = np.abs(gp - wr) / dr, np.abs(gl - wc) / dc
        K.report(f"vjp[{impl}] {label} {route}", unit=max(unit_r.max(), unit_c.max()), error=max(rr.max(), rc.max()),
                 error_over_tol=max((rr / K.vjp_tol(unit_r)).max(), (rc / K.vjp_tol(unit_c)).max()))
        # the condition on the inputs: a float64 evaluation of this system is this well determined
        assert unit_r.max() <= K.UNIT_CEILING and unit_c.max() <= K.UNIT_CEILING, (label, unit_r.max(), unit_c.max())
        assert np.all(rr <= K.vjp_tol(unit_r)), (label, rr)
        assert np.all(rc <= K.vjp_tol(unit_c)), (label, rc)
        assert np.all(gp[zr] == 0.0) and np.all(gl[zc] == 0.0), (label, gp[zr], gl[zc])
        if unit.ttv is not None:
            ws, ds, _ = K.want_gshift(unit, t, pick, go[:, 0])
            unit_s, rs = np.abs(ugs[0] - ws) / ds, np.abs(gs[0] - ws) / ds
            K.report(f"shift cotangent[{impl}] {label}", unit=unit_s, error=rs, error_over_tol=rs / K.vjp_tol(unit_s))
            assert unit_s.max() <= K.UNIT_CEILING and np.all(rs <= K.vjp_tol(unit_s)), (label, rs)


@pytest.mark.parametrize("impl", ["numpy", "c"])
def test_out_of_transit_series_is_all_zero(impl, g):
    """a series made only of t_out: flux exactly 0, every cotangent exactly 0"""
    for label, idx in RECORD_UNITS:
        unit = K.Unit(g, label, idx)
        go = K.cotangent(label, "host/out", (K.N_OUT,))
        fl, gp, gl, *gs = _eval(impl, unit, unit.t_out, go, False)
        assert np.all(fl == 0.0) and np.all(gp == 0.0) and np.all(gl == 0.0) and all(np.all(x == 0.0) for x in gs), label


@pytest.mark.parametrize("label,idx", DELAY_UNITS, ids=[u[0] for u in DELAY_UNITS])
def test_light_delay_flux_end_to_end(label, idx, g):
    """numpy_port.KeplerianOrbit + LimbDarkLightCurve / SecondaryEclipseLightCurve .get_light_curve(light_delay=True) from the
    table's user inputs against the fixture's flux (a function of the fixture's own float64 record).  The class forms its
    own record, every slot rounded once: the allowance is the record-level one plus EPS (|t0| + |M0 / n|) |dF/dtp| for the
    stored t_periastron plus EPS sum over the other slots of |slot dF/dslot| (one rounding of each), from the fixture's
    Jacobian -- plus what the reference's own form of the delay (keplerian.py:451-462, which the port restates as it
    stands) loses: (c / az) ((1 + vz / c) - sqrt((1 + vz / c)^2 - ...)) subtracts two numbers of size 1, so the delay carries
    2 EPS c / |az| days, which |dF/dt| = |dF/dtp| multiplies.  (The kernel evaluates the algebraically identical
    2 q / (c (w + s)), without the subtraction: it is held to the fixture without this term, on the GPU.)"""
    unit = K.Unit(g, label, idx)
    s = K.SYSTEMS[idx[0]]
    kw = dict(period=s["period"], t0=s["t0"], b=s["b"], m_star=s["m_star"], r_star=s["r_star"], m_planet=s["m_planet"])
    if s["ecc"] is not None:
        kw.update(ecc=s["ecc"], omega=s["omega"])
    orbit = P.KeplerianOrbit(**kw)
    t = np.concatenate([unit.t_in, unit.t_out])
    if unit.secondary:
        lc = P.SecondaryEclipseLightCurve(s["u"], s["u2"], s["sbr"])
    else:
        lc = P.LimbDarkLightCurve(*s["u"])
    got = lc.get_light_curve(orbit=orbit, r=s["r"], t=t, light_delay=True)[:, 0]
    pick = np.concatenate([np.arange(K.N_IN), np.full(K.N_OUT, -1)])
    want, J, _ = unit.expected(pick)
    rec = unit.rec[0, 0]
    slots = K.grad_slots(True)
    M0_over_n = abs(rec[P.P_T0] - rec[P.P_TP])
    tol = (unit.flux_tol(t, J)[0] + K.EPS * (abs(rec[P.P_T0]) + M0_over_n) * np.abs(J[:, 0, K.COL_TP])
           + K.EPS * np.abs(J[:, 0, :] * rec[slots][None, :]).sum(axis=1))
    # |az| = n^2 |z| (a / r)^3 in stellar radii per day^2, from the record in float64 (a magnitude)
    n, e, cw, sw = rec[P.P_N], rec[P.P_ECC], rec[P.P_COSW], rec[P.P_SINW]
    sinf, cosf = P.kepler((t - rec[P.P_TP]) * n, e + np.zeros_like(t))
    r_over_a = (1 - e) * (1 + e) / (1 + e * cosf)
    az = n * n * np.abs(rec[P.P_SINI] * rec[P.P_AOR] * r_over_a * (sw * cosf + cw * sinf)) / r_over_a ** 3
    tol = tol + 2 * K.EPS * rec[P.P_CLIGHT] / az * np.abs(J[:, 0, K.COL_TP])
    err = np.abs(got - want[:, 0])
    K.report(f"light delay end to end {label}", worst_error=err, worst_error_over_tol=err / tol,
             delay_visible=np.abs(J[:, 0, 10]).max())
    assert np.all(err <= tol)
    assert np.abs(J[:, 0, 10]).max() > 0          # (the speed of light carries a derivative: the delay is in the fixture)


def test_series_helper(g):
    """the interleaved, tiled series of the GPU tests: every block of 256 holds in-transit cadences, the sorted order holds
    the same cadences"""
    unit = K.Unit(g, *UNITS[0])
    t, pick = unit.series(600)
    assert t.size == 600 and all((pick[k:k + 256] >= 0).any() and (pick[k:k + 256] < 0).any() for k in (0, 256, 512))
    assert set(pick[pick >= 0]) == set(range(K.N_IN))
    ts, ps = unit.series(600, "sorted")
    assert np.all(np.diff(ts) >= 0) and sorted(ps) == sorted(pick)
    assert np.array_equal(np.where(ps >= 0, unit.t_in[np.maximum(ps, 0)], ts), ts)
    to, po = unit.series(600, "out")
    assert np.all(po == -1) and set(to) == set(unit.t_out)


# ------------------------------------------------------------------------------------------------------------------------
# user level: numpy_port.KeplerianOrbit + get_cl against the fixture's record, flux from user inputs, and the chain to jac_user
# ------------------------------------------------------------------------------------------------------------------------
USER_UNITS = [u for u in UNITS if all(K.user_ok(K.SYSTEMS[i]) for i in u[1])]


def _port_orbit(unit, idx):
    rows = [K.SYSTEMS[i] for i in idx]
    kw = {k: np.array([r[k] for r in rows], dtype=float) for k in ("period", "t0", "b", "m_star", "r_star", "m_planet")}
    kw["m_star"], kw["r_star"] = float(kw["m_star"][0]), float(kw["r_star"][0])
    if not unit.user["circular"]:
        kw.update(ecc=np.array([r["ecc"] for r in rows], dtype=float), omega=np.array([r["omega"] for r in rows], dtype=float))
    return P.KeplerianOrbit(**kw), np.array([r["r"] for r in rows], dtype=float)


def _port_record(orbit, r, unit, s):
    """the port's own record in the fixture's column order [P, 11] (tests/test_gpu_transit.py::make_record's slots)"""
    n_p = r.size
    ecc = orbit.ecc if orbit.ecc is not None else np.zeros(n_p)
    cw = orbit.cos_omega if orbit.ecc is not None else np.ones(n_p)
    sw = orbit.sin_omega if orbit.ecc is not None else np.zeros(n_p)
    ror = r / orbit.r_star
    fr = (s["sbr"] * ror ** 2) if s["sbr"] is not None else np.zeros(n_p)
    cols = [orbit.n, orbit.t_periastron, ecc, cw, sw, orbit.cos_incl, orbit.a / orbit.r_star, ror, fr, orbit.sin_incl,
            np.full(n_p, P.c_light / orbit.r_star)]
    return np.stack([np.broadcast_to(np.asarray(c, dtype=float), (n_p,)) for c in cols], axis=-1)


def test_user_table_is_consistent(g):
    assert len(USER_UNITS) == len(UNITS) - 1            # (only the entry given by t_periastron is out of a user call's reach)
    assert g["pk_in"].shape == (len(K.PACK_ONLY), 10) and np.all(g["pk_in"][:, 3] >= 1 - 1e-6)
    assert K.REC_COLS[:9] == tuple(K.grad_slots()) and K.REC_COLS[9:] == (P.P_SINI, P.P_CLIGHT)


@pytest.mark.parametrize("label,idx", USER_UNITS, ids=[u[0] for u in USER_UNITS])
def test_port_orbit_record_and_limb_darkening(label, idx, g):
    """numpy_port.KeplerianOrbit(period, t0, b, ecc, omega, ...) and get_cl from the table's inputs: every slot of the record
    and every component of c against the fixture's (allowance: lightcurve_mp_cases.pack_value_tol; c: 8 EPS of the component)"""
    unit = K.Unit(g, label, idx)
    s = K.SYSTEMS[idx[0]]
    orbit, r = _port_orbit(unit, idx)
    got = _port_record(orbit, r, unit, s)
    want = unit.rec[0][:, list(K.REC_COLS)].copy()
    if not unit.light_delay:
        got[:, 10] = 0.0                              # (the fixture's record carries the speed of light only where it is used)
    tol = K.pack_value_tol(want, unit.user["inp"][0])
    ratio = np.abs(got - want) / np.where(tol > 0, tol, 1.0)
    c = P.get_cl(*s["u"])
    rc = np.abs(c - unit.c[0, :3]) / (8 * K.EPS * np.abs(unit.c[0, :3]))
    K.report(f"port record {label}", worst_error_over_tol=ratio, worst_slot=float(np.argmax(ratio.max(axis=0))), c_error_over_tol=rc)
    assert np.all(np.abs(got - want) <= tol), (label, ratio.max(axis=0))
    assert np.all(rc <= 1.0)


FLUX_USER_UNITS = [u for u in USER_UNITS if not K.SYSTEMS[u[1][0]]["ttv"] and not K.SYSTEMS[u[1][0]]["light_delay"]
                   and K.SYSTEMS[u[1][0]]["grad"]]


@pytest.mark.parametrize("label,idx", FLUX_USER_UNITS, ids=[u[0] for u in FLUX_USER_UNITS])
def test_flux_from_user_inputs(label, idx, g):
    """get_light_curve of numpy_port's classes from the table's user inputs: per cadence 8 EPS (1 + |t - tp| |dF/dtp|) +
    EPS (|t0| + |M0 / n|) |dF/dtp| for the stored t_periastron + the other slots' roundings (pack_value_tol) carried through
    the fixture's Jacobian.  (Light delay: test_light_delay_flux_end_to_end.  Timing variations: the record level only --
    numpy_port.TTVOrbit builds its own tables from transit times.)"""
    unit = K.Unit(g, label, idx)
    s = K.SYSTEMS[idx[0]]
    orbit, r = _port_orbit(unit, idx)
    t = np.concatenate([unit.t_in, unit.t_out])
    kw = {}
    if s["stencil"]:
        kw = dict(texp=s["stencil"][0], oversample=s["stencil"][1], order=s["stencil"][2])
    lc = P.SecondaryEclipseLightCurve(s["u"], s["u2"], s["sbr"]) if unit.secondary else P.LimbDarkLightCurve(*s["u"])
    got = lc.get_light_curve(orbit=orbit, r=r, t=t, use_in_transit=False, **kw)
    pick = np.concatenate([np.arange(K.N_IN), np.full(K.N_OUT, -1)])
    want, J, _ = unit.expected(pick)
    rec11 = unit.rec[0][:, list(K.REC_COLS)]
    slot_tol = K.pack_value_tol(rec11, unit.user["inp"][0])[:, :9]
    tol = unit.flux_tol(t, J)[1] + np.einsum("ps,nps->np", slot_tol, np.abs(J[:, :, :9]))
    err = np.abs(got - want)
    K.report(f"flux from user inputs {label}", worst_error=err, worst_error_over_tol=err / tol)
    assert np.all(err <= tol)


@pytest.mark.parametrize("label,idx", [u for u in USER_UNITS if not K.SYSTEMS[u[1][0]]["light_delay"] and K.SYSTEMS[u[1][0]]["grad"]],
                         ids=[u[0] for u in USER_UNITS if not K.SYSTEMS[u[1][0]]["light_delay"] and K.SYSTEMS[u[1][0]]["grad"]])
def test_user_level_gradient_chain(label, idx, g):
    """the port's record-level VJP carried to (period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr) and (u1, u2[, u1s,
    u2s]) through the fixture's jac_user / jac_cu in float64, against the fixture's own VJP carried likewise: per user
    parameter |error| / sum |terms| <= UNIT_CEILING (the condition on the inputs at user level)"""
    unit = K.Unit(g, label, idx)
    t = np.concatenate([unit.t_in, unit.t_out])
    pick = np.concatenate([np.arange(K.N_IN), np.full(K.N_OUT, -1)])
    go = K.cotangent(label, "host/user", (t.size, unit.P))
    _, gp, gl, *_ = K.oracle_vjp(unit, t, go, per_planet=True)
    wr, dr, wc, dc, _, _ = K.want_vjp(unit, pick, go)
    J = unit.user["jac"][:, :9, :]
    got, want = np.einsum("ps,psk->pk", gp, J), np.einsum("ps,psk->pk", wr, J)
    den = np.einsum("ps,psk->pk", dr * (np.abs(wr) > 0), np.abs(J))
    ratio = np.abs(got - want) / np.where(den > 0, den, 1.0)
    gu, wu = gl @ unit.user["jac_cu"][:gl.size], wc @ unit.user["jac_cu"][:gl.size]
    du = (dc * (np.abs(wc) > 0)) @ np.abs(unit.user["jac_cu"][:gl.size])
    ru = np.abs(gu - wu) / np.where(du > 0, du, 1.0)
    K.report(f"user-level chain {label}", unit=ratio, unit_u=ru)
    assert ratio.max() <= K.UNIT_CEILING and ru.max() <= K.UNIT_CEILING, (label, ratio, ru)


def test_inexpressible_pairs_are_few():
    """the cap on (unit, route) pairs that tests/test_gpu_lightcurve_mp.py cannot express: it needs no GPU, and that module
    carries the gpu mark"""
    import test_gpu_lightcurve_mp as G

    G.test_inexpressible_pairs_are_few()
