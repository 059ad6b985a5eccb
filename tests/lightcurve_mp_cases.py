"""What tools/make_lightcurve_golden.py, tests/test_lightcurve_mp_host.py and tests/test_gpu_lightcurve_mp.py share: the table
of systems behind the multiprecision fixture tests/golden/lightcurve_mp.npz, the tolerances -- each one derived here or in
tests/orbit_mp_cases.py, none taken from the code under test -- and the float64 oracle's own error ("unit") on the same
input.  numpy only: the generator imports the table, the tests import everything.

The fixture holds, per entry (one planet's float64 record, the float64 limb-darkening vector c[6], an optional exposure
stencil), the flux at ``t_in`` (N_IN cadences spanning both contacts, limb cadences on either side, the first and last just
outside) and its derivative to every gradient slot of the record (oracle.numpy_port.GRAD_SLOTS order) and to c, all as
functions of the float64 inputs, evaluated at 40 digits.  ``t_out`` are N_OUT times at which the flux is exactly 0: mpmath
verified b > 1 + r + 1e-3, or the body behind the star without an occultation asked for, at every sub-exposure.  Entries with
the same ``group`` are planets of one star and share their times.

Tolerances (EPS, VJP_FLOOR, UNIT_CEILING, vjp_want, vjp_tol, report: tests/orbit_mp_cases.py)
----------
* flux at record level, per cadence:  8 EPS (1 + |t - tp| |dF/dtp|), dF/dtp from the fixture: eight roundings of a value of
  size 1 (F + 1 is the normalised flux), plus the two roundings of the plain product (t - tp) n, which move the time by
  EPS |t - tp| each, as the orbit fixture allows.  Summed over the planets of a group.
* t_out: exactly 0, and a series made only of t_out has an all-zero VJP.
* VJPs, per (entry, slot) and per component of c:  |got - g.J| / sum_n |g_n J_n| <= max(16 unit, 1e-13), unit that same ratio
  for oracle.numpy_port.transit_flux_vjp on the same input and cotangent; 16 covers the summation order across lanes,
  waves, blocks and the Jacobian route's different order (the project's convention, tests/test_gpu_estimators.py).
* a slot or component whose fixture Jacobian is identically 0 reads exactly 0.
* condition on the inputs: every gradient entry's unit <= UNIT_CEILING (asserted in the host test).
* light delay: oracle.numpy_port has no record-level light delay, so there is no unit: the allowance of those two entries is
  the floor 1e-13 alone.  Their flux is also held end to end through numpy_port's classes (host test).
* timing variations: a time acts as t - shift[bin]; the cotangent of shift[k] is that of t_periastron restricted to bin k.
"""
import os

import numpy as np

from orbit_mp_cases import EPS, GOLD, UNIT_CEILING, VJP_FLOOR, report, vjp_tol, vjp_want  # noqa: F401

N_IN, N_OUT = 20, 16
N_SUB_MAX = 7
PI = float(np.pi)

# ------------------------------------------------------------------------------------------------------------------------
# The systems.  period, b, ecc, omega, r (in R_sun), m_star, r_star; t0 or tp (t_periastron);
# ``at``: the transit picked for the cadences is the one nearest this time.  u: quadratic limb darkening of the star;
# sbr / u2: occultation asked for (FLAG_SECONDARY), surface-brightness ratio and the planet's own limb darkening.
# stencil = (texp, oversample, order).  grad=False: values only.  ecc=None: the circular packing (M0 = pi / 2).
# light_delay: the record carries the speed of light and the flux is that of FLAG_LIGHT_DELAY.  ttv = (d0, d1, d2): three
# transits, the k-th displaced by d_k from the linear ephemeris; the cadences are dealt round the three.
# ------------------------------------------------------------------------------------------------------------------------
_BASE = dict(period=3.5, t0=1.0, b=0.3, ecc=0.3, omega=1.1, r=0.1, u=(0.3, 0.2))


def _s(name, **kw):
    d = dict(m_star=1.0, r_star=1.0, m_planet=0.0, t0=0.0, tp=None, at=None, omega=None, sbr=None,
             u2=None, stencil=None, grad=True, group=None, u=(0.3, 0.2), light_delay=False, ttv=None)
    d.update(kw)
    d["name"] = name
    return d


SYSTEMS = [
    _s("mild_e03", **_BASE),
    _s("circular_packing", period=3.5, t0=1.0, b=0.3, ecc=None, r=0.1),
    _s("e_zero_exactly", period=3.5, t0=1.0, b=0.3, ecc=0.0, omega=0.7, r=0.1),
    _s("e095_near_periastron", period=20.0, t0=2.0, b=0.4, ecc=0.95, omega=1.2, r=0.1),
    _s("e099", period=50.0, t0=-3.0, b=0.4, ecc=0.99, omega=-1.2, r=0.1),
    _s("e0995", period=1000.0, t0=5.0, b=0.4, ecc=0.995, omega=1.2, r=0.1),
    # (omega as the float64 angle, so that the user-level routes can express these entries: cos(fl(pi / 2)) = 6e-17, not 0)
    _s("omega_plus_half_pi", period=8.0, t0=0.7, b=0.5, ecc=0.5, omega=0.5 * PI, r=0.1),
    _s("omega_minus_half_pi", period=8.0, t0=0.7, b=0.5, ecc=0.5, omega=-0.5 * PI, r=0.1),
    _s("omega_zero", period=8.0, t0=0.7, b=0.5, ecc=0.5, omega=0.0, r=0.1),
    _s("omega_pi", period=8.0, t0=0.7, b=0.5, ecc=0.5, omega=PI, r=0.1),
    _s("b_zero_exactly", period=3.5, t0=1.0, b=0.0, ecc=0.3, omega=1.1, r=0.1),
    _s("b_1e-9", period=3.5, t0=1.0, b=1e-9, ecc=0.3, omega=1.1, r=0.1),
    _s("grazing_b105", period=3.5, t0=1.0, b=1.05, ecc=0.3, omega=1.1, r=0.1),
    _s("b_just_grazing", period=3.5, t0=1.0, b=1 - 0.1 + 1e-6, ecc=0.3, omega=1.1, r=0.1),
    _s("b_just_inside", period=3.5, t0=1.0, b=1 - 0.1 - 1e-6, ecc=0.3, omega=1.1, r=0.1),
    _s("r06_b09_circular", period=3.5, t0=1.0, b=0.9, ecc=None, r=0.6),
    _s("r12_larger_than_star", period=3.5, t0=1.0, b=0.1, ecc=0.2, omega=0.4, r=1.2),
    _s("multi_a_e01", period=10.0, t0=0.5, b=0.2, ecc=0.1, omega=0.5, r=0.1, m_star=1.45, r_star=1.5, m_planet=0.3,
       u=(0.2, 0.3), group=0),
    _s("multi_b_e08", period=5.3, t0=0.56, b=0.5, ecc=0.8, omega=1.3, r=0.05, m_star=1.45, r_star=1.5, m_planet=0.5,
       u=(0.2, 0.3), group=0),
    _s("multi_c_circular", period=7.1, t0=3.0, b=0.7, ecc=0.0, omega=0.0, r=0.15, m_star=1.45, r_star=1.5, m_planet=0.1,
       u=(0.2, 0.3), group=0),
    _s("occultation_ror008", period=3.5, t0=1.0, b=0.3, ecc=0.2, omega=0.6, r=0.08, sbr=0.3, u2=(0.1, 0.4)),
    _s("occultation_ror03_circular", period=2.2, t0=0.4, b=0.5, ecc=None, r=0.3, sbr=0.3, u2=(0.5, 0.1), u=(0.4, 0.25)),
    _s("stencil_order0_os7", stencil=(0.015, 7, 0), **_BASE),
    _s("stencil_order1_os5", stencil=(0.015, 5, 1), **_BASE),
    _s("stencil_order2_os5", stencil=(0.015, 5, 2), **_BASE),
    _s("light_delay_eccentric", period=3.456, t0=1.45, b=0.35, ecc=0.35, omega=-1.3, m_star=1.2, r_star=1.1, r=0.11,
       light_delay=True),
    _s("light_delay_circular_occultation", period=2.2, t0=0.4, b=0.5, ecc=None, r=0.3, sbr=0.3, u2=(0.5, 0.1), u=(0.4, 0.25),
       light_delay=True),
    _s("ttv_three_transits", ttv=(0.003, -0.002, 0.0045), **_BASE),
    _s("bjd_t0", period=3.5, t0=2458001.0, b=0.3, ecc=0.3, omega=1.1, r=0.1),
    _s("bjd_times_tp_03", period=3.5, tp=0.3, at=2458001.0, t0=None, b=0.3, ecc=0.3, omega=1.1, r=0.1),
]

# Packing only (no light curve): records and their user-level Jacobian where 1 - e^2 has to be formed as (1 - e)(1 + e)
PACK_ONLY = [
    dict(period=3.5, t0=1.0, b=1e-9, ecc=1 - 1e-8, omega=1.2, r=0.1, m_star=1.0, r_star=1.0, m_planet=0.0, u=(0.3, 0.2)),
    dict(period=11.0, t0=-2.0, b=1e-7, ecc=1 - 1e-6, omega=-0.7, r=0.05, m_star=1.3, r_star=1.2, m_planet=0.01, u=(0.5, 0.1)),
]
USER_NAMES = ("period", "t0", "b", "ecc", "omega", "r", "m_star", "r_star", "m_planet", "sbr")     # ops.IN_* order
# the record slots in the fixture's column order (jac_rec's columns, jac_user's rows): numpy_port / ops slot numbers
REC_COLS = (0, 1, 2, 3, 4, 5, 7, 8, 13, 6, 16)
EXO_PACK_CIRCULAR = 8


def user_vector(s):
    """the ten packing inputs of a table entry (0 where the constructor's default applies)"""
    return np.array([s["period"], s["t0"] if s.get("t0") is not None else 0.0, s["b"], s["ecc"] or 0.0, s.get("omega") or 0.0,
                     s["r"], s["m_star"], s["r_star"], s["m_planet"], s.get("sbr") or 0.0])


def user_ok(s):
    """can a user-level call (period, t0, b, ecc, omega, ...) reproduce this entry's record up to rounding?"""
    return s.get("tp") is None


# slots of the record that carry a gradient without light delay, in the fixture's column order
SLOT_NAMES = ("n", "tp", "ecc", "cosw", "sinw", "cosi", "aor", "ror", "fratio")
DELAY_SLOT_NAMES = ("sini", "clight")       # ... and with light delay (the fixture's columns 9 and 10)
COL_TP = 1


def load():
    return np.load(os.path.join(GOLD, "lightcurve_mp.npz"))


# ------------------------------------------------------------------------------------------------------------------------
# units of work: one entry, or the entries of a group as the planets of one star
# ------------------------------------------------------------------------------------------------------------------------
def units():
    """[(label, [entry indices])]: every ungrouped entry alone, every group together"""
    out, seen = [], {}
    for i, s in enumerate(SYSTEMS):
        if s["group"] is None:
            out.append((s["name"], [i]))
        elif s["group"] not in seen:
            seen[s["group"]] = len(out)
            out.append((f"group{s['group']}", [i]))
        else:
            out[seen[s["group"]]][1].append(i)
    return out


class Unit:
    """the fixture's view of one unit: record [1, P, NPAR], c [1, 3|6], the two time lists, flux [N_IN, P], the Jacobians
    jac_rec [N_IN, P, 9 | 11 with light delay] and jac_c [N_IN, P, 3|6], the keyword arguments of the exposure stencil, the
    timing tables (edges [1, 1, 2], shift [1, 1, 3]) or None"""

    def __init__(self, g, label, idx):
        i0 = idx[0]
        self.label, self.idx = label, idx
        self.secondary = bool(g["secondary"][i0])
        self.grad = bool(g["grad"][i0])
        nld = 6 if self.secondary else 3
        self.rec = np.ascontiguousarray(g["rec"][idx][None])
        self.c = np.ascontiguousarray(g["c"][i0, :nld][None])
        self.t_in, self.t_out = g["t_in"][i0], g["t_out"][i0]
        self.flux = np.stack([g["flux"][i] for i in idx], axis=-1)
        self.light_delay = bool(g["rec"][i0, 16] != 0)           # (EXO_P_CLIGHT)
        ncol = 11 if self.light_delay else 9
        self.jac_rec = np.stack([g["jac_rec"][i][:, :ncol] for i in idx], axis=1)
        assert not np.any(g["jac_rec"][idx][:, :, ncol:])
        self.user = None
        if all(user_ok(SYSTEMS[i]) for i in idx):
            self.user = dict(inp=g["user_in"][idx][None], u=g["user_u"][i0, :4 if self.secondary else 2][None],
                             jac=g["jac_user"][idx], jac_cu=g["jac_cu"][i0], circular=SYSTEMS[i0]["ecc"] is None)
            assert all((SYSTEMS[i]["ecc"] is None) == self.user["circular"] for i in idx)      # (one packing flag per call)
        self.ttv = None
        if int(g["ttv_n"][i0]):
            self.ttv = (g["ttv_edges"][i0][None, None].copy(), g["ttv_shift"][i0][None, None].copy())
        self.jac_c = np.stack([g["jac_c"][i][:, :nld] for i in idx], axis=1)
        ns = int(g["n_sub"][i0])
        self.stencil = dict(texp=float(g["texp"][i0]), stencil_dt=g["sdt"][i0, :ns].copy(),
                            stencil_w=g["sw"][i0, :ns].copy()) if ns else {}
        self.P = len(idx)

    def series(self, n, order="interleaved"):
        """(t [n], pick [n]): t_in interleaved with t_out and tiled to n cadences; pick[k] is the index into t_in of
        cadence k, or -1 where it is a t_out cadence.  order='sorted': the same cadences in time order; 'out': t_out only"""
        m = min(N_IN, N_OUT)
        one = np.empty(N_IN + N_OUT, dtype=np.int64)
        one[0:2 * m:2] = np.arange(m)
        one[1:2 * m:2] = -1 - np.arange(m)
        one[2 * m:] = np.arange(m, N_IN) if N_IN > m else -1 - np.arange(m, N_OUT)
        if order == "out":
            one = -1 - np.arange(N_OUT)
        code = np.resize(one, n)
        t = np.where(code >= 0, self.t_in[np.maximum(code, 0)], self.t_out[np.maximum(-1 - code, 0)])
        if order == "sorted":
            k = np.argsort(t, kind="stable")
            t, code = t[k], code[k]
        return t, np.where(code >= 0, code, -1)

    def expected(self, pick):
        """(flux [n, P], jac_rec [n, P, 9], jac_c [n, P, nld]) of a series: the fixture's rows, exact zeros at t_out"""
        inn = (pick >= 0)
        k = np.maximum(pick, 0)
        return (np.where(inn[:, None], self.flux[k], 0.0), np.where(inn[:, None, None], self.jac_rec[k], 0.0),
                np.where(inn[:, None, None], self.jac_c[k], 0.0))

    def flux_tol(self, t, jac_rec):
        """[n] for the summed flux, [n, P] per planet: 8 EPS (1 + |t - tp| |dF/dtp|)"""
        tp = self.rec[0, :, COL_TP]
        if self.ttv is not None:
            t = t - self.ttv[1][0, 0][np.searchsorted(self.ttv[0][0, 0], t)]
        per = 8 * EPS * (1 + np.abs(t[:, None] - tp[None, :]) * np.abs(jac_rec[:, :, COL_TP]))
        return per.sum(axis=1), per


def seed(label, route):
    """the fixed seed of (unit, route)"""
    import zlib

    return zlib.crc32(f"{label}/{route}".encode())


def cotangent(label, route, shape):
    """the seeded cotangent of (unit, route): the same one wherever that pair is checked"""
    return np.random.default_rng(seed(label, route)).normal(size=shape)


def grad_slots(light_delay=False):
    from oracle import numpy_port as P

    return list(P.GRAD_SLOTS) + ([P.P_SINI, P.P_CLIGHT] if light_delay else [])


def want_vjp(unit, pick, go):
    """fixture VJP of a series with cotangent go [n] (summed flux) or [n, P]: (g.J [P, 9], sum |g J| [P, 9], g.Jc [nld],
    sum |g Jc| [nld], and where the two sums are 0: the wanted value is then exactly 0, the denominator returned is 1)"""
    _, J, Jc = unit.expected(pick)
    gp = go if go.ndim == 2 else np.repeat(go[:, None], unit.P, axis=1)
    wr = np.einsum("np,npk->pk", gp, J)
    dr = np.einsum("np,npk->pk", np.abs(gp), np.abs(J))
    wc = np.einsum("np,npk->k", gp, Jc)
    dc = np.einsum("np,npk->k", np.abs(gp), np.abs(Jc))
    return wr, np.where(dr > 0, dr, 1.0), wc, np.where(dc > 0, dc, 1.0), (dr == 0), (dc == 0)


def want_gshift(unit, t, pick, go):
    """fixture cotangent of the shift table [3]: the shift enters exactly like t_periastron, so bin k gets
    sum over its cadences of g_n dF_n/dtp; (wanted, sum |terms| or 1, where that sum is 0)"""
    _, J, _ = unit.expected(pick)
    bins = np.searchsorted(unit.ttv[0][0, 0], t)
    term = go * J[:, 0, COL_TP]
    w = np.array([term[bins == k].sum() for k in range(3)])
    d = np.array([np.abs(term[bins == k]).sum() for k in range(3)])
    return w, np.where(d > 0, d, 1.0), d == 0


def oracle_vjp(unit, t, go, per_planet=False, delay_free=False):
    """oracle.numpy_port on the unit's record: (flux, gparams [P, 9], gld [nld][, gshift [3]]).  The oracle has no light
    delay at record level: None for such a unit (its allowance is then the floor alone)"""
    from oracle import numpy_port as P

    if unit.light_delay and not delay_free:      # (delay_free: the same record without its delay, for magnitudes only)
        return None
    kw = dict(unit.stencil)
    if unit.ttv is not None:
        kw["ttv"] = unit.ttv
    out = P.transit_flux_vjp(t, unit.rec, unit.c, go[None], per_planet=per_planet, secondary=unit.secondary, **kw)
    return (out[0][0], out[1][0][:, grad_slots()], out[2][0]) + ((out[3][0, 0],) if unit.ttv is not None else ())


# ------------------------------------------------------------------------------------------------------------------------
# user level: d record / d (period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr) and d c / d u from the fixture
# ------------------------------------------------------------------------------------------------------------------------
def pack_value_tol(rec11, user):
    """allowance of a packed record against the fixture's, in the fixture's column order: 8 EPS of the slot (eight
    roundings: cbrt, sincos, atan2, the quotients), 8 EPS absolute for cos w, sin w and sin i (values of size 1 that may
    be 0), and for t_periastron = t0 - M0 / n one rounding at the size of t0 -- EPS |t0|, about one ulp of a BJD -- plus
    the roundings inside M0 / n: M0 = E0 - e sin E0 is a difference (at e = 0.99 its terms are ten times M0), so
    4 EPS (|E0| + e |sin E0|) / n, with E0 solved in float64 from the fixture's own M0 = n (t0 - tp) (a magnitude)"""
    from oracle import numpy_port as P

    M0 = rec11[..., 0] * (user[..., 1] - rec11[..., 1])
    E0 = P.kepler_E(M0, rec11[..., 2])[0]
    tol = 8 * EPS * np.abs(rec11)
    tol[..., [3, 4, 9]] = 8 * EPS
    tol[..., 1] = EPS * np.abs(user[..., 1]) + 4 * EPS * (np.abs(E0) + rec11[..., 2] * np.abs(np.sin(E0))) / rec11[..., 0]
    return tol


def want_user_vjp(grec, gc, jac_user, jac_cu):
    """(g.J [P, 10], sum |g J| or 1, exactly-zero mask; the same three for u [4]) for record cotangents grec [P, 11] (fixture
    column order) and gc [6]"""
    w = np.einsum("ps,psk->pk", grec, jac_user)
    d = np.einsum("ps,psk->pk", np.abs(grec), np.abs(jac_user))
    wu = gc @ jac_cu[:gc.size]
    du = np.abs(gc) @ np.abs(jac_cu[:gc.size])
    return w, np.where(d > 0, d, 1.0), d == 0, wu, np.where(du > 0, du, 1.0), du == 0


def record_sensitivity(unit, t, go, per_planet=False, h=1e-7):
    """what one rounding of each record slot does to the oracle's record-level VJP: the device packs its own float64 record
    (every slot within pack_value_tol of the fixture's), and the VJP is evaluated THERE.  By differences of
    oracle.numpy_port at a relative step h, scaled to pack_value_tol: (|d (g.J) [P, 9]|, |d (g.Jc) [nld]|) summed over the
    perturbed slots.  A magnitude from the oracle, nothing from the code under test.  A light-delay unit takes it from the
    delay-free oracle on the same record: the delay moves the times by ~1e-4 d, which changes a magnitude by nothing that
    matters."""
    from oracle import numpy_port as P

    base = oracle_vjp(unit, t, go, per_planet, delay_free=True)
    out_r, out_c = np.zeros_like(base[1]), np.zeros_like(base[2])
    cols = grad_slots()
    rec11 = unit.rec[0][:, list(REC_COLS)]
    tol = pack_value_tol(rec11, unit.user["inp"][0])
    keep = unit.rec.copy()
    try:
        for j, slot in enumerate(cols[:8]):                  # (the flux ratio enters linearly through its own column)
            for p in range(unit.P):
                # relative step; absolute (1e-7) for the slots that may be 0 or, t_periastron, sit at a BJD
                step = h if slot in (P.P_TP, P.P_COSW, P.P_SINW, P.P_COSI) else h * abs(keep[0, p, slot])
                if step == 0:
                    continue          # (e = 0 exactly: nothing is rounded)
                unit.rec = keep.copy()
                unit.rec[0, p, slot] += step
                step = unit.rec[0, p, slot] - keep[0, p, slot]
                pert = oracle_vjp(unit, t, go, per_planet, delay_free=True)
                scale = tol[p, REC_COLS.index(slot)] / step
                out_r += np.abs(pert[1] - base[1]) * scale
                out_c += np.abs(pert[2] - base[2]) * scale
    finally:
        unit.rec = keep
    return out_r, out_c
