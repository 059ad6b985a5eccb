"""End-to-end light curves in arbitrary precision (TEST INFRASTRUCTURE ONLY; see oracle/__init__.py).

The whole chain of `LimbDarkLightCurve.get_light_curve` / `SecondaryEclipseLightCurve.get_light_curve`
evaluated with mpmath from the reference's own formulas -- written here directly from the reference
lines cited below, NOT through oracle/numpy_port.py, so that a fixture generated from this module pins
the numpy port, the C port and the device kernels to something none of them shares code with:

  orbit algebra     src/exoplanet/orbits/keplerian.py:146 (n), :205-214 (E0, M0, incl_factor),
                    :217-228 (cos i from b), :267-281 (t_periastron, sin i), :849-934 (Kepler's third law)
  positions         keplerian.py:283-334 (rotation, true anomaly), :380-409 (r), :517-542 (relative position)
  flipped orbit     keplerian.py:779-804
  exposure stencil  src/exoplanet/light_curves/limb_dark.py:178-226
  flux              limb_dark.py:11-24, :234-252;  blend: light_curves/secondary_eclipse.py:45-70
  Kepler's equation, solution vector: the DEFINITIONS of oracle/mp_reference.py (quadrature).
"""
import mpmath as mp

from . import mp_reference as R

G_GRAV = mp.mpf("2942.2062175044193")     # R_sun^3 / M_sun / day^2, orbits/constants.py:32
C_LIGHT = mp.mpf("37231.66360672704")     # R_sun / day, orbits/constants.py:36


class Orbit:
    """standard transit parameterisation: period, t0, b, (ecc, omega), m_star, r_star, m_planet"""

    def __init__(self, period, t0=0.0, b=0.0, ecc=None, omega=None, m_star=1.0, r_star=1.0, m_planet=0.0,
                 t_periastron=None, incl=None):
        f = mp.mpf
        self.period, self.m_star, self.r_star, self.m_planet = f(period), f(m_star), f(r_star), f(m_planet)
        self.a = (G_GRAV * (self.m_star + self.m_planet) * self.period ** 2 / (4 * mp.pi ** 2)) ** (mp.mpf(1) / 3)   # :925-928
        self.n = 2 * mp.pi / self.period                                                                       # :146
        self.ecc = None if ecc is None else f(ecc)
        if self.ecc is None:
            self.M0 = mp.pi / 2                                                                                # :184
            self.cw, self.sw = mp.mpf(1), mp.mpf(0)
            incl_factor = mp.mpf(1)
        else:
            w = f(omega)
            self.omega = w
            self.cw, self.sw = mp.cos(w), mp.sin(w)
            E0 = 2 * mp.atan2(mp.sqrt(1 - self.ecc) * self.cw, mp.sqrt(1 + self.ecc) * (1 + self.sw))        # :205-209
            self.M0 = E0 - self.ecc * mp.sin(E0)                                                               # :210
            incl_factor = (1 + self.ecc * self.sw) / (1 - self.ecc ** 2)                                       # :212-214
        if incl is not None:
            self.cos_incl = mp.cos(f(incl))
            self.sin_incl = mp.sin(f(incl))
        else:
            self.cos_incl = incl_factor * self.r_star / self.a * f(b)                                          # :217-228
            self.sin_incl = mp.sin(mp.acos(self.cos_incl))                                                     # :281
        if t_periastron is not None:
            self.t_periastron = f(t_periastron)
            self.t0 = self.t_periastron + self.M0 / self.n
        else:
            self.t0 = f(t0)
            self.t_periastron = self.t0 - self.M0 / self.n                                                     # :277

    def relative_position(self, t):
        """(X, Y, Z) of the planet relative to the star (a -> -a, keplerian.py:540)"""
        M = (mp.mpf(t) - self.t_periastron) * self.n                                                          # :324-330
        if self.ecc is None:
            sinf, cosf = mp.sin(M), mp.cos(M)
            r = -self.a
        else:
            sinf, cosf = R.kepler(M, self.ecc)[:2]
            r = -self.a * (1 - self.ecc ** 2) / (1 + self.ecc * cosf)                                          # :403
        x, y = r * cosf, r * sinf
        x1 = self.cw * x - self.sw * y                                                                         # :303-308
        y1 = self.sw * x + self.cw * y
        return x1, self.cos_incl * y1, -self.sin_incl * y1                                                     # :311-314

    def flip(self, r_planet):
        """keplerian.py:779-804"""
        if self.ecc is None:
            o = Orbit(self.period, m_star=self.m_planet, m_planet=self.m_star, r_star=r_planet,
                      t_periastron=self.t_periastron + self.period / 2, incl=mp.acos(self.cos_incl))
        else:
            o = Orbit(self.period, ecc=self.ecc, omega=self.omega - mp.pi, m_star=self.m_planet, m_planet=self.m_star,
                      r_star=r_planet, t_periastron=self.t_periastron, incl=mp.acos(self.cos_incl))
        return o


def get_cl(u1, u2):
    """limb_dark.py:11-18"""
    u1, u2 = mp.mpf(u1), mp.mpf(u2)
    c = [1 - u1 - mp.mpf(3) / 2 * u2, u1 + 2 * u2, -u2 / 4]
    norm = mp.pi * (c[0] + c[1] / mp.mpf("1.5"))
    return [v / norm for v in c]


def stencil(oversample=7, order=0):
    """limb_dark.py:181-197 -> (offsets in units of texp, weights)"""
    oversample = int(oversample)
    oversample += 1 - oversample % 2
    w = [mp.mpf(1)] * oversample
    if order == 0:
        full = [mp.mpf(-1) / 2 + mp.mpf(k) / (2 * oversample) for k in range(2 * oversample + 1)]
        dt = full[1:-1:2]
    elif order == 1:
        dt = [mp.mpf(-1) / 2 + mp.mpf(k) / (oversample - 1) for k in range(oversample)]
        for k in range(1, oversample - 1):
            w[k] = mp.mpf(2)
    elif order == 2:
        dt = [mp.mpf(-1) / 2 + mp.mpf(k) / (oversample - 1) for k in range(oversample)]
        for k in range(1, oversample - 1, 2):
            w[k] = mp.mpf(4)
        for k in range(2, oversample - 1, 2):
            w[k] = mp.mpf(2)
    else:
        raise ValueError("order must be <= 2")
    tot = sum(w)
    return dt, [v / tot for v in w]


def flux_one(orbit, r, c, t):
    """limb_dark.py:215-252 for one planet, one time"""
    X, Y, Z = orbit.relative_position(t)
    if not (Z > 0):
        return mp.mpf(0)
    b = mp.sqrt(X * X + Y * Y) / orbit.r_star
    ror = mp.mpf(r) / orbit.r_star
    if b >= 1 + ror:
        return mp.mpf(0)
    s = R.quad_sv(b, ror)
    return s[0] * c[0] + s[1] * c[1] + s[2] * c[2] - 1


# ------------------------------------------------------------------------------------------------------------------------
# The flux as a function of the kernel's record (include/exoplanet_amd.h): n, t_periastron, e, cos w, sin w, cos i, sin i,
# a / R_star, r / R_star, the flux ratio, and the limb-darkening vector c[0:3] (star) / c[3:6] (planet).  The same
# reference lines as above, with the record's slots in place of the constructor's attributes; sin i only gives Z its sign.
# ------------------------------------------------------------------------------------------------------------------------
REC_SLOTS = ("n", "tp", "e", "cw", "sw", "ci", "aor", "ror")      # the slots the geometry depends on
DELAY_SLOTS = ("si", "cl")                                        # ... and, with light delay, sin i and c / R_star


def _anomaly(t, q, circular, memo):
    M = (t - q["tp"]) * q["n"]                                                                                # :324-330
    key = (mp.mp.prec, M, q["e"], circular)      # (mp.diff works at a higher precision: never hand it a coarser value)
    if memo is not None and key in memo:
        return memo[key]
    if circular:
        out = (mp.sin(M), mp.cos(M))                                                                          # :331-332
    else:
        out = R.kepler(M, q["e"])[:2]
    if memo is not None:
        if len(memo) > 64:
            memo.clear()
        memo[key] = out
    return out


def record_geometry(t, q, circular=False, _memo=None):
    """q = dict of the slots (mpf) -> (b, y1) with Z = -sin i y1 (keplerian.py:303-314, :403, :540)"""
    sinf, cosf = _anomaly(t, q, circular, _memo)
    r = -q["aor"] * (1 - q["e"]) * (1 + q["e"]) / (1 + q["e"] * cosf)                                          # :403
    x, y = r * cosf, r * sinf
    x1 = q["cw"] * x - q["sw"] * y
    y1 = q["sw"] * x + q["cw"] * y
    Ys = q["ci"] * y1
    return mp.sqrt(x1 * x1 + Ys * Ys), y1


def record_delay(t, q, circular=False, sigma=1, _memo=None):
    """keplerian.py:411-470 with z0 = 0 for the relative orbit (a -> -a, :540) in units of R_star: the light-travel delay of
    the body seen at t.  sigma = -1: the flipped orbit of an occultation (:779-804: omega - pi, so that its position,
    velocity and acceleration are the negatives)"""
    n, e, a, c = q["n"], q["e"], -q["aor"], q["cl"]
    sinf, cosf = _anomaly(t, q, circular, _memo)
    r = a * (1 - e) * (1 + e) / (1 + e * cosf)                                                                # :437
    vamp = n * a / mp.sqrt((1 - e) * (1 + e))                                                                 # :438
    cwf = q["cw"] * cosf - q["sw"] * sinf                                                                     # :439
    vz = sigma * vamp * q["si"] * (e * q["cw"] + cwf)                                                         # :440
    y1 = q["sw"] * r * cosf + q["cw"] * r * sinf
    z = sigma * (-q["si"] * y1)                                                                               # :443
    az = -(n ** 2) * (a / r) ** 3 * z                                                                         # :446
    if abs(az) < mp.mpf("1e-10"):                                                                             # :451-462
        return (0 - z) / (c + vz)
    w = 1 + vz / c
    return (c / az) * (w - mp.sqrt(w * w - 2 * az * (0 - z) / c ** 2))


def _seen(t, q, circular, sigma, light_delay, memo):
    """(b, y1) of the body as seen at t"""
    if light_delay:
        t = t - record_delay(t, q, circular, sigma, memo)                                                     # :465-470
    return record_geometry(t, q, circular, memo)


def record_sample(t, rec, c, secondary, grad=True, light_delay=False):
    """One planet, one time -> (F, dF/d(n, tp, e, cw, sw, ci, aor, ror, fratio, si, cl) [11], dF/dc [6], b, occulted).

    rec: dict with the REC_SLOTS, 'si', 'fr' and 'cl' (mpf images of the float64 record); c: six mpf.  With ``secondary`` the
    flux is the blend of secondary_eclipse.py:45-70: the transit weighs 1 / (1 + fr), the occultation -- the star of radius
    1 / ror passing the planet at b / ror, in units of the planet's radius (:56-58) -- weighs fr / (1 + fr).  With
    ``light_delay`` either body is seen where it was one light-travel time ago (record_delay), the occultation by the
    flipped orbit's own delay.
    dF/d(b, r) comes from the boundary integrals R.quad_sv_grad, d(b, r)/d slot from mp.diff of the orbit algebra (never
    through the quadrature), dF/dc is the solution vector, dF/dfr is in closed form.  Where the flux is defined as 0 (body
    not in front, or b >= 1 + ror) every derivative is 0; sin i and c / R_star carry a derivative only with light delay."""
    zero = mp.mpf(0)
    circular = rec["e"] == 0
    memo = {}
    ror, fr = rec["ror"], rec["fr"]
    found = None
    for sigma in ((1, -1) if secondary else (1,)):
        b, y1 = _seen(t, rec, circular, sigma, light_delay, memo)
        Z = -rec["si"] * y1
        if (Z > 0 if sigma > 0 else Z < 0) and b < 1 + ror:
            found = (sigma, b)
            break
    if found is None:
        return zero, [zero] * 11, [zero] * 6, b, False
    sigma, b = found
    occ = sigma < 0
    bq, rq = (b / ror, 1 / ror) if occ else (b, ror)
    s = R.quad_sv(bq, rq)
    cc = c[3:6] if occ else c[0:3]
    Fq = s[0] * cc[0] + s[1] * cc[1] + s[2] * cc[2] - 1
    wq = (fr / (1 + fr) if occ else 1 / (1 + fr)) if secondary else mp.mpf(1)
    F = wq * Fq
    if not grad:
        return F, None, None, b, occ
    dsdb, dsdr = R.quad_sv_grad(bq, rq)
    dF_db = wq * sum(d * k for d, k in zip(dsdb, cc))
    dF_dr = wq * sum(d * k for d, k in zip(dsdr, cc))

    def pair(q):
        # (a perturbed e off an exactly circular record takes the eccentric branch: one-sided derivative at e = 0)
        bb = _seen(t, q, circular and q["e"] == 0, sigma, light_delay, memo)[0]
        return (bb / q["ror"], 1 / q["ror"]) if occ else (bb, q["ror"])

    dF = {}
    for k in REC_SLOTS + (DELAY_SLOTS if light_delay else ()):
        if k == "ci" and rec["ci"] == 0:
            dF[k] = zero               # b is even in cos i: the derivative at cos i = 0 is 0 identically
            continue
        seen = {}

        def at(x, k=k, seen=seen):
            if x not in seen:
                q = dict(rec)
                q[k] = x
                seen[x] = pair(q)
            return seen[x]

        opts = dict(direction=1) if (k == "e" and circular) else {}
        dbq = mp.diff(lambda x: at(x)[0], rec[k], **opts)
        drq = mp.diff(lambda x: at(x)[1], rec[k], **opts) if k == "ror" else zero
        dF[k] = dF_db * dbq + dF_dr * drq
    dfr = ((Fq if occ else -Fq) / (1 + fr) ** 2) if secondary else zero
    out = [dF[k] for k in REC_SLOTS] + [dfr] + [dF.get(k, zero) for k in DELAY_SLOTS]
    dc = [zero] * 6
    o = 3 if occ else 0
    for j in range(3):
        dc[o + j] = wq * s[j]
    return F, out, dc, b, occ


def record_cadence(t, rec, c, secondary, texp=None, sdt=None, sw=None, grad=True, light_delay=False):
    """record_sample summed over an exposure stencil given as numbers (offsets in units of texp, weights)"""
    if texp is None:
        return record_sample(mp.mpf(t), rec, c, secondary, grad, light_delay)[:3]
    F, dF, dc = mp.mpf(0), [mp.mpf(0)] * 11, [mp.mpf(0)] * 6
    for dk, wk in zip(sdt, sw):
        f, a, b_, _, _ = record_sample(mp.mpf(t) + mp.mpf(texp) * mp.mpf(dk), rec, c, secondary, grad, light_delay)
        F += mp.mpf(wk) * f
        if grad:
            dF = [x + mp.mpf(wk) * y for x, y in zip(dF, a)]
            dc = [x + mp.mpf(wk) * y for x, y in zip(dc, b_)]
    return F, dF, dc


def light_curve(orbit, r, u, times, texp=None, oversample=7, order=0):
    c = get_cl(*u)
    if texp is None:
        return [flux_one(orbit, r, c, t) for t in times]
    dt, w = stencil(oversample, order)
    texp = mp.mpf(texp)
    return [sum(wk * flux_one(orbit, r, c, mp.mpf(t) + texp * dk) for dk, wk in zip(dt, w)) for t in times]


def secondary_light_curve(orbit, r, u_primary, u_secondary, sbr, times, texp=None, oversample=7, order=0):
    """secondary_eclipse.py:45-70"""
    lc1 = light_curve(orbit, r, u_primary, times, texp, oversample, order)
    o2 = orbit.flip(mp.mpf(r))
    lc2 = light_curve(o2, orbit.r_star, u_secondary, times, texp, oversample, order)
    k = mp.mpf(r) / orbit.r_star
    fr = mp.mpf(sbr) * k * k
    return [(a + fr * b) / (1 + fr) for a, b in zip(lc1, lc2)]
