"""What tools/make_contact_golden.py, tests/test_contact_host.py and tests/test_gpu_contact.py share: the table of geometries
behind the multiprecision fixture tests/golden/contact_mp.npz, the allowances -- derived here, none taken from the code
under test -- and a float64 transcription of the acceptance rules of exo::contact_solve's fast path, which only NAMES the
path an entry takes (no value of it is compared with anything).  numpy only: the generator imports the table, the tests
import everything.

Definition (the generator's, in the true anomaly f)
----------
Delta^2(f) = rho(f)^2 (1 - sin^2 i sin^2(omega + f)),  rho(f) = a (1 - e)(1 + e) / (1 + e cos f);  conjunction f_c = pi/2 - omega;
contacts = the first zero of g = Delta^2 - L^2 on each side of f_c within +-pi/2;  no contact: Delta(f_c) >= L or no such
zero.  M = E - e sin E with E on the branch continuous with f.  Two solves per entry: ``M_left / M_right`` with the seven
float64 numbers ops.contact_points receives (``inputs``), and the windows ``ts, te, ts2, te2`` with the constructor's algebra
carried out in mpmath on the float64 constructor inputs (``ctor``), wrap rules of keplerian.py:755-763 included.

Allowances (EPS = 2.3e-16; theta = omega + f - pi/2 is the angle the solvers work in, d theta = d f)
----------
* a root.  The solvers stop where the computed g changes sign, so the error of theta is (rounding of g) / |g'|.  g is
  rho^2 q - L^2 with q = 1 - sin^2 i sin^2(omega + f) and rho = p / D, D = 1 + e cos f, cos f = sin w cos theta - cos w sin theta.
  Each factor carries a few roundings of its own size, except D: the rounding of e cos f is of the size of the two products
  behind cos f, |sin w cos theta| + |cos w sin theta|, whatever is left of D after the cancellation away from periastron,
  and rho^2 doubles it.  Sum of magnitudes:
      T = rho^2 q (1 + 2 e (|sin w cos theta| + |cos w sin theta|) / D) + L^2        (``T_*`` in the fixture)
  Then d M = (dM/df) T / |g'|, dM/df = (1 - e^2)^(3/2) / D^2, plus the last step M = E - e sin E, a difference whose rounding
  is of the size of its terms, |E| + e |sin E| (>= |M|; at e = 0.999 near periastron M is 1e-3 of E):
  and the turn from theta to f = theta + pi/2 - omega, three angles added at their own sizes, which dM/df carries too
  (89 at the apoapsis of e = 0.999, where it is the largest term):
      allow_M = C EPS ((dM/df)(T / |g'| + |theta| + pi/2 + |omega|) + |E| + e |sin E|)
  (With EPS |M| for the last step and without the angles, the float64 oracle is 430 x and 7 500 x over at e = 0.999 near
  periastron and at apoapsis; with them the constant below is 2.6 and the allowance tighter everywhere else.)
  sin^2 i is 1 - cos^2 i of the float64 cos i: no implementation reads the sin i it is handed.
* a window slot.  ts = ((M_left - M0) / n wrapped): the same with M0's own |E0| + e |sin E0|, the constructor's roundings
  of a (cbrt of a product: 4) and cos i (4) entering g as 2 rho^2 q each (8 x 2 = 16 rho^2 q more in T), all divided by n,
  and 4 EPS P for the wrap (+ hp, - P floor, - hp, the fold) at the size of P; ts2 / te2: 4 EPS P more for the shift.
      allow_t = C EPS ((dM/df)((T + 16 rho^2 q) / |g'| + angles) + |E| + e |sin E| + |E0| + e |sin E0|) / n + 4 (8) EPS P
* a cadence's distance to a contact additionally carries the rounding of the window's centre at the size of t0:
  EPS |t0| (5.4e-10 d at BJD 2 458 001), and of the cadence's own phase, EPS |t - t0|.
* the circular closed form hdur = (P / 2) asin(x) / pi, x = R sqrt(arg) / (a sin i), arg = (1 + k)^2 - b^2:
      allow = EPS hdur (4 + kappa (8 + kappa_arg)),  kappa = x / (sqrt(1 - x^2) asin x),  kappa_arg = ((1 + k)^2 + b^2) / arg
  (four roundings after the asin; before it the eight of a, sin i, the quotient, the root and the product, and the
  difference arg amplified by the size of its terms).
C is the one constant the derivation leaves open (how many roundings each factor of g carries, and the stopping width of
the solvers).  It is set from oracle.numpy_port.contact_points -- an 80-step bisection on libm, independent of the kernel's
fast path and false position -- measured against this fixture on the CPU: worst ratio at C = 1 is ORACLE_WORST below, and
C = 4 x that.  Never from the kernel or from the host build of its header.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.3e-16
PI = float(np.pi)
G_GRAV = 2942.2062175044193          # R_sun^3 / M_sun / day^2 (orbits/constants.py:32)
N_CAD = 64
BJD = 2458001.0
ORACLE_WORST = 0.66                  # measured 0.655: tests/test_contact_host.py prints and bounds it
C = 4.0 * ORACLE_WORST

# ------------------------------------------------------------------------------------------------------------------------
# The geometries.  aor = a / R_star (the period follows from it), ecc (None: the circular packing, PACK_CIRCULAR), omega,
# b: a number, or ("graze", k): (1 + r / R)(1 - 10^-k), or ("miss", x): (1 + r / R)(1 + x); r in R_sun; sec: an occultation is
# asked for; path: what the entry is BUILT for -- "fast" / "bracket" (both contacts) or None (whatever it takes) -- and why.
# ------------------------------------------------------------------------------------------------------------------------
QUADRANTS = (0.0, 0.5 * PI, PI, -0.5 * PI)        # float64 angles: cos(fl(pi / 2)) = 6e-17, not 0


def _c(name, aor, ecc, omega, b, r, **kw):
    d = dict(name=name, aor=aor, ecc=ecc, omega=omega, b=b, r=r, r_star=1.0, m_star=1.0, t0=0.37, sec=False, path=None,
             why="", flag=False)
    d.update(kw)
    return d


def _table():
    out = []
    # A. eccentricity x omega; periastron at 3 R_star or beyond; transits at periastron (omega = pi/2), apoapsis (-pi/2),
    #    quadrature (0, pi) and between.  Every other one with an occultation.
    for e in (0.0, 0.3, 0.9, 0.95, 0.99, 0.995, 0.999):
        for j, w in enumerate(QUADRANTS + (1.1, -2.3, 0.4)):
            out.append(_c(f"A_e{e}_w{j}", max(12.0, 3.0 / (1 - e)), e, w, 0.4, 0.1, sec=(j % 2 == 0),
                          r_star=0.9 if j == 4 else 1.0, m_star=1.1 if j == 4 else 1.0))
    # B. size: a / R from 1.5 (periastron just outside L) to 500, r / R from 1e-3 to 1.2
    for aor in (1.5, 1.6, 2.0, 3.0, 5.0, 20.0, 100.0, 500.0):
        for r in (1e-3, 0.01, 0.1, 0.5, 1.0, 1.2):
            e = 0.2
            if aor == 1.5:       # periastron distance = L (1 + 1e-3)
                e = 0.05
                aor_ = (1 + r) * (1 + 1e-3) / (1 - e)
                out.append(_c(f"B_peri_r{r}", aor_, e, 0.7, 0.3, r))
            else:
                out.append(_c(f"B_a{aor}_r{r}", aor, e, 0.7, 0.3, r, sec=(r == 0.1)))
    # C. impact parameter: 0 exactly, 1e-9, grazing
    for e in (0.3, 0.9, 0.99):
        for jw, w in enumerate((1.1, -2.0)):
            for b in (0.0, 1e-9, ("graze", 2), ("graze", 4), ("graze", 6), ("graze", 8)):
                bn = b if not isinstance(b, tuple) else f"g{b[1]}"
                out.append(_c(f"C_e{e}_w{jw}_b{bn}", 15.0 / (1 - e), e, w, b, 0.1, why="grazing chord" if isinstance(b, tuple) else ""))
    for r in (1e-3, 1.2):
        for b in (0.0, 1e-9, ("graze", 2), ("graze", 4), ("graze", 6), ("graze", 8)):
            bn = b if not isinstance(b, tuple) else f"g{b[1]}"
            out.append(_c(f"C_r{r}_b{bn}", 25.0, 0.3, 1.1, b, r))
    # D. no contact: the chord misses, or the orbit is so small that the disks never part
    for e in (0.3, 0.9, 0.99):
        for jw, w in enumerate((1.1, -2.0)):
            for x in (1e-6, 0.3):
                out.append(_c(f"D_e{e}_w{jw}_miss{x}", 15.0 / (1 - e), e, w, ("miss", x), 0.1, flag=True, sec=(x == 0.3)))
    for aor, e, r in ((1.05, 0.0, 0.1), (1.2, 0.1, 0.5), (1.4, 0.3, 0.1), (1.3, 0.05, 1.2), (1.02, 0.0, 0.05), (1.8, 0.4, 0.2),
                      (2.0, 0.0, 1.2), (1.1, 0.02, 0.3)):
        out.append(_c(f"D_small_a{aor}_e{e}", aor, e, 0.7, 0.2, r, flag=True))
    # E. both sides of each acceptance rule of the fast path
    #    |sin theta| <= 0.5: central transits of nearly circular orbits, sin theta ~ (1 + r) / (a / R) = 1.1 / aor
    for aor in (1.9, 2.0, 2.1, 2.15, 2.19, 2.21, 2.25, 2.3, 2.5, 3.0):
        out.append(_c(f"E_wide_a{aor}", aor, 0.01, 0.3, 0.0, 0.1, path="bracket" if aor < 2.19 else ("fast" if aor > 2.21 else None),
                      why="window beyond 30 degrees" if aor < 2.19 else "window within 30 degrees"))
    #    S < 0.98 in the fixed-point rounds: S ~ (L / rho)^2
    for aor in (1.105, 1.108, 1.112, 1.12, 1.2):
        out.append(_c(f"E_S_a{aor}", aor, 0.0, 0.3, 0.0, 0.1, path="bracket", why="S >= 0.98" if aor < 1.111 else "S < 0.98, window beyond 30 degrees"))
    #    a distance that changes fast across the window: high e, small periastron, transits off the apsides
    for e in (0.8, 0.9, 0.95):
        for q in (1.5, 2.5, 4.0):
            for jw, w in enumerate((0.0, 0.3, PI - 0.3, 2.5)):
                out.append(_c(f"E_fast_e{e}_q{q}_w{jw}", q / (1 - e), e, w, 0.2, 0.1, sec=(jw == 1)))
    # F. an occultation at apoapsis of e = 0.99 whose window is nearly the whole period (the boundary
    #    fallback itself cannot be reached with consistent inputs), and occultations of high-e transits near periastron
    out.append(_c("F_occ_apoapsis_e099", 120.0, 0.99, 0.5 * PI, 0.0, 0.1, sec=True))
    out.append(_c("F_occ_apoapsis_e0999", 1100.0, 0.999, 1.5, 0.1, 0.1, sec=True))
    out.append(_c("F_occ_near_transit_w0", 200.0, 0.99, 0.0, 0.1, 0.1, sec=True))
    out.append(_c("F_occ_near_transit_wpi", 200.0, 0.99, PI, 0.1, 0.1, sec=True))
    out.append(_c("F_occ_e09_wm2", 40.0, 0.9, -2.0, 0.3, 0.1, sec=True))
    # H. the circular packing (closed form), degenerate ones included: b > 1 + k (arg < 0) and a sin i so small that x > 1
    for aor in (1.05, 3.0, 12.0, 100.0):
        for b in (0.0, 0.5, ("graze", 4), ("miss", 1e-6), ("miss", 0.3)):
            bn = b if not isinstance(b, tuple) else f"{b[0]}{b[1]}"
            miss = isinstance(b, tuple) and b[0] == "miss"
            out.append(_c(f"H_circ_a{aor}_b{bn}", aor, None, 0.0, b, 0.1, sec=(aor == 12.0), flag=miss or (aor == 1.05 and b in (0.0, 0.5))))
    # G. time layout: BJD-sized t0 (transits long enough that 1e-6 of the duration clears the rounding of t0)
    for name in ("A_e0.3_w4", "A_e0.9_w5", "A_e0.95_w0", "A_e0.99_w4", "A_e0.995_w6", "A_e0.999_w2", "A_e0.0_w4", "B_a5.0_r0.1",
                 "B_a20.0_r0.5", "B_a100.0_r1.2", "C_e0.3_w0_b0.0", "C_e0.9_w1_b1e-09", "C_e0.3_w0_bg2", "E_wide_a2.0", "E_wide_a2.5",
                 "E_fast_e0.9_q2.5_w1", "F_occ_e09_wm2", "H_circ_a12.0_b0.5", "H_circ_a3.0_b0.0", "D_e0.3_w0_miss0.3"):
        src = next(c for c in out if c["name"] == name)
        d = dict(src)
        d.update(name="G_bjd_" + name, t0=BJD + 0.123)
        out.append(d)
    return out


CASES = _table()
NAMES = [c["name"] for c in CASES]


def b_of(c):
    k = c["r"] / c["r_star"]
    b = c["b"]
    if isinstance(b, tuple):
        return (1 + k) * (1 - 10.0 ** -b[1]) if b[0] == "graze" else (1 + k) * (1 + b[1])
    return float(b)


def period_of(c):
    a = c["aor"] * c["r_star"]
    return float(2 * PI * np.sqrt(a ** 3 / (G_GRAV * c["m_star"])))


def ctor_inputs(c):
    """(period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr): the EXO_IN_* order of ops.pack_records; the circular
    packing reads ecc = omega = 0"""
    e = 0.0 if c["ecc"] is None else c["ecc"]
    return np.array([period_of(c), c["t0"], b_of(c), e, c["omega"], c["r"], c["m_star"], c["r_star"], 0.0, 0.3])


def contact_inputs(ct):
    """(a, e, cos w, sin w, cos i, sin i, L) in float64 from a row of ctor_inputs, as KeplerianOrbit.__init__ forms them"""
    P, t0, b, e, w, r, ms, rs, mp_, sbr = ct
    a = np.cbrt(G_GRAV * (ms + mp_) * P * P / (4 * PI * PI))
    cw, sw = np.cos(w), np.sin(w)
    ci = (1 + e * sw) / ((1 - e) * (1 + e)) * rs / a * b
    si = np.sqrt(max(0.0, 1 - ci * ci))
    return np.array([a, e, cw, sw, ci, si, rs + r])


# ------------------------------------------------------------------------------------------------------------------------
# which path exo::contact_solve takes (float64 transcription of its acceptance rules: sqrt, + - * / only, so the same
# on every IEEE machine).  Returns per side "fast" or the rule that sent it to the bracketing solver.
# ------------------------------------------------------------------------------------------------------------------------
def _gs(s, p, e, cw, sw, ci, L):
    c = np.sqrt(max(1.0 - s * s, 0.0))
    D = 1.0 + e * (sw * c - cw * s)
    rho = p / D
    q = ci * ci + (1.0 - ci * ci) * s * s
    dD = -e * (sw * s / max(c, 1e-300) + cw)
    return rho * rho * q - L * L, rho * rho * (2.0 * (1.0 - ci * ci) * s - 2.0 * q * dD / D)


def fast_path(inp, max_abs_s=0.5, probes=True):
    a, e, cw, sw, ci, si, L = [float(x) for x in inp]
    p = a * (1.0 - e * e)
    out = []
    with np.errstate(all="ignore"):
        for sgn in (-1.0, 1.0):
            si2 = 1.0 - ci * ci
            if not si2 > 1e-12:
                out.append("face-on"); continue
            s, why = 0.0, None
            for _ in range(2):
                c = np.sqrt(max(1.0 - s * s, 0.0))
                rho = p / (1.0 + e * (sw * c - cw * s))
                S = (L * L / (rho * rho) - ci * ci) / si2
                if not (S > 0.0 and S < 0.98):
                    why = "S"; break
                s = sgn * np.sqrt(max(S, 0.0))
            if why:
                out.append(why); continue
            step = 1.0
            for _ in range(8):
                g, dg = _gs(s, p, e, cw, sw, ci, L)
                step = g / dg
                s -= step
                if not ((s * sgn > 0.0) and (abs(s) < 0.99) and (step == step)):
                    why = "newton"; break
                if abs(step) <= 1e-16 * abs(s):
                    break
            if why:
                out.append(why); continue
            if not abs(step) <= 4e-16 * abs(s):
                out.append("converge"); continue
            if not abs(s) <= max_abs_s:
                out.append("wide"); continue
            if probes and not all(_gs(0.25 * k * s, p, e, cw, sw, ci, L)[0] < 0.0 for k in (1, 2, 3)):
                out.append("probe"); continue
            out.append("fast")
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------
# fixture and allowances
# ------------------------------------------------------------------------------------------------------------------------
def load():
    g = dict(np.load(os.path.join(GOLD, "contact_mp.npz")))
    assert [str(x) for x in g["names"]] == NAMES, "tests/golden/contact_mp.npz is not the fixture of this case table"
    return g


def has_contacts(g):
    return g["flag"] == 0


def allow_M(g, c=None):
    """(n_entry, 2): allowance of M_left, M_right (NaN for the entries without contacts)"""
    c = C if c is None else c
    w = np.abs(np.arctan2(g["inputs"][:, 3], g["inputs"][:, 2]))[:, None]
    return c * EPS * (g["dMdf"] * (g["T"] / g["gprime"] + np.abs(g["theta"]) + 0.5 * PI + w) + g["Eterm"])


def allow_t(g, c=None):
    """(n_entry, 4): allowance of ts, te, ts2, te2 as the packing kernel and KeplerianOrbit._transit_window form them"""
    c = C if c is None else c
    n = (2 * PI / g["ctor"][:, 0])[:, None]
    ang = np.abs(g["w_theta"]) + 0.5 * PI + np.abs(g["ctor"][:, 4:5]) + np.array([0.0, 0.0, PI, PI])
    core = c * EPS * (g["w_dMdf"] * ((g["w_T"] + 16 * g["w_Tin"]) / g["w_gprime"] + ang) + g["w_Eterm"] + g["w_E0term"]) / n
    wrap = EPS * g["ctor"][:, :1] * np.array([4.0, 4.0, 8.0, 8.0])
    return core + wrap


def allow_circ(g):
    """(n_entry,): allowance of the closed-form half duration (NaN where the entry is not circular or degenerate)"""
    x, arg = g["circ_x"], g["circ_arg"]
    k = g["ctor"][:, 5] / g["ctor"][:, 7]
    b = g["ctor"][:, 2]
    with np.errstate(all="ignore"):
        kappa = x / (np.sqrt(1 - x * x) * np.arcsin(x))
        kappa_arg = ((1 + k) ** 2 + b * b) / arg
        return EPS * g["circ_hdur"] * (4 + kappa * (8 + kappa_arg))


def allow_cadence(g, i, t):
    """allowance of the distance of cadence(s) t of entry i to the nearest contact: the widest window slot, the rounding
    of the window's centre at the size of t0 and of the phase at the size of t - t0"""
    a = np.nanmax(allow_t(g)[i]) if g["circular"][i] == 0 else allow_circ(g)[i] + 8 * EPS * g["ctor"][i, 0]
    return a + EPS * abs(g["ctor"][i, 1]) + EPS * np.abs(t - g["ctor"][i, 1])


FLUX_RESOLUTION = 1e-13      # 20 x the absolute tolerance of the solution vector (5e-15, tests/test_gpu_orbit_mp.py)


def flux_floor(g, i, limb=0.18, limb_occ=0.05):
    """a lower bound of |flux| at the inside cadences of entry i from the mp overlap depth d = L - Delta (R_star): the lens
    of two disks of radii 1 and k overlapping by d << min(1, k) is two segments on a chord of half-length h, h^2 = 2 d k / (1 + k),
    with sagittas adding to d: area (4/3) h d; times the intensity at the limb of the disk being covered, which for quadratic
    limb darkening is the smallest on it: (1 - u1 - u2) / (pi (1 - u1/3 - u2/6)) = 0.184 for u = (0.3, 0.2), and for an
    occultation sbr times that of the planet's u = (0.4, 0.1): 0.3 x 0.187 = 0.056.  A cadence whose true flux is below what
    float64 resolves of a flux of size 1 may come out 0 on any route; above FLUX_RESOLUTION it may not."""
    k = g["ctor"][i, 5] / g["ctor"][i, 7]
    d = np.minimum(g["cad_depth"][i], 0.1 * min(1.0, k))
    with np.errstate(invalid="ignore"):
        area = 4.0 / 3.0 * np.sqrt(2 * k / (1 + k)) * d ** 1.5
    return np.where(g["cad_in"][i] == 2, limb_occ, limb) * area


def report(label, **figures):
    with np.errstate(all="ignore"):
        print(label + ": " + "  ".join(f"{k} = {float(np.nanmax(v)):.3g}" for k, v in figures.items()))
