"""What tests/test_orbit_mp_host.py and tests/test_gpu_orbit_mp.py share: the multiprecision fixture
tests/golden/orbit_mp.npz (tools/make_orbit_golden.py), the tolerances -- each one derived here, none taken from the code
under test -- and the float64 oracle's own error ("unit") on the same input.

Tolerances
----------
EPS = 2.3e-16 throughout (a little over one ulp of 1).

* sin f, cos f of the Kepler op, M exact:  8 EPS (1 + |M_red| df/dM), with M_red (M reduced to [-pi, pi] in mpmath) and
  df/dM = hypot(d sinf / dM, d cosf / dM) from the fixture: eight roundings of a value of size 1, plus the rounding of the
  reduced argument carried through the solve.
* values of the radial velocity and of the orbit vectors:  8 EPS (S + |t - tp| |dv/dtp|) per element, S the system's largest
  |value| over its series, dv/dtp from the fixture Jacobian (= -n dv/dM, so the second term is |M| |dv/dM|: the two roundings
  of a plain product (t - tp) n).
* elementwise partials of the Kepler op, entry by entry:  |want| max(16 u, 8 ulp) + (first-order propagation of the value
  bound above through the closed form), where u is the relative error against the fixture of the float64 closed form in
  (1 - e)(1 + e) form fed with the fixture's correctly rounded sin f, cos f, on the same points.  With F = df/dM,
  G = df/de = (1 + q) sin f / (1 - e^2), q = 1 + e cos f and d the value bound:
      d sinf/dM = cos f F :   d (F + |cos f| F 2 e / q)            d cosf/dM = -sin f F :   d (F + |sin f| F 2 e / q)
      d sinf/de = cos f G :   d (|G| + |cos f| (e |sin f| + (1 + q)) / (1 - e^2))
      d cosf/de = -sin f G:   d (2 |sin f| (1 + q) + e sin^2 f) / (1 - e^2)
  The 2 e / q terms are the bound divided by 1 + e cos f: the reverse pass of the op only has the rounded cos f, and
  1 + e cos f cancels at apoapsis as e -> 1.
* vector-Jacobian products, per (system, parameter):  |error| / sum_n |g_n dv_n/dp| <= max(16 unit, 1e-13), the sum from
  the fixture Jacobian, the unit that same ratio for oracle.numpy_port on the same input and cotangent (the convention of
  tests/test_gpu_estimators.py; 16 covers the summation order across 256 lanes and the reduction tree).
"""
import os

import numpy as np

from oracle import numpy_port as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.3e-16
ULP = 2.220446049250313e-16
MODES = ("pos", "vel", "acc")
UNIT_CEILING = 1e-12        # condition on the inputs: the oracle's unit of every gradient system (host test)
VJP_FLOOR = 1e-13


def load():
    return np.load(os.path.join(GOLD, "orbit_mp.npz"))


# ------------------------------------------------------------------------------------------------
# Kepler op
# ------------------------------------------------------------------------------------------------
def kepler_points(g, which):
    """(M, e, M_red, sinf, cosf, dsinf_dM, dcosf_dM, dsinf_de, dcosf_de) of 'wide' (orbit_mp.npz) or 'r1' (kepler.npz,
    whose M_red is taken with the float64 remainder: its |M| <= 400)"""
    if which == "wide":
        return tuple(g["kw_" + k] for k in ("M", "e", "Mred", "sinf", "cosf", "dsinf_dM", "dcosf_dM", "dsinf_de", "dcosf_de"))
    k = np.load(os.path.join(GOLD, "kepler.npz"))
    Mred = np.remainder(k["M"] + np.pi, 2 * np.pi) - np.pi
    return (k["M"], k["ecc"], Mred) + tuple(k[n] for n in ("sinf", "cosf", "dsinf_dM", "dcosf_dM", "dsinf_de", "dcosf_de"))


def kepler_value_tol(pts):
    M, e, Mred, s, c, dsM, dcM, dse, dce = pts
    return 8 * EPS * (1 + np.abs(Mred) * np.hypot(dsM, dcM))


def kepler_closed_form(sinf, cosf, e):
    """the four partials from the float64 closed form, 1 - e^2 as (1 - e)(1 + e)"""
    ome2 = (1 - e) * (1 + e)
    q = 1 + e * cosf
    dfdM = q * q / ome2 ** 1.5
    dfde = (1 + q) * sinf / ome2
    return cosf * dfdM, -sinf * dfdM, cosf * dfde, -sinf * dfde


def _kepler_propagation(pts):
    """|d partial / d sinf| + |d partial / d cosf| of the four closed-form partials (module docstring)"""
    M, e, Mred, s, c, dsM, dcM, dse, dce = pts
    ome2 = (1 - e) * (1 + e)
    F = np.hypot(dsM, dcM)
    q = np.sqrt(F) * ome2 ** 0.75          # 1 + e cos f from the fixture's df/dM: no cancellation
    G = (1 + q) * np.abs(s) / ome2
    return (F + np.abs(c) * F * 2 * e / q,
            F + np.abs(s) * F * 2 * e / q,
            G + np.abs(c) * (e * np.abs(s) + (1 + q)) / ome2,
            (2 * np.abs(s) * (1 + q) + e * s * s) / ome2)


def kepler_partial_tol(pts):
    """absolute allowances of (dsinf_dM, dcosf_dM, dsinf_de, dcosf_de), and the closed form's own relative error u"""
    want = pts[5:]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = [np.where(w != 0, np.abs(cf - w) / np.abs(w), 0.0) for cf, w in zip(kepler_closed_form(pts[3], pts[4], pts[1]), want)]
    d = kepler_value_tol(pts)
    tol = [np.abs(w) * np.maximum(16 * uu, 8 * ULP) + d * pp for w, uu, pp in zip(want, u, _kepler_propagation(pts))]
    return tol, u


def kepler_closed_form_bound(pts):
    """what a float64 closed form fed with the fixture's ROUNDED sin f, cos f can keep: 16 ulp of the partial (about ten
    roundings and a pow) plus the half-ulp rounding of each input carried through (which 1 + e cos f amplifies at apoapsis)"""
    return [np.abs(w) * 16 * ULP + 0.5 * ULP * pp for w, pp in zip(pts[5:], _kepler_propagation(pts))]


# ------------------------------------------------------------------------------------------------
# radial velocity and orbit vectors
# ------------------------------------------------------------------------------------------------
def n_systems(g):
    return g["t"].shape[0]


def case(g, i, op):
    """(record, want [N(,3)], Jacobian [N(,3),npar]) of system i for op in ('rv', 'pos', 'vel', 'acc')"""
    if op == "rv":
        return g["rv_params"][i], g["rv"][i], g["rv_jac"][i]
    return g["ov_params"][i], g[f"ov_{op}"][i], g[f"ov_{op}_jac"][i]


def value_tol(g, i, op):
    rec, want, J = case(g, i, op)
    dt = np.abs(g["t"][i] - rec[1])
    dt = dt if want.ndim == 1 else dt[:, None]
    return 8 * EPS * (np.abs(want).max() + dt * np.abs(J[..., 1]))


def cotangent(i, op, shape):
    """the seeded cotangent of (system, op): the same one wherever that pair is checked"""
    return np.random.default_rng(7000 + 10 * i + (("rv",) + MODES).index(op)).normal(size=shape)


def vjp_want(J, go):
    """(g . J, sum |g| |J|) over the epochs (and components), per parameter"""
    ax = tuple(range(go.ndim))
    den = np.tensordot(np.abs(go), np.abs(J), axes=(ax, ax))
    return np.tensordot(go, J, axes=(ax, ax)), np.where(den > 0, den, 1.0)


def oracle(t, rec, op, go=None):
    """oracle.numpy_port on one record: values, and the VJP with ``go`` if given"""
    rec = np.asarray(rec)[None, None]
    if op == "rv":
        if go is None:
            return P.radial_velocity(t, rec)[0, :, 0], None
        out, gp = P.radial_velocity_vjp(t, rec, go[None, :, None])
        return out[0, :, 0], gp[0, 0]
    mode = MODES.index(op)
    if go is None:
        return P.orbit_vector(t, rec, mode)[0, :, 0], None
    out, gp = P.orbit_vector_vjp(t, rec, go[None, :, None, :], mode)
    return out[0, :, 0], gp[0, 0]


def oracle_unit(g, i, op):
    """the oracle's VJP error over sum |terms|, per parameter, with the cotangent every test uses for (i, op)"""
    rec, want, J = case(g, i, op)
    go = cotangent(i, op, want.shape)
    _, gp = oracle(g["t"][i], rec, op, go)
    gw, den = vjp_want(J, go)
    return np.abs(gp - gw) / den


def vjp_tol(unit):
    return np.maximum(16 * unit, VJP_FLOOR)


def report(label, **figures):
    with np.errstate(all="ignore"):
        print(label + ": " + "  ".join(f"{k} = {float(np.nanmax(v)):.3g}" for k, v in figures.items()))
