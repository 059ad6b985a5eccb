"""What tests/test_astrometry_host.py and tests/test_gpu_astrometry.py share: the multiprecision fixture
tests/golden/astrometry_mp.npz (tools/make_astrometry_golden.py), the tolerance -- the rule of tests/rv_like_cases.py, derived
there and restated here, not taken from the code under test -- and the float64 restatement's own error ("unit") on the same
inputs.

Tolerance
---------
Every output of exo_astrometry_loglike_vjp_f64 is a sum over the epochs.  For each scalar output

    |error| / (sum of the absolute values of its terms)  <=  max(16 unit, 1e-13),

where the terms are the products that are added, before any cancellation between them -- wr r^2 / 2, |log s2r| / 2,
wt delta^2 / 2, |log s2t| / 2 and the constant n log 2 pi for the value; per epoch |kappa d rho_m / d rec_k| and
|lambda d theta_m / d rec_k| for the record's gradient; (kappa^2 + wr) / 2 and (lambda^2 + wt) / 2 for the jitters -- summed in
mpmath by the fixture's generator, and `unit` is that same ratio for the float64 numpy restatement below
(oracle.numpy_port.orbit_vector with its Jacobian, plain numpy for the rest) on the same inputs.  A term carries the rounding
of r = rho_n - rho_m and of delta, each a difference of numbers of the size of the signal: relative to the sum of absolute
terms that is a few EPS times signal / residual, the same for any float64 evaluation, and it is what the unit measures; the
factor 16 covers the order of summation (up to 256 lanes, a shuffle tree, the waves in turn) against numpy's pairwise sums, and
the floor 1e-13 a unit that happens to be tiny.

Condition on the inputs: every system's unit <= 1e-12 (UNIT_CEILING).  The generator checks it when it writes the fixture,
the host test asserts it.
"""
import os
from types import SimpleNamespace

import numpy as np

from oracle import numpy_port as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYSTEMS = ("a", "b", "c", "d")
OUTPUTS = ("loglike", "gparams", "gjit2_rho", "gjit2_theta")
UNIT_CEILING = 1e-12
FLOOR = 1e-13
NARROW_CAD = 128                 # exo_astrometry_core.hpp kNarrowCad (system c has NARROW_CAD + 1 epochs)
WIDE = 256                       # kWide (system d has WIDE + 44 epochs: some lanes take two epochs, the others one)
N_EPOCH = dict(a=1, b=45, c=NARROW_CAD + 1, d=WIDE + 44)


def load():
    return np.load(os.path.join(GOLD, "astrometry_mp.npz"))


def case(g, name):
    """inputs of system ``name`` (jit2_rho / jit2_theta: None where the fixture passes a null pointer) and the wanted outputs
    with their normalisers (``want``, ``norm``: dicts over OUTPUTS)"""
    get = lambda k: g[f"{name}_{k}"] if f"{name}_{k}" in g.files else None  # noqa: E731
    c = SimpleNamespace(name=name, **{k: get(k) for k in ("t", "rho", "theta", "var_rho", "var_theta", "params", "jit2_rho",
                                                          "jit2_theta")})
    c.want = {k: get(k) for k in OUTPUTS}
    c.norm = {k: get("n_" + k) for k in OUTPUTS}
    return c


def restatement(c):
    """the definitions of include/exoplanet_amd.h (exo_astrometry_loglike_vjp_f64) in float64 numpy"""
    D, N = c.params.shape[0], c.t.size
    out, J = P.orbit_vector(c.t, c.params[:, None, :], jac=True)          # (D, N, 1, 3), (D, N, 1, 3, 10)
    X, Y, JX, JY = out[:, :, 0, 0], out[:, :, 0, 1], J[:, :, 0, 0, :], J[:, :, 0, 1, :]
    cn, sn = np.cos(c.theta)[None, :], np.sin(c.theta)[None, :]
    rho2 = X * X + Y * Y
    rho_m = np.sqrt(rho2)
    delta = np.arctan2(Y * cn - X * sn, X * cn + Y * sn)
    zero = np.zeros(D)
    s2r = np.broadcast_to(c.var_rho, (N,))[None, :] + (zero if c.jit2_rho is None else c.jit2_rho)[:, None]
    s2t = np.broadcast_to(c.var_theta, (N,))[None, :] + (zero if c.jit2_theta is None else c.jit2_theta)[:, None]
    wr, wt = 1.0 / s2r, 1.0 / s2t
    r = c.rho[None, :] - rho_m
    kappa, lam = wr * r, -wt * delta
    drho = (X[..., None] * JX + Y[..., None] * JY) / rho_m[..., None]
    dtheta = (X[..., None] * JY - Y[..., None] * JX) / rho2[..., None]
    return dict(loglike=-0.5 * (wr * r * r + np.log(s2r) + wt * delta * delta + np.log(s2t)).sum(1) - N * np.log(2 * np.pi),
                gparams=np.einsum("dn,dnk->dk", kappa, drho) + np.einsum("dn,dnk->dk", lam, dtheta),
                gjit2_rho=0.5 * (kappa * kappa - wr).sum(1), gjit2_theta=0.5 * (lam * lam - wt).sum(1))


def ratio(got, want, norm):
    """|got - want| over the normaliser; where there are no terms: 0 for an exact 0, inf otherwise"""
    err = np.abs(np.asarray(got) - want)
    return np.where(norm > 0, err / np.where(norm > 0, norm, 1.0), np.where(err == 0, 0.0, np.inf))


def units(c):
    """per output, the restatement's error over the normaliser (same shape as the output)"""
    got = restatement(c)
    return {k: ratio(got[k], c.want[k], c.norm[k]) for k in OUTPUTS}


def oracle_unit(g, name):
    """the largest unit of system ``name``"""
    return max(float(u.max()) for u in units(case(g, name)).values())


def tol(unit):
    return np.maximum(16 * unit, FLOOR)


def check(label, c, got, unit=None):
    """print the figures of every output in ``got`` (dict over OUTPUTS; the value is required), then assert them against the
    fixture"""
    unit = units(c) if unit is None else unit
    bad = []
    assert "loglike" in got
    for k in OUTPUTS:
        if k not in got:
            continue
        err = ratio(got[k], c.want[k], c.norm[k])
        print(f"{label} system {c.name} {k}: worst error / normaliser = {err.max():.3g}, unit = {unit[k].max():.3g}, "
              f"worst error / tolerance = {(err / tol(unit[k])).max():.3g}")
        if not np.all(err <= tol(unit[k])):
            bad.append((k, float(err.max()), float((err / tol(unit[k])).max())))
    assert not bad, (label, c.name, bad)
