#!/usr/bin/env python
"""Writes tests/golden/astrometry_mp.npz: the astrometric likelihood of include/exoplanet_amd.h
(exo_astrometry_loglike_vjp_f64) -- value and every gradient -- computed with mpmath at the digits of
tools/make_orbit_golden.py.  The sky-plane position (X, Y) is that file's `outputs` (the position from the DEFINITIONS in the
eccentric anomaly) and its Jacobian that file's `jacobian` (mpmath.diff, one-sided in e at e = 0); the rest is the definition
of the likelihood written out in mpmath, the wrapped angle difference as atan2(sin(theta_m - theta_n), cos(theta_m - theta_n)).
None of the kernel's closed forms is restated, and nothing of the package is imported.  The observed series is the model of
draw 0 plus seeded noise of the size of the error bars.

    python tools/make_astrometry_golden.py          (about a minute on 8 cores)

Three draws per system; per system `s` in a..d (float64; an absent `s_jit2_rho` / `s_jit2_theta`: a null pointer):
  s_t (N,)  s_rho (N,)  s_theta (N,)  s_var_rho, s_var_theta (1,) or (N,)  s_params (3, 10)  s_jit2_rho (3,)  s_jit2_theta (3,)
  s_loglike (3,)  s_gparams (3, 10)  s_gjit2_rho (3,)  s_gjit2_theta (3,)
  s_n_loglike, s_n_gparams, s_n_gjit2_rho, s_n_gjit2_theta: for each of those outputs the sum of the absolute values of the
  terms that are added to form it, before any cancellation between them (tests/astrometry_cases.py: the normaliser)

After writing, the float64 restatement of tests/astrometry_cases.py is run on the fixture: its error over the normaliser
("unit") must be <= 1e-12 for every system, the condition on the inputs that tests/test_astrometry_host.py asserts.
"""
import functools
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_orbit_golden as G  # noqa: E402

mp.mp.dps = G.DPS
# (outputs() solves Kepler's equation once per call; the columns of a Jacobian that share (M, e) share the solve -- at one
# working precision: mpmath.diff raises it, and a one-sided difference must not meet a value solved at fewer digits)
_solve = functools.lru_cache(maxsize=16)(lambda M, e, prec, plane=G.plane: plane(M, e))
G.plane = lambda M, e: _solve(M, e, mp.mp.prec)

N_DRAW = 3
NARROW_CAD, WIDE = 128, 256      # exo_astrometry_core.hpp kNarrowCad, kWide: system c is one epoch past the narrow limit,
N_C, N_D = NARROW_CAD + 1, WIDE + 44      # and in system d 44 lanes of the wide workgroup take two epochs, the others one
AU_PER_R_SUN = 0.00465046726096215
YEAR = 365.25


def _records(rng, period, tp, e, w, incl, amp, Omega, circular=False):
    """(3, 10): draw 0, and two draws a little away from it (a circular record stays ECC = 0, COSW = 1, SINW = 0; without an
    Omega COSO = 1, SINO = 0)"""
    out = np.empty((N_DRAW, 10))
    for d in range(N_DRAW):
        u = (lambda: rng.uniform(-1, 1)) if d else (lambda: 0.0)
        ed = min(max(e + 0.01 * u(), 0.0), 0.95)
        wd, id_ = w + 0.03 * u(), incl + 0.02 * u()
        Od = None if Omega is None else Omega + 0.03 * u()
        out[d] = [2 * np.pi / period * (1 + 1e-3 * u()), tp + 2e-3 * period * u(), ed, np.cos(wd), np.sin(wd), np.cos(id_),
                  np.sin(id_), amp * (1 + 0.03 * u()), 1.0 if Od is None else np.cos(Od), 0.0 if Od is None else np.sin(Od)]
        if circular:
            out[d, 2:5] = [0.0, 1.0, 0.0]
    return out


def systems():
    rng = np.random.default_rng(20261)
    S = {}
    # a: one epoch; the angle's jitter only
    S["a"] = dict(t=np.array([3.7]), var_rho=np.array([0.02 ** 2]), var_theta=np.array([0.05 ** 2]),
                  params=_records(rng, 10.0, 1.0, 0.3, 0.8, 1.1, -0.4, 0.6), jit2_rho=None,
                  jit2_theta=np.array([0.03, 0.035, 0.025]) ** 2, two_pi=False)
    # b: the tutorial's series -- 45 epochs over 22 yr, P = 25 yr, a = 0.3", e = 0.3, cos i = 0.3, an Omega; per-epoch error
    # bars, no jitters
    t = np.sort(rng.uniform(0.0, 22.0 * YEAR, 45))
    S["b"] = dict(t=t, var_rho=rng.uniform(0.01, 0.02, 45) ** 2, var_theta=rng.uniform(0.02, 0.05, 45) ** 2,
                  params=_records(rng, 25.0 * YEAR, 3.1 * YEAR, 0.3, 1.9, np.arccos(0.3), -0.3, 2.4), jit2_rho=None,
                  jit2_theta=None, two_pi=False)
    # c: one epoch more than the narrow width; BJD-sized times over 3000 d, P = 1100 d, e = 0.9, the amplitude as
    # a parallax au_per_R_sun, both jitters, observed angles in [0, 2 pi): the orbit crosses the branch cut
    t = 2458000.0 + np.sort(rng.uniform(0.0, 3000.0, N_C))
    amp = -(451.0 * 0.04 * AU_PER_R_SUN)
    S["c"] = dict(t=t, var_rho=rng.uniform(0.002, 0.004, N_C) ** 2, var_theta=rng.uniform(0.02, 0.05, N_C) ** 2,
                  params=_records(rng, 1100.0, 2458000.0 + 312.0, 0.9, -2.1, 0.9, amp, 1.3),
                  jit2_rho=np.array([0.001, 0.0012, 0.0008]) ** 2, jit2_theta=np.array([0.02, 0.025, 0.015]) ** 2, two_pi=True)
    # d: on the wide workgroup some lanes take one epoch and some two; circular record, no Omega, one error bar for the series,
    # the separation's jitter only
    t = np.sort(rng.uniform(0.0, 900.0, N_D))
    S["d"] = dict(t=t, var_rho=np.array([0.015 ** 2]), var_theta=np.array([0.04 ** 2]),
                  params=_records(rng, 340.0, 41.0, 0.0, 0.0, 0.7, -0.25, None, circular=True),
                  jit2_rho=np.array([0.005, 0.006, 0.004]) ** 2, jit2_theta=None, two_pi=False)
    for name, s in S.items():
        s["noise"] = np.random.default_rng(40000 + ord(name)).normal(size=(2, s["t"].size))
    return S


def position_one(arg):
    """(X, Y, d X / d record[10], d Y / d record[10]) of one epoch and one record, as decimal strings"""
    mp.mp.dps = G.DPS
    tn, rec = arg
    tm = mp.mpf(tn)
    x = [mp.mpf(v) for v in rec]

    def fvec(x10):
        return G.outputs(tm, tuple(x10) + (mp.mpf(0),))[1:3]

    v = fvec(x)
    J = G.jacobian(fvec, x, 2)
    return [mp.nstr(q, G.DPS + 5) for q in list(v) + J[0] + J[1]]


def likelihood(s, XY, J):
    """the definitions of include/exoplanet_amd.h in mpmath; XY [3][N] of (X, Y), J [3][N] of (dX[10], dY[10])"""
    N = s["t"].size
    out = {k: np.zeros(shape) for k, shape in (("loglike", (N_DRAW,)), ("gparams", (N_DRAW, 10)), ("gjit2_rho", (N_DRAW,)),
                                               ("gjit2_theta", (N_DRAW,)))}
    out.update({"n_" + k: np.zeros_like(v) for k, v in list(out.items())})
    half, log2pi, two_pi = mp.mpf(1) / 2, mp.log(2 * mp.pi), 2 * mp.pi
    rho = theta = None
    crossings = 0
    for d in range(N_DRAW):
        jr = mp.mpf(0) if s["jit2_rho"] is None else mp.mpf(float(s["jit2_rho"][d]))
        jt = mp.mpf(0) if s["jit2_theta"] is None else mp.mpf(float(s["jit2_theta"][d]))
        s2r = [mp.mpf(float(s["var_rho"][0 if s["var_rho"].size == 1 else n])) + jr for n in range(N)]
        s2t = [mp.mpf(float(s["var_theta"][0 if s["var_theta"].size == 1 else n])) + jt for n in range(N)]
        rho_m = [mp.sqrt(X * X + Y * Y) for X, Y in XY[d]]
        theta_m = [mp.atan2(Y, X) for X, Y in XY[d]]
        if rho is None:      # the observed series: the model of draw 0, rounded, plus noise of the size of its error bars
            rho = np.array([float(rho_m[n]) + float(mp.sqrt(s2r[n])) * s["noise"][0, n] for n in range(N)])
            theta = np.array([float(theta_m[n]) + float(mp.sqrt(s2t[n])) * s["noise"][1, n] for n in range(N)])
            if s["two_pi"]:
                theta = np.mod(theta, 2 * np.pi)
        diff = [theta_m[n] - mp.mpf(float(theta[n])) for n in range(N)]
        crossings += sum(1 for x in diff if abs(x) > mp.pi)
        delta = [mp.atan2(mp.sin(x), mp.cos(x)) for x in diff]
        wr, wt = [1 / x for x in s2r], [1 / x for x in s2t]
        r = [mp.mpf(float(rho[n])) - rho_m[n] for n in range(N)]
        kappa = [wr[n] * r[n] for n in range(N)]
        lam = [-wt[n] * delta[n] for n in range(N)]
        const = N * log2pi
        out["loglike"][d] = -half * mp.fsum(wr[n] * r[n] ** 2 + mp.log(s2r[n]) + wt[n] * delta[n] ** 2 + mp.log(s2t[n])
                                            for n in range(N)) - const
        out["n_loglike"][d] = half * mp.fsum(wr[n] * r[n] ** 2 + abs(mp.log(s2r[n])) + wt[n] * delta[n] ** 2 + abs(mp.log(s2t[n]))
                                             for n in range(N)) + const
        for k in range(10):
            a = [kappa[n] * (XY[d][n][0] * J[d][n][0][k] + XY[d][n][1] * J[d][n][1][k]) / rho_m[n] for n in range(N)]
            b = [lam[n] * (XY[d][n][0] * J[d][n][1][k] - XY[d][n][1] * J[d][n][0][k]) / rho_m[n] ** 2 for n in range(N)]
            out["gparams"][d, k] = mp.fsum(a) + mp.fsum(b)
            out["n_gparams"][d, k] = mp.fsum(abs(x) for x in a) + mp.fsum(abs(x) for x in b)
        out["gjit2_rho"][d] = half * mp.fsum(kappa[n] ** 2 - wr[n] for n in range(N))
        out["n_gjit2_rho"][d] = half * mp.fsum(kappa[n] ** 2 + wr[n] for n in range(N))
        out["gjit2_theta"][d] = half * mp.fsum(lam[n] ** 2 - wt[n] for n in range(N))
        out["n_gjit2_theta"][d] = half * mp.fsum(lam[n] ** 2 + wt[n] for n in range(N))
    return rho, theta, crossings, out


def main():
    S = systems()
    tasks, where = [], []
    for name, s in S.items():
        for d in range(N_DRAW):
            for n, tn in enumerate(s["t"]):
                tasks.append((float(tn), [float(x) for x in s["params"][d]]))
                where.append((name, d, n))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(position_one, tasks, chunksize=16)
    XY = {name: [[None] * s["t"].size for _ in range(N_DRAW)] for name, s in S.items()}
    J = {name: [[None] * s["t"].size for _ in range(N_DRAW)] for name, s in S.items()}
    for (name, d, n), r in zip(where, res):
        v = [mp.mpf(x) for x in r]
        XY[name][d][n] = (v[0], v[1])
        J[name][d][n] = (v[2:12], v[12:22])
    out = {}
    for name, s in S.items():
        rho, theta, crossings, want = likelihood(s, XY[name], J[name])
        if s["two_pi"]:      # the unwrapped difference is off by 2 pi somewhere: forgetting the wrap fails this system
            assert crossings > 0 and theta.min() >= 0.0 and theta.max() < 2 * np.pi, (name, crossings)
            print(f"system {name}: {crossings} (draw, epoch) pairs with |theta_m - theta_obs| > pi")
        out.update({f"{name}_{k}": s[k] for k in ("t", "var_rho", "var_theta", "params")})
        out.update({f"{name}_{k}": s[k] for k in ("jit2_rho", "jit2_theta") if s[k] is not None})
        out[f"{name}_rho"], out[f"{name}_theta"] = rho, theta
        out.update({f"{name}_{k}": v for k, v in want.items()})
    path = os.path.join(ROOT, "tests", "golden", "astrometry_mp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(tasks), "(epoch, record) pairs")
    assert os.path.getsize(path) < 200_000
    # the condition on the inputs
    import astrometry_cases as K

    g = K.load()
    for name in K.SYSTEMS:
        assert g[f"{name}_t"].size == K.N_EPOCH[name], name
        unit = K.oracle_unit(g, name)
        print(f"system {name}: unit of the float64 restatement = {unit:.3g}")
        assert unit <= K.UNIT_CEILING, (name, unit)


if __name__ == "__main__":
    main()
