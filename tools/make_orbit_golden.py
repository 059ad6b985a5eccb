#!/usr/bin/env python
"""Writes tests/golden/orbit_mp.npz: the Kepler op, the radial velocity and the position / velocity / acceleration vectors
of ops.orbit_vector, with every partial derivative, computed with mpmath at 40 digits from the DEFINITIONS in the eccentric
anomaly E -- the root of E - e sin E = M (oracle/mp_reference.kepler_E, bisection + Newton) and the orbit-plane vector
(cos E - e, sqrt(1 - e^2) sin E) with its first and second M-derivatives written in E -- not from the true-anomaly closed
forms that the kernels and oracle/numpy_port.py evaluate.  Every derivative is mpmath.diff of the value function
(one-sided in e at e = 0); none comes from an analytic partial.  Nothing of the package or of numpy_port is imported.

    python tools/make_orbit_golden.py          (under a minute on 8 cores)

Arrays (float64 only):
  kw_M, kw_e, kw_Mred, kw_sinf, kw_cosf, kw_dsinf_dM, kw_dcosf_dM, kw_dsinf_de, kw_dcosf_de      "kepler_wide", (K,)
  rv_params (S, 6)   t (S, N)   rv (S, N)   rv_jac (S, N, 6)
  ov_params (S, 10)  ov_pos / ov_vel / ov_acc (S, N, 3)   ov_pos_jac / ov_vel_jac / ov_acc_jac (S, N, 3, 10)
  sys_grad (S,)  1.0 where summed gradients are to be checked (e <= 0.999), 0.0 for the value-only systems
  sys_period (S,)  the period whose mean motion fl(2 pi / period) is the record's n
  sys_layout (S,)  0: t, tp near 0;  1: t, tp near 2 457 000;  2: t near 2 457 000, tp = 0.3, period 0.5 d (|M| ~ 3e7)
System s shares (n, tp, e, cos w, sin w) between its rv and ov record; epochs are per system.
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.mp_reference import kepler_E  # noqa: E402

DPS = 40
mp.mp.dps = DPS
N_EPOCH = 20
ECC_WIDE = [0.0, 1e-16, 1e-8, 0.3, 0.9, 0.99, 0.999, 1 - 1e-6, 1 - 1e-8, 1 - 1e-12]
ECC_SYS = [0.0, 1e-12, 0.3, 0.9, 0.99, 0.999, 1 - 1e-6, 1 - 1e-8]   # the last two: values only


# ------------------------------------------------------------------------------------------------
# definitions
# ------------------------------------------------------------------------------------------------
def plane(M, e):
    """(position, velocity, acceleration) in the orbital plane for unit amplitude, in E:
    position (cos E - e, sqrt(1-e^2) sin E); velocity sqrt(1-e^2) d position / d M; acceleration (1-e^2) d^2 position / d M^2
    (the normalisations of keplerian.py:380-409, :572-578, :679-688)"""
    E = kepler_E(M, e)
    cE, sE = mp.cos(E), mp.sin(E)
    b2 = (1 - e) * (1 + e)
    b = mp.sqrt(b2)
    q = 1 - e * cE
    pos = (cE - e, b * sE)
    vel = (-b * sE / q, b2 * cE / q)
    acc = (b2 * (e - cE) / q ** 3, -b2 * b * sE / q ** 3)
    return pos, vel, acc


def sincos_f(M, e):
    E = kepler_E(M, e)
    cE, sE = mp.cos(E), mp.sin(E)
    q = 1 - e * cE
    return mp.sqrt((1 - e) * (1 + e)) * sE / q, (cE - e) / q


def rotate(u, v, cw, sw, ci, si, cO, sO):
    """keplerian.py:283-322"""
    x1 = cw * u - sw * v
    y1 = sw * u + cw * v
    y2 = ci * y1
    return cO * x1 - sO * y2, sO * x1 + cO * y2, -si * y1


def outputs(t, p):
    """p = (n, tp, e, cw, sw, ci, si, amp, cO, sO, amp_rv) -> [rv, pos XYZ, vel XYZ, acc XYZ]"""
    n, tp, e, cw, sw, ci, si, amp, cO, sO, amp_rv = p
    pos, vel, acc = plane((t - tp) * n, e)
    out = [amp_rv * (sw * vel[0] + cw * vel[1])]          # keplerian.py:660-669: K (cos w (cos f + e) - sin w sin f)
    for u, v in (pos, vel, acc):
        out.extend(amp * c for c in rotate(u, v, cw, sw, ci, si, cO, sO))
    return out


def jacobian(fvec, x, n_out):
    """d fvec / d x[k] by mpmath.diff, one output at a time; the vector is evaluated once per abscissa"""
    J = [[None] * len(x) for _ in range(n_out)]
    for k in range(len(x)):
        memo = {}

        def at(xk, k=k, memo=memo):
            if xk not in memo:
                memo[xk] = fvec(x[:k] + [xk] + x[k + 1:])
            return memo[xk]

        opts = dict(direction=1) if (k == 2 and x[k] == 0) else {}
        for j in range(n_out):
            J[j][k] = mp.diff(lambda xk, j=j: at(xk)[j], x[k], **opts)
    return J


# ------------------------------------------------------------------------------------------------
# kepler_wide
# ------------------------------------------------------------------------------------------------
def wide_M(rng):
    two_pi = 2 * np.pi
    M = []
    for mag in (1e3, 1e5, 3e7, 7e8):
        r = mag * rng.uniform(0.9, 1.1, 36) * np.where(np.arange(36) % 2, -1.0, 1.0)
        if mag == 7e8:
            r = np.clip(r, -7.9e8, 7.9e8)      # sincos_any documents |x| < 8e8
        M.extend(r)
        for sign in (1.0, -1.0):
            k = np.floor(mag * rng.uniform(0.95, 1.05) / two_pi)
            a, b = sign * two_pi * k, sign * two_pi * (k + 0.5)
            M.extend([a, a + 1e-9, a - 1e-9, b, b + 1e-7, b - 1e-7])
    return np.array(M)


def wide_points():
    rng = np.random.default_rng(20251)
    M0 = wide_M(rng)
    Ms, es = [], []
    for e in ECC_WIDE:
        Ms.extend(M0)
        es.extend([e] * M0.size)
        if e >= 0.999:                         # small |M|, near-parabolic
            small = 10.0 ** np.arange(-14, -1) * rng.uniform(1.0, 3.0, 13)
            Ms.extend(np.concatenate([small, -small]))
            es.extend([e] * 26)
    return np.array(Ms), np.array(es)


def wide_one(arg):
    mp.mp.dps = DPS
    M, e = mp.mpf(arg[0]), mp.mpf(arg[1])
    s, c = sincos_f(M, e)
    Mred = M - 2 * mp.pi * mp.nint(M / (2 * mp.pi))
    memo = {}

    def at(key, Mx, ex):
        if key not in memo:
            memo[key] = sincos_f(Mx, ex)
        return memo[key]

    opts = dict(direction=1) if e == 0 else {}
    dM = [mp.diff(lambda x, j=j: at(("M", x), x, e)[j], M) for j in (0, 1)]
    de = [mp.diff(lambda x, j=j: at(("e", x), M, x)[j], e, **opts) for j in (0, 1)]
    return [float(v) for v in (Mred, s, c, dM[0], dM[1], de[0], de[1])]


# ------------------------------------------------------------------------------------------------
# systems
# ------------------------------------------------------------------------------------------------
OMEGA = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), None]          # four quadrants exactly, then general position
INCL = [(0.0, 1.0), (1.0, 0.0), None]                                     # cos i = 0, sin i = 0, general


def systems():
    rng = np.random.default_rng(20252)
    rv, ov, ts, grad, layout, periods = [], [], [], [], [], []
    s = 0
    for lay in range(3):
        for e in ECC_SYS:
            if lay == 0:
                period, tp, t_lo = rng.uniform(2.0, 9.0), rng.uniform(-0.5, 0.5), rng.uniform(-5.0, 0.0)
            elif lay == 1:
                period, tp, t_lo = rng.uniform(2.0, 40.0), 2457000.0 + rng.uniform(0.0, 3.0), 2457000.0
            else:
                period, tp, t_lo = 0.5, 0.3, 2457000.0 + rng.uniform(0.0, 400.0)
            n = 2 * np.pi / period
            span = 2.6 * period if lay < 2 else 30.0
            t = t_lo + span * rng.uniform(0.0, 1.0, N_EPOCH)
            k0 = 0.0 if lay < 2 else np.ceil((t_lo - tp) / period) + 1     # (tp lies inside the series of layouts 0 and 1)
            t[0] = tp + k0 * period + 3e-7 * period * (1 if s % 2 else -1)     # within 1e-6 of a period of periastron
            t[1] = tp + (k0 + 0.5) * period                                    # apoapsis
            t = np.sort(t)
            w = OMEGA[s % 5]
            if w is None:
                a = rng.uniform(-np.pi, np.pi)
                w = (np.cos(a), np.sin(a))
            i = INCL[(s // 2) % 3]
            if i is None:
                a = rng.uniform(0.1, 1.5)
                i = (np.cos(a), np.sin(a))
            O = rng.uniform(-np.pi, np.pi)
            # no node rotation on every other edge-on system (those map onto KeplerianOrbit(b=0, Omega=None) exactly) and on s % 4 == 3
            cO, sO = (1.0, 0.0) if (s % 4 == 3 or (i == INCL[0] and s % 2 == 1)) else (np.cos(O), np.sin(O))
            amp = rng.uniform(1.0, 9.0) * 10.0 ** ((s % 4) - 1) * (-1 if s % 3 == 1 else 1)
            amp_rv = rng.uniform(1.0, 9.0) * 10.0 ** (((s + 2) % 4) - 1)
            rv.append([n, tp, e, w[0], w[1], amp_rv])
            ov.append([n, tp, e, w[0], w[1], i[0], i[1], amp, cO, sO])
            ts.append(t)
            grad.append(1.0 if e <= 0.999 else 0.0)
            layout.append(float(lay))
            periods.append(period)
            s += 1
    return np.array(rv), np.array(ov), np.array(ts), np.array(grad), np.array(layout), np.array(periods)


def system_one(arg):
    mp.mp.dps = DPS
    rvp, ovp, t = arg
    x = [mp.mpf(v) for v in ovp] + [mp.mpf(rvp[5])]
    val = np.zeros((t.size, 10))
    jac = np.zeros((t.size, 10, 11))
    for i, ti in enumerate(t):
        tm = mp.mpf(ti)
        solve = {}

        def fvec(p, tm=tm, solve=solve):
            key = (p[0], p[1], p[2])
            if key not in solve:
                solve.clear()
                solve[key] = plane((tm - p[1]) * p[0], p[2])
            pos, vel, acc = solve[key]
            n, tp, e, cw, sw, ci, si, amp, cO, sO, amp_rv = p
            out = [amp_rv * (sw * vel[0] + cw * vel[1])]
            for u, v in (pos, vel, acc):
                out.extend(amp * c for c in rotate(u, v, cw, sw, ci, si, cO, sO))
            return out

        val[i] = [float(v) for v in outputs(tm, x)]
        J = jacobian(fvec, x, 10)
        jac[i] = [[float(v) for v in row] for row in J]
    return val, jac


def main():
    Mw, ew = wide_points()
    rvp, ovp, ts, grad, layout, periods = systems()
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        wide = np.array(pool.map(wide_one, list(zip(Mw, ew)), chunksize=16))
        res = pool.map(system_one, list(zip(rvp, ovp, ts)), chunksize=1)
    val = np.stack([r[0] for r in res])            # (S, N, 10)
    jac = np.stack([r[1] for r in res])            # (S, N, 10, 11)
    rv_cols = [0, 1, 2, 3, 4, 10]
    out = dict(kw_M=Mw, kw_e=ew, kw_Mred=wide[:, 0], kw_sinf=wide[:, 1], kw_cosf=wide[:, 2], kw_dsinf_dM=wide[:, 3],
               kw_dcosf_dM=wide[:, 4], kw_dsinf_de=wide[:, 5], kw_dcosf_de=wide[:, 6],
               rv_params=rvp, ov_params=ovp, t=ts, sys_grad=grad, sys_layout=layout, sys_period=periods,
               rv=val[:, :, 0], rv_jac=jac[:, :, 0][:, :, rv_cols])
    for k, name in enumerate(("pos", "vel", "acc")):
        out[f"ov_{name}"] = val[:, :, 1 + 3 * k:4 + 3 * k]
        out[f"ov_{name}_jac"] = jac[:, :, 1 + 3 * k:4 + 3 * k, :10]
    path = os.path.join(ROOT, "tests", "golden", "orbit_mp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", Mw.size, "Kepler points,", rvp.shape[0], "systems x", N_EPOCH, "epochs")


if __name__ == "__main__":
    main()
