#!/usr/bin/env python
"""Writes tests/golden/priors.npz: the constrained values, the log prior, its gradient and the Jacobian of the values of
every space of tests/priors_cases.py, computed with mpmath at 50 digits straight from the DENSITY definitions -- the density
of the constrained value (Beta, half-normal, Rayleigh, normal; truncation masses from mpmath.betainc / ncdf) times the
Jacobian of the transform -- not from the simplified forms the package evaluates.  Derivatives: mpmath.diff of those
functions.  Nothing of the package is imported.

    python tools/make_priors_golden.py          (about two minutes)
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import priors_cases as C  # noqa: E402

mp.mp.dps = 50


def s(z):
    return 1 / (1 + mp.exp(-z))


def log_jac_interval(z, w=1):
    return mp.log(w * s(z) * (1 - s(z)))          # d/dz of lo + w s(z)


def normal_logpdf(x, mu, sd):
    return mp.log(mp.npdf(x, mu, sd))


def positive_hyper(z, mu, sd):
    """x = exp z under a normal truncated below at 0: density / (mass above 0) times dx/dz = x"""
    x = mp.exp(z)
    return x, normal_logpdf(x, mu, sd) - mp.log(1 - mp.ncdf(0, mu, sd)) + mp.log(x)


def beta_logpdf(e, a, b):
    return (a - 1) * mp.log(e) + (b - 1) * mp.log(1 - e) - mp.log(mp.beta(a, b))


def mixture_logpdf(e, sg, sr, f):
    half_normal = mp.sqrt(2 / mp.pi) / sg * mp.exp(-e * e / (2 * sg * sg))
    rayleigh = e / (sr * sr) * mp.exp(-e * e / (2 * sr * sr))
    return mp.log((1 - f) * half_normal + f * rayleigh)


def evaluate(case, z):
    """-> (values in the order ParameterSpace.outputs lists them, log prior)"""
    z = list(z)
    values, lp, at, first = [], mp.mpf(0), 0, {}
    for name, ctor, args, kw in C.CASES[case]:
        n = (kw.get("shape") or (1,))[0]
        take = lambda k: [z[at + i] for i in range(k)]  # noqa: E731
        first[name] = len(values)
        if ctor in ("normal", "lognormal"):
            for zz in take(n):
                values.append(zz if ctor == "normal" else mp.exp(zz))
                lp += normal_logpdf(zz, *args)       # lognormal: density of x = exp z times dx/dz is the normal density of z
            at += n
        elif ctor == "uniform":
            lo, hi = args
            for zz in take(n):
                values.append(lo + (hi - lo) * s(zz))
                lp += -mp.log(hi - lo) + log_jac_interval(zz, hi - lo)
            at += n
        elif ctor == "impact_parameter":
            for j, zz in enumerate(take(n)):
                ror = args[0]
                if isinstance(ror, str):
                    ctor_r = [c for c in C.CASES[case] if c[0] == ror][0]
                    n_r = (ctor_r[3].get("shape") or (1,))[0]
                    ror = values[first[ror] + (j if n_r > 1 else 0)]
                values.append(s(zz) * (1 + ror))
                lp += -mp.log(1 + ror) + log_jac_interval(zz, 1 + ror)
            at += n
        elif ctor == "angle":
            zs = take(2 * n)
            reg = kw.get("regularization", 10.0)
            for j in range(n):
                z1, z2 = zs[j], zs[n + j]
                values.append(mp.atan2(z1, z2))
                lp += normal_logpdf(z1, 0, 1) + normal_logpdf(z2, 0, 1)
                if reg is not None:
                    lp += reg * mp.log(z1 * z1 + z2 * z2)
            at += 2 * n
        elif ctor == "unit_disk":
            zs = take(2 * n)
            xs, ys = [], []
            for j in range(n):
                x = 2 * s(zs[j]) - 1
                root = mp.sqrt(1 - x * x)
                xs.append(x); ys.append((2 * s(zs[n + j]) - 1) * root)
                # the potentials the reference's model carries: the two unit-interval Jacobians and log sqrt(1 - x^2)
                lp += log_jac_interval(zs[j]) + log_jac_interval(zs[n + j]) + mp.log(root)
            values += xs + ys
            at += 2 * n
        elif ctor == "quad_limb_dark":
            zs = take(2 * n)
            u1, u2 = [], []
            for j in range(n):
                q1, q2 = s(zs[j]), s(zs[n + j])
                u1.append(2 * mp.sqrt(q1) * q2); u2.append(mp.sqrt(q1) * (1 - 2 * q2))
                lp += log_jac_interval(zs[j]) + log_jac_interval(zs[n + j])
            values += u1 + u2
            at += 2 * n
        elif ctor == "kipping13":
            short = kw.get("long") is False
            a_mu, a_sd, b_mu, b_sd = (0.697, 0.4, 3.27, 0.3) if short else (1.12, 0.1, 3.09, 0.3)
            lo, hi = kw.get("lower") or 0.0, 1.0 if kw.get("upper") is None else kw["upper"]
            lo, hi, a_mu, a_sd, b_mu, b_sd = (mp.mpf(repr(v)) for v in (lo, hi, a_mu, a_sd, b_mu, b_sd))
            hyper = []
            if kw.get("fixed", True):
                a, b = a_mu, b_mu
            else:
                (za, zb) = take(2)
                at += 2
                a, lpa = positive_hyper(za, a_mu, a_sd)
                b, lpb = positive_hyper(zb, b_mu, b_sd)
                lp += lpa + lpb
                hyper = [a, b]
            for zz in take(n):
                e = lo + (hi - lo) * s(zz)
                values.append(e)
                lp += beta_logpdf(e, a, b) - mp.log(mp.betainc(a, b, lo, hi, regularized=True)) + log_jac_interval(zz, hi - lo)
            values += hyper
            at += n
        elif ctor == "vaneylen19":
            multi = kw.get("multi", False)
            mus = (0.049, 0.26, 0.08 if multi else 0.76)
            sds = (0.02, 0.05, 0.08 if multi else 0.2)
            lo, hi = kw.get("lower") or 0.0, 1.0 if kw.get("upper") is None else kw["upper"]
            lo, hi = mp.mpf(repr(lo)), mp.mpf(repr(hi))
            mus, sds = [mp.mpf(repr(v)) for v in mus], [mp.mpf(repr(v)) for v in sds]
            hyper = []
            if kw.get("fixed", True):
                sg, sr, f = mus
            else:
                zg, zr, zf = take(3)
                at += 3
                sg, lpg = positive_hyper(zg, mus[0], sds[0])
                sr, lpr = positive_hyper(zr, mus[1], sds[1])
                f = s(zf)
                lpf = normal_logpdf(f, mus[2], sds[2]) - mp.log(mp.ncdf(1, mus[2], sds[2]) - mp.ncdf(0, mus[2], sds[2])) + log_jac_interval(zf)
                lp += lpg + lpr + lpf
                hyper = [sg, sr, f]
            for zz in take(n):
                e = lo + (hi - lo) * s(zz)
                values.append(e)
                # uniform on [lo, hi] times the interval Jacobian, and the (not renormalised) mixture as a potential
                lp += -mp.log(hi - lo) + log_jac_interval(zz, hi - lo) + mixture_logpdf(e, sg, sr, f)
            values += hyper
            at += n
        else:
            raise ValueError(ctor)
    assert at == len(z)
    return values, lp


def main():
    out = {}
    for seed, case in enumerate(C.CASES):
        Z = C.z_grid(case, 1000 + seed)
        vals, lps, dlps, jacs = [], [], [], []
        for row in Z:
            zr = [mp.mpf(float(v)) for v in row]
            v, lp = evaluate(case, zr)
            n = len(zr)
            partial = lambda fn, k: mp.diff(fn, tuple(zr), tuple(int(i == k) for i in range(n)))  # noqa: E731
            vals.append([float(x) for x in v])
            lps.append(float(lp))
            dlps.append([float(partial(lambda *a: evaluate(case, a)[1], k)) for k in range(n)])
            jacs.append([[float(partial(lambda *a, o=o: evaluate(case, a)[0][o], k)) for k in range(n)] for o in range(len(v))])
        out[case + "/z"] = Z
        out[case + "/values"] = np.array(vals)
        out[case + "/log_prior"] = np.array(lps)
        out[case + "/dlog_prior"] = np.array(dlps)
        out[case + "/jacobian"] = np.array(jacs)
        print(case, Z.shape, "done", flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "priors.npz"), **out)


if __name__ == "__main__":
    main()
