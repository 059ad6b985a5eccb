#!/usr/bin/env python
"""Writes tests/golden/rv_like_mp.npz: the radial-velocity likelihood of include/exoplanet_amd.h (exo_rv_loglike_vjp_f64) --
value and every gradient -- computed with mpmath at the digits of tools/make_orbit_golden.py.  The Keplerian part is that
file's `outputs` (the radial velocity from the DEFINITIONS in the eccentric anomaly) and `jacobian` (mpmath.diff, one-sided in
e at e = 0); the rest is the definition of the likelihood written out in mpmath.  None of the kernel's closed forms is
restated, and nothing of the package is imported.  The observed series is the model of draw 0 plus seeded noise.

    python tools/make_rv_like_golden.py          (a few minutes on 8 cores)

Three draws per system; per system `s` in a..f (float64 unless noted; an absent `s_offset` / `s_jit2`: a null pointer):
  s_t (N,)  s_tref ()  [tau = s_t - s_tref, the float64 difference]  s_inst (N,) int32  s_rv (N,)  s_var (1,) or (N,)
  s_params (3, P, 6)  s_trend (3, T)  s_offset (3, I)  s_jit2 (3, I)
  s_loglike (3,)  s_gparams (3, P, 6)  s_gtrend (3, T)  s_goffset (3, I)  s_gjit2 (3, I)
  s_n_loglike, s_n_gparams, s_n_gtrend, s_n_goffset, s_n_gjit2: for each of those outputs the sum of the absolute values of
  the terms that are added to form it, before any cancellation between them (tests/rv_like_cases.py: the normaliser)

After writing, the float64 restatement of tests/rv_like_cases.py is run on the fixture: its error over the normaliser ("unit")
must be <= 1e-12 for every system, the condition on the inputs that tests/test_rv_like_host.py asserts.
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
import make_orbit_golden as G  # noqa: E402

mp.mp.dps = G.DPS
# (outputs() solves Kepler's equation once per call; the columns of a Jacobian that share (M, e) share the solve -- at one
# working precision: mpmath.diff raises it, and a one-sided difference must not meet a value solved at fewer digits)
_solve = functools.lru_cache(maxsize=16)(lambda M, e, prec, plane=G.plane: plane(M, e))
G.plane = lambda M, e: _solve(M, e, mp.mp.prec)

N_DRAW = 3
TILE = 1024          # exo_rv_like_core.hpp kTile: system e is one epoch longer


def _angles(w):
    return np.cos(w), np.sin(w)


def _records(rng, period, tp, e, w, K, circular=()):
    """(3, P, 6): draw 0, and two draws a little away from it (a circular record stays ECC = 0, COSW = 1, SINW = 0)"""
    period, tp, e, w, K = (np.asarray(x, dtype=np.float64) for x in (period, tp, e, w, K))
    out = np.empty((N_DRAW, period.size, 6))
    for d in range(N_DRAW):
        u = (lambda: rng.uniform(-1, 1, period.size)) if d else (lambda: np.zeros(period.size))
        ed = np.clip(e + 0.01 * u(), 0.0, 0.95)
        cw, sw = _angles(w + 0.03 * u())
        out[d] = np.stack([2 * np.pi / period * (1 + 1e-3 * u()), tp + 0.02 * u(), ed, cw, sw, K * (1 + 0.03 * u())], -1)
        for p in circular:
            out[d, p, 2:5] = [0.0, 1.0, 0.0]
    return out


def _per_draw(rng, base, rel):
    base = np.asarray(base, dtype=np.float64)
    return np.stack([base * (1 + (rel * rng.uniform(-1, 1, base.shape) if d else 0.0)) for d in range(N_DRAW)])


def systems():
    rng = np.random.default_rng(20253)
    S = {}

    def trend(T, span):
        return _per_draw(rng, [0.3 * rng.uniform(0.5, 1.5) * (-1) ** k / (0.5 * span) ** k for k in range(T)], 0.1)

    def errs(n):
        return rng.uniform(0.3, 0.7, n) ** 2

    # a: one epoch, one planet, one error bar for the series, no jitter
    S["a"] = dict(t=np.array([3.7]), inst=np.zeros(1, np.int32), var=np.array([0.25]),
                  params=_records(rng, [10.0], [1.0], [0.3], [0.8], [5.0]), trend=np.zeros((N_DRAW, 0)),
                  offset=_per_draw(rng, [[0.3]], 0.2)[:, 0], jit2=None)
    # b: the tutorial's series
    t = np.sort(rng.uniform(0.0, 50.0, 20))
    S["b"] = dict(t=t, inst=np.zeros(20, np.int32), var=errs(20),
                  params=_records(rng, [10.0], [rng.uniform(0, 10)], [0.3], [rng.uniform(-np.pi, np.pi)], [5.0]),
                  trend=trend(1, 50.0), offset=_per_draw(rng, [[-0.4]], 0.2)[:, 0], jit2=_per_draw(rng, [[0.09]], 0.3)[:, 0])
    # c: three instruments of which the last has no epochs, one circular record
    t = np.sort(rng.uniform(0.0, 120.0, 257))
    S["c"] = dict(t=t, inst=rng.integers(0, 2, 257).astype(np.int32), var=errs(257),
                  params=_records(rng, [7.3, 31.0], [2.0, 11.0], [0.0, 0.6], [0.0, -2.1], [4.0, 9.0], circular=(0,)),
                  trend=trend(3, 120.0), offset=_per_draw(rng, [[1.5, -0.7, 0.2]], 0.1)[:, 0],
                  jit2=_per_draw(rng, [[0.04, 0.16, 0.01]], 0.3)[:, 0])
    # d: BJD-sized times, e = 0.9
    t = 2458000.0 + np.sort(rng.uniform(0.0, 400.0, 1000))
    per = np.array([3.9, 17.1, 112.0])
    S["d"] = dict(t=t, inst=rng.integers(0, 2, 1000).astype(np.int32), var=errs(1000),
                  params=_records(rng, per, 2458000.0 + rng.uniform(0, 1, 3) * per, [0.1, 0.9, 0.4], rng.uniform(-np.pi, np.pi, 3),
                                  [3.0, 12.0, 6.0]),
                  trend=trend(4, 400.0), offset=_per_draw(rng, [[0.8, -1.1]], 0.1)[:, 0],
                  jit2=_per_draw(rng, [[0.05, 0.2]], 0.3)[:, 0])
    # e: one epoch more than the kernel's tile; no zero point, no jitter (null pointers)
    t = np.sort(rng.uniform(0.0, 300.0, TILE + 1))
    S["e"] = dict(t=t, inst=np.zeros(TILE + 1, np.int32), var=np.array([0.16]),
                  params=_records(rng, [23.0], [5.0], [0.2], [1.9], [7.0]), trend=np.zeros((N_DRAW, 0)), offset=None, jit2=None)
    # f: sixteen planets, eight instruments
    t = np.sort(rng.uniform(0.0, 90.0, 33))
    S["f"] = dict(t=t, inst=(np.arange(33) % 8).astype(np.int32), var=errs(33),
                  params=_records(rng, 10 ** np.linspace(0.5, 2.3, 16), rng.uniform(0, 3, 16), rng.uniform(0, 0.5, 16),
                                  rng.uniform(-np.pi, np.pi, 16), rng.uniform(1, 10, 16)),
                  trend=np.zeros((N_DRAW, 0)), offset=_per_draw(rng, [rng.uniform(-2, 2, 8)], 0.1)[:, 0],
                  jit2=_per_draw(rng, [rng.uniform(0.1, 0.5, 8) ** 2], 0.3)[:, 0])
    for name, s in S.items():
        s["tref"] = np.float64(0.5 * (s["t"].min() + s["t"].max()))
        s["noise"] = np.random.default_rng(30000 + ord(name)).normal(size=s["t"].size)
    return S


def kepler_one(arg):
    """(rv, d rv / d record[6]) of one epoch and one record, as decimal strings"""
    mp.mp.dps = G.DPS
    tn, rec = arg
    tm = mp.mpf(tn)
    x = [mp.mpf(v) for v in rec]

    def fvec(x6):
        n, tp, e, cw, sw, amp = x6
        return G.outputs(tm, (n, tp, e, cw, sw, mp.mpf(0), mp.mpf(1), mp.mpf(0), mp.mpf(1), mp.mpf(0), amp))[:1]

    v = fvec(x)[0]
    J = G.jacobian(fvec, x, 1)[0]
    return [mp.nstr(q, G.DPS + 5) for q in [v] + J]


def likelihood(s, V, J):
    """the definitions of include/exoplanet_amd.h in mpmath; V (3, N, P), J (3, N, P, 6) of mpf"""
    N, P = s["t"].size, s["params"].shape[1]
    T, I = s["trend"].shape[1], int(s["inst"].max()) + 1 if s["offset"] is None else s["offset"].shape[1]
    tau = [mp.mpf(float(x)) for x in (s["t"] - s["tref"])]
    inst = [int(i) for i in s["inst"]]
    out = {k: np.zeros(shape) for k, shape in (("loglike", (N_DRAW,)), ("gparams", (N_DRAW, P, 6)), ("gtrend", (N_DRAW, T)),
                                               ("goffset", (N_DRAW, I)), ("gjit2", (N_DRAW, I)))}
    out.update({"n_" + k: np.zeros_like(v) for k, v in list(out.items())})
    half, log2pi = mp.mpf(1) / 2, mp.log(2 * mp.pi)
    rv = None
    for d in range(N_DRAW):
        off = [mp.mpf(0)] * I if s["offset"] is None else [mp.mpf(float(x)) for x in s["offset"][d]]
        jit = [mp.mpf(0)] * I if s["jit2"] is None else [mp.mpf(float(x)) for x in s["jit2"][d]]
        tr = [mp.mpf(float(x)) for x in s["trend"][d]]
        m = [mp.fsum(V[d][n]) + mp.fsum(tr[k] * tau[n] ** k for k in range(T)) + off[inst[n]] for n in range(N)]
        s2 = [mp.mpf(float(s["var"][0 if s["var"].size == 1 else n])) + jit[inst[n]] for n in range(N)]
        if rv is None:      # the observed series: the model of draw 0, rounded, plus noise of the size of its error bars
            rv = np.array([float(m[n]) + float(mp.sqrt(s2[n])) * s["noise"][n] for n in range(N)])
        w = [1 / x for x in s2]
        r = [mp.mpf(float(rv[n])) - m[n] for n in range(N)]
        rho = [w[n] * r[n] for n in range(N)]
        const = half * N * log2pi
        out["loglike"][d] = -half * mp.fsum(w[n] * r[n] ** 2 + mp.log(s2[n]) for n in range(N)) - const
        out["n_loglike"][d] = half * mp.fsum(w[n] * r[n] ** 2 + abs(mp.log(s2[n])) for n in range(N)) + const
        for p in range(P):
            for k in range(6):
                terms = [rho[n] * J[d][n][p][k] for n in range(N)]
                out["gparams"][d, p, k] = mp.fsum(terms)
                out["n_gparams"][d, p, k] = mp.fsum(abs(x) for x in terms)
        for k in range(T):
            terms = [rho[n] * tau[n] ** k for n in range(N)]
            out["gtrend"][d, k] = mp.fsum(terms)
            out["n_gtrend"][d, k] = mp.fsum(abs(x) for x in terms)
        for i in range(I):
            mine = [n for n in range(N) if inst[n] == i]
            out["goffset"][d, i] = mp.fsum(rho[n] for n in mine)
            out["n_goffset"][d, i] = mp.fsum(abs(rho[n]) for n in mine)
            out["gjit2"][d, i] = half * mp.fsum(rho[n] ** 2 - w[n] for n in mine)
            out["n_gjit2"][d, i] = half * mp.fsum(rho[n] ** 2 + w[n] for n in mine)
    return rv, out


def main():
    S = systems()
    tasks, where = [], []
    for name, s in S.items():
        for d in range(N_DRAW):
            for n, tn in enumerate(s["t"]):
                for p in range(s["params"].shape[1]):
                    tasks.append((float(tn), [float(x) for x in s["params"][d, p]]))
                    where.append((name, d, n, p))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(kepler_one, tasks, chunksize=32)
    V = {name: [[[None] * s["params"].shape[1] for _ in s["t"]] for _ in range(N_DRAW)] for name, s in S.items()}
    J = {name: [[[None] * s["params"].shape[1] for _ in s["t"]] for _ in range(N_DRAW)] for name, s in S.items()}
    for (name, d, n, p), r in zip(where, res):
        V[name][d][n][p] = mp.mpf(r[0])
        J[name][d][n][p] = [mp.mpf(x) for x in r[1:]]
    out = {}
    for name, s in S.items():
        rv, want = likelihood(s, V[name], J[name])
        out.update({f"{name}_{k}": s[k] for k in ("t", "tref", "inst", "var", "params", "trend")})
        out.update({f"{name}_{k}": s[k] for k in ("offset", "jit2") if s[k] is not None})
        out[f"{name}_rv"] = rv
        out.update({f"{name}_{k}": v for k, v in want.items()})
    path = os.path.join(ROOT, "tests", "golden", "rv_like_mp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(tasks), "(epoch, record) pairs")
    # the condition on the inputs
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rv_like_cases as K

    g = K.load()
    for name in K.SYSTEMS:
        unit = K.oracle_unit(g, name)
        print(f"system {name}: unit of the float64 restatement = {unit:.3g}")
        assert unit <= K.UNIT_CEILING, (name, unit)


if __name__ == "__main__":
    main()
