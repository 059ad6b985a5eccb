#!/usr/bin/env python
"""Writes tests/golden/gp_like_mp.npz: the celerite log-likelihood and every gradient of it -- with respect to the series, the
diagonal and each coefficient of each term -- from the DENSE definitions in mpmath at 40 digits: the kernel function and its
derivatives summed term by term, A = K + diag, its Cholesky factor L, alpha = A^-1 y, A^-1 = L^-T L^-1 and
W = 1/2 (alpha alpha^T - A^-1).  None of the recurrences is restated and nothing of the package is imported; Cholesky and the
triangular solves are those of make_gp_cond_golden.py.

    python tools/make_gp_like_golden.py          (61 s on 8 cores)

Per entry `e` of tests/gp_like_cases.py (ENTRIES), float64 unless noted:
  inputs    e_t (N,)  e_diag (N,)  e_coef_real (Jr, 2)  e_pairs (Jc, 4)  e_pair_kind (Jc,) int32  e_y (N,)
  expected  e_loglike ()  e_gy (N,)  e_gdiag (N,)  e_greal (Jr, 2)  e_gpairs (Jc, 4)
  e_scale_<q>, e_unit_<q>: the scale of quantity q (per coefficient for greal, gpairs) and the error in it of the float64
            yardstick, oracle.c_port.celerite(grad=True) (tests/gp_like_cases.py)
y = L x' rounded to float64 (a draw from the process), x' white.

After writing, every unit is printed and the cap of tests/gp_like_cases.py is asserted: 16 unit <= 1e-6 for every entry and
quantity, without exception.
"""
import os
import sys
import time
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gp_like_cases as K  # noqa: E402
from gp_cond_cases import error  # noqa: E402
from make_gp_cond_golden import DPS, cholesky, slot_kernels, solve_lower, solve_upper_t  # noqa: E402

mp.mp.dps = DPS


def slot_derivatives(t, real, pairs, kind):
    """per slot (k, [dk / d coefficient ...]) as lower triangles over the times t (rows of mpf): exp, cos and sin once per slot
    and pair of times.  A real slot (a, c): 2 derivatives; a pair slot: 4 -- (a, b, c, d) of a complex term,
    (a1, c1, a2, c2) of a kind-1 slot"""
    n = len(t)
    tau = [[t[i] - t[j] for j in range(i + 1)] for i in range(n)]      # (sorted times: >= 0)
    tri = lambda: [[None] * (i + 1) for i in range(n)]  # noqa: E731
    out = []
    for a, c in real:
        k, da, dc = tri(), tri(), tri()
        for i in range(n):
            for j in range(i + 1):
                x = tau[i][j]
                e = mp.exp(-c * x)
                k[i][j], da[i][j], dc[i][j] = a * e, e, -a * x * e
        out.append((k, [da, dc]))
    for (a, b, c, d), kd in zip(pairs, kind):
        k, d0, d1, d2, d3 = tri(), tri(), tri(), tri(), tri()
        for i in range(n):
            for j in range(i + 1):
                x = tau[i][j]
                if kd:       # a exp(-b x) + c exp(-d x)
                    e1, e2 = mp.exp(-b * x), mp.exp(-d * x)
                    k[i][j] = a * e1 + c * e2
                    d0[i][j], d1[i][j], d2[i][j], d3[i][j] = e1, -a * x * e1, e2, -c * x * e2
                else:        # exp(-c x) (a cos d x + b sin d x)
                    e, cs, sn = mp.exp(-c * x), mp.cos(d * x), mp.sin(d * x)
                    k[i][j] = e * (a * cs + b * sn)
                    d0[i][j], d1[i][j], d2[i][j], d3[i][j] = e * cs, e * sn, -x * k[i][j], x * e * (b * cs - a * sn)
        out.append((k, [d0, d1, d2, d3]))
    return out


def entry(name):
    mp.mp.dps = DPS
    s = K.inputs(name)
    n = len(s["t"])
    M = lambda v: [mp.mpf(float(x)) for x in v]  # noqa: E731
    f64 = lambda v: np.array([float(x) for x in v])  # noqa: E731
    t, diag = M(s["t"]), M(s["diag"])
    real, pairs = [M(r) for r in s["coef_real"]], [M(r) for r in s["pairs"]]
    slots = slot_derivatives(t, real, pairs, s["pair_kind"])
    A = [[mp.fsum(k[max(i, j)][min(i, j)] for k, _ in slots) + (diag[i] if i == j else 0) for j in range(n)] for i in range(n)]
    if n <= 2:      # (the kernel as the sibling generator writes it)
        ks = slot_kernels(t, real, pairs, s["pair_kind"])
        assert all(mp.fsum(k[i][j] for k in ks) + (diag[i] if i == j else 0) == A[i][j] for i in range(n) for j in range(n))
    L = cholesky(A)
    white = M(s["xy"])
    y = f64([mp.fsum(L[i][k] * white[k] for k in range(i + 1)) for i in range(n)])
    ym = M(y)
    alpha = solve_upper_t(L, solve_lower(L, ym))
    # A^-1 = L^-T L^-1, lower triangle: column j of L^-1 is zero above row j
    Linv = [[mp.mpf(0)] * j + solve_lower([row[j:] for row in L[j:]], [mp.mpf(1)] + [mp.mpf(0)] * (n - j - 1)) for j in range(n)]
    Ainv = [[mp.fsum(Linv[i][k] * Linv[j][k] for k in range(i, n)) for j in range(i + 1)] for i in range(n)]
    half, two_pi = mp.mpf(1) / 2, 2 * mp.pi
    quad = half * mp.fsum(a * b for a, b in zip(ym, alpha))
    logs = [2 * mp.log(L[i][i]) for i in range(n)]
    want = {"loglike": np.float64(float(-quad - half * mp.fsum(logs) - half * n * mp.log(two_pi))),
            "gy": f64([-a for a in alpha])}
    gdiag = [half * (alpha[i] ** 2 - Ainv[i][i]) for i in range(n)]
    want["gdiag"] = f64(gdiag)
    scale = {"loglike": float(abs(quad) + half * mp.fsum(abs(v) for v in logs) + half * n * mp.log(two_pi)),
             "gy": float(max(abs(a) for a in alpha)), "gdiag": float(max(abs(v) for v in gdiag))}
    grads, scales = [], []
    for _, ders in slots:
        for dk in ders:      # the whole symmetric matrix from its lower triangle: twice the strict triangle + the diagonal
            sym = lambda f: 2 * mp.fsum(f(i, j) * dk[i][j] for i in range(n) for j in range(i)) + mp.fsum(  # noqa: E731
                f(i, i) * dk[i][i] for i in range(n))
            h1 = half * sym(lambda i, j: alpha[i] * alpha[j])
            h2 = half * sym(lambda i, j: Ainv[i][j])
            grads.append(float(h1 - h2))
            scales.append(float(abs(h1) + abs(h2)))
    jr, jc = len(real), len(pairs)
    want["greal"], want["gpairs"] = np.array(grads[:2 * jr]).reshape(jr, 2), np.array(grads[2 * jr:]).reshape(jc, 4)
    scale["greal"], scale["gpairs"] = np.array(scales[:2 * jr]).reshape(jr, 2), np.array(scales[2 * jr:]).reshape(jc, 4)
    out = {k: s[k] for k in ("t", "diag", "coef_real", "pairs", "pair_kind")}
    out["y"] = y
    out.update(want)
    out.update({"scale_" + q: np.asarray(v, dtype=np.float64) for q, v in scale.items()})
    return name, out


def main(names=K.ENTRIES):
    t0 = time.time()
    # the widest and longest entries first, so that the pool ends together
    order = sorted(names, key=lambda e: -(K.SPEC[e].get("n", K.N) ** 3 + 30 * K.SPEC[e].get("n", K.N) ** 2 * sum(K.SPEC[e].get("layout", (0, 1)))))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = dict(pool.map(entry, order, chunksize=1))
    out = {}
    for name in names:
        o = res[name]
        out.update({f"{name}_{k}": v for k, v in o.items()})
        # the units: the float64 yardstick on these inputs
        o.update({"unit_" + q: 0.0 for q in K.QUANTITIES})
        c = K.Case({f"{name}_{k}": v for k, v in o.items()}, name)
        got = K.yardstick(c)
        for q in K.QUANTITIES:
            out[f"{name}_unit_{q}"] = np.float64(error(c, q, got[q]))
    if tuple(names) != K.ENTRIES:       # (a trial run of some entries: print, write nothing)
        for name in names:
            print(name, " ".join(f"{q}={float(out[f'{name}_unit_{q}']):.2g}" for q in K.QUANTITIES))
        print(f"{time.time() - t0:.0f} s")
        return
    path = os.path.join(K.GOLD, "gp_like_mp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", f"{time.time() - t0:.0f} s")
    g = K.load()
    worst = 0.0
    for name in K.ENTRIES:
        c = K.Case(g, name)
        print(f"{name}: N = {c.n}, J = {c.J}, score = {c.score():.3g},", " ".join(f"{q}={c.unit[q]:.2g}" for q in K.QUANTITIES))
        for q in K.QUANTITIES:
            assert K.FACTOR * c.unit[q] <= K.CAP, (name, q, c.unit[q])
            worst = max(worst, c.unit[q])
    print(f"the cap holds: 16 x {worst:.3g} = {16 * worst:.3g} <= {K.CAP:g}")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]) or K.ENTRIES)
