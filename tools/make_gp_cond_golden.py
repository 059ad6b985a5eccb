#!/usr/bin/env python
"""Writes tests/golden/gp_cond_mp.npz: the conditional half of the celerite GP -- (K + diag)^-1 y, L x, the predictive mean,
variance and covariance, for the whole kernel and for component masks -- from the DENSE definitions in mpmath at 40 digits:
the kernel function summed term by term, a Cholesky factorisation and triangular solves written out here.  None of the
recurrences is restated and nothing of the package is imported.

    python tools/make_gp_cond_golden.py          (a minute or two on 8 cores)

Per entry `e` of tests/gp_cond_cases.py (ENTRIES), float64 unless noted:
  inputs    e_t (N,)  e_diag (N,)  e_coef_real (Jr, 2)  e_pairs (Jc, 4)  e_pair_kind (Jc,) int32  e_tq (M,)  e_x (N,)  e_y (N,)
            e_masks (n_mask, Jr + Jc) int32
  expected  e_alpha = (K + diag)^-1 y   e_z = L x   e_mu_t, e_mu_q = K alpha at t, tq   e_var_t, e_var_q   e_cov_q (M, M)
            and with the suffix _m<i> the last five for component mask i (K2 restricted to the mask, K + diag whole)
  e_scale_<q>, e_unit_<q>: the scale of quantity q and the float64 yardstick's error in it (tests/gp_cond_cases.py)
y = L x' rounded to float64 (a draw from the process), x' white; for white_y, y = x'.

After writing, the caps of tests/gp_cond_cases.py are asserted: 16 unit <= 1e-6 for every entry and quantity, except alpha of
the entries listed there as RESIDUAL_ONLY, which must be exactly the entries whose alpha breaks the cap.
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gp_cond_cases as K  # noqa: E402

DPS = 40
mp.mp.dps = DPS


def slot_kernels(p, real, pairs, kind):
    """per slot s the symmetric matrix k_s(|p_i - p_j|) over the points p (lists of rows of mpf; lower triangle mirrored)"""
    n = len(p)
    tau = [[abs(p[i] - p[j]) for j in range(i + 1)] for i in range(n)]
    fns = []
    for a, c in real:
        fns.append(lambda x, a=a, c=c: a * mp.exp(-c * x))
    for (a, b, c, d), kd in zip(pairs, kind):
        if kd:
            fns.append(lambda x, a=a, b=b, c=c, d=d: a * mp.exp(-b * x) + c * mp.exp(-d * x))
        else:
            fns.append(lambda x, a=a, b=b, c=c, d=d: mp.exp(-c * x) * (a * mp.cos(d * x) + b * mp.sin(d * x)))
    out = []
    for f in fns:
        low = [[f(x) for x in row] for row in tau]
        out.append([[low[max(i, j)][min(i, j)] for j in range(n)] for i in range(n)])
    return out


def cholesky(A):
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = A[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))
            if i == j:
                assert s > 0, ("not positive definite at row", i)
                L[i][i] = mp.sqrt(s)
            else:
                L[i][j] = s / L[j][j]
    return L


def solve_lower(L, b):
    x = []
    for i in range(len(L)):
        x.append((b[i] - mp.fsum(L[i][k] * x[k] for k in range(i))) / L[i][i])
    return x


def solve_upper_t(L, b):
    """L^T x = b"""
    n = len(L)
    x = [None] * n
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - mp.fsum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
    return x


def entry(name):
    mp.mp.dps = DPS
    s = K.inputs(name)
    n, m = len(s["t"]), len(s["tq"])
    M = lambda v: [mp.mpf(float(x)) for x in v]  # noqa: E731
    real = [M(r) for r in s["coef_real"]]
    pairs = [M(r) for r in s["pairs"]]
    pts = M(s["t"]) + M(s["tq"])
    ks = slot_kernels(pts, real, pairs, s["pair_kind"])
    n_slot = len(ks)
    summed = lambda keep: [[mp.fsum(ks[q][i][j] for q in range(n_slot) if keep[q]) for j in range(n + m)]  # noqa: E731
                           for i in range(n + m)]
    full = summed([1] * n_slot)
    diag = M(s["diag"])
    A = [[full[i][j] + (diag[i] if i == j else 0) for j in range(n)] for i in range(n)]
    L = cholesky(A)
    dot = lambda x: [mp.fsum(L[i][k] * x[k] for k in range(i + 1)) for i in range(n)]  # noqa: E731
    f64 = lambda v: np.array([float(x) for x in v])  # noqa: E731
    y = s["xy"].copy() if name == "white_y" else f64(dot(M(s["xy"])))
    alpha = solve_upper_t(L, solve_lower(L, M(y)))
    out = {k: s[k] for k in ("t", "diag", "coef_real", "pairs", "pair_kind", "tq", "x", "masks")}
    out["y"] = y
    want = {"alpha": f64(alpha), "z": f64(dot(M(s["x"])))}
    scale = {"alpha": max(abs(v) for v in alpha), "z": np.abs(want["z"]).max()}
    for i in [None] + list(range(len(s["masks"]))):
        k2, sfx = (full, "") if i is None else (summed(list(s["masks"][i])), f"_m{i}")
        mu = [mp.fsum(k2[r][c] * alpha[c] for c in range(n)) for r in range(n + m)]
        B = [solve_lower(L, [k2[c][r] for c in range(n)]) for r in range(n + m)]     # L^-1 K2(t, p_r)
        var = [k2[r][r] - mp.fsum(b * b for b in B[r]) for r in range(n + m)]
        cov = [[k2[n + r][n + c] - mp.fsum(a * b for a, b in zip(B[n + r], B[n + c])) for c in range(m)] for r in range(m)]
        want["mu_t" + sfx], want["mu_q" + sfx] = f64(mu[:n]), f64(mu[n:])
        want["var_t" + sfx], want["var_q" + sfx] = f64(var[:n]), f64(var[n:])
        want["cov_q" + sfx] = np.array([[float(v) for v in row] for row in cov])
        smu = max(abs(v) for v in mu[:n])
        for q in ("mu_t", "mu_q"):
            scale[q + sfx] = smu
        for q in ("var_t", "var_q", "cov_q"):
            scale[q + sfx] = k2[0][0]
    out.update(want)
    out.update({"scale_" + q: np.float64(float(v)) for q, v in scale.items()})
    return name, out


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(entry, K.ENTRIES, chunksize=1)
    out = {}
    for name, o in res:
        out.update({f"{name}_{k}": v for k, v in o.items()})
        # the units: the float64 yardstick on these inputs
        o.update({"unit_" + q: 0.0 for q in K.quantities(len(o["masks"]))})
        c = K.Case({f"{name}_{k}": v for k, v in o.items()}, name)
        got = K.yardstick(c)
        for q in c.quantities:
            out[f"{name}_unit_{q}"] = np.float64(K.error(c, q, got[q]))
    path = os.path.join(K.GOLD, "gp_cond_mp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    g = K.load()
    broken = []
    for name in K.ENTRIES:
        c = K.Case(g, name)
        print(name, "J =", c.J, " ".join(f"{q}={c.unit[q]:.2g}" for q in c.quantities))
        for q in c.quantities:
            if K.FACTOR * c.unit[q] <= K.CAP:
                continue
            assert q == "alpha" and name in K.RESIDUAL_ONLY_ALLOWED, (name, q, c.unit[q])
            broken.append(name)
    print("alpha above the cap:", broken)
    assert tuple(broken) == tuple(K.RESIDUAL_ONLY), (broken, K.RESIDUAL_ONLY)


if __name__ == "__main__":
    main()
