"""Writes tests/golden/diagnostics_mp.npz: the cases of tests/diagnostics_cases.py with every output of
exoplanet_amd.diagnostics -- mean, sd, quantiles, mcse_mean, the three effective sample sizes, r_hat and the integer max_t of
the four truncated sequences -- computed here with mpmath at 40 digits from the definitions of DESIGN.md section 16 (Phi^-1,
the moments and the autocovariances in multiprecision; ranks and order statistics are exact), and E_host: the largest error
of the double build of exoplanet_amd/csrc/exo_diagnostics_core.hpp (tests/diagnostics_harness.cpp) against that.

The truncation and the monotone step are comparisons.  Asserted for every case: each pair sum against zero, each pair sum
against the previous one, the last term against zero, tau against its floor and every draw against the tail quantiles (in
units of sd) is away from its threshold by at least diagnostics_cases.MARGIN, relative; the ranks of |x - median| are the same in double
and in exact arithmetic.  A case that is not gets another seed in diagnostics_cases.SHAPES.

    python tests/make_diagnostics_golden.py
"""
import os
import sys
from bisect import bisect_left, bisect_right

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diagnostics_cases as K  # noqa: E402

mp.mp.dps = 40
_Z = {}


def z_of_rank(rank2, S):
    """Phi^-1((r - 3/8) / (S + 1/4)) with r = rank2 / 2"""
    num, den = 4 * rank2 - 3, 8 * S + 2
    if 2 * num > den:
        return -z_of_rank(2 * (S + 1) - rank2, S)
    key = (num, den)
    if key not in _Z:
        _Z[key] = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(num) / den - 1)
    return _Z[key]


def rank_normalise(values):
    """values: list of mpf -> list of mpf normal scores of the average ranks (ties exact)"""
    S = len(values)
    ordered = sorted(values)
    return [z_of_rank(bisect_left(ordered, v) + bisect_right(ordered, v) + 1, S) for v in values], ordered


def quantile(ordered, percent):
    n = len(ordered)
    num = (n - 1) * percent
    lo, rem = divmod(num, 100)
    if rem == 0 or lo + 1 >= n:
        return ordered[lo]
    return ordered[lo] + mp.mpf(rem) / 100 * (ordered[lo + 1] - ordered[lo])


def rel(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m else mp.mpf(0)


def sequence(y, L, M, margins):
    """y: list of S mpf laid out [n][m] -> (ess, max_t, rhat)"""
    S = L * M
    cols = [[y[n * M + m] for n in range(L)] for m in range(M)]
    means = [mp.fsum(c) / L for c in cols]
    d = [[v - mu for v in c] for c, mu in zip(cols, means)]

    def abar(t):
        return mp.fsum(mp.fdot(c[t:], c[:L - t]) for c in d) / L / M

    W = abar(0) * L / (L - 1)
    mm = mp.fsum(means) / M
    vb = mp.fsum((m - mm) ** 2 for m in means) / (M - 1)
    var_plus = W * (L - 1) / L + vb
    if var_plus == 0:                    # an indicator that is the same everywhere
        return mp.mpf(S), -1, mp.nan
    rhat = mp.sqrt(var_plus / W) if W else mp.inf
    rho = {0: mp.mpf(1)}

    def r(t):
        if t not in rho:
            rho[t] = 1 - (W - abar(t)) / var_plus
        return rho[t]

    re, ro, t = mp.mpf(1), r(1), 1
    while True:
        if t < L - 3:
            margins.append(abs(re + ro) / (abs(re) + abs(ro)))
        if not (t < L - 3 and re + ro > 0):
            break
        re, ro = r(t + 1), r(t + 2)
        t += 2
    max_t = t - 2
    margins.append(abs(re))
    t = 1
    while t <= max_t - 2:
        cur, prev = rho[t + 1] + rho[t + 2], rho[t - 1] + rho[t]
        margins.append(rel(cur, prev))
        if cur > prev:
            rho[t + 1] = rho[t + 2] = prev / 2
        t += 2
    tau = -1 + 2 * mp.fsum(rho[k] for k in range(max_t + 1)) + (re if re > 0 else 0)
    floor = 1 / mp.log10(S)
    margins.append(rel(tau, floor))
    return S / max(tau, floor), max_t, rhat


def one_series(x, margins):
    """x (N, C) float64 -> {column: value}"""
    N, C = x.shape
    nan = float("nan")
    out = {k: nan for k in K.FLOATS}
    out.update({k: -1 for k in K.INTS})
    if N < 4 or not np.isfinite(x).all():
        return out
    allv = sorted(mp.mpf(float(v)) for v in x.ravel())
    n = len(allv)
    mean = mp.fsum(allv) / n
    sd = mp.sqrt(mp.fsum((v - mean) ** 2 for v in allv) / (n - 1))
    q05, q50, q95 = (quantile(allv, pc) for pc in (5, 50, 95))
    out.update(mean=mean, sd=sd, q05=q05, q50=q50, q95=q95)
    L, M = N // 2, 2 * C
    S = L * M
    if allv[0] == allv[-1]:
        out.update(ess_bulk=S, ess_tail=S, ess_mean=S, mcse_mean=sd / mp.sqrt(S))
        return out
    xs = np.concatenate([x[:L], x[N - L:]], axis=1)                   # (L, M): pooled index n M + m
    v = [mp.mpf(float(a)) for a in xs.ravel()]
    z, ordered = rank_normalise(v)
    a, b = ordered[(S - 1) // 2], ordered[S // 2]
    fold = [abs(w - (a + b) / 2) for w in v]
    zf, _ = rank_normalise(fold)
    # the same ranks from the folded values as double arithmetic forms them
    fa, fb = float(a), float(b)
    fold64 = np.abs(((xs.ravel() - fa) + (xs.ravel() - fb)) / 2.0)
    s64 = np.sort(fold64)
    r64 = np.searchsorted(s64, fold64, "left") + np.searchsorted(s64, fold64, "right") + 1
    fs = sorted(fold)
    rmp = np.array([bisect_left(fs, w) + bisect_right(fs, w) + 1 for w in fold])
    assert np.array_equal(r64, rmp), "the ranks of |x - median| differ between double and exact arithmetic"
    for q in (q05, q95):
        # (in units of the spread: beside an offset of 1e8 it is the spread that separates a draw from the quantile)
        margins.append(min((abs(w - q) / sd for w in v if w != q), default=mp.mpf(1)))
    low = [mp.mpf(1) if w <= q05 else mp.mpf(0) for w in v]
    high = [mp.mpf(1) if w <= q95 else mp.mpf(0) for w in v]
    ess_bulk, t_bulk, rz = sequence(z, L, M, margins)
    _, _, rf = sequence_rhat_only(zf, L, M)
    ess_low, t_low, _ = sequence(low, L, M, margins)
    ess_high, t_high, _ = sequence(high, L, M, margins)
    ess_mean, t_mean, _ = sequence(v, L, M, margins)
    out.update(ess_bulk=ess_bulk, ess_tail=min(ess_low, ess_high), ess_mean=ess_mean, mcse_mean=sd / mp.sqrt(ess_mean),
               r_hat=max(rz, rf), max_t_bulk=t_bulk, max_t_low=t_low, max_t_high=t_high, max_t_mean=t_mean)
    return out


def sequence_rhat_only(y, L, M):
    cols = [[y[n * M + m] for n in range(L)] for m in range(M)]
    means = [mp.fsum(c) / L for c in cols]
    W = mp.fsum(mp.fsum((v - mu) ** 2 for v in c) for c, mu in zip(cols, means)) / M / (L - 1)
    mm = mp.fsum(means) / M
    vb = mp.fsum((m - mm) ** 2 for m in means) / (M - 1)
    return None, None, mp.sqrt((W * (L - 1) / L + vb) / W)


def main():
    lib = K.harness()
    arrays, e_host, worst = {}, 0.0, {}
    for name, x in K.cases().items():
        N, C, P = x.shape
        margins = []
        rows = [one_series(x[:, :, p], margins) for p in range(P)]
        want = {k: np.array([float(r[k]) for r in rows]) for k in K.FLOATS}
        want.update({k: np.array([int(r[k]) for r in rows], dtype=np.int64) for k in K.INTS})
        low = min([float(m) for m in margins], default=1.0)
        assert low >= K.MARGIN, (name, low)
        for long_double in (True, False):
            err = K.errors(K.run_harness(lib, x, long_double), want)
            if not long_double:
                for k, v in err.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                e_host = max(e_host, max(err.values()))
            print("%-10s %-11s smallest margin %.1e  errors %s" % (name, "long double" if long_double else "double", low,
                                                                   {k: "%.1e" % v for k, v in err.items()}), flush=True)
        print("   ess_bulk / S", np.round(want["ess_bulk"] / (2 * C * (N // 2)), 3), "r_hat", np.round(want["r_hat"], 4),
              "max_t_bulk", want["max_t_bulk"], flush=True)
        arrays[name + "/x"] = x
        for k, v in want.items():
            arrays[f"{name}/{k}"] = v
    arrays["E_host"] = np.asarray(e_host)
    np.savez_compressed(K.GOLD, **arrays)
    print("E_host = %.3e (per column: %s); %d bytes" % (e_host, {k: "%.1e" % v for k, v in worst.items()}, os.path.getsize(K.GOLD)))


if __name__ == "__main__":
    main()
