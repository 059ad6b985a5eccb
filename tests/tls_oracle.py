"""The yardstick of the transit-least-squares tests: a brute-force numpy restatement of the definition in DESIGN.md section 18,
on top of tests/estimators_oracle.py (weights, the plan of the bins, the fragile band).  A helper module, not a test.  It forms
every window by a gather and ``sum`` -- deliberately not the kernel's loop of fused multiply-adds over ascending j -- and takes a
``dtype`` so that it can run in ``np.longdouble``: the difference between the float64 and the longdouble oracle on an input, at
the same maximiser, is what sets the tests' tolerance on it."""
import numpy as np

import estimators_oracle as O

FIELDS = O.FIELDS
STATS = ("depth", "depth_err", "depth_snr", "log_likelihood")
U = (0.4804, 0.1867)


def tls_hist(t, y, yerr, p, delta, oversample, dtype=np.float64):
    """-> hy, hw [n_bins + 1] (bin sums, wrapped; NOT prefix sums), Y, W, t_min, fragile for one period"""
    t = np.asarray(t, dtype=dtype)
    y, w = O._weights(y, yerr, dtype)
    p, delta = dtype(p), dtype(delta)
    t_min = t.min()
    n_bins = int(np.ceil(np.float64(p) / np.float64(delta))) + oversample
    q = np.fmod(t - t_min, p) / delta
    fragile = bool(np.any((np.abs(q - np.round(q)) < O.FRAGILE_BAND) & (t > t_min)))
    ind = 1 + np.floor(q).astype(np.int64)
    hy, hw = np.zeros(n_bins + 1, dtype=dtype), np.zeros(n_bins + 1, dtype=dtype)
    np.add.at(hy, ind, w * y)
    np.add.at(hw, ind, w)
    hy[n_bins - oversample + 1:] = hy[1:oversample + 1]
    hw[n_bins - oversample + 1:] = hw[1:oversample + 1]
    return hy, hw, (w * y).sum(), w.sum(), t_min, fragile


def tls_windows(hy, hw, Y, W, s, g):
    """the four statistics of the windows starting at bin(s) s under template g; inadmissible ones NaN"""
    g = np.asarray(g, dtype=hy.dtype)
    idx = np.asarray(s)[:, None] + 1 + np.arange(len(g))[None, :]
    A, B, C, w_in = (g * hw[idx]).sum(1), (g * g * hw[idx]).sum(1), (g * hy[idx]).sum(1), hw[idx].sum(1)
    with np.errstate(all="ignore"):
        D = B - A * A / W
        depth = (A * Y / W - C) / D
        out = np.stack([depth, 1 / np.sqrt(D), depth * np.sqrt(D), depth * depth * D / 2])
    return np.where((w_in > 0) & (W - w_in > 0) & (D > 0), out, np.nan)


def tls_power(t, y, yerr, periods, durations, templates, oversample=10, objective="likelihood", dtype=np.float64, at=None):
    """-> dict of (P,) arrays (FIELDS), 'fragile' (P,) bool and 'arg' (P, 2) int: the maximiser (k, s), -1 without one.
    ``at`` (P, 2): evaluate these (k, s) instead of searching (the other precision's maximiser)."""
    delta, ms = O.bls_plan(durations, oversample)
    assert [len(g) for g in templates] == list(ms)
    res = {k: np.full(len(periods), np.nan, dtype=dtype) for k in FIELDS}
    res["fragile"] = np.zeros(len(periods), dtype=bool)
    res["arg"] = np.full((len(periods), 2), -1, dtype=np.int64)
    row = 3 if objective == "likelihood" else 2
    for i, p in enumerate(np.asarray(periods, dtype=np.float64)):
        hy, hw, Y, W, t_min, res["fragile"][i] = tls_hist(t, y, yerr, p, delta, oversample, dtype)
        n_bins = len(hy) - 1
        best = (-np.inf, None, None, None)
        if at is not None:
            k, s = at[i]
            if k >= 0:
                st = tls_windows(hy, hw, Y, W, np.array([s]), templates[k])[:, 0]
                best = (st[row], s, k, st)
        else:
            for k, m in enumerate(ms):                    # (k, s) order; strict > keeps the first maximiser
                if n_bins - m + 1 <= 0:
                    continue
                st = tls_windows(hy, hw, Y, W, np.arange(0, n_bins - m + 1), templates[k])
                obj = np.where(np.isnan(st[row]), -np.inf, st[row])
                j = int(np.argmax(obj))
                if obj[j] > best[0]:
                    best = (obj[j], j, k, st[:, j])
        res["power"][i] = best[0]
        if best[1] is not None:
            _, s, k, st = best
            m = int(ms[k])
            res["depth"][i], res["depth_err"][i], res["depth_snr"][i], res["log_likelihood"][i] = st
            res["duration"][i] = m * dtype(delta)
            res["transit_time"][i] = np.fmod(s * dtype(delta) + dtype(0.5) * m * dtype(delta) + t_min, dtype(p))
            res["arg"][i] = k, s
    return res


def tls_at(t, y, yerr, p, durations, templates, oversample, duration, transit_time, dtype=np.float64):
    """the statistics (STATS) of the window that a returned (duration, transit_time) names: the first duration of that many bins"""
    delta, ms = O.bls_plan(durations, oversample)
    hy, hw, Y, W, t_min, _ = tls_hist(t, y, yerr, p, delta, oversample, dtype)
    n_bins = len(hy) - 1
    m = int(round(float(duration) / delta))
    k = list(ms).index(m)
    x = (float(transit_time) - float(t_min) - 0.5 * m * delta) / delta
    cands = [int(round(x + c * float(p) / delta)) for c in range(-2, 3)]
    want = [s for s in cands if 0 <= s <= n_bins - m and
            abs(np.fmod(s * delta + 0.5 * m * delta + float(t_min), float(p)) - float(transit_time)) < 1e-6 * delta]
    assert want, ("no start bin reproduces the transit time", p, duration, transit_time)
    return tls_windows(hy, hw, Y, W, np.array(want[:1]), templates[k])[:, 0]


def unit_and_reference(t, y, yerr, periods, durations, templates, oversample, objective):
    """-> (the float64 oracle, keep mask, unit): unit = the largest relative difference, over the kept periods and the five
    statistics, between the float64 oracle and the longdouble oracle AT THE float64 ORACLE'S MAXIMISER"""
    want = tls_power(t, y, yerr, periods, durations, templates, oversample, objective)
    exact = tls_power(t, y, yerr, periods, durations, templates, oversample, objective, dtype=np.longdouble, at=want["arg"])
    keep = ~(want["fragile"] | exact["fragile"])
    sel = keep & np.isfinite(want["power"])
    unit = max([O.rel_diff(want[k][sel], exact[k][sel]) for k in ("power",) + STATS]) if sel.any() else 0.0
    return want, keep, unit


FLOOR, FACTOR, MAX_FRAGILE = 1e-13, 16.0, 0.02


def check(name, got, t, y, yerr, periods, durations, templates, oversample, objective, reference=None):
    """``got``: host arrays (FIELDS) of one series.  DESIGN.md 9.5's rule: tolerance = 16 x unit, floor 1e-13, relative to each
    period's own value.  ``power`` is compared on every kept period; where the maximiser is the oracle's the other fields are
    too, and where a near-tie picked another window they are checked for consistency through tls_at.  Prints, then asserts.
    -> (tolerance, oracle)"""
    want, keep, unit = reference if reference is not None else unit_and_reference(t, y, yerr, periods, durations, templates,
                                                                                  oversample, objective)
    tol = max(FACTOR * unit, FLOOR)
    finite = np.isfinite(want["power"])
    sel = keep & finite
    err = O.rel_diff(got["power"][sel], want["power"][sel]) if sel.any() else 0.0
    same = sel & (np.abs(got["duration"] - want["duration"]) <= 1e-9) & (np.abs(got["transit_time"] - want["transit_time"]) <= 1e-9)
    worst = max([O.rel_diff(got[k][same], want[k][same]) for k in STATS]) if same.any() else 0.0
    row = 3 if objective == "likelihood" else 2
    other = 0.0
    for i in np.flatnonzero(sel & ~same):
        st = tls_at(t, y, yerr, periods[i], durations, templates, oversample, got["duration"][i], got["transit_time"][i])
        mine = np.array([got[k][i] for k in STATS])
        other = max(other, float(np.max(np.abs(mine - st) / np.abs(st))), abs(got["power"][i] - st[row]) / abs(st[row]))
    print(f"[{name}] periods {len(periods)}, fragile {int((~keep).sum())}, float64 vs longdouble oracle {unit:.2e}, tolerance "
          f"{tol:.2e}, power error {err:.2e}, other fields {worst:.2e} ({int(same.sum())} of {int(sel.sum())} periods at the oracle's "
          f"maximiser; consistency of the others {other:.2e})")
    assert (~keep).sum() <= MAX_FRAGILE * len(periods)
    assert np.array_equal(np.isfinite(got["power"][keep]), finite[keep])
    assert np.all(got["power"][keep & ~finite] == -np.inf)
    for k in FIELDS[1:]:
        assert np.all(np.isnan(got[k][keep & ~finite])), k
    assert err <= tol and worst <= tol and other <= tol
    return tol, want


# ---- the template and the inputs of the tests ----------------------------------------------------------------------------------

def lc_deficit(z, ror, u=U):
    """1 - flux of a quadratically limb-darkened star behind a planet at separation z (oracle/numpy_port's solution vector)"""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import numpy_port as P

    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    s = P.quad_solution_vector(z, np.full_like(z, ror))[0]
    return 1.0 - s @ np.asarray(P.get_cl(*u))


def transit_template(m, ror=0.1, b=0.0, u=U):
    x = (2.0 * np.arange(m) + 1.0) / m - 1.0
    z = np.sqrt(b * b + ((1 + ror) ** 2 - b * b) * x * x)
    return lc_deficit(z, ror, u) / lc_deficit(b, ror, u)[0]


TRUE = dict(period=2.345, t0=1.0, ror=0.1, b=0.3, duration=0.2)


def true_depth():
    return float(lc_deficit(TRUE["b"], TRUE["ror"])[0])


def main_input(seed=721, n=5000, span=27.0, noise=2e-3, offset=0.0):
    """the injected limb-darkened transit of the issue: straight-line chord, first-to-fourth-contact duration 0.2;
    the median is subtracted (``offset`` is added afterwards: the y-near-1 variant)"""
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, span, n))
    y = noise * rs.randn(n)
    P0, b, ror = TRUE["period"], TRUE["b"], TRUE["ror"]
    x = ((t - TRUE["t0"] + 0.5 * P0) % P0 - 0.5 * P0) / (0.5 * TRUE["duration"])
    inside = np.abs(x) < 1
    y[inside] -= lc_deficit(np.sqrt(b * b + ((1 + ror) ** 2 - b * b) * x[inside] ** 2), ror)
    return t, y - np.median(y) + offset


def main_periods():
    return np.concatenate([np.exp(np.linspace(np.log(0.7), np.log(13.0), 200)), [2.345, 2.3449, 4.69]])
