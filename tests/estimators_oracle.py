"""The yardstick of the period-search tests: a brute-force numpy restatement of the definitions in DESIGN.md section 9 (box least
squares, the binned method; floating-mean Lomb-Scargle by least squares per frequency -- deliberately not the closed form the
kernel uses).  A helper module, not a test.  Every function takes a ``dtype`` so that it can run in ``np.longdouble``: the
difference between the float64 and the longdouble oracle on an input is what sets the tests' tolerance on it."""
import numpy as np

FIELDS = ("power", "depth", "depth_err", "depth_snr", "log_likelihood", "duration", "transit_time")
FRAGILE_BAND = 1e-9


def _weights(y, yerr, dtype):
    y = np.asarray(y, dtype=dtype)
    w = np.ones_like(y) if yerr is None else 1 / np.broadcast_to(np.asarray(yerr, dtype=dtype), y.shape) ** 2
    return y, w


def bls_plan(durations, oversample):
    durations = np.asarray(durations, dtype=np.float64)
    delta = durations.min() / oversample
    return delta, np.round(durations / delta).astype(np.int64)


def bls_prefix(t, y, yerr, p, delta, oversample, dtype=np.float64):
    """-> cy, cw [n_bins + 1], Y, W, t_min, fragile for one period"""
    t = np.asarray(t, dtype=dtype)
    y, w = _weights(y, yerr, dtype)
    p, delta = dtype(p), dtype(delta)
    t_min = t.min()
    n_bins = int(np.ceil(np.float64(p) / np.float64(delta))) + oversample
    q = np.fmod(t - t_min, p) / delta
    fragile = bool(np.any((np.abs(q - np.round(q)) < FRAGILE_BAND) & (t > t_min)))
    ind = 1 + np.floor(q).astype(np.int64)
    hy, hw = np.zeros(n_bins + 1, dtype=dtype), np.zeros(n_bins + 1, dtype=dtype)
    np.add.at(hy, ind, w * y)
    np.add.at(hw, ind, w)
    hy[n_bins - oversample + 1:] = hy[1:oversample + 1]
    hw[n_bins - oversample + 1:] = hw[1:oversample + 1]
    return np.cumsum(hy), np.cumsum(hw), (w * y).sum(), w.sum(), t_min, fragile


def bls_box(cy, cw, Y, W, s, m):
    """the four statistics of the boxes starting at bin(s) s, m bins wide; inadmissible ones NaN"""
    y_in, w_in = cy[s + m] - cy[s], cw[s + m] - cw[s]
    y_out, w_out = Y - y_in, W - w_in
    with np.errstate(all="ignore"):
        depth = y_out / w_out - y_in / w_in
        depth_err = np.sqrt(1 / w_in + 1 / w_out)
        out = np.stack([depth, depth_err, depth / depth_err, 0.5 * w_in * depth ** 2])
    return np.where((w_in > 0) & (w_out > 0), out, np.nan)


def bls_power(t, y, yerr, periods, durations, oversample=10, objective="likelihood", dtype=np.float64):
    """-> dict of (P,) arrays (FIELDS) and 'fragile' (P,) bool"""
    delta, ms = bls_plan(durations, oversample)
    res = {k: np.full(len(periods), np.nan, dtype=dtype) for k in FIELDS}
    res["fragile"] = np.zeros(len(periods), dtype=bool)
    row = 3 if objective == "likelihood" else 2
    for i, p in enumerate(np.asarray(periods, dtype=np.float64)):
        cy, cw, Y, W, t_min, res["fragile"][i] = bls_prefix(t, y, yerr, p, delta, oversample, dtype)
        n_bins = len(cy) - 1
        best = (-np.inf, None, None, None)
        for m in ms:                                   # (k, s) order; strict > keeps the first maximiser
            s = np.arange(0, n_bins - m + 1)
            box = bls_box(cy, cw, Y, W, s, m)
            obj = np.where(np.isnan(box[row]), -np.inf, box[row])
            j = int(np.argmax(obj)) if len(obj) else 0
            if len(obj) and obj[j] > best[0]:
                best = (obj[j], j, m, box[:, j])
        res["power"][i] = best[0]
        if best[1] is not None:
            _, s, m, box = best
            res["depth"][i], res["depth_err"][i], res["depth_snr"][i], res["log_likelihood"][i] = box
            res["duration"][i] = m * dtype(delta)
            res["transit_time"][i] = np.fmod(s * dtype(delta) + dtype(0.5) * m * dtype(delta) + t_min, dtype(p))
    return res


def bls_at(t, y, yerr, p, durations, oversample, duration, transit_time, dtype=np.float64):
    """the statistics (depth, depth_err, depth_snr, log_likelihood) of the box that a returned (duration, transit_time) names"""
    delta, _ = bls_plan(durations, oversample)
    cy, cw, Y, W, t_min, _ = bls_prefix(t, y, yerr, p, delta, oversample, dtype)
    n_bins = len(cy) - 1
    m = int(round(float(duration) / delta))
    # transit_time = fmod(s delta + m delta / 2 + t_min, p): the start bin, up to whole periods
    x = (float(transit_time) - float(t_min) - 0.5 * m * delta) / delta
    cands = [int(round(x + k * float(p) / delta)) for k in range(-2, 3)]
    want = [s for s in cands if 0 <= s <= n_bins - m and
            abs(np.fmod(s * delta + 0.5 * m * delta + float(t_min), float(p)) - float(transit_time)) < 1e-6 * delta]
    assert want, ("no start bin reproduces the transit time", p, duration, transit_time)
    return bls_box(cy, cw, Y, W, np.array(want[:1]), m)[:, 0]


def _misfit(A, b, dtype):
    """min |A x - b|^2"""
    if dtype == np.float64:
        x = np.linalg.lstsq(A, b, rcond=None)[0]
        r = b - A @ x
        return r @ r
    q = []                                                 # longdouble: Gram-Schmidt, twice
    r = b.copy()
    for j in range(A.shape[1]):
        v = A[:, j].copy()
        for _ in range(2):
            for u in q:
                v = v - (u @ v) * u
        nv = np.sqrt(v @ v)
        if nv > 1e-12 * np.sqrt(A[:, j] @ A[:, j]):
            q.append(v / nv)
    for _ in range(2):
        for u in q:
            r = r - (u @ r) * u
    return r @ r


def lomb_scargle_power(t, y, yerr, frequencies, dtype=np.float64):
    t = np.asarray(t, dtype=dtype)
    y, w = _weights(y, yerr, dtype)
    sw = np.sqrt(w)
    ybar = (w * y).sum() / w.sum()
    chi2_0 = (w * (y - ybar) ** 2).sum()
    two_pi = 2 * np.pi if dtype == np.float64 else 2 * np.arctan(dtype(1)) * 4
    out = np.empty(len(frequencies), dtype=dtype)
    for i, f in enumerate(frequencies):
        x = two_pi * dtype(f) * t
        A = np.stack([np.sin(x), np.cos(x), np.ones_like(x)], axis=1) * sw[:, None]
        out[i] = 0.5 * (chi2_0 - _misfit(A, sw * y, dtype))
    return out


def bls_autoperiod(t, durations, minimum_period=None, maximum_period=None, minimum_n_transit=3, frequency_factor=1.0):
    t, durations = np.asarray(t, dtype=np.float64), np.atleast_1d(np.asarray(durations, dtype=np.float64))
    T = t.max() - t.min()
    df = frequency_factor * durations.min() / T ** 2
    maximum_period = T / (minimum_n_transit - 1) if maximum_period is None else maximum_period
    minimum_period = 2 * durations.max() if minimum_period is None else minimum_period
    f_hi, f_lo = 1 / minimum_period, 1 / maximum_period
    return 1 / (f_hi - df * np.arange(1 + int(np.round((f_hi - f_lo) / df))))


def rel_diff(a, b, scale=None):
    """max |a - b| / scale (default: |b| elementwise)"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    scale = np.abs(b) if scale is None else scale
    return float(np.max(np.abs(a - b) / scale))
