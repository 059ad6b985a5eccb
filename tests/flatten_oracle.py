"""The running location filters of exoplanet_amd.estimators (running_location, flatten, sde), restated in brute-force numpy:
one window at a time, straight from the definition of DESIGN.md section 19, in float64 or in np.longdouble.  numpy only.
This is the yardstick of tests/test_flatten_host.py and tests/test_gpu_flatten.py; it shares no code with the kernels."""
import numpy as np


def windows(t, window_length, break_tolerance=None, edge_cutoff=0.0):
    """-> lo, hi (int arrays: cadence i's window is lo[i] .. hi[i], both included) and the edge flags.  The bounds
    t[i] - h and t[i] + h are ONE float64 operation each, as in the kernel."""
    t = np.asarray(t, dtype=np.float64)
    n = t.size
    h = np.float64(0.5 * window_length)
    opens = np.zeros(n, dtype=bool)
    opens[0] = True
    if break_tolerance is not None:
        opens[1:] = (t[1:] - t[:-1]) > np.float64(break_tolerance)
    starts = np.flatnonzero(opens)
    ends = np.append(starts[1:], n) - 1
    lo, hi, edge = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for s, e in zip(starts, ends):
        for i in range(s, e + 1):
            below, above = t[i] - h, t[i] + h
            inside = np.flatnonzero((t[s:e + 1] >= below) & (t[s:e + 1] <= above)) + s
            lo[i], hi[i] = inside[0], inside[-1]
            assert np.array_equal(inside, np.arange(lo[i], hi[i] + 1))          # (t is sorted: a window is a run)
            edge[i] = (t[i] - t[s] < edge_cutoff) or (t[e] - t[i] < edge_cutoff)
    return lo, hi, edge


def median(v):
    """of a non-empty 1-D array, by the definition: the middle of the sorted values, or half the sum of the middle two"""
    s = np.sort(v)
    m = s.size
    return s[(m - 1) // 2] if m % 2 else s.dtype.type(0.5) * (s[m // 2 - 1] + s[m // 2])


def mad(v, med):
    return median(np.abs(v - med))


def biweight(v, med, scale, cval=5.0, n_iter=10):
    dtype = v.dtype.type
    x = dtype(med)
    if scale == 0:
        return x
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = dtype(1.0) / (dtype(cval) * dtype(scale))
        for _ in range(n_iter):
            d = v - x
            u = d * s
            w = np.where(np.abs(u) < 1, (dtype(1.0) - u * u) ** 2, dtype(0.0))
            sw = w.sum()
            if sw == 0:
                break
            x = x + (d * w).sum() / sw
    return x


def running_location(t, y, window_length, method="biweight", exclude=None, break_tolerance=None, edge_cutoff=0.0, cval=5.0,
                     n_iter=10, dtype=np.float64):
    """-> trend, scale (the MAD), each of y's shape.  The windows are always formed in float64 (they are part of the
    definition); `dtype` is the arithmetic inside a window."""
    y = np.asarray(y, dtype=np.float64)
    rows = np.atleast_2d(y)
    ex = np.zeros(rows.shape, dtype=bool) if exclude is None else np.broadcast_to(np.atleast_2d(np.asarray(exclude, dtype=bool)), rows.shape)
    lo, hi, edge = windows(t, window_length, break_tolerance, edge_cutoff)
    trend, scale = np.full(rows.shape, np.nan, dtype=dtype), np.full(rows.shape, np.nan, dtype=dtype)
    for b in range(rows.shape[0]):
        for i in range(rows.shape[1]):
            if edge[i]:
                continue
            v = rows[b, lo[i]:hi[i] + 1][~ex[b, lo[i]:hi[i] + 1]].astype(dtype)
            if v.size == 0:
                continue
            med = median(v)
            scale[b, i] = mad(v, med)
            trend[b, i] = med if method == "median" else biweight(v, med, scale[b, i], cval, n_iter)
    return trend.reshape(y.shape), scale.reshape(y.shape)


def sde(power, window=151):
    power = np.asarray(power, dtype=np.float64)
    out = ~np.isfinite(power)
    trend, _ = running_location(np.arange(power.size, dtype=np.float64), np.where(out, 0.0, power), float(window - 1), "median",
                                exclude=out)
    resid = power - trend
    ok = np.isfinite(resid) & ~out
    res = np.full(power.shape, np.nan)
    res[ok] = resid[ok] / np.std(resid[ok])
    return res


def main_input(variant="plain"):
    """the main input of tests/test_gpu_flatten.py: N = 1519, a gap, a lone last cadence, transits, outliers"""
    rs = np.random.RandomState(19)
    t = np.sort(rs.uniform(0, 6, 1800))
    t = t[(t < 2.0) | (t > 2.9)]
    t = np.append(t, t[-1] + 3.0)
    y = 1 + 5e-3 * np.sin(2 * np.pi * t / 1.7) + 1e-3 * rs.randn(t.size)
    in_transit = np.abs((t - 0.4 + 0.6) % 1.2 - 0.6) < 0.06
    y[in_transit] -= 0.012
    y[rs.choice(t.size, 12, replace=False)] += 0.03
    exclude = None
    if variant == "ties":
        y = np.round(y * 2000) / 2000
    elif variant == "excluded":
        exclude = in_transit
    elif variant != "plain":
        raise ValueError(variant)
    return t, y, exclude
