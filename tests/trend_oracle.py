"""The robust local-polynomial trend of exoplanet_amd.estimators (running_location / flatten with order = 1, 2), restated in
brute-force numpy: one window at a time, straight from the definition of DESIGN.md section 21, in float64 or in
np.longdouble.  numpy only.  This is the yardstick of tests/test_trend_host.py and tests/test_gpu_trend.py; it shares no code
with the kernels.  The windows, the median and the MAD are those of section 19 (tests/flatten_oracle.py)."""
import numpy as np

import flatten_oracle as F

PIVOT_FLOOR = 1e-10


def _sum(a):
    """in the window's order (numpy's own sum is pairwise)"""
    return np.add.accumulate(a)[-1]


def _horner(c, x):
    r = np.full(x.shape, c[-1], dtype=x.dtype)
    for k in range(len(c) - 2, -1, -1):
        r = r * x + c[k]
    return r


def _stage(v, x, c, scale, cval, n_iter, pivots):
    """exactly n_iter steps c += M^-1 b -> (c, whether the stage ran to its end)"""
    dtype = v.dtype.type
    p = len(c) - 1
    r = dtype(1.0) / (dtype(cval) * scale)
    for _ in range(n_iter):
        d = v - _horner(c, x)
        u = d * r
        inside = np.abs(u) < 1
        q = dtype(1.0) - u * u
        wk = np.where(inside, q * q, dtype(0.0))
        M, b = [], []
        for k in range(2 * p + 1):
            M.append(_sum(wk))
            if k <= p:
                b.append(_sum(d * wk))
            wk = wk * x
        if M[0] == 0:
            return c, False
        floor = dtype(PIVOT_FLOOR) * M[0]
        if p == 0:
            step = [b[0] / M[0]]
        elif p == 1:
            l10 = M[1] / M[0]
            d1 = M[2] - l10 * M[1]
            pivots.append(float(d1 / M[0]))
            if d1 <= floor:
                return c, False
            a1 = (b[1] - l10 * b[0]) / d1
            step = [b[0] / M[0] - l10 * a1, a1]
        else:
            l10, l20 = M[1] / M[0], M[2] / M[0]
            d1 = M[2] - l10 * M[1]
            pivots.append(float(d1 / M[0]))
            if d1 <= floor:
                return c, False
            e = M[3] - l20 * M[1]
            l21 = e / d1
            d2 = (M[4] - l20 * M[2]) - l21 * e
            pivots.append(float(d2 / M[0]))
            if d2 <= floor:
                return c, False
            z1 = b[1] - l10 * b[0]
            z2 = (b[2] - l20 * b[0]) - l21 * z1
            a2 = z2 / d2
            a1 = z1 / d1 - l21 * a2
            step = [(b[0] / M[0] - l10 * a1) - l20 * a2, a1, a2]
        c = [ck + sk for ck, sk in zip(c, step)]
    return c, True


def window_trend(v, tv, t0, t_first, t_last, order, cval=5.0, n_iter=10, rescale=1, dtype=np.float64, pivots=None):
    """One window: `v`, `tv` the m >= 1 participating values and their times in the window's order, `t0` the cadence's own
    time, `t_first`, `t_last` the times at the window's two ends (participating or not).  -> (trend, last scale used);
    every pivot ratio pivot / M_0 met on the way is appended to `pivots`."""
    pivots = [] if pivots is None else pivots
    kind = np.dtype(dtype).type
    v = np.asarray(v, dtype=np.float64).astype(kind)
    tv, t0, t_first, t_last = np.asarray(tv, dtype=np.float64).astype(kind), kind(t0), kind(t_first), kind(t_last)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        med = F.median(v)
        scale = F.mad(v, med)
        if scale == 0:
            return med, scale
        span = max(t_last - t0, t0 - t_first)
        if span == 0:
            return med, scale
        x = (tv - t0) * (kind(1.0) / span)
        p = min(order, np.unique(tv).size - 1)
        c = [med] + [kind(0.0)] * p
        c, ran = _stage(v, x, c, scale, cval, n_iter, pivots)
        for _ in range(rescale):
            if not ran:
                break
            s = F.median(np.abs(v - _horner(c, x)))
            if s == 0:
                break
            scale = s
            c, ran = _stage(v, x, c, scale, cval, n_iter, pivots)
    return c[0], scale


def running_trend(t, y, window_length, order, exclude=None, break_tolerance=None, edge_cutoff=0.0, cval=5.0, n_iter=10, rescale=1,
                  dtype=np.float64, cadences=None, pivots=None):
    """-> trend, scale, each of y's shape (one series); `cadences`: evaluate these only (the others stay NaN).  The windows
    are always formed in float64 (they are part of the definition); `dtype` is the arithmetic inside a window.  order = 0:
    section 19's biweight (tests/flatten_oracle.py), which `rescale` does not touch."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ex = np.zeros(y.shape, dtype=bool) if exclude is None else np.asarray(exclude, dtype=bool)
    lo, hi, edge = F.windows(t, window_length, break_tolerance, edge_cutoff)
    trend, scale = np.full(y.shape, np.nan, dtype=dtype), np.full(y.shape, np.nan, dtype=dtype)
    for i in (range(t.size) if cadences is None else cadences):
        keep = ~ex[lo[i]:hi[i] + 1]
        if edge[i] or not keep.any():
            continue
        v, tv = y[lo[i]:hi[i] + 1][keep], t[lo[i]:hi[i] + 1][keep]
        if order == 0:
            v = v.astype(dtype)
            med = F.median(v)
            scale[i] = F.mad(v, med)
            trend[i] = F.biweight(v, med, scale[i], cval, n_iter)
        else:
            trend[i], scale[i] = window_trend(v, tv, t[i], t[lo[i]], t[hi[i]], order, cval, n_iter, rescale, dtype, pivots)
    return trend, scale


def science_input():
    """the input of the table of DESIGN.md 21.3: 10-minute cadence on [0, 12) and [13.5, 25.5) d, two sines times a
    ramp after each segment's start, box transits, noise 1e-3 -> t, y, the true trend, the in-transit flags"""
    dt = 10.0 / 1440.0
    t = np.concatenate([np.arange(0.0, 12.0 - 0.5 * dt, dt), np.arange(13.5, 25.5 - 0.5 * dt, dt)])
    start = np.where(t < 12.75, 0.0, 13.5)
    truth = (1 + 8e-3 * np.sin(2 * np.pi * t / 4) + 2e-3 * np.sin(2 * np.pi * t / 1.7 + 1)) * (1 + 4e-3 * np.exp(-(t - start) / 0.4))
    period, t0, duration, depth = 2.345, 0.8, 0.12, 2.5e-3
    in_transit = np.abs((t - t0 + 0.5 * period) % period - 0.5 * period) < 0.5 * duration
    rs = np.random.RandomState(1)
    y = truth * np.where(in_transit, 1 - depth, 1.0) + 1e-3 * rs.randn(t.size)
    return t, y, truth, in_transit
