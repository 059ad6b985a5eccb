"""The numpy statement of the quantile definition of exoplanet_amd/predictive.py, for the tests: drop
NaN, np.sort, the position from whole numbers, the four-operation interpolation."""
from fractions import Fraction

import numpy as np


def fraction(percent):
    """percent -> (a, b), percent / 100 = a / b in lowest terms"""
    f = Fraction(str(percent)) / 100
    return f.numerator, f.denominator


def column_quantile(col, percent):
    x = np.asarray(col, dtype=np.float64)
    x = np.sort(x[~np.isnan(x)]) + 0.0          # (an order statistic is a number: -0 -> +0)
    m = x.size
    if m == 0:
        return np.float64(np.nan)
    a, b = fraction(percent)
    num = (m - 1) * a
    lo, rem = num // b, num % b
    if rem == 0:
        return x[lo]
    with np.errstate(invalid="ignore", over="ignore"):
        frac = np.float64(rem) / np.float64(b)
        d = x[lo + 1] - x[lo]
        s = frac * d
        return x[lo] + s


def quantiles(values, percent):
    """values (S, N) -> (Q, N) and the (N,) counts of values that are not NaN"""
    values = np.asarray(values, dtype=np.float64)
    out = np.array([[column_quantile(values[:, j], p) for j in range(values.shape[1])] for p in percent], dtype=np.float64)
    return out.reshape(len(percent), values.shape[1]), (~np.isnan(values)).sum(0).astype(np.int32)


def quantiles_dense(values, percent):
    """the same statement for an array without NaN, all columns at once (what a large case can afford)"""
    x = np.sort(np.asarray(values, dtype=np.float64), axis=0) + 0.0
    m = x.shape[0]
    rows = []
    for p in percent:
        a, b = fraction(p)
        lo, rem = divmod((m - 1) * a, b)
        if rem == 0:
            rows.append(x[lo].copy())
        else:
            frac = np.float64(rem) / np.float64(b)
            d = x[lo + 1] - x[lo]
            s = frac * d
            rows.append(x[lo] + s)
    return np.stack(rows)


def column_families(S, rs):
    """the columns the tests run: name -> (S,) array"""
    tiny = 5e-324
    special = np.array([1e300, -1e300, tiny, -tiny, np.inf, -np.inf, 2.2250738585072014e-308, -1e-310])
    pool = np.concatenate([special, 1e-310 * rs.randn(S)])
    some_nan = rs.randn(S)
    some_nan[rs.rand(S) < 0.3] = np.nan
    return {
        "no ties": rs.randn(S),
        "many ties": np.round(3 * rs.randn(S)) / 4,
        "zeros of both signs": np.where(rs.rand(S) < 0.5, -0.0, 0.0) * 1.0,
        "denormals, 1e300, inf": pool[rs.permutation(pool.size)[:S]],
        "one value": np.full(S, -2.5),
        "some NaN": some_nan,
        "all NaN": np.full(S, np.nan),
        "model-like": 1.0 - 0.01 * (rs.rand() < 0.5) + 1e-4 * rs.randn(S),
    }


def same(a, b):
    """exact equality, both sides NaN where either is, and the sign of a zero"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b))))
