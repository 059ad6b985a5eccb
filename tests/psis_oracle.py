"""The numpy statement of the PSIS-LOO / WAIC definition of exoplanet_amd/comparison.py, for the tests:
one column at a time, in float64 or -- through ``dtype`` -- in np.longdouble, every sum taken one term after the other in the
order the definition names.  Vehtari, Gelman & Gabry (2017), Vehtari et al. (2024); the generalised-Pareto fit is Zhang &
Stephens (2009) as ArviZ's ``_gpdfit`` applies it."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)          # the definition's eps is that of float64, whatever the arithmetic runs in
DBL_MIN = float(np.finfo(np.float64).tiny)
OUTPUTS = ("elpd", "k", "lppd", "p_waic")


def tail_length(S, reff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / reff)))"""
    return int(math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / reff)))) if S > 0 else 0


def _sum(terms, dtype):
    acc = dtype(0.0)
    for t in terms:
        acc = acc + t
    return acc


def gpd_fit(u, dtype=np.float64):
    """u ascending, n > 4 of them -> (k, sigma)"""
    n = len(u)
    m = 30 + int(math.floor(math.sqrt(n)))
    quart = u[int(math.floor(n / 4.0 + 0.5)) - 1]
    b = np.empty(m, dtype=dtype)
    kk = np.empty(m, dtype=dtype)
    L = np.empty(m, dtype=dtype)
    for i in range(1, m + 1):
        b[i - 1] = (dtype(1.0) - np.sqrt(dtype(m) / (dtype(i) - dtype(0.5)))) / (dtype(3.0) * quart) + dtype(1.0) / u[n - 1]
        kk[i - 1] = _sum(np.log1p(-b[i - 1] * u), dtype) / dtype(n)
        L[i - 1] = dtype(n) * (np.log(-b[i - 1] / kk[i - 1]) - kk[i - 1] - dtype(1.0))
    w = np.empty(m, dtype=dtype)
    for i in range(m):
        w[i] = dtype(1.0) / _sum(np.exp(L - L[i]), dtype)          # (an overflow to inf: weight 0)
    keep = w >= dtype(10.0 * EPS)
    total = _sum(w[keep], dtype)
    b_post = _sum(b[keep] * (w[keep] / total), dtype)
    k1 = _sum(np.log1p(-b_post * u), dtype) / dtype(n)
    sigma = -k1 / b_post
    k = (dtype(n) * k1 + dtype(5.0)) / (dtype(n) + dtype(10.0))
    return k, sigma


def column(values, M, dtype=np.float64):
    """one column -> dict(elpd, k, lppd, p_waic, n_tail) and, for the regularity check, u_quartile"""
    nan = dtype(np.nan)
    l = np.asarray(values, dtype=np.float64).astype(dtype)
    S = l.size
    if S == 0 or not np.all(np.isfinite(l)):
        return dict(elpd=nan, k=nan, lppd=nan, p_waic=nan, n_tail=0, u_quartile=None)
    with np.errstate(all="ignore"):
        lmin, lmax = l.min(), l.max()
        x = lmin - l
        c = max(np.sort(x)[max(S - M - 1, 0)], np.log(dtype(DBL_MIN)))
        tail = x > c
        n = int(tail.sum())
        xt = np.sort(x[tail])
        ec = np.exp(c)
        k, xs, uq = dtype(np.inf), xt.copy(), None
        if n > 4:
            u = np.exp(xt) - ec
            uq = u[int(math.floor(n / 4.0 + 0.5)) - 1]
            k, sigma = gpd_fit(u, dtype)
            if np.isfinite(k):
                p = (np.arange(n).astype(dtype) + dtype(0.5)) / dtype(n)
                if abs(k) < EPS:
                    q = -sigma * np.log1p(-p)
                else:
                    q = sigma * np.expm1(-k * np.log1p(-p)) / k
                xs = np.minimum(np.log(q + ec), dtype(0.0))
        # the draws outside the tail enter lse through exp(x_s), in the rows' order, and the elpd sum as a count
        body = _sum(np.exp(x[~tail]), dtype)
        lse = np.log(body + _sum(np.exp(xs), dtype))
        t = xs + (lmin - xt)
        mx = max(t.max() if n else dtype(-np.inf), lmin if n < S else dtype(-np.inf))
        acc = dtype(S - n) * np.exp(lmin - mx) if n < S else dtype(0.0)
        acc = acc + _sum(np.exp(t - mx), dtype)
        elpd = np.log(acc) + mx - lse
        lppd = np.log(_sum(np.exp(l - lmax), dtype)) + lmax - np.log(dtype(S))
        mean = _sum(l, dtype) / dtype(S)
        var = _sum((l - mean) * (l - mean), dtype) / dtype(S)
    return dict(elpd=elpd, k=k, lppd=lppd, p_waic=var, n_tail=n, u_quartile=uq)


def columns(values, M, dtype=np.float64):
    """values (S, N) -> {elpd, k, lppd, p_waic: (N,) of dtype; n_tail: int32 (N,)}"""
    values = np.asarray(values, dtype=np.float64)
    res = [column(values[:, j], M, dtype) for j in range(values.shape[1])]
    out = {key: np.array([r[key] for r in res], dtype=dtype) for key in OUTPUTS}
    out["n_tail"] = np.array([r["n_tail"] for r in res], dtype=np.int32)
    return out


BAD = ("a NaN", "a +inf", "a -inf")


def column_families(S, rs):
    """the columns the tests run: name -> (S,) array of log-likelihoods.  The three of BAD give NaN everywhere; every other one
    is regular (tests/test_psis_host.py asserts it)."""
    M = tail_length(S)
    normal = -0.5 * math.log(2 * math.pi) - 0.5 * (0.7 - 0.3 * rs.randn(S)) ** 2
    two = np.full(S, -1.0)
    # fewer than M draws above the cut-off: ties across it.  (Equal u_j make b_i = 0 where m / (i - 0.5) = 16, i.e. a tail of
    # 100 .. 120 or 676 .. 728 values: M / 3 + 1 stays clear of both at the sizes the tests run.)
    two[rs.permutation(S)[:M // 3 + 1 if S > 1 else 0]] = -2.0
    far = -0.5 * (0.2 * rs.randn(S)) ** 2
    far[rs.randint(S)] -= 30.0
    fam = {
        "normal model": normal,
        "Student-t outlier": -0.5 * (4.0 - rs.standard_t(4, S)) ** 2,      # an outlying point, heavy-tailed draws: k > 0.7
        "constant": np.full(S, -1.25),
        "two values, ties across the cut-off": two,
        "one far draw": far,
        "near -1e6, spread 1e-3": -1e6 + 1e-3 * rs.randn(S),
        "exp underflows": -20000.0 * rs.rand(S),
    }
    for name, bad in zip(BAD, (np.nan, np.inf, -np.inf)):
        col = normal.copy()
        col[rs.randint(S)] = bad
        fam[name] = col
    return fam


def allowance(got, f64, ld, key, family=None):
    """the error of `got` in units of the float64 statement's own error against long double (floor: one eps): relative to
    max(1, |value|) for elpd, lppd and p_waic, absolute for k.  `family`: an integer per column; the columns of one family (and
    size) share one unit, the largest error of the float64 statement among them -- without it every column is a family of its
    own.  NaN and inf must agree exactly: those entries count as 0 where they do, inf where they do not."""
    got, f64, ld = (np.asarray(a, dtype=np.longdouble) for a in (got, f64, ld))
    fin = np.isfinite(ld)
    agree = (np.isnan(got) & np.isnan(ld)) | (got == ld)
    scale = np.ones_like(ld) if key == "k" else np.maximum(1.0, np.abs(np.where(fin, ld, 1.0)))
    with np.errstate(invalid="ignore"):
        unit = np.maximum(np.abs(np.where(fin, f64 - ld, 0.0)) / scale, EPS)
        err = np.abs(np.where(fin, got - ld, 0.0)) / scale
    if family is not None:
        family = np.asarray(family)
        unit = np.array([unit[family == f].max() for f in family], dtype=np.longdouble)
    ratio = np.where(fin, err / unit, np.where(agree, 0.0, np.inf))
    ratio = np.where(fin & ~np.isfinite(got), np.inf, ratio)
    return ratio.astype(np.float64)
