"""The five operations of the dense metric (exoplanet_amd/csrc/exo_metric_core.hpp) stated in numpy at a
chosen precision -- long double is the reference, float64 the yardstick --, the inputs the tests share, and the rule that
measures an error.

The rule is the project's (tests/psis_oracle.py, tests/astrometric_oracle.py): one unit is the error of the FLOAT64 numpy
statement against long double, and the allowance is 16 units.  Here the outputs of one operation on one case share one unit:
the largest error of the float64 statement among them, and at least one eps of the output's scale (its largest magnitude).  The
triangular products, the substitution and the factorisation are backward stable, i.e. their error bounds are normwise -- an
entry that cancels to nearly nothing carries the absolute error of its neighbours in any arithmetic, so an entrywise unit
would measure nothing but that cancellation."""
import numpy as np

EPS = np.finfo(np.float64).eps
FORWARD, TRANSPOSED, SOLVE = 0, 1, 2
SIZES_N = (1, 2, 7, 33, 64)
SIZES_D = (1, 3, 64, 65)
CONDITIONS = (1.0, 1e2, 1e4, 1e6, 1e8)


def covariance(n, condition, rng):
    """C = Q diag(logspace(0, -log10(condition), n)) Q^T, Q from a QR of a seeded normal matrix"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    C = (Q * np.logspace(0.0, -np.log10(condition), n)) @ Q.T
    return 0.5 * (C + C.T)


def apply(chol, center, rows, mode, dtype):
    L, c, X = (np.asarray(a, dtype=dtype) for a in (np.tril(chol), center, rows))
    n = L.shape[0]
    out = np.empty_like(X)
    if mode == FORWARD:
        for i in range(n):
            acc = L[i, 0] * X[:, 0]
            for j in range(1, i + 1):
                acc = acc + L[i, j] * X[:, j]
            out[:, i] = c[i] + acc
    elif mode == TRANSPOSED:
        for j in range(n):
            acc = X[:, j] * L[j, j]
            for i in range(j + 1, n):
                acc = acc + X[:, i] * L[i, j]
            out[:, j] = acc
    else:
        for i in range(n):
            acc = X[:, i] - c[i]
            for j in range(i):
                acc = acc - L[i, j] * out[:, j]
            out[:, i] = acc / L[i, i]
    return out


def accumulate(q, shift, dtype):
    """(sum1 (n), sum2 (n, n) lower triangle, count) of the rows of q without a non-finite element, from zero sums"""
    q = np.asarray(q)
    n = q.shape[1]
    sum1, sum2, count = np.zeros(n, dtype=dtype), np.zeros((n, n), dtype=dtype), 0
    s = np.asarray(shift, dtype=dtype)
    for row in q:
        if not np.isfinite(row).all():
            continue
        dq = row.astype(dtype) - s
        sum1 = sum1 + dq
        sum2 = sum2 + np.tril(np.outer(dq, dq))
        count += 1
    return sum1, sum2, count


def update(sum1, sum2, count, shift, dtype, shrink=True):
    """(status, cov, chol, center); status 0 ok, 1 fewer than two rows, 2 a non-finite entry, 3 a pivot <= 0"""
    if count < 2:
        return 1, None, None, None
    s1, s2, s = (np.asarray(a, dtype=dtype) for a in (sum1, sum2, shift))
    n = s1.shape[0]
    N = dtype(count)
    m = s + s1 / N
    full = np.tril(s2) + np.tril(s2, -1).T
    S = (full - np.outer(s1, s1) / N) / (N - dtype(1))
    Sigma = N / (N + dtype(5)) * S + dtype(1e-3) * (dtype(5) / (N + dtype(5))) * np.diag(np.diag(S)) if shrink else S
    if not (np.isfinite(m).all() and np.isfinite(Sigma).all()):
        return 2, None, None, None
    L = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        for j in range(i + 1):
            acc = Sigma[i, j] - (L[i, :j] * L[j, :j]).sum()
            if i == j:
                if not np.isfinite(acc):
                    return 2, None, None, None
                if not acc > 0:
                    return 3, None, None, None
                L[i, i] = np.sqrt(acc)
            else:
                L[i, j] = acc / L[j, j]
    return 0, Sigma, L, m


def ratio(got, f64, ld):
    """the largest error of `got` against long double in units of the float64 statement's (module docstring)"""
    got, f64, ld = (np.asarray(a, dtype=np.longdouble) for a in (got, f64, ld))
    assert np.isfinite(ld).all() and np.isfinite(f64).all()
    if not np.isfinite(got).all():
        return np.inf
    unit = max(np.abs(f64 - ld).max(), EPS * np.abs(ld).max())
    return float(np.abs(got - ld).max() / unit)


def case(n, D, condition, seed):
    """the inputs of one (n, D): a metric of the condition number, rows for the three maps, a warm-up window whose mean is 1e4
    times its spread (with a NaN row and an infinite one where there are rows to spare), and the sums of a longer window of the
    same kind for the update.  Everything float64: the inputs are exact for every statement."""
    rng = np.random.RandomState(seed)
    C = covariance(n, condition, rng)
    chol = np.linalg.cholesky(C)
    center = 10.0 * rng.standard_normal(n)
    x = rng.standard_normal((D, n))
    gq = rng.standard_normal((D, n)) * np.logspace(-2, 2, n)
    q = np.asarray(apply(chol, center, x, FORWARD, np.longdouble), dtype=np.float64)
    spread = 1e-3
    mean = 1e4 * spread * (1.0 + rng.uniform(size=n))
    window = mean + spread * rng.standard_normal((D, n)) @ chol.T
    if D >= 3:
        window[1, n // 2] = np.nan
        window[D - 1, 0] = np.inf
    shift = mean + spread * rng.standard_normal(n)
    longer = mean + spread * rng.standard_normal((4 * n + 3, n)) @ chol.T
    s1, s2, count = accumulate(longer, shift, np.longdouble)
    return dict(n=n, D=D, condition=condition, chol=chol, center=center, x=x, gq=gq, q=q, window=window, shift=shift,
                sum1=np.asarray(s1, dtype=np.float64), sum2=np.asarray(s2, dtype=np.float64), count=count)


def cases(sizes_d=SIZES_D):
    out = []
    for a, n in enumerate(SIZES_N):
        for b, D in enumerate(sizes_d):
            out.append(case(n, D, CONDITIONS[(a + b) % len(CONDITIONS)], 1000 + 10 * a + b))
    return out


def statements(c, dtype):
    """the five operations on a case at one precision"""
    out = {"forward": apply(c["chol"], c["center"], c["x"], FORWARD, dtype),
           "transposed": apply(c["chol"], c["center"], c["gq"], TRANSPOSED, dtype),
           "solve": apply(c["chol"], c["center"], c["q"], SOLVE, dtype)}
    s1, s2, count = accumulate(c["window"], c["shift"], dtype)
    out["sum1"], out["sum2"], out["count"] = s1, s2, count
    status, cov, chol, center = update(c["sum1"], c["sum2"], c["count"], c["shift"], dtype)
    assert status == 0
    out["cov"], out["chol"], out["center"] = cov, chol, center
    return out


FLOATS = ("forward", "transposed", "solve", "sum1", "sum2", "cov", "chol", "center")
