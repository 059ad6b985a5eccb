"""The two operations of the Laplace approximation (exoplanet_amd/csrc/exo_laplace_core.hpp) stated in
numpy at a chosen precision -- long double is the reference, float64 the yardstick --, the inputs the tests share, and the rule
that measures an error.  This statement is the definition.

The rule is the project's (tests/metric_oracle.py): one unit is the error of the FLOAT64 numpy statement against long double,
and the allowance is 16 units.  The chains of one case share one unit per output: the largest error of the float64 statement
among them, and at least one eps of the output's scale (its largest magnitude over the chains).  The factorisation, the
inverse and the products are backward stable, i.e. their error bounds are normwise."""
import numpy as np

EPS = np.finfo(np.float64).eps
CBRT_EPS = 6.0554544523933395e-06          # EPS ** (1 / 3), the constant of the core
OK, NOT_FINITE, NOT_POSITIVE = 0, 1, 2
SIZES_N = (1, 2, 7, 64)
SIZES_D = (1, 3, 65)
CONDITIONS = (1e2, 1e8)
MASKED = (0, 2, 3, 6)                      # the masked case: n = 7, m = 4
FLOATS = ("hess", "cov", "sd", "logdet", "log_evidence", "asymmetry", "fd_error")


# ---- the definition ------------------------------------------------------------------------------------------------------------
def steps(x, free, scale, hess, delta, dtype):
    """h (D, m): the pilot step eps^(1/3) scale_k (scale: (n,), (D, n) or None: max(|x|, 1)); with a previous pass's hess (D, m,
    m), delta / sqrt(H_kk) where H_kk and the quotient are finite and positive"""
    x = np.asarray(x, dtype=dtype)
    xf = x[:, free]
    sc = np.maximum(np.abs(xf), dtype(1)) if scale is None else np.broadcast_to(np.asarray(scale, dtype=dtype), x.shape)[:, free]
    h = dtype(CBRT_EPS) * sc
    if hess is not None:
        hkk = np.diagonal(np.asarray(hess, dtype=dtype), axis1=1, axis2=2)
        with np.errstate(all="ignore"):
            good = np.isfinite(hkk) & (hkk > 0)
            hf = dtype(delta) / np.sqrt(np.where(good, hkk, dtype(1)))
            good &= np.isfinite(hf) & (hf > 0)
        h = np.where(good, hf, h)
    return h


def points(x, free, scale, hess, delta, order, dtype):
    """(points (D, order m, n), dx (D, order m)): row r = s m + k moves coordinate free[k] by +h, -h, +2h, -2h (s = 0 .. 3);
    dx is the realised offset fl(fl(x + off) - x)"""
    x = np.asarray(x, dtype=dtype)
    D, n = x.shape
    m = len(free)
    h = steps(x, free, scale, hess, delta, dtype)
    pts = np.repeat(x[:, None, :], order * m, axis=1)
    dx = np.empty((D, order * m), dtype=dtype)
    for s in range(order):
        off = (h, -h, dtype(2) * h, -(dtype(2) * h))[s]
        for k, j in enumerate(free):
            p = x[:, j] + off[:, k]
            pts[:, s * m + k, j] = p
            dx[:, s * m + k] = p - x[:, j]
    return pts, dx


def _nanmax0(values):
    """the largest of 0 and the values that are not NaN"""
    acc = values.dtype.type(0)
    for v in values:
        if v > acc:
            acc = v
    return acc


def factor_chain(grad, dx, logp, free, order, dtype):
    """one chain: grad (order m, n) -- the gradient of logp at the stencil's points --, dx (order m), logp -> a dict of the
    outputs and "status" """
    with np.errstate(all="ignore"):
        return _factor_chain(grad, dx, logp, free, order, dtype)


def _factor_chain(grad, dx, logp, free, order, dtype):
    free = list(free)
    m = len(free)
    g = np.asarray(grad, dtype=dtype)[:, free]                      # (order m, m): row r, free coordinate i
    dx = np.asarray(dx, dtype=dtype)
    nan = dtype(np.nan)

    def raw(s):
        den = dx[s * m:(s + 1) * m] - dx[(s + 1) * m:(s + 2) * m]
        A = -(g[s * m:(s + 1) * m] - g[(s + 1) * m:(s + 2) * m]) / den[:, None]     # [k][i]
        return A.T, den                                                               # [i][k]

    A1, den1 = raw(0)
    bad = not (np.isfinite(g).all() and np.isfinite(dx).all()) or bool((den1 == 0).any())
    A = A1
    H1 = H2 = None
    if order == 4:
        A2, den2 = raw(2)
        bad = bad or bool((den2 == 0).any())
        A = (dtype(4) * A1 - A2) / dtype(3)
        H1, H2 = dtype(0.5) * (A1 + A1.T), dtype(0.5) * (A2 + A2.T)
    H = dtype(0.5) * (A + A.T)
    hd = np.diagonal(H).copy()
    scale = np.sqrt(np.abs(np.outer(hd, hd)))
    low = np.tril_indices(m, -1)
    out = {"hess": H, "asymmetry": _nanmax0((np.abs(A - A.T) / scale)[low])}
    lowd = np.tril_indices(m)
    out["fd_error"] = _nanmax0((np.abs(H1 - H2) / scale)[lowd]) if order == 4 else nan
    status = NOT_FINITE if bad or not np.isfinite(hd).all() else (NOT_POSITIVE if (hd <= 0).any() else OK)
    R = np.zeros((m, m), dtype=dtype)
    if status == OK:
        s = dtype(1) / np.sqrt(hd)
        C = (s[:, None] * H) * s[None, :]
        C[np.diag_indices(m)] = dtype(1)
        for i in range(m):
            for j in range(i + 1):
                acc = C[i, j]
                for k in range(j):
                    acc = acc - R[i, k] * R[j, k]
                if i == j:
                    if not acc > dtype(m) * dtype(EPS):
                        status = NOT_POSITIVE
                        break
                    R[i, i] = np.sqrt(acc)
                else:
                    R[i, j] = acc / R[j, j]
            if status != OK:
                break
    out["status"] = status
    if status != OK:
        out.update(cov=np.full((m, m), nan), sd=np.full(m, nan), logdet=nan, log_evidence=nan)
        return out
    a, b = np.log(hd[0]), np.log(R[0, 0])
    for i in range(1, m):
        a = a + np.log(hd[i])
        b = b + np.log(R[i, i])
    logdet = a + dtype(2) * b
    T = np.zeros((m, m), dtype=dtype)
    for k in range(m):
        T[k, k] = dtype(1) / R[k, k]
        for i in range(k + 1, m):
            acc = -(R[i, k] * T[k, k])
            for j in range(k + 1, i):
                acc = acc - R[i, j] * T[j, k]
            T[i, k] = acc / R[i, i]
    cov = np.empty((m, m), dtype=dtype)
    for i in range(m):
        for k in range(i + 1):
            acc = T[i, i] * T[i, k]
            for l in range(i + 1, m):
                acc = acc + T[l, i] * T[l, k]
            cov[i, k] = cov[k, i] = s[i] * s[k] * acc
    log2pi = np.log(dtype(8) * np.arctan(dtype(1)))
    out.update(cov=cov, sd=np.sqrt(np.diagonal(cov)), logdet=logdet,
               log_evidence=(dtype(logp) + dtype(0.5) * dtype(m) * log2pi) - dtype(0.5) * logdet)
    return out


def factor(grad, dx, logp, free, order, dtype):
    """all chains: a dict of stacked outputs, "status" int32 (D,)"""
    chains = [factor_chain(grad[d], dx[d], logp[d], free, order, dtype) for d in range(len(grad))]
    out = {key: np.stack([np.asarray(c[key]) for c in chains]) for key in FLOATS}
    out["status"] = np.array([c["status"] for c in chains], dtype=np.int32)
    return out


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def ratio(got, f64, ld):
    """the largest error of `got` against long double in units of the float64 statement's (module docstring); NaNs must sit
    where the statement has them"""
    got, f64, ld = (np.asarray(a, dtype=np.longdouble) for a in (got, f64, ld))
    if not (np.array_equal(np.isnan(got), np.isnan(ld)) and np.array_equal(np.isnan(f64), np.isnan(ld))):
        return np.inf
    keep = ~np.isnan(ld)
    if not keep.any():
        return 0.0
    got, f64, ld = got[keep], f64[keep], ld[keep]
    if not np.isfinite(got).all():
        return np.inf
    unit = max(np.abs(f64 - ld).max(), EPS * np.abs(ld).max())
    err = np.abs(got - ld).max()
    return float(err / unit) if unit > 0 else (0.0 if err == 0 else np.inf)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def hessian(m, condition, rng):
    """(H, sigma): H = S^-1 C S^-1, C with a unit diagonal and the condition number asked for, parameter scales sigma spread
    over 1e-5 .. 1e2.  C is a symmetric circulant matrix -- its diagonal is constant whatever its eigenvalues lambda_k =
    condition^(-min(k, m - k) / (m // 2)) -- with random signs and a random permutation of the coordinates."""
    k = np.arange(m)
    lam = condition ** (-np.minimum(k, m - k) / max(m // 2, 1))
    C = (lam[None, None, :] * np.cos(2.0 * np.pi * k[None, None, :] * (k[:, None, None] - k[None, :, None]) / m)).sum(2)
    C = 0.5 * (C + C.T) / C[0, 0]
    sign, perm = np.sign(rng.standard_normal(m)), rng.permutation(m)
    C = (C * np.outer(sign, sign))[np.ix_(perm, perm)]
    sigma = 10.0 ** rng.uniform(-5.0, 2.0, size=m) if m > 1 else np.array([3e-4])
    if m > 1:
        sigma[0], sigma[-1] = 1e-5, 1e2
    return C / np.outer(sigma, sigma), sigma


def case(n, free, D, order, condition, seed):
    """synthetic gradient rows of a known symmetric H per chain plus a small antisymmetric part: g(x + e_k dx) = g0 - (H + N)[:, k]
    dx, and for the 2h rows a slightly different H, as a stencil's truncation error makes it.  The steps are realised ones
    (dx = fl(fl(x + h) - x)).  Everything float64: the inputs are exact for every statement."""
    rng = np.random.RandomState(seed)
    free = list(range(n)) if free is None else list(free)
    m = len(free)
    grad = np.zeros((D, order * m, n))
    dx = np.zeros((D, order * m))
    logp = -100.0 * rng.uniform(1.0, 2.0, size=D)
    x = np.zeros((D, n))
    for d in range(D):
        H, sigma = hessian(m, condition, rng)
        x[d, free] = sigma * rng.standard_normal(m) * 10.0
        N = 1e-7 * rng.standard_normal((m, m)) / np.outer(sigma, sigma)
        N = N - N.T
        g0 = 1e-3 * rng.standard_normal(n) / np.maximum(np.abs(x[d]), 1e-5)
        h = 1e-3 * sigma
        for s in range(order):
            off = (h, -h, 2 * h, -2 * h)[s]
            Hs = (H + N) * (1.0 + (1e-11 if s < 2 else 4e-11) * np.sign(rng.standard_normal((m, m))))
            for k, j in enumerate(free):
                r = s * m + k
                dx[d, r] = (x[d, j] + off[k]) - x[d, j]
                grad[d, r] = g0 * (1.0 + 1e-3 * rng.standard_normal(n))         # (the held coordinates carry something too)
                grad[d, r, free] = g0[free] - Hs[:, k] * dx[d, r]
    return dict(n=n, m=m, D=D, order=order, condition=condition, free=free, grad=grad, dx=dx, logp=logp, x=x)


def cases():
    out = []
    shapes = [(n, None) for n in SIZES_N] + [(7, MASKED)]
    for a, (n, free) in enumerate(shapes):
        for b, D in enumerate(SIZES_D):
            if n == 64 and D == 65:
                D = 5                                              # (the 64 x 64 chains in long double: seconds each)
            out.append(case(n, free, D, (2, 4)[(a + b) % 2], CONDITIONS[(a + b // 2) % 2], 2000 + 10 * a + b))
    return out


def statement(c, dtype):
    return factor(c["grad"], c["dx"], c["logp"], c["free"], c["order"], dtype)


def failing_chains():
    """(label, status, grad (2, n), dx (2), order 2, n) of one chain each: an indefinite H with a positive diagonal; a negative
    diagonal entry; a NaN in one gradient row; a step lost to rounding at x = 1e20"""
    def rows(H, dx):
        m = H.shape[0]
        g = np.zeros((2 * m, m))
        for k in range(m):
            g[k] = -H[:, k] * dx[k]
            g[m + k] = -H[:, k] * dx[m + k]
        return g

    h = np.array([1e-3, 1e-3, -1e-3, -1e-3])
    ind = np.array([[1.0, 2.0], [2.0, 1.0]])
    neg = np.array([[1.0, 0.5], [0.5, -1.0]])
    good = np.array([[2.0, 0.5], [0.5, 1.0]])
    nan_rows = rows(good, h)
    nan_rows[2, 1] = np.nan
    lost = np.array([(1e20 + 1e-3) - 1e20, 1e-3, (1e20 - 1e-3) - 1e20, -1e-3])
    return [("indefinite", NOT_POSITIVE, rows(ind, h), h), ("negative diagonal", NOT_POSITIVE, rows(neg, h), h),
            ("a NaN gradient", NOT_FINITE, nan_rows, h), ("a lost step", NOT_FINITE, rows(good, h), lost)]
