"""The astrometric orbit search of DESIGN.md section 23 stated in numpy, in float64 or longdouble: what
exoplanet_amd.estimators.astrometric_power is held to.  Nothing of the package is used: Kepler's equation is solved here by
Newton's iteration to convergence, the 4 x 4 systems by a Cholesky factorisation written here, and the rotation that makes the
test series and takes the elements back to the Thiele-Innes constants is written out here as well."""
import numpy as np

PIVOT_FLOOR = 1e-12     # kPivotFloor: part of the definition
AU_PER_R_SUN = 0.00465046726096215


def _pi(dtype):
    return np.pi if dtype == np.float64 else 4 * np.arctan(dtype(1))


def phase_turns(f, tt, dtype):
    """f * tt less its nearest integer, from the exact product (ls_phase_turns): in longdouble the product of two doubles is
    good to 2^-64; in float64 it is split into hi + lo (Veltkamp / Dekker) so that the integer comes off hi exactly"""
    if dtype != np.float64:
        p = dtype(f) * tt.astype(dtype)
        return p - np.rint(p)
    f, tt = np.float64(f), tt.astype(np.float64)
    hi = f * tt
    split = lambda a: ((a * 134217729.0) - ((a * 134217729.0) - a), a - ((a * 134217729.0) - ((a * 134217729.0) - a)))  # noqa: E731
    fh, fl = split(f)
    th, tl = split(tt)
    lo = ((fh * th - hi) + fh * tl + fl * th) + fl * tl
    return (hi - np.rint(hi)) + lo


def solve_kepler(M, e, dtype):
    """E - e sin E = M, 0 <= e < 1: Newton from E = pi on the folded |M| <= pi (the residual is convex on [0, pi], so the
    iteration descends monotonically) until no element moves by more than a few roundings; in longdouble from the converged
    float64 solution"""
    pi = _pi(dtype)
    M = np.asarray(M, dtype=dtype)
    Mr = M - 2 * pi * np.rint(M / (2 * pi))
    sgn = np.where(Mr < 0, -1, 1).astype(dtype)
    Mr = np.abs(Mr)
    e = np.broadcast_to(np.asarray(e, dtype=dtype), Mr.shape)
    if dtype == np.float64:
        E = np.full(Mr.shape, pi, dtype=dtype)
    else:
        E = np.abs(solve_kepler(Mr.astype(np.float64), e.astype(np.float64), np.float64)).astype(dtype)
    eps = np.finfo(dtype).eps
    for _ in range(200):
        dE = (E - e * np.sin(E) - Mr) / (1 - e * np.cos(E))
        E = E - dE
        if np.max(np.abs(dE)) <= 4 * eps:
            break
    else:
        raise RuntimeError("Kepler's equation did not converge")
    return sgn * E


def orbit_plane(M, e, dtype):
    """-> xi = cos E - e, eta = sqrt(1 - e^2) sin E by the half-angle forms: X = sqrt(1 - e) cos E/2, Y = sqrt(1 + e) sin E/2"""
    e = np.asarray(e, dtype=dtype)
    E = solve_kepler(M, e, dtype)
    X, Y = np.sqrt(1 - e) * np.cos(E / 2), np.sqrt(1 + e) * np.sin(E / 2)
    return X * X - Y * Y, 2 * X * Y


def columns(rho, rho_err, theta, theta_err, dtype):
    """per epoch: x, y, the precision matrix (pxx, pxy, pyy) of the radial and the tangential error, q = P (x, y); and chi2_0"""
    rho, theta = np.asarray(rho, dtype=dtype), np.asarray(theta, dtype=dtype)
    re = np.broadcast_to(np.asarray(rho_err, dtype=dtype), rho.shape)
    te = np.broadcast_to(np.asarray(theta_err, dtype=dtype), rho.shape)
    c, s = np.cos(theta), np.sin(theta)
    x, y = rho * c, rho * s
    wr, wt = 1 / re ** 2, 1 / (rho * te) ** 2
    pxx, pxy, pyy = wr * c * c + wt * s * s, (wr - wt) * c * s, wr * s * s + wt * c * c
    qx, qy = pxx * x + pxy * y, pxy * x + pyy * y
    return dict(x=x, y=y, pxx=pxx, pxy=pxy, pyy=pyy, qx=qx, qy=qy, chi2_0=(x * qx + y * qy).sum())


def scaled_cholesky(Nm, b):
    """Nm (C, 4, 4), b (C, 4) -> power, beta (C, 4), the smallest squared pivot, live: N scaled by sqrt(diag N) to a unit
    diagonal, unpivoted Cholesky; a non-positive diagonal or a squared pivot below the floor: no candidate"""
    dtype = Nm.dtype.type
    C = Nm.shape[0]
    diag = np.stack([Nm[:, k, k] for k in range(4)], 1)
    pos = np.all(diag > 0, 1)
    d = np.sqrt(np.where(pos[:, None], diag, 1))
    M, c = Nm / (d[:, :, None] * d[:, None, :]), b / d
    L, piv = np.zeros((C, 4, 4), dtype), np.ones((C, 4), dtype)
    with np.errstate(all="ignore"):
        for k in range(4):
            p = 1 - (L[:, k, :k] ** 2).sum(1)
            piv[:, k] = p
            L[:, k, k] = np.sqrt(np.where(p > 0, p, 1))
            for i in range(k + 1, 4):
                L[:, i, k] = (M[:, i, k] - (L[:, i, :k] * L[:, k, :k]).sum(1)) / L[:, k, k]
        z = np.zeros((C, 4), dtype)
        for k in range(4):
            z[:, k] = (c[:, k] - (L[:, k, :k] * z[:, :k]).sum(1)) / L[:, k, k]
        u = np.zeros((C, 4), dtype)
        for k in range(3, -1, -1):
            u[:, k] = (z[:, k] - (L[:, k + 1:, k] * u[:, k + 1:]).sum(1)) / L[:, k, k]
    pivot = piv.min(1)
    live = pos & (pivot >= PIVOT_FLOOR)
    return 0.5 * (z * z).sum(1), u / d, pivot, live


def campbell(beta, dtype=np.float64):
    """(..., 4) = TA, TB, TF, TG -> a_angular, incl, omega, Omega in the package's convention (amplitude -a_angular), Omega
    in [0, pi), omega in (-pi, pi]"""
    pi = _pi(dtype)
    beta = np.asarray(beta, dtype=dtype)
    ta, tb, tf, tg = (beta[..., k] for k in range(4))
    k = (ta * ta + tb * tb + tf * tf + tg * tg) / 2
    m = ta * tg - tb * tf
    j = np.sqrt(np.maximum(k * k - m * m, 0))
    a = np.sqrt(j + k)
    with np.errstate(all="ignore"):
        incl = np.arccos(np.clip(m / (j + k), -1, 1))
    p, q = np.arctan2(tb - tf, ta + tg), np.arctan2(-tb - tf, ta - tg)
    Om, om = (p - q) / 2, (p + q) / 2
    shift = np.where(Om < 0, pi, np.where(Om >= pi, -pi, 0))
    Om, om = Om + shift, om + shift - pi
    om = np.where(om <= -pi, om + 2 * pi, om)
    om = np.where(om <= -pi, om + 2 * pi, om)
    om = np.where(om > pi, om - 2 * pi, om)
    return a, incl, om, Om


def thiele_innes(a_angular, incl, omega, Omega, dtype=np.float64):
    """the package's rotation (_rotate_vector) of the orbital plane with the amplitude -a_angular, written out: (TA, TB, TF, TG)
    such that X = TA xi + TF eta, Y = TB xi + TG eta"""
    a, i, w, O = (np.asarray(v, dtype=dtype) for v in (a_angular, incl, omega, Omega))
    cw, sw, ci, cO, sO = np.cos(w), np.sin(w), np.cos(i), np.cos(O), np.sin(O)
    return np.stack([-a * (cO * cw - sO * ci * sw), -a * (sO * cw + cO * ci * sw),
                     -a * (-cO * sw - sO * ci * cw), -a * (-sO * sw + cO * ci * cw)], -1)


def positions(t, period, ecc, t_periastron, beta, dtype=np.float64):
    """(X, Y) of the model at the epochs t"""
    t = np.asarray(t, dtype=dtype)
    xi, eta = orbit_plane(2 * _pi(dtype) * (t - dtype(t_periastron)) / dtype(period), dtype(ecc), dtype)
    beta = np.asarray(beta, dtype=dtype)
    return beta[0] * xi + beta[2] * eta, beta[1] * xi + beta[3] * eta


def sky_model(t, period, ecc, t_periastron, a_angular, incl, omega, Omega, dtype=np.float64):
    """-> rho, theta of a companion with these elements"""
    X, Y = positions(t, period, ecc, t_periastron, thiele_innes(a_angular, incl, omega, Omega, dtype), dtype)
    return np.hypot(X, Y), np.arctan2(Y, X)


def _grid(ecc, n_phase, dtype):
    ej = np.repeat(ecc, n_phase).astype(dtype)                                 # candidate j * n_phase + k
    kk = np.tile(np.arange(n_phase), ecc.size)
    return ej, kk.astype(dtype) / dtype(n_phase), (ej != 0) | (kk == 0)


_plane_cache = {}


def _planes(tt, freq, ecc, n_phase, dtype):
    """xi, eta (candidates, epochs) of every frequency: they depend on the epochs and the grids alone; the last two sets are kept"""
    key = (tt.tobytes(), freq.tobytes(), ecc.tobytes(), n_phase, np.dtype(dtype).name)
    if key not in _plane_cache:
        while len(_plane_cache) >= 2:
            _plane_cache.pop(next(iter(_plane_cache)))
        ej, phik, _ = _grid(ecc, n_phase, dtype)
        two_pi = 2 * _pi(dtype)
        _plane_cache[key] = [orbit_plane(two_pi * (phase_turns(f, tt, dtype)[None, :] - phik[:, None]), ej[:, None], dtype) for f in freq]
    return _plane_cache[key]


def astrometric(t, rho, rho_err, theta, theta_err, freq, ecc, n_phase, dtype=np.float64):
    """-> dict: power (F,), candidate (F,) (-1: none), beta (F, 4), table (F, n_ecc * n_phase) with -inf where there is no
    candidate, pivot (F, C): every candidate's smallest squared pivot (NaN where the grid has none), gap (F,): best minus
    second best over the largest power, chi2_0, chi2; and the derived ecc, t_periastron, a_angular, incl, omega, Omega"""
    t = np.asarray(t, dtype=np.float64)
    col = columns(rho, rho_err, theta, theta_err, dtype)
    freq, ecc = np.atleast_1d(np.asarray(freq, dtype=np.float64)), np.atleast_1d(np.asarray(ecc, dtype=np.float64))
    t_min = t.min()
    tt = t - t_min
    _, _, grid_live = _grid(ecc, n_phase, dtype)
    C, F = grid_live.size, freq.size
    out = dict(power=np.zeros(F, dtype), candidate=np.full(F, -1, np.int64), beta=np.full((F, 4), np.nan, dtype),
               table=np.empty((F, C), dtype), pivot=np.empty((F, C), dtype), gap=np.empty(F), chi2_0=col["chi2_0"])
    P = (col["pxx"], col["pxy"], col["pyy"])
    idx = {(0, 0): 0, (0, 1): 1, (1, 0): 1, (1, 1): 2}
    for i, (xi, eta) in enumerate(_planes(tt, freq, ecc, n_phase, dtype)):
        basis = (xi, eta)
        Nm, b = np.empty((C, 4, 4), dtype), np.empty((C, 4), dtype)
        for g in range(2):                                                     # (rows and columns: TA, TB, TF, TG)
            for r in range(2):
                b[:, 2 * g + r] = (basis[g] * (col["qx"], col["qy"])[r]).sum(1)
                for h in range(2):
                    for s in range(2):
                        Nm[:, 2 * g + r, 2 * h + s] = (basis[g] * basis[h] * P[idx[r, s]]).sum(1)
        power, beta, pivot, live = scaled_cholesky(Nm, b)
        live = live & grid_live
        power = np.where(live, power, -np.inf)
        out["table"][i], out["pivot"][i] = power, np.where(grid_live, pivot, np.nan)
        out["gap"][i] = np.inf
        if live.any():
            c = int(np.argmax(power))                                          # the first of equal maxima
            out["candidate"][i], out["power"][i], out["beta"][i] = c, power[c], beta[c]
            rest = np.delete(power, c)
            if rest.size and np.isfinite(rest.max()):
                out["gap"][i] = float(power[c] - rest.max())
    peak = float(out["power"].max())
    out["gap"] = out["gap"] / peak if peak > 0 else out["gap"]
    found = out["candidate"] >= 0
    c = np.maximum(out["candidate"], 0)
    a, incl, om, Om = campbell(out["beta"], dtype)
    out.update(ecc=np.where(found, ecc[c // n_phase], np.nan), t_periastron=np.where(found, t_min + ((c % n_phase) / n_phase) / freq, np.nan),
               a_angular=a, incl=incl, omega=om, Omega=Om, chi2=np.where(found, out["chi2_0"] - 2 * out["power"], np.nan))
    return out


def isotropic(t, x, y, w, freq, ecc, n_phase, dtype=np.float64):
    """the same search when P = w I: the fit falls apart into two independent 2 x 2 fits, (TA, TF) of x and (TB, TG) of y, with
    one matrix [[sum w xi^2, sum w xi eta], [., sum w eta^2]]; scaled to a unit diagonal its one pivot is 1 - r^2.  -> power
    (F,), candidate (F,)"""
    t = np.asarray(t, dtype=np.float64)
    x, y, w = (np.asarray(v, dtype=dtype) for v in (x, y, w))
    freq, ecc = np.atleast_1d(np.asarray(freq, dtype=np.float64)), np.atleast_1d(np.asarray(ecc, dtype=np.float64))
    _, _, grid_live = _grid(ecc, n_phase, dtype)
    power, cand = np.zeros(freq.size, dtype), np.full(freq.size, -1, np.int64)
    for i, (xi, eta) in enumerate(_planes(t - t.min(), freq, ecc, n_phase, dtype)):
        sxx, sxe, see = (w * xi * xi).sum(1), (w * xi * eta).sum(1), (w * eta * eta).sum(1)
        with np.errstate(all="ignore"):
            dx, de = np.sqrt(sxx), np.sqrt(see)
            r = sxe / (dx * de)
            piv = 1 - r * r
            p = np.zeros_like(piv)
            for v in (x, y):
                z0 = (w * xi * v).sum(1) / dx
                z1 = ((w * eta * v).sum(1) / de - r * z0) / np.sqrt(piv)
                p = p + 0.5 * (z0 * z0 + z1 * z1)
        p = np.where(grid_live & (sxx > 0) & (see > 0) & (piv >= PIVOT_FLOOR), p, -np.inf)
        if np.isfinite(p.max()):
            cand[i], power[i] = int(np.argmax(p)), p.max()
    return power, cand


def chi2_of(col, X, Y):
    """the chi-square of the positions (X, Y) under the epochs' precision matrices, in longdouble"""
    ld = np.longdouble
    dx, dy = np.asarray(col["x"], ld) - np.asarray(X, ld), np.asarray(col["y"], ld) - np.asarray(Y, ld)
    return float((col["pxx"] * dx * dx + 2 * col["pxy"] * dx * dy + col["pyy"] * dy * dy).sum())


def rel_diff(a, b, scale):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / scale))


def tolerance(f64, ld, scale):
    """the rule of DESIGN.md 9.5: 16 x (float64 statement against longdouble statement, relative to `scale`), floor 1e-13"""
    return max(16 * rel_diff(f64, ld, scale), 1e-13)


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------

MAIN = dict(period=27.0, ecc=0.6, t_periastron=3.0, a_angular=0.8, incl=1.0, Omega=2.2, omega=0.7, n_phase=32)
TILE = 256              # epochs staged in LDS at a time (csrc/exo_astrometric.hip, kTile)


def series(n, seed, span=40.0, period=27.0, ecc=0.6, rho_err=(0.005, 0.02), theta_err=(0.005, 0.03)):
    """n epochs over `span` days of the main input's orbit with that period and eccentricity, noise drawn from the error bars"""
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, span, n))
    re, te = rs.uniform(*rho_err, n), rs.uniform(*theta_err, n)
    rho, theta = sky_model(t, period, ecc, MAIN["t_periastron"], MAIN["a_angular"], MAIN["incl"], MAIN["omega"], MAIN["Omega"])
    return dict(t=t, rho=rho + re * rs.randn(n), theta=theta + te * rs.randn(n), rho_err=re, theta_err=te)


def main_input():
    """the main input of DESIGN.md 23.4: 30 epochs over 40 days, an e = 0.6 orbit of 27 days, 40 periods from 10 to 120 days
    (log-spaced, descending: the frequencies ascend), 10 x 32 candidates (289 of them in the grid: more than one pass of a
    256-lane workgroup)"""
    d = series(30, 7)
    d.update(f=1 / np.geomspace(120.0, 10.0, 40), ecc=np.linspace(0, 0.9, 10), n_phase=MAIN["n_phase"])
    return d


F8 = 1 / np.geomspace(90.0, 12.0, 8)


def shapes():
    """the smallest shapes at which the kernel can still go wrong: name -> (series, f, ecc, n_phase)"""
    iso = series(40, 19)
    iso["theta_err"] = iso["rho_err"] / iso["rho"]
    out = {
        "one tile exactly": (series(TILE, 11), F8, [0.0, 0.45, 0.8], 8),
        "one tile and one epoch": (series(TILE + 1, 12), F8, [0.0, 0.45, 0.8], 8),
        "three epochs": (series(3, 13), F8, [0.0, 0.5], 4),
        "two epochs": (series(2, 14), F8, [0.0, 0.5], 4),
        "one epoch": (series(1, 15), F8, [0.0, 0.5], 4),
        "one candidate": (series(40, 16), F8, [0.0], 64),
        "one phase": (series(40, 16), F8, [0.0, 0.3, 0.6], 1),
        "a candidate per lane": (series(40, 16), F8, [0.15, 0.35, 0.55, 0.75], 64),
        "two candidates per lane": (series(40, 16), F8, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], 64),
        "one frequency": (series(40, 16), F8[3:4], [0.0, 0.45, 0.8], 16),
        "scalar errors": (dict(series(40, 17), rho_err=0.01, theta_err=0.02), F8, [0.0, 0.45, 0.8], 16),
        "isotropic weights": (iso, F8, [0.0, 0.45, 0.8], 16),
        # (what the search shared with the Keplerian one owns, csrc/exo_orbit_search.hpp: 128 lanes of which 63 have no
        # candidate; 64 lanes and three passes; three tiles with a short last one)
        "65 candidates": (series(40, 16), F8, [0.15, 0.3, 0.45, 0.6, 0.75], 13),
        "192 candidates": (series(40, 16), F8, [0.2, 0.5, 0.8], 64),
        "three tiles": (series(2 * TILE + 5, 18), F8, [0.0, 0.45, 0.8], 8),
    }
    return out


EXACT_FIT_ONLY = ("two epochs",)      # four equations, four unknowns: every well-conditioned candidate fits exactly, all tie


def statement(s, f, ecc, n_phase, dtype=np.float64):
    return astrometric(s["t"], s["rho"], s["rho_err"], s["theta"], s["theta_err"], f, ecc, n_phase, dtype=dtype)


_cache = {}


def cached(key, make):
    """a statement computed once per process and shared by the tests that need it (they do not modify it)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def statements(key, s, f, ecc, n_phase):
    """the float64 and the longdouble statement of one input, each computed once"""
    return (cached((key, "f64"), lambda: statement(s, f, ecc, n_phase)),
            cached((key, "ld"), lambda: statement(s, f, ecc, n_phase, dtype=np.longdouble)))
