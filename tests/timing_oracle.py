"""The yardstick of the per-transit timing tests: a numpy statement of the definition in DESIGN.md section 20 (a helper module, not
a test).  Every (transit, shift) is evaluated on the whole window at once -- no bisection of the template's cadences, no lanes --
and every sum is a ``cumsum`` along the window, so that it runs in the window's cadence order.  It takes a ``dtype`` so that it
can run in ``np.longdouble``: the difference between the float64 and the longdouble statement on an input is what sets the
tests' tolerance on it.  The windows and the epochs are always decided in float64: they are integers."""
import numpy as np

import tls_oracle as T

FLOAT_FIELDS = ("transit_time", "shift", "time_err", "depth", "depth_err", "log_likelihood", "depth_snr")
INT_FIELDS = ("n_window", "n_in", "valid", "at_edge")
FLOOR, FACTOR, MAX_LEFT_OUT, NEAR_CONTACT = 1e-13, 16.0, 0.02, 1e-9


def epochs(t, period, t0, window):
    """all integers n with t0 + period n inside [t[0] - window / 2, t[-1] + window / 2] (float64)"""
    t = np.asarray(t, dtype=np.float64)
    a, b = t[0] - window / 2, t[-1] + window / 2
    n = np.arange(int(np.floor((a - t0) / period)) - 1, int(np.ceil((b - t0) / period)) + 2, dtype=np.int64)
    T_k = t0 + period * n.astype(np.float64)
    return n[(T_k >= a) & (T_k <= b)]


def windows(t, T_k, window):
    """-> lo, hi (int): the first and the last cadence with |t - T_k| <= window / 2; none: hi = lo - 1"""
    t = np.asarray(t, dtype=np.float64)
    lo = np.array([np.searchsorted(t - Tk, -window / 2, side="left") for Tk in T_k], dtype=np.int64)
    hi = np.array([np.searchsorted(t - Tk, window / 2, side="right") - 1 for Tk in T_k], dtype=np.int64)
    return lo, hi


def shifts(max_shift, n_shift, dtype=np.float64):
    h = 2 * dtype(max_shift) / (n_shift - 1)
    return -dtype(max_shift) + np.arange(n_shift).astype(dtype) * h, h


def template_value(g, x):
    """the table g (m,), samples at the centres (2 q + 1) / m - 1, as a continuous function: linear between the centres, linear
    to 0 at -1 and +1 beyond the outermost, 0 for |x| >= 1"""
    g = np.asarray(g)
    dtype = g.dtype.type
    x = np.asarray(x, dtype=dtype)
    m = len(g)
    centres = (2 * np.arange(m).astype(dtype) + 1) / m - 1
    xs = np.concatenate([[dtype(-1)], centres, [dtype(1)]])
    gs = np.concatenate([[dtype(0)], g, [dtype(0)]])
    i = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, m)
    val = gs[i] + (x - xs[i]) * (gs[i + 1] - gs[i]) / (xs[i + 1] - xs[i])
    return np.where(np.abs(x) < 1, val, dtype(0))


def _seq(a):
    """sum along the last axis in its order"""
    return np.cumsum(a, axis=-1)[..., -1] if a.shape[-1] else np.zeros(a.shape[:-1], dtype=a.dtype)


def vertex_at(L, j, shifts_, h):
    """-> j, shift, time_err, at_edge for the maximum taken at shift j of the curve L"""
    M = len(L)
    edge = j == 0 or j == M - 1 or L[j - 1] == -np.inf or L[j + 1] == -np.inf
    S = None if edge else (L[j - 1] - 2 * L[j]) + L[j + 1]
    if edge or S >= 0:
        return j, shifts_[j], L.dtype.type(np.nan), True
    return j, shifts_[j] - 0.5 * h * (L[j + 1] - L[j - 1]) / S, h / np.sqrt(-S), False


def vertex(L, shifts_, h):
    """-> j* (the lowest index of the maximum), shift, time_err, at_edge of one curve; all of it -inf: None"""
    if not np.any(L > -np.inf):
        return None
    return vertex_at(L, int(np.argmax(L)), shifts_, h)


def transit_times(t, y, yerr=None, *, period, t0, duration, max_shift=None, n_shift=201, window=None, template, depth=None,
                  min_in_transit=3, exclude=None, dtype=np.float64, at=None):
    """One series y (N,).  -> dict of (K,) arrays (FLOAT_FIELDS in ``dtype``, INT_FIELDS), ``transit_ind`` and ``linear_time``
    (K,), ``curve`` (K, M), ``shifts`` (M,), ``j_star`` (K,; -1: invalid), ``near_contact`` (K,) bool: a w > 0 cadence within 1e-9
    of |x| = 1 at j*, and ``chi2_0`` (K,).  ``at`` (K,): take these j* instead of the curve's maximum (the other precision's)."""
    max_shift = duration / 2 if max_shift is None else max_shift
    window = 3 * duration + 2 * max_shift if window is None else window
    tf = np.asarray(t, dtype=np.float64)
    n_k = epochs(tf, period, t0, window)
    T_k = t0 + period * n_k.astype(np.float64)
    lo, hi = windows(tf, T_k, window)
    K, M = len(n_k), n_shift
    y = np.asarray(y, dtype=dtype)
    w = np.ones(len(tf), dtype=dtype) if yerr is None else np.broadcast_to(1 / np.asarray(yerr, dtype=dtype) ** 2, y.shape).copy()
    if exclude is not None:
        w[np.asarray(exclude, dtype=bool)] = 0
    g = np.asarray(template, dtype=dtype)
    delta, h = shifts(max_shift, M, dtype)
    res = {k: np.full(K, np.nan, dtype=dtype) for k in FLOAT_FIELDS}
    res.update({k: np.zeros(K, dtype=np.int64) for k in INT_FIELDS})
    res.update(transit_ind=n_k, linear_time=T_k, curve=np.full((K, M), -np.inf, dtype=dtype), shifts=delta,
               j_star=np.full(K, -1, dtype=np.int64), near_contact=np.zeros(K, dtype=bool), chi2_0=np.full(K, np.nan, dtype=dtype))
    for k in range(K):
        sl = slice(lo[k], hi[k] + 1)
        res["n_window"][k] = max(hi[k] - lo[k] + 1, 0)
        wk = w[sl]
        if not np.any(wk > 0):
            continue
        tp = np.asarray(t, dtype=dtype)[sl] - dtype(T_k[k])
        W = _seq(wk)
        yp = y[sl] - _seq(wk * y[sl]) / W
        res["chi2_0"][k] = _seq(wk * yp * yp)
        x = (tp[None, :] - delta[:, None]) / (dtype(duration) / 2)
        gx = template_value(g, x)
        G, GG, GY = _seq(wk * gx), _seq(wk * gx * gx), _seq(wk * gx * yp)
        inside = (np.abs(x) < 1) & (wk > 0)
        n_in = inside.sum(1)
        with np.errstate(all="ignore"):
            D = GG - G * G / W
            ok = (n_in >= min_in_transit) & ((wk > 0).sum() - n_in >= 1) & (D > 0)
            if depth is None:
                d, derr, L = -GY / D, 1 / np.sqrt(D), GY ** 2 / (2 * D)
            else:
                d = np.full(M, dtype(depth))
                derr, L = np.full(M, dtype(np.nan)), -d * GY - d * d * D / 2
        L = np.where(ok, L, -np.inf)
        res["curve"][k] = L
        if at is not None and at[k] >= 0 and L[at[k]] > -np.inf:       # the other precision's maximum
            v = vertex_at(L, int(at[k]), delta, h)
        else:
            v = vertex(L, delta, h)
        if v is None:
            continue
        j, shift, time_err, edge = v
        res["j_star"][k], res["valid"][k], res["at_edge"][k], res["n_in"][k] = j, 1, int(edge), n_in[j]
        res["shift"][k], res["time_err"][k], res["transit_time"][k] = shift, time_err, dtype(T_k[k]) + shift
        res["depth"][k], res["depth_err"][k], res["log_likelihood"][k], res["depth_snr"][k] = d[j], derr[j], L[j], d[j] / derr[j]
        res["near_contact"][k] = bool(np.any((np.abs(np.abs(x[j]) - 1) < NEAR_CONTACT) & (wk > 0)))
    return res


def reference(t, y, yerr=None, **kw):
    """-> (the longdouble statement at the float64 statement's maxima, the float64 statement, unit (K,)): unit = the largest
    difference between the two over the curve, depth and depth_err, relative to the transit's largest finite |L|"""
    f64 = transit_times(t, y, yerr, **kw)
    ld = transit_times(t, y, yerr, dtype=np.longdouble, at=f64["j_star"], **kw)
    K = len(f64["transit_ind"])
    unit = np.zeros(K)
    for k in range(K):
        fin = np.isfinite(f64["curve"][k]) & np.isfinite(ld["curve"][k])
        if not fin.any() or not f64["valid"][k]:
            continue
        scale = float(np.abs(ld["curve"][k][fin]).max())
        diffs = [np.abs(f64["curve"][k][fin] - ld["curve"][k][fin]).max(), abs(f64["depth"][k] - ld["depth"][k])]
        if np.isfinite(ld["depth_err"][k]):
            diffs.append(abs(f64["depth_err"][k] - ld["depth_err"][k]))
        unit[k] = float(max(diffs)) / scale
    return ld, f64, unit


def check(name, got, ref):
    """``got``: host arrays of one series under FLOAT_FIELDS, INT_FIELDS, ``transit_ind`` and ``curve``; ``ref``: what
    :func:`reference` returned.  The rule of DESIGN.md 20.4: per transit, tolerance = max(16 unit, 1e-13) relative to its largest
    finite |L| -> eta (absolute) for the curve, depth and depth_err; shift gets 3 h eta / |S|, time_err 2 time_err eta / |S|;
    counts, flags and j* are exact.  A transit whose best and second-best L lie within eta, or with a w > 0 cadence within 1e-9 of
    a contact at j*, is left out (at most 2 % of the case's transits).  Prints, then asserts.  -> the printed figures"""
    ld, f64, unit = ref
    K, M = ld["curve"].shape
    assert np.array_equal(got["transit_ind"], ld["transit_ind"])
    assert np.array_equal(got["n_window"], ld["n_window"])
    assert got["curve"].shape == (K, M)
    h = float(ld["shifts"][1] - ld["shifts"][0])
    left_out, worst = 0, dict(curve=0.0, depth=0.0, depth_err=0.0, shift=0.0, time_err=0.0)
    tol_max, failures = 0.0, []
    for k in range(K):
        Lw = ld["curve"][k]
        # which shifts are admissible is a matter of integers: the float64 statement's (a cadence on a contact may fall on the
        # other side in long double; values are compared where both statements have one)
        fin = np.isfinite(f64["curve"][k])
        assert np.array_equal(np.isfinite(got["curve"][k]), fin), (name, k, "admissible shifts")
        assert np.all(got["curve"][k][~fin] == -np.inf)
        fin = fin & np.isfinite(Lw)
        if not ld["valid"][k]:
            assert not got["valid"][k] and not got["at_edge"][k] and got["n_in"][k] == 0, (name, k)
            assert all(np.isnan(got[f][k]) for f in FLOAT_FIELDS), (name, k)
            continue
        scale = float(np.abs(Lw[fin]).max())
        tol = max(FACTOR * unit[k], FLOOR)
        eta = tol * scale
        tol_max = max(tol_max, tol)
        err = float(np.abs(got["curve"][k][fin] - Lw[fin]).max())
        worst["curve"] = max(worst["curve"], err / scale)
        if err > eta:
            failures.append((k, "curve", err, eta))
        top = np.sort(np.asarray(Lw[fin], dtype=np.float64))[::-1]
        fragile = (len(top) > 1 and top[0] - top[1] <= eta) or ld["near_contact"][k] or f64["near_contact"][k]
        # the integers are the float64 statement's (its x is the kernel's, operation for operation); a fragile transit is left
        # out only where they differ
        exact = (got["valid"][k] and int(np.argmax(got["curve"][k])) == f64["j_star"][k] and got["n_in"][k] == f64["n_in"][k]
                 and bool(got["at_edge"][k]) == bool(f64["at_edge"][k]) == bool(ld["at_edge"][k]))
        if not exact:
            assert fragile, (name, k, "j*, n_in or at_edge", got["n_in"][k], f64["n_in"][k], f64["j_star"][k])
            left_out += 1
            continue
        for f in ("depth", "depth_err"):
            if np.isnan(ld[f][k]):
                assert np.isnan(got[f][k]), (name, k, f)
                continue
            e = abs(float(got[f][k]) - float(ld[f][k]))
            worst[f] = max(worst[f], e / scale)
            if e > eta:
                failures.append((k, f, e, eta))
        assert abs(got["log_likelihood"][k] - got["curve"][k][ld["j_star"][k]]) == 0
        if np.isfinite(ld["depth_err"][k]):
            assert abs(got["depth_snr"][k] - got["depth"][k] / got["depth_err"][k]) <= 4e-16 * abs(got["depth_snr"][k])
        else:
            assert np.isnan(got["depth_snr"][k])
        if ld["at_edge"][k]:
            assert got["shift"][k] == f64["shifts"][f64["j_star"][k]] and np.isnan(got["time_err"][k]), (name, k)
        else:
            j = ld["j_star"][k]
            S = abs(float((Lw[j - 1] - 2 * Lw[j]) + Lw[j + 1]))
            for f, bound in (("shift", 3 * h * eta / S), ("time_err", 2 * float(ld["time_err"][k]) * eta / S)):
                e = abs(float(got[f][k]) - float(ld[f][k]))
                worst[f] = max(worst[f], e / bound if bound > 0 else 0.0)
                if e > bound:
                    failures.append((k, f, e, bound))
        assert abs(got["transit_time"][k] - (float(ld["linear_time"][k]) + got["shift"][k])) <= 2e-16 * abs(got["transit_time"][k])
    print(f"[{name}] transits {K} (invalid {int((ld['valid'] == 0).sum())}, left out {left_out}), shifts {M}, float64 vs longdouble "
          f"statement (unit) {unit.max() if K else 0.0:.2e}, tolerance {tol_max:.2e} of max |L|; errors / max |L|: curve "
          f"{worst['curve']:.2e}, depth {worst['depth']:.2e}, depth_err {worst['depth_err']:.2e}; shift {worst['shift']:.2e} and "
          f"time_err {worst['time_err']:.2e} of their propagated bounds")
    assert left_out <= MAX_LEFT_OUT * K, (name, left_out, K)
    assert not failures, (name, failures[:5])
    return dict(unit=float(unit.max()) if K else 0.0, tolerance=tol_max, **worst)


def vertex_from_curve(curve, shifts_, valid):
    """the vertex formula applied to a returned curve (K, M) -> shift, time_err (K,): what the kernel's own record must equal"""
    K = curve.shape[0]
    h = 2 * (-shifts_[0]) / (len(shifts_) - 1)
    shift, err = np.full(K, np.nan), np.full(K, np.nan)
    for k in range(K):
        v = vertex(curve[k], shifts_, h) if valid[k] else None
        if v is not None:
            shift[k], err[k] = v[1], v[2]
    return shift, err


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------

SEARCH = dict(period=2.345, t0=1.0, duration=0.2, max_shift=0.03, n_shift=121, window=0.66)
CASES = {"2min": (2.0 / 1440, 1e-3), "10min": (10.0 / 1440, 2e-3), "30min": (30.0 / 1440, 5e-4)}


def true_shift(n):
    return 0.01 * np.sin(2 * np.pi * np.asarray(n, dtype=np.float64) / 9)


def main_input(case, offset=0.0):
    """-> t, y, sigma: cadence c over 27 d without (12.5, 14.0), noise sigma RandomState(11), and a straight-line chord transit
    (b = 0.3, ror = 0.1, duration 0.2) at the mid-times 1.0 + 2.345 n + 0.01 sin(2 pi n / 9); out of transit y is around ``offset``"""
    c, sigma = CASES[case]
    t = np.arange(0, 27, c)
    t = t[~((t > 12.5) & (t < 14.0))]
    y = sigma * np.random.RandomState(11).randn(len(t)) + offset
    b, ror = T.TRUE["b"], T.TRUE["ror"]
    n = np.round((t - 1.0) / 2.345)
    x = (t - (1.0 + 2.345 * n + true_shift(n))) / (0.5 * 0.2)
    inside = np.abs(x) < 1
    y[inside] -= T.lc_deficit(np.sqrt(b * b + ((1 + ror) ** 2 - b * b) * x[inside] ** 2), ror)
    return t, y, sigma


def science(name, res):
    """the bounds of the science test on one series' host arrays (any of the three main inputs): exactly epoch 5 (in the gap) is
    invalid, nothing sits on an end of the grid, every pull (shift - true) / time_err is below 4, their rms lies in (0.4, 2), and
    every depth is within 5 depth_err of the true one.  Prints, then asserts.  -> the printed figures"""
    n_k = np.asarray(res["transit_ind"])
    valid = np.asarray(res["valid"]).astype(bool)
    shift, err = np.asarray(res["shift"], dtype=np.float64)[valid], np.asarray(res["time_err"], dtype=np.float64)[valid]
    pull = (shift - true_shift(n_k[valid])) / err
    depth, derr = np.asarray(res["depth"], dtype=np.float64)[valid], np.asarray(res["depth_err"], dtype=np.float64)[valid]
    dev = np.abs(depth - T.true_depth()) / derr
    rep = dict(time_err=(float(err.min()), float(err.max())), depth_err=float(derr.mean()), max_pull=float(np.abs(pull).max()),
               rms_pull=float(np.sqrt((pull ** 2).mean())), max_depth_dev=float(dev.max()))
    print(f"[{name}] windows {len(n_k)}, invalid {n_k[~valid].tolist()}, at_edge {int(np.asarray(res['at_edge']).sum())}, time_err "
          f"{rep['time_err'][0]:.2e} .. {rep['time_err'][1]:.2e}, depth_err {rep['depth_err']:.2e}, largest |pull| {rep['max_pull']:.2f}, "
          f"rms pull {rep['rms_pull']:.2f}, largest depth deviation {rep['max_depth_dev']:.2f} depth_err")
    assert n_k[~valid].tolist() == [5]
    assert not np.asarray(res["at_edge"]).any()
    assert np.all(np.abs(pull) < 4) and 0.4 < rep["rms_pull"] < 2
    assert np.all(dev < 5)
    return rep


_template = {}


def main_template(m=256):
    if m not in _template:
        _template[m] = T.transit_template(m, 0.1, 0.3)
    return _template[m]
