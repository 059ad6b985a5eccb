"""The Keplerian periodogram of DESIGN.md section 22 stated in numpy, in float64 or longdouble: what
exoplanet_amd.estimators.keplerian_power is held to.  Nothing of the package is used: Kepler's equation is solved here by
Newton's iteration to convergence, and the model that makes the test series is written out here as well."""
import numpy as np


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
    """E - e sin E = M for M of any size, 0 <= e < 1: Newton from E = pi on the folded |M| <= pi (the residual is convex on
    [0, pi], so the iteration descends monotonically), until no element moves by more than a few roundings.  In longdouble
    the iteration starts from the converged float64 solution (longdouble sines are slow; two steps from there)"""
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


def true_anomaly(M, e, dtype):
    """-> cos nu, sin nu by the half-angle forms: X = sqrt(1 - e) cos E/2, Y = sqrt(1 + e) sin E/2"""
    e = np.asarray(e, dtype=dtype)
    E = solve_kepler(M, e, dtype)
    X, Y = np.sqrt(1 - e) * np.cos(E / 2), np.sqrt(1 + e) * np.sin(E / 2)
    den = X * X + Y * Y
    return (X * X - Y * Y) / den, 2 * X * Y / den


def centred_fit(YS, YC, SS, CC, CS, W):
    """power and (A, B) of [[SS, CS], [CS, CC]] (B, A) = (YS, YC) by rotation; a direction with no variance gives nothing"""
    d = CC - SS
    h = np.hypot(d, 2 * CS)
    ok = h > 0
    hs = np.where(ok, h, 1)
    c2t, s2t = np.where(ok, d / hs, 1), np.where(ok, 2 * CS / hs, 0)
    pos = c2t >= 0
    ct_p = np.sqrt(0.5 * (1 + np.where(pos, c2t, 1)))
    st_n = np.where(s2t >= 0, 1, -1) * np.sqrt(0.5 * (1 - np.where(pos, -1, c2t)))
    ct = np.where(pos, ct_p, 0.5 * s2t / np.where(pos, 1, st_n))
    st = np.where(pos, 0.5 * s2t / ct_p, st_n)
    yc, ys = YC * ct + YS * st, YS * ct - YC * st
    cc = CC * ct * ct + 2 * CS * ct * st + SS * st * st
    ss = SS * ct * ct - 2 * CS * ct * st + CC * st * st
    tiny = 1e-14 * W
    okc, oks = cc > tiny, ss > tiny
    ac = np.where(okc, yc / np.where(okc, cc, 1), 0)
    as_ = np.where(oks, ys / np.where(oks, ss, 1), 0)
    power = 0.5 * (np.where(okc, yc * ac, 0) + np.where(oks, ys * as_, 0))
    return power, ac * ct - as_ * st, ac * st + as_ * ct


def weights(y, yerr, dtype):
    y = np.asarray(y, dtype=dtype)
    w = np.ones_like(y) if yerr is None else 1 / np.broadcast_to(np.asarray(yerr, dtype=dtype), y.shape) ** 2
    return y, w


def keplerian(t, y, yerr, inst, freq, ecc, n_phase, dtype=np.float64):
    """-> dict: power (F,), candidate (F,), A, B (F,), const (F, n_inst), table (F, n_ecc * n_phase) with -inf where there
    is no candidate, gap (F,): best minus second best over the largest power, chi2_0; and the derived ecc, omega, t_periastron,
    K, zero_point"""
    t = np.asarray(t, dtype=np.float64)
    y, w = weights(y, yerr, dtype)
    inst = np.zeros(t.size, dtype=np.int64) if inst is None else np.asarray(inst, dtype=np.int64)
    n_inst = int(inst.max()) + 1
    freq, ecc = np.asarray(freq, dtype=np.float64), np.asarray(ecc, dtype=np.float64)
    t_min = t.min()
    tt = t - t_min
    masks = [inst == k for k in range(n_inst)]
    Wk = np.array([w[m].sum() for m in masks], dtype=dtype)
    Yk = np.array([(w * y)[m].sum() for m in masks], dtype=dtype)
    chi2_0 = sum((w * y * y)[m].sum() - Yk[k] ** 2 / Wk[k] for k, m in enumerate(masks))
    ej = np.repeat(ecc, n_phase).astype(dtype)                                 # candidate j * n_phase + k
    phik = np.tile(np.arange(n_phase, dtype=dtype) / dtype(n_phase), ecc.size)
    live = (ej != 0) | (np.tile(np.arange(n_phase), ecc.size) == 0)
    C, F = ej.size, freq.size
    out = dict(power=np.empty(F, dtype), candidate=np.empty(F, np.int64), A=np.empty(F, dtype), B=np.empty(F, dtype),
               const=np.empty((F, n_inst), dtype), table=np.empty((F, C), dtype), gap=np.empty(F), chi2_0=chi2_0)
    anomalies = _anomalies(tt, freq, ecc, n_phase, ej, phik, dtype)
    for i, f in enumerate(freq):
        cosn, sinn = anomalies[i]
        YS, YC = (w * y * sinn).sum(1), (w * y * cosn).sum(1)
        SS, CC, CS = (w * sinn * sinn).sum(1), (w * cosn * cosn).sum(1), (w * cosn * sinn).sum(1)
        sk = np.stack([(w * sinn)[:, mk].sum(1) for mk in masks], 1)
        ck = np.stack([(w * cosn)[:, mk].sum(1) for mk in masks], 1)
        YS, YC = YS - (Yk / Wk * sk).sum(1), YC - (Yk / Wk * ck).sum(1)
        SS, CC, CS = SS - (sk * sk / Wk).sum(1), CC - (ck * ck / Wk).sum(1), CS - (ck * sk / Wk).sum(1)
        power, A, B = centred_fit(YS, YC, SS, CC, CS, Wk.sum())
        power = np.where(live, power, -np.inf)
        c = int(np.argmax(power))                                              # the first of equal maxima
        out["table"][i], out["candidate"][i], out["power"][i], out["A"][i], out["B"][i] = power, c, power[c], A[c], B[c]
        out["const"][i] = (Yk - A[c] * ck[c] - B[c] * sk[c]) / Wk
        rest = np.delete(power, c)
        out["gap"][i] = float(power[c] - rest.max()) if rest.size and np.isfinite(rest.max()) else np.inf
    out["gap"] = out["gap"] / float(out["power"].max())
    j, k = out["candidate"] // n_phase, out["candidate"] % n_phase
    out.update(ecc=ecc[j], K=np.hypot(out["A"], out["B"]), omega=np.arctan2(-out["B"], out["A"]),
               t_periastron=t_min + (k / n_phase) / freq, zero_point=out["const"] - (ecc[j] * out["A"])[:, None])
    return out


_anomaly_cache = {}


def _anomalies(tt, freq, ecc, n_phase, ej, phik, dtype):
    """cos nu, sin nu (candidates, epochs) of every frequency.  They depend on the epochs and the grids alone, not on y or yerr:
    the last two sets are kept, so that statements on one time axis (the main input with and without yerr) solve Kepler's
    equation once"""
    key = (tt.tobytes(), freq.tobytes(), ecc.tobytes(), n_phase, np.dtype(dtype).name)
    if key not in _anomaly_cache:
        while len(_anomaly_cache) >= 2:
            _anomaly_cache.pop(next(iter(_anomaly_cache)))
        two_pi = 2 * _pi(dtype)
        _anomaly_cache[key] = [true_anomaly(two_pi * (phase_turns(f, tt, dtype)[None, :] - phik[:, None]), ej[:, None], dtype)
                               for f in freq]
    return _anomaly_cache[key]


def rv_model(t, period, ecc, omega, K, t_periastron, zero_point, inst, dtype=np.float64):
    """zero_point[inst] + K (cos w (cos nu + e) - sin w sin nu): the package's convention, written out"""
    t = np.asarray(t, dtype=dtype)
    cosn, sinn = true_anomaly(2 * _pi(dtype) * (t - dtype(t_periastron)) / dtype(period), dtype(ecc), dtype)
    zp = np.atleast_1d(np.asarray(zero_point, dtype=dtype))[np.zeros(t.size, dtype=np.int64) if inst is None else inst]
    return zp + dtype(K) * (np.cos(dtype(omega)) * (cosn + dtype(ecc)) - np.sin(dtype(omega)) * sinn)


def chi2(t, y, yerr, model):
    y, w = weights(y, yerr, np.longdouble)
    return float((w * (y - np.asarray(model, dtype=np.longdouble)) ** 2).sum())


def rel_diff(a, b, scale):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / scale))


def tolerance(f64, ld, scale):
    """the rule of DESIGN.md 9.5: 16 x (float64 statement against longdouble statement, relative to `scale`), floor 1e-13"""
    return max(16 * rel_diff(f64, ld, scale), 1e-13)


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------

MAIN = dict(period=17.3, ecc=0.6, omega=1.1, K=30.0, zero_point=(5.0, -12.0), n_phase=32)


def main_input():
    """the main input of DESIGN.md 22.4: 40 epochs over 200 days on two instruments, an e = 0.6 planet, 197 frequencies,
    10 x 32 candidates (289 of them live: more than one pass of a 256-lane workgroup)"""
    rs = np.random.RandomState(5)
    N = 40
    t = np.sort(rs.uniform(0, 200, N))
    tp = t.min() + 0.37 * MAIN["period"]
    inst = (rs.rand(N) < 0.4).astype(np.int64)
    err = rs.uniform(1, 3, N)
    model = rv_model(t, MAIN["period"], MAIN["ecc"], MAIN["omega"], MAIN["K"], tp, MAIN["zero_point"], inst)
    y = model + err * rs.randn(N)
    T = t.max() - t.min()
    f = np.arange(0.5 / (5 * T), 0.2, 1 / (5 * T))
    return dict(t=t, y=y, err=err, inst=inst, f=f, ecc=np.linspace(0, 0.9, 10), n_phase=MAIN["n_phase"], tp=tp, T=T)


_cache = {}


def cached(key, make):
    """a statement computed once per process and shared by the tests that need it (they do not modify it)"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]
