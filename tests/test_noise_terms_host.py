"""CPU: the data-side terms of the white-noise likelihood with a sampled mean and jitter -- exoplanet_amd/csrc/exo_noise_core.hpp
compiled for the host (tests/noise_harness.cpp: the kernels' arithmetic and order of summation) against a numpy longdouble
evaluation of the definitions (include/exoplanet_amd.h, exo_white_noise_terms_f64), and the host-side argument checks of the new
entry points.  The kernels themselves: tests/test_gpu_noise.py.

Tolerance: 16 x (float64 numpy against longdouble numpy on the same input), floor 1e-13, relative to the sum of
the absolute terms of each quantity."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.c_int64
LD = np.longdouble


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "noise_harness.so")
    srcs = [os.path.join(ROOT, "tests", "noise_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_noise_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_terms.argtypes = [_dp, _dp, _i64, _i64, _dp, _i64, _dp, _i64, _i64, ctypes.c_int, _dp]
    lib.harness_sum_log.restype = ctypes.c_double
    lib.harness_sum_log.argtypes = [_dp, _i64, ctypes.c_int]
    return lib


def _p(a):
    return a.ctypes.data_as(_dp)


def definitions(y, var, mean, jit2, dtype):
    """(terms (5, D), sums of absolute terms (5, D)) straight from the definitions, in `dtype`"""
    y, var, mean, jit2 = (np.asarray(a, dtype=dtype) for a in (y, var, mean, jit2))
    x = var[None, :] + jit2[:, None]
    w = 1 / x
    r = y[None, :] - mean[:, None]
    lg = np.log(x)
    terms = [w * r * r, lg, w * r, w * w * r * r, w]
    return np.stack([a.sum(1) for a in terms]), np.stack([np.abs(a).sum(1) for a in terms])


def series(n, seed):
    rs = np.random.RandomState(seed)
    y = 1.0 + 1e-4 * rs.randn(n)
    y[n // 3: n // 3 + max(n // 20, 1)] -= 5e-3          # a transit
    var = 10.0 ** rs.uniform(-12, 6, n)                  # eighteen decades inside one series
    return y, var


def cases(n, D, seed):
    """(label, var, mean, jit2 | None) over the three regimes"""
    y, var = series(n, seed)
    rs = np.random.RandomState(seed + 1)
    ybar = float(np.mean(y))
    ybar_w = float(np.sum(y / var) / np.sum(1 / var))
    per_draw_mean = np.array([(ybar, ybar + 1e-4, ybar + 0.5, ybar_w, ybar_w - 1e-4)[d % 5] for d in range(D)])
    means = [("equal", np.array([ybar])), ("equal-weighted", np.array([ybar_w])), ("near", np.array([ybar + 1e-4])),
             ("far", np.array([ybar + 0.5])), ("per-draw", per_draw_mean)]
    jits = [("none", None), ("zero", np.array([0.0])), ("1e-8", np.array([1e-8])),
            ("per-draw", (2e-4 * rs.uniform(0.5, 1.5, D)) ** 2)]
    for vl, v in (("one-var", np.array([2.5e-7])), ("per-cadence", var)):
        for ml, m in means:
            for jl, j in jits:
                yield f"{vl}/{ml}/{jl}", y, v, m, j


@pytest.mark.parametrize("n", [1, 63, 65, 2049, 6001])
@pytest.mark.parametrize("D", [1, 5, 9])
def test_terms_match_the_longdouble_definitions(harness, n, D):
    worst = {}
    for lanes in (1, 64):      # one lane: 2049 and 6001 cross a renormalisation of the mantissa product; 64: a tile edge
        for label, y, v, m, j in cases(n, D, 100 * n + D):
            got = np.empty((5, D))
            regime = harness.harness_terms(_p(y), _p(v), n, v.size, _p(m), m.size, _p(j) if j is not None else None,
                                           0 if j is None else j.size, D, lanes, _p(got))
            assert regime == (0 if (j is None or v.size == 1) else 1) or n == 0
            vv = np.broadcast_to(v, (n,))
            mm = np.broadcast_to(m, (D,))
            jj = np.zeros(D) if j is None else np.broadcast_to(j, (D,))
            want, scale = definitions(y, vv, mm, jj, LD)
            f64, _ = definitions(y, vv, mm, jj, np.float64)
            # (one cadence with the mean on it: every term of Q, G, H is zero, and zero is what must come out)
            rel = lambda d: np.where(scale > 0, d / np.where(scale > 0, scale, 1), np.where(d == 0, 0.0, np.inf))
            tol = np.maximum(16 * rel(np.abs(f64 - want)), 1e-13)
            err = rel(np.abs(got - want))
            for q, name in enumerate("Q Lam G H A".split()):
                key = (name, regime)
                worst[key] = max(worst.get(key, 0.0), float(err[q].max()))
            assert np.all(err <= tol), (label, lanes, (err / tol).max(1), err.max(1))
    print(f"n = {n}, D = {D}: worst error relative to the sum of absolute terms:",
          {f"{k[0]}[regime {k[1]}]": f"{v:.1e}" for k, v in sorted(worst.items())})


def test_product_of_mantissas_is_no_worse_than_the_sum_of_logarithms(harness):
    """the choice of exo_noise_core.hpp (LogProd): both forms against longdouble, on variances of eighteen decades and on the
    narrow range of a real series (yerr^2 + jitter^2 ~ 1e-7)"""
    rs = np.random.RandomState(7)
    rows = []
    for label, x in (("1e-12..1e6", 10.0 ** rs.uniform(-12, 6, 6001)), ("~1e-7", 2.5e-7 * rs.uniform(0.5, 1.5, 6001) + 4e-8),
                     ("~1e-7, N = 150000", 2.5e-7 * rs.uniform(0.5, 1.5, 150000) + 4e-8)):
        want = np.log(x.astype(LD)).sum()
        scale = np.abs(np.log(x.astype(LD))).sum()
        e_log = abs(harness.harness_sum_log(_p(x), x.size, 0) - want) / scale
        e_prod = abs(harness.harness_sum_log(_p(x), x.size, 1) - want) / scale
        rows.append((label, float(e_log), float(e_prod)))
    print("sum of log x, error relative to sum |log x| (plain logs, mantissa product):", rows)
    for label, e_log, e_prod in rows:
        assert e_prod <= max(e_log, 1e-16), (label, e_log, e_prod)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    return _lib.load()


def test_new_entry_points_check_their_arguments_on_the_host(lib):
    from exoplanet_amd import ops

    INVALID = 1
    # exo_white_noise_terms_f64(y, var, n_cad, n_var, mean, n_mean, jit2, n_jit, n_draw, series, series_ready, terms, ws, bytes, stream)
    ok = [8, 8, 100, 100, 8, 4, 8, 4, 4, 8, 0, 8, 8, 1 << 30, None]

    def terms(**kw):
        names = "y var n_cad n_var mean n_mean jit2 n_jit n_draw series series_ready terms ws bytes stream".split()
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.exo_white_noise_terms_f64(*a)

    for bad in (dict(y=None), dict(var=None), dict(mean=None), dict(jit2=None), dict(terms=None), dict(n_var=7), dict(n_var=0),
                dict(n_mean=3), dict(n_mean=0), dict(n_jit=2), dict(n_jit=-1), dict(n_cad=-1, n_var=1), dict(n_draw=-1),
                dict(series=None, n_jit=0)):
        assert terms(**bad) == INVALID, bad
    assert terms(n_draw=0, n_mean=1, n_jit=0) == 0
    assert terms(n_draw=0, n_mean=0, n_jit=0, y=None, var=None, mean=None, terms=None) == 0
    assert terms(ws=None) == 3 and terms(bytes=8) == 3                       # per-cadence variances + jitter: the workspace
    assert lib.exo_white_noise_workspace_bytes(150000, 1024) > 0
    assert lib.exo_white_noise_workspace_bytes(-1, 1) == -1

    # the sweeps: (..., flags, y, var, n_var, mean, n_mean, jit2, n_jit, chi2, gmean, gjit2, gparams, gld, workspace, bytes, stream)
    head = [8, 10, None, 0, None, None, 1, 8, 8, 2, 1]
    data = [8, 8, 10, 8, 2, 8, 2, 8, 8, 8, 8, 8, 8, 1 << 30, None]
    names = "y var n_var mean n_mean jit2 n_jit chi2 gmean gjit2 gparams gld ws bytes stream".split()

    def sweep(flags=0, head=head, ttv=None, gshift=8, **kw):
        a = list(data)
        for k, v in kw.items():
            a[names.index(k)] = v
        if ttv is None:
            return lib.exo_transit_noise_vjp_f64(*head, flags, *a)
        return lib.exo_transit_noise_ttv_vjp_f64(*head, flags, *ttv, *a[:12], gshift, *a[12:])

    tables = (8, 8, 3)
    for ttv in (None, tables):
        for bad in (dict(y=None), dict(var=None), dict(mean=None), dict(jit2=None), dict(chi2=None), dict(gmean=None),
                    dict(gjit2=None), dict(gparams=None), dict(gld=None), dict(n_var=5), dict(n_var=0), dict(n_mean=3),
                    dict(n_mean=0), dict(n_jit=3), dict(n_jit=-1)):
            assert sweep(ttv=ttv, **bad) == INVALID, (ttv, bad)
        # the flags the chi2 entries refuse
        for flag in (ops.FLAG_PER_PLANET, ops.FLAG_SPARSE, ops.FLAG_EXACT_SCAN):
            assert sweep(flags=flag, ttv=ttv) == INVALID
            assert (lib.exo_transit_chi2_vjp_f64(*head, flag, 8, 8, 1, 8, 8, 8, 8, 1 << 30, None) == INVALID)
        none = [8, 10, None, 0, None, None, 1, 8, 8, 0, 1]
        assert sweep(head=none, ttv=ttv, n_mean=1, n_jit=0) == 0              # no draws: nothing to do
        assert sweep(ttv=ttv, ws=None) == 3
    for flag in (ops.FLAG_SECONDARY, ops.FLAG_LIGHT_DELAY):
        assert sweep(flags=flag, ttv=tables) == INVALID
    assert sweep(ttv=(None, 8, 3)) == INVALID and sweep(ttv=(8, 8, 0)) == INVALID and sweep(ttv=tables, gshift=None) == INVALID
    empty = [8, 0, None, 0, None, None, 1, 8, 8, 2, 1]
    assert sweep(head=empty, ttv=tables, n_var=1) == INVALID                  # timing tables need a series
