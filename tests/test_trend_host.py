"""CPU: the local-polynomial trend of exoplanet_amd/csrc/exo_detrend_core.hpp (window_trend) compiled for the host
(tests/trend_harness.cpp) against the numpy restatement of DESIGN.md section 21 (tests/trend_oracle.py), window by window;
its exactness on polynomials; what it buys on a light curve with ramps (asserted on the oracle); the argument checks of the
C entry point and of the Python functions.  The kernel itself: tests/test_gpu_trend.py."""
import ctypes
import functools
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flatten_oracle as F  # noqa: E402
import trend_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_f64, _i64, _int = ctypes.c_double, ctypes.c_int64, ctypes.c_int


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "trend_harness.so")
    srcs = [os.path.join(ROOT, "tests", "trend_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_detrend_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.trend_harness_excluded.restype = _f64
    lib.trend_harness_window.restype = _f64
    lib.trend_harness_window.argtypes = [_dp, _dp, _int, _f64, _int, _f64, _int, _int, _dp]
    lib.trend_harness_running.argtypes = [_dp, _dp, ctypes.c_void_p, _ip, _ip, _i64, _i64, _int, _f64, _int, _int, _dp, _dp]
    return lib


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


# ---- window by window ------------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 3, 4, 9, 63, 64, 65)
SETTINGS = list(itertools.product((1, 2), (0, 1), (1, 10), (2.0, 5.0)))       # order, rescale, n_iter, cval


def windows_under_test():
    """-> name, values (NaN: excluded), times, the index of the cadence the window belongs to"""
    rs = np.random.RandomState(2121)
    for m in SIZES:
        t = np.sort(rs.uniform(0.0, 0.7, m)) + 3.0
        v = 1 + 0.02 * (t - 3.3) - 0.05 * (t - 3.3) ** 2 + 1e-3 * rs.randn(m)
        own = int(rs.randint(m))
        yield f"plain m={m}", v, t, own
        # outliers beyond cval MADs: weight 0
        w = v.copy()
        w[::5] += 0.03
        yield f"outliers m={m}", w, t, own
        # the same values with excluded cadences strewn between them (the window's ends and its own cadence among them)
        size = 2 * m + 3
        tt = np.sort(rs.uniform(0.0, 0.7, size)) + 3.0
        vv = np.full(size, np.nan)
        at = np.sort(rs.choice(size, m, replace=False))
        vv[at] = 1 + 0.02 * (tt[at] - 3.3) + 1e-3 * rs.randn(m)
        yield f"excluded m={m}", vv, tt, int(rs.randint(size))
        # runs of equal times: two distinct times (a parabola has to become a line) ...
        yield f"two times m={m}", v, 3.0 + 0.25 * (np.arange(m) >= (m + 1) // 2), own
        # ... one distinct time among the participating cadences of a window that still has an extent (a line has to become a location) ...
        one = np.concatenate([[np.nan], v, [np.nan]])
        yield f"one time m={m}", one, np.concatenate([[2.9], np.full(m, 3.0), [3.2]]), 1 + own
        # ... and no extent at all
        yield f"all times equal m={m}", v, np.full(m, 3.0), own
        # more than half the values equal: the MAD is 0
        flat = v.copy()
        flat[: m // 2 + 1] = 1.25
        yield f"mad 0 m={m}", flat, t, own
    yield "nothing left", np.full(4, np.nan), np.arange(4.0), 2


def oracle_window(v, t, own, order, rescale, n_iter, cval, dtype, pivots):
    keep = ~np.isnan(v)
    if not keep.any():
        return np.nan, np.nan
    return O.window_trend(v[keep], t[keep], t[own], t[0], t[-1], order, cval, n_iter, rescale, dtype, pivots)


def test_host_build_against_the_oracle_window_by_window(harness):
    """the rule of DESIGN.md 9.5 / 19.4: `unit` is what float64 costs the oracle itself on the case; the build under test may
    differ from the long-double oracle by 16 units (floor: 1e-13 of the values' size).  No window is left out."""
    ex = harness.trend_harness_excluded()
    assert np.isnan(ex)
    worst, count, seen = 0.0, 0, set()
    smallest = {1: np.inf, 2: np.inf}
    for name, v, t, own in windows_under_test():
        staged = np.ascontiguousarray(np.where(np.isnan(v), ex, v))
        t = np.ascontiguousarray(t, dtype=np.float64)
        size = np.nanmax(np.abs(v)) if not np.all(np.isnan(v)) else 1.0
        for order, rescale, n_iter, cval in SETTINGS:
            piv64, pivld = [], []
            f64, s64 = oracle_window(v, t, own, order, rescale, n_iter, cval, np.float64, piv64)
            want, swant = oracle_window(v, t, own, order, rescale, n_iter, cval, np.longdouble, pivld)
            # the condition on the inputs: no case sits on the stop rule, in float64 and in long double alike
            for r in piv64 + pivld:
                assert not 1e-13 <= r <= 1e-7, (name, order, rescale, n_iter, cval, r)
            for r in piv64:
                if r > 1e-7:
                    smallest[order] = min(smallest[order], r)
            sc = ctypes.c_double(-1.0)
            got = harness.trend_harness_window(_p(staged), _p(t), staged.size, float(t[own]), order, cval, n_iter, rescale, ctypes.byref(sc))
            count += 1
            if np.isnan(want):
                assert np.isnan(got) and np.isnan(sc.value) and np.isnan(f64), name
                seen.add("nan")
                continue
            unit = abs(float(f64) - float(want))
            err = abs(got - float(want))
            worst = max(worst, err / size)
            assert err <= max(16 * unit, 1e-13 * size), (name, order, rescale, n_iter, cval, got, float(f64), float(want))
            sunit = abs(float(s64) - float(swant))
            assert abs(sc.value - float(swant)) <= max(16 * sunit, 1e-13 * size), (name, order, rescale, n_iter, cval, sc.value, float(swant))
            # the rules of the definition, each met by some case
            keep = ~np.isnan(v)
            if F.mad(v[keep], F.median(v[keep])) == 0 or t[0] == t[-1]:
                assert got == F.median(v[keep]), name
                seen.add("median")
            if piv64 and min(piv64) <= 1e-10:
                seen.add("stopped on a pivot")
            if len(piv64) and len(piv64) < order * n_iter * (1 + rescale):
                seen.add("fewer pivots than a full run")
    print(f"{count} windows, worst |host build - long double| = {worst:.2e} of the values' size; smallest pivot ratio above the "
          f"floor: order 1 {smallest[1]:.1e}, order 2 {smallest[2]:.1e}")
    assert {"nan", "median", "fewer pivots than a full run"} <= seen, seen


def test_a_reduced_order_is_the_lower_order_fit(harness):
    """two distinct times: order 2 is order 1; one distinct time: both are the biweight location with the rescaling on top
    (rescale = 0: section 19's biweight exactly, as the host build of the same header gives it)"""
    from test_flatten_host import build_harness as build_location_harness

    location = build_location_harness()
    for name, v, t, own in windows_under_test():
        if not name.startswith(("two times", "one time")):
            continue
        staged = np.ascontiguousarray(np.where(np.isnan(v), harness.trend_harness_excluded(), v))
        t = np.ascontiguousarray(t)
        sc = ctypes.c_double()
        call = lambda order, rescale: harness.trend_harness_window(_p(staged), _p(t), staged.size, float(t[own]), order, 5.0, 10,  # noqa: E731
                                                                   rescale, ctypes.byref(sc))
        assert call(2, 1) == call(1, 1) and call(2, 0) == call(1, 0), name
        if name.startswith("one time"):
            vv = np.ascontiguousarray(v[~np.isnan(v)])
            med = F.median(vv)
            assert call(1, 0) == location.harness_biweight(_p(vv), vv.size, med, F.mad(vv, med), 5.0, 10), name


# ---- exactness on polynomials ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def science_windows(window_length):
    t = O.science_input()[0]
    lo, hi, _ = F.windows(t, window_length, break_tolerance=0.5)
    return lo.astype(np.int32), hi.astype(np.int32)


def host_series(harness, t, y, window_length, order, rescale=1):
    """the trend of one series through the host build (order 0: section 19's biweight through the oracle's windows)"""
    lo, hi = science_windows(window_length)
    trend = np.empty(t.size)
    y = np.ascontiguousarray(y)
    harness.trend_harness_running(_p(t), _p(y), None, _p(lo, _ip), _p(hi, _ip), 0, t.size, order, 5.0, 10, rescale, _p(trend), None)
    return trend


def test_exact_on_polynomials_up_to_the_order(harness):
    t = np.ascontiguousarray(O.science_input()[0])
    assert t.size == 3456 and np.isclose(t[1728], 13.5)
    line = 1.0 + 2.5e-3 * (t - 12.0)
    parabola = line + 4e-4 * (t - 12.0) ** 2
    floor = {"line": 1e-13 * np.abs(line).max(), "parabola": 1e-13 * np.abs(parabola).max()}
    some = np.unique(np.concatenate([np.arange(0, t.size, 96), [0, 1, 1726, 1727, 1728, 1729, t.size - 2, t.size - 1]]))
    for wl in (0.75, 1.5):
        off = {}
        for name, y in (("line", line), ("parabola", parabola)):
            zero, _ = O.running_trend(t, y, wl, 0, break_tolerance=0.5, cadences=some)
            off[name, 0] = np.abs(zero - y)[some].max()
            for order in (1, 2):
                for rescale in (0, 1):
                    got = host_series(harness, t, y, wl, order, rescale)
                    off[name, order] = max(off.get((name, order), 0.0), np.abs(got - y).max())
                want, _ = O.running_trend(t, y, wl, order, break_tolerance=0.5, cadences=some)
                off[name, order] = max(off[name, order], np.abs(want - y)[some].max())
        print(f"window {wl}: " + ", ".join(f"{name} order {order}: {e:.1e}" for (name, order), e in sorted(off.items())))
        assert off["line", 1] <= floor["line"] and off["line", 2] <= floor["line"]
        assert off["line", 0] > 1e-4                       # the location's edge bias: slope * window / 4
        assert off["parabola", 2] <= floor["parabola"]
        assert off["parabola", 1] > 1e-6 and off["parabola", 0] > 1e-4


# ---- the science -------------------------------------------------------------------------------------------------------------------

def test_the_trend_follows_ramps_and_extrema_where_the_location_cannot(harness):
    """The table of DESIGN.md 21.3, re-measured with the oracle (float64) on every fourth cadence and on every cadence within
    0.3 d of a segment's end; asserted: a line's edge rms is below a third of the location's at the same window, a parabola's
    overall rms at 1.5 d below half of the location's at 1.5 d.  The host build gives the oracle's trend on these cadences (to
    the floor of the rule above), so the figures are the header's as well."""
    t, y, truth, in_transit = O.science_input()
    ends = np.array([t[0], t[1727], t[1728], t[-1]])
    edge = np.abs(t[:, None] - ends[None, :]).min(axis=1) < 0.3
    chosen = np.flatnonzero(edge | (np.arange(t.size) % 4 == 0))
    rms, rms_edge, depth = {}, {}, {}
    for wl in (0.75, 1.5):
        for order in (0, 1, 2):
            trend, _ = O.running_trend(t, y, wl, order, break_tolerance=0.5, cadences=chosen)
            if order:
                built = host_series(harness, np.ascontiguousarray(t), y, wl, order)
                assert np.abs(built[chosen] - trend[chosen]).max() <= 1e-13 * np.abs(y).max()
            rel = trend / truth - 1
            every4 = chosen[chosen % 4 == 0]                  # (the edge cadences must not weigh more than the others)
            rms[order, wl] = np.sqrt(np.mean(rel[every4] ** 2))
            rms_edge[order, wl] = np.sqrt(np.mean(rel[edge] ** 2))
            flat = y[chosen] / trend[chosen]
            depth[order, wl] = np.mean(flat[~in_transit[chosen]]) - np.mean(flat[in_transit[chosen]])
            print(f"order {order} window {wl}: rms all {rms[order, wl]:.2e}, rms edge {rms_edge[order, wl]:.2e}, depth {depth[order, wl]:.2e}")
    for wl in (0.75, 1.5):
        print(f"window {wl}: edge rms order 1 / order 0 = {rms_edge[1, wl] / rms_edge[0, wl]:.3f}")
        assert rms_edge[1, wl] < rms_edge[0, wl] / 3
    print(f"overall rms at 1.5 d, order 2 / order 0 = {rms[2, 1.5] / rms[0, 1.5]:.3f}; order 2 at 1.5 d / order 0 at 0.75 d = "
          f"{rms[2, 1.5] / rms[0, 0.75]:.3f}")
    assert rms[2, 1.5] < rms[0, 1.5] / 2


# ---- arguments -----------------------------------------------------------------------------------------------------------------------

def test_abi_of_the_trend_entry_point():
    """every argument check happens on the host, before any launch (the pointers are never followed)"""
    import re

    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib
    from exoplanet_amd import estimators as E

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    cap = int(consts["EXO_TREND_MAX_WINDOW"])
    assert cap == E.MAX_TREND_WINDOW >= 4096 and 2 * (256 + 2 * cap - 2) * 8 <= 160 * 1024
    assert cap <= int(consts["EXO_LOCATION_MAX_WINDOW"]) == E.MAX_WINDOW
    INVALID = 1
    names = ["t", "y", "exclude", "n_exclude", "n", "n_series", "lo", "hi", "edge", "max_window", "order", "cval", "n_iter", "rescale",
             "trend", "scale", "stream"]
    ok = [8, 8, None, 0, 100, 3, 8, 8, None, 64, 2, 5.0, 10, 1, 8, None, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_running_trend_f64(*args)

    for bad in (dict(t=None), dict(y=None), dict(lo=None), dict(hi=None), dict(trend=None), dict(n=0), dict(n=-5), dict(n_series=0),
                dict(n_series=-1), dict(order=0), dict(order=3), dict(order=-1), dict(cval=0.0), dict(cval=-5.0), dict(cval=float("nan")),
                dict(n_iter=-1), dict(rescale=-1), dict(max_window=0), dict(max_window=cap + 1), dict(n_exclude=2, exclude=8),
                dict(n_exclude=-1, exclude=8), dict(n_exclude=1), dict(n_exclude=3)):
        assert call(**bad) == INVALID, bad


def test_python_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    params = inspect.signature(E.running_location).parameters
    assert params["order"].default == 0 and params["rescale"].default == 1
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("order", "rescale"))
    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    with pytest.raises(ValueError, match="order must be 0, 1 or 2"):
        E.running_location(t, t, 1.0, order=3)
    with pytest.raises(ValueError, match="order must be 0, 1 or 2"):
        E.running_location(t, t, 1.0, order=1.5)
    with pytest.raises(ValueError, match="needs method 'biweight'"):
        E.running_location(t, t, 1.0, order=1, method="median")
    with pytest.raises(ValueError, match="rescale"):
        E.running_location(t, t, 1.0, order=1, rescale=-1)
    with pytest.raises(ValueError, match="rescale"):
        E.running_location(t, t, 1.0, order=2, rescale=1.5)
    # a plan wider than the cap of the new kernel (and within the location's own)
    index = torch.zeros(50, dtype=torch.int32)
    plan = E.LocationPlan(index, index, index.bool(), E.MAX_TREND_WINDOW + 1)
    with pytest.raises(ValueError, match=rf"{E.MAX_TREND_WINDOW + 1} cadences, more than the {E.MAX_TREND_WINDOW}"):
        E.running_location(t, t, plan=plan, order=2)
    # order 0 reads none of this, and stays what it was: the next refusal is the missing device
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.running_location(t, t, 1.0, order=0, rescale=-1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.running_location(t, t, 1.0, order=1, rescale=0)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no CPU fallback"):
            E.flatten(t, t, 1.0, order=2)
