"""CPU: the per-window arithmetic of exoplanet_amd/csrc/exo_detrend_core.hpp compiled for the host (tests/flatten_harness.cpp)
against the numpy restatement of the definition (tests/flatten_oracle.py), the argument checks of the two C entry points
and of the Python functions.  The kernels themselves: tests/test_gpu_flatten.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flatten_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_f64, _i64, _u64 = ctypes.c_double, ctypes.c_int64, ctypes.c_uint64


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "flatten_harness.so")
    srcs = [os.path.join(ROOT, "tests", "flatten_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_detrend_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_key.restype, lib.harness_key.argtypes = _u64, [_f64]
    lib.harness_unkey.restype, lib.harness_unkey.argtypes = _f64, [_u64]
    lib.harness_excluded.restype = _f64
    lib.harness_count_valid.argtypes = [_dp, ctypes.c_int]
    lib.harness_select.restype, lib.harness_select.argtypes = _f64, [_dp, ctypes.c_int, ctypes.c_int]
    lib.harness_median.restype, lib.harness_median.argtypes = _f64, [_dp, ctypes.c_int]
    lib.harness_mad.restype, lib.harness_mad.argtypes = _f64, [_dp, ctypes.c_int, _f64]
    lib.harness_biweight.restype, lib.harness_biweight.argtypes = _f64, [_dp, ctypes.c_int, _f64, _f64, _f64, ctypes.c_int]
    lib.harness_windows.argtypes = [_dp, _i64, _i64, _f64, _i64, _i64, _ip, _ip]
    lib.harness_running_location.argtypes = [_dp, ctypes.c_void_p, _ip, _ip, _i64, _i64, ctypes.c_int, _f64, ctypes.c_int, _dp, _dp]
    return lib


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def test_key_map_is_monotone_and_invertible(harness):
    tiny = np.float64(5e-324)
    xs = [-np.inf, -1e300, np.nextafter(-1e300, 0), -1.0, np.nextafter(-1.0, 0), -2.3e-308, -1e-310, -tiny, -0.0, 0.0, tiny, 1e-310,
          2.2250738585072014e-308, np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), 1e300, np.nextafter(1e300, np.inf), np.inf]
    keys = [harness.harness_key(float(x)) for x in xs]
    assert all(a < b for a, b in zip(keys, keys[1:])), keys
    assert keys[9] == keys[8] + 1                        # -0 immediately before +0
    for x, k in zip(xs, keys):
        back = harness.harness_unkey(k)
        assert back == x and np.signbit(back) == np.signbit(x)
    # adjacent doubles have adjacent keys, on both sides of zero
    rs = np.random.RandomState(5)
    for x in np.concatenate([rs.randn(50), 1e-310 * rs.randn(20), 1e300 * rs.randn(20)]):
        assert harness.harness_key(float(np.nextafter(x, np.inf))) == harness.harness_key(float(x)) + 1
    # the NaN an excluded cadence holds lies beyond +inf
    ex = harness.harness_excluded()
    assert np.isnan(ex) and harness.harness_key(ex) > harness.harness_key(np.inf)


def _windows_under_test():
    rs = np.random.RandomState(811)
    for m in list(range(1, 10)) + [63, 64, 65]:
        yield m, rs.randn(m)                                           # no ties
        yield m, np.round(3 * rs.randn(m)) / 4                         # many ties, zeros among them
        yield m, np.where(rs.rand(m) < 0.5, -0.0, 0.0) * 1.0           # nothing but zeros of both signs
        yield m, np.concatenate([[1e300, -1e300, 5e-324, -5e-324], 1e-310 * rs.randn(m)])[:m]
        yield m, np.full(m, -2.5)                                      # one value


def test_selection_median_and_mad_equal_the_oracle(harness):
    ex = harness.harness_excluded()
    rs = np.random.RandomState(3)
    for m, v in _windows_under_test():
        v = np.ascontiguousarray(v, dtype=np.float64)
        # the same values with excluded cadences strewn between them
        w = np.full(2 * m + 3, ex)
        w[np.sort(rs.choice(w.size, m, replace=False))] = v
        s = np.sort(v)
        for arr in (v, w):
            assert harness.harness_count_valid(_p(arr), arr.size) == m
            for k in range(m):
                assert harness.harness_select(_p(arr), arr.size, k) == s[k], (m, k)
            med = harness.harness_median(_p(arr), arr.size)
            assert med == O.median(v), m
            assert harness.harness_mad(_p(arr), arr.size, med) == O.mad(v, O.median(v)), m
    # nothing left in the window
    none = np.full(4, ex)
    assert harness.harness_count_valid(_p(none), 4) == 0


def biweight_cases():
    rs = np.random.RandomState(77)
    for m in (1, 2, 3, 8, 65, 300):
        v = 1 + 1e-3 * rs.randn(m)
        v[::7] += 0.03                                                  # outliers beyond cval MADs
        yield v
    yield np.round(2000 * (1 + 1e-3 * rs.randn(200))) / 2000            # ties
    yield np.full(9, 1.25)                                              # mad = 0


@pytest.mark.parametrize("cval,n_iter", [(5.0, 10), (5.0, 1), (5.0, 40), (2.0, 10), (5.0, 0)])
def test_biweight_within_the_rounding_of_the_oracle(harness, cval, n_iter):
    """the rule of DESIGN.md 9.5: `unit` is what float64 costs the oracle itself; the core may differ from the long-double
    oracle by 16 units (floor: 1e-13 of the values' size)"""
    for v in biweight_cases():
        v = np.ascontiguousarray(v)
        med = O.median(v)
        scale = O.mad(v, med)
        f64 = float(O.biweight(v, med, scale, cval, n_iter))
        vl = v.astype(np.longdouble)
        want = O.biweight(vl, O.median(vl), O.mad(vl, O.median(vl)), cval, n_iter)
        unit = abs(f64 - float(want))
        got = harness.harness_biweight(_p(v), v.size, med, scale, cval, n_iter)
        print(f"m = {v.size}: unit = {unit:.2e}, |got - want| = {abs(got - float(want)):.2e}")
        assert unit <= 1e-12 * np.abs(v).max()
        assert abs(got - float(want)) <= max(16 * unit, 1e-13 * np.abs(v).max())
        if n_iter == 0 or scale == 0:
            assert got == med


def test_windows_and_the_whole_filter_on_the_host(harness):
    """the window search and window_location over a series, as the kernel strings them together"""
    for variant in ("plain", "excluded"):
        t, y, exclude = O.main_input(variant)
        for wl in (0.02, 1.0):
            lo_w, hi_w, _ = O.windows(t, wl, break_tolerance=0.5)
            opens = np.flatnonzero(np.concatenate([[True], np.diff(t) > 0.5]))
            lo, hi = np.empty(t.size, dtype=np.int32), np.empty(t.size, dtype=np.int32)
            for s, e in zip(opens, np.append(opens[1:], t.size) - 1):
                harness.harness_windows(_p(t), s, e, 0.5 * wl, s, e + 1, _p(lo, _ip), _p(hi, _ip))
            assert np.array_equal(lo, lo_w) and np.array_equal(hi, hi_w)
            trend, scale = np.empty(t.size), np.empty(t.size)
            ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint8)
            harness.harness_running_location(_p(y), None if ex is None else ex.ctypes.data, _p(lo, _ip), _p(hi, _ip), 0, t.size, 0, 5.0,
                                             10, _p(trend), _p(scale))
            want, want_scale = O.running_location(t, y, wl, "median", exclude=exclude, break_tolerance=0.5)
            assert np.array_equal(trend, want, equal_nan=True) and np.array_equal(scale, want_scale, equal_nan=True)


def test_abi_of_the_detrending_entry_points():
    """every argument check happens on the host, before any launch (the pointers are never followed)"""
    import re

    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib
    from exoplanet_amd import estimators as E

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    cap = int(consts["EXO_LOCATION_MAX_WINDOW"])
    assert cap == E.MAX_WINDOW >= 8192 and (256 + 2 * cap - 2) * 8 <= 160 * 1024
    assert E._METHODS == {"median": int(consts["EXO_LOCATION_MEDIAN"]), "biweight": int(consts["EXO_LOCATION_BIWEIGHT"])}
    assert lib.exo_abi_version() == 21
    INVALID = 1
    names_w = ["t", "n", "half_window", "break_tolerance", "edge_cutoff", "lo", "hi", "edge", "widest", "stream"]
    ok_w = [8, 100, 0.5, float("inf"), 0.0, 8, 8, 8, 8, None]
    names_r = ["y", "exclude", "n_exclude", "n", "n_series", "lo", "hi", "edge", "max_window", "method", "cval", "n_iter", "trend",
               "scale", "stream"]
    ok_r = [8, None, 0, 100, 3, 8, 8, None, 64, 1, 5.0, 10, 8, None, None]

    def call(fn, names, ok, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)

    for bad in (dict(t=None), dict(lo=None), dict(hi=None), dict(edge=None), dict(widest=None), dict(n=0), dict(n=-5),
                dict(half_window=-1e-9), dict(half_window=float("nan")), dict(break_tolerance=0.0), dict(break_tolerance=float("nan")),
                dict(edge_cutoff=-1.0), dict(edge_cutoff=float("nan"))):
        assert call(lib.exo_location_windows_f64, names_w, ok_w, **bad) == INVALID, bad
    for bad in (dict(y=None), dict(lo=None), dict(hi=None), dict(trend=None), dict(n=0), dict(n_series=0), dict(cval=0.0),
                dict(cval=-5.0), dict(cval=float("nan")), dict(n_iter=-1), dict(method=2), dict(method=-1), dict(max_window=0),
                dict(max_window=cap + 1), dict(n_exclude=2, exclude=8), dict(n_exclude=-1, exclude=8), dict(n_exclude=1),
                dict(n_exclude=3)):
        assert call(lib.exo_running_location_f64, names_r, ok_r, **bad) == INVALID, bad


def test_python_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    assert {"location_plan", "running_location", "flatten", "sde"} <= set(E.__all__)
    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.location_plan(t, 1.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.running_location(t, t, 1.0)
    with pytest.raises(ValueError, match="torch.Tensor"):
        E.running_location(t.numpy(), t.numpy(), 1.0)
    with pytest.raises(ValueError, match="method"):
        E.running_location(t, t, 1.0, method="mean")
    with pytest.raises(ValueError, match="cval"):
        E.running_location(t, t, 1.0, cval=0.0)
    with pytest.raises(ValueError, match="n_iter"):
        E.running_location(t, t, 1.0, n_iter=-1)
    with pytest.raises(ValueError, match="window"):
        E.sde(np.ones(10), window=0)
    if not torch.cuda.is_available():
        for call in (lambda: E.flatten(t, t, 1.0), lambda: E.sde(np.ones(10))):
            with pytest.raises(ValueError, match="no CPU fallback"):
                call()
        return
    d = t.cuda()
    with pytest.raises(ValueError, match="shape"):
        E.running_location(d, d[:-1], 1.0)
    with pytest.raises(ValueError, match="exclude"):
        E.running_location(d, d, 1.0, exclude=torch.zeros(7, dtype=torch.bool, device=d.device))
    with pytest.raises(ValueError, match="exclude"):
        E.running_location(d, d, 1.0, exclude=torch.zeros(50, device=d.device))
    with pytest.raises(ValueError, match="window_length"):
        E.running_location(d, d)
    with pytest.raises(ValueError, match="window_length"):
        E.location_plan(d, -1.0)
    with pytest.raises(ValueError, match="break_tolerance"):
        E.location_plan(d, 1.0, break_tolerance=0.0)
    with pytest.raises(ValueError, match="non-decreasing"):
        E.location_plan(d.flip(0), 1.0)
    with pytest.raises(ValueError, match="plan was made"):
        E.running_location(d, d, plan=E.location_plan(d[:-1], 1.0))
    wide = torch.arange(E.MAX_WINDOW + 1, dtype=torch.float64, device=d.device)
    with pytest.raises(ValueError, match=rf"{E.MAX_WINDOW + 1} cadences, more than the {E.MAX_WINDOW}"):
        E.location_plan(wide, 2.0 * E.MAX_WINDOW)
