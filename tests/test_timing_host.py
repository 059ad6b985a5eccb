"""CPU: the arithmetic of exoplanet_amd/csrc/exo_timing_core.hpp compiled for the host (tests/timing_harness.cpp) against the
numpy statement of the definition (tests/timing_oracle.py), the numbers the science test relies on from the statement alone, the
argument checks of the two C entry points and of the Python functions.  The kernels themselves: tests/test_gpu_timing.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timing_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_int64)
_f64, _i64, _int = ctypes.c_double, ctypes.c_int64, ctypes.c_int


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "timing_harness.so")
    srcs = [os.path.join(ROOT, "tests", "timing_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_timing_core.hpp"),
            os.path.join(ROOT, "include", "exoplanet_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_cap.argtypes = [_int]
    lib.harness_lds_bytes.restype, lib.harness_lds_bytes.argtypes = _i64, [_i64, _i64, _i64]
    lib.harness_template_value.restype, lib.harness_template_value.argtypes = _f64, [_dp, _int, _f64]
    lib.harness_shift_value.restype, lib.harness_shift_value.argtypes = _f64, [_f64, _int, _int]
    lib.harness_windows.argtypes = [_dp, _i64, _lp, _i64, _f64, _f64, _f64, _dp, _ip, _ip]
    lib.harness_vertex.argtypes = [_f64, _f64, _f64, _int, _int, _f64, _f64, _dp]
    lib.harness_transit.argtypes = [_dp, _dp, _dp, _f64, ctypes.c_int32, ctypes.c_int32, _f64, _f64, _int, _dp, _int, _dp, _int, _dp, _ip,
                                    _dp]
    lib.harness_all.restype = _f64
    lib.harness_all.argtypes = [_dp, _dp, _dp, _i64, _i64, _dp, _ip, _ip, _i64, _f64, _f64, _int, _dp, _int, _int, _dp, _ip]
    return lib


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def host_transit_times(lib, t, y, yerr, template, depth=None, min_in_transit=3, exclude=None, **search):
    """every transit of one series through the harness, in the layout tests/timing_oracle.py's check reads"""
    t, y = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    n_k = O.epochs(t, search["period"], search["t0"], search["window"])
    K, M = len(n_k), search["n_shift"]
    T_k, lo, hi = np.empty(K), np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
    lib.harness_windows(_p(t), t.size, _p(n_k, _lp), K, search["period"], search["t0"], search["window"], _p(T_k), _p(lo, _ip), _p(hi, _ip))
    ivar = None
    if yerr is not None or exclude is not None:
        ivar = np.ones(t.size) if yerr is None else np.ascontiguousarray(np.broadcast_to(1 / np.asarray(yerr, dtype=np.float64) ** 2, t.shape))
        if exclude is not None:
            ivar = np.where(exclude, 0.0, ivar)
    g = np.ascontiguousarray(template, dtype=np.float64)
    got = {k: np.empty(K) for k in O.FLOAT_FIELDS}
    got.update({k: np.empty(K, dtype=np.int64) for k in O.INT_FIELDS})
    got.update(transit_ind=n_k, linear_time=T_k, lo=lo, hi=hi, curve=np.empty((K, M)))
    d = None if depth is None else ctypes.byref(ctypes.c_double(depth))
    for k in range(K):
        rec, irec = np.empty(7), np.empty(4, dtype=np.int32)
        lib.harness_transit(_p(t), _p(y), None if ivar is None else _p(ivar), T_k[k], int(lo[k]), int(hi[k]), search["duration"],
                            search["max_shift"], M, _p(g), g.size, ctypes.cast(d, _dp) if d is not None else None, min_in_transit,
                            _p(rec), _p(irec, _ip), _p(got["curve"][k]))
        for f, v in zip(O.FLOAT_FIELDS, rec):
            got[f][k] = v
        for f, v in zip(O.INT_FIELDS, irec):
            got[f][k] = v
    return got


def test_template_interpolation(harness):
    rs = np.random.RandomState(4)
    for m in (1, 2, 3, 7, 256, 1024):
        g = np.ascontiguousarray(0.2 + rs.rand(m))
        centres = (2.0 * np.arange(m) + 1.0) / m - 1.0
        xs = np.concatenate([centres, 0.5 * (centres[1:] + centres[:-1]), 0.5 * (centres[:1] - 1), 0.5 * (centres[-1:] + 1),
                             rs.uniform(-1, 1, 50), [np.nextafter(1.0, 0), np.nextafter(-1.0, 0), 0.0]])
        want = O.template_value(g.astype(np.longdouble), xs.astype(np.longdouble))
        got = np.array([harness.harness_template_value(_p(g), m, float(x)) for x in xs])
        # u = (x + 1) m / 2 - 1/2 <= m carries three roundings, below 2 m eps in all (eps = 2^-52); g(u) has a slope of at most
        # 2 max|g| per bin (the two outer segments; max|g| between centres here), and the interpolation adds a few eps of its own
        bound = (4.0 * m + 8) * 2.0 ** -52 * g.max()
        assert np.abs(got - np.asarray(want, dtype=np.float64)).max() <= bound, m
        at_nodes = np.array([harness.harness_template_value(_p(g), m, float(x)) for x in centres])
        assert np.abs(at_nodes - g).max() <= bound
        for x in (1.0, -1.0, 1.5, -3.0, np.inf, -np.inf, np.nan):
            assert harness.harness_template_value(_p(g), m, x) == 0.0, (m, x)
    g1 = np.array([0.8])                                               # m = 1: a triangle
    for x, want in ((0.0, 0.8), (0.5, 0.4), (-0.5, 0.4), (0.75, 0.2)):
        assert harness.harness_template_value(_p(g1), 1, x) == pytest.approx(want, abs=1e-16)


def test_shifts_are_the_expression_not_a_running_sum(harness):
    for max_shift, M in ((0.03, 121), (0.1, 4097), (0.07, 3)):
        want, _ = O.shifts(max_shift, M)
        got = np.array([harness.harness_shift_value(max_shift, M, j) for j in range(M)])
        assert np.array_equal(got, want)
        assert got[0] == -max_shift


def test_vertex_formula(harness):
    out = np.empty(2)
    h = 0.001
    # symmetric: the grid's shift
    assert harness.harness_vertex(-3.0, -1.0, -3.0, 5, 11, 0.0, h, _p(out)) == 0 and out[0] == 0.0
    assert out[1] == h / np.sqrt(4.0)
    # a known parabola L = -(d - 0.3 h)^2 / (2 s^2) sampled at -h, 0, h
    s = 2.5e-3
    L = [-(d - 0.3 * h) ** 2 / (2 * s * s) for d in (-h, 0.0, h)]
    assert harness.harness_vertex(L[0], L[1], L[2], 1, 3, 0.0, h, _p(out)) == 0
    assert out[0] == pytest.approx(0.3 * h, rel=1e-12) and out[1] == pytest.approx(s, rel=1e-12)
    want = O.vertex_at(np.array(L), 1, np.array([-h, 0.0, h]), h)
    assert out[0] == want[1] and out[1] == want[2]                    # the same IEEE operations
    # flat, an end of the grid, a neighbour without a fit: at_edge, the grid's shift, no error
    for args in ((-1.0, -1.0, -1.0, 5, 11), (-3.0, -1.0, -3.0, 0, 11), (-3.0, -1.0, -3.0, 10, 11), (-np.inf, -1.0, -3.0, 5, 11),
                 (-3.0, -1.0, -np.inf, 5, 11), (0.0, -1.0, 0.0, 5, 11)):
        assert harness.harness_vertex(*args, 0.25, h, _p(out)) == 1, args
        assert out[0] == 0.25 and np.isnan(out[1])


def test_window_search_equals_searchsorted(harness):
    rs = np.random.RandomState(9)
    t = np.sort(np.concatenate([rs.uniform(0, 10, 300), [3.0, 3.0, 3.0], np.arange(20, 21, 0.01)]))
    for period, t0, window in ((1.7, 0.3, 0.4), (0.5, 0.1, 0.05), (2.345, 1.0, 0.66), (9.0, 15.0, 2.0)):
        n_k = O.epochs(t, period, t0, window)
        K = len(n_k)
        T_k, lo, hi = np.empty(K), np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
        harness.harness_windows(_p(t), t.size, _p(n_k, _lp), K, period, t0, window, _p(T_k), _p(lo, _ip), _p(hi, _ip))
        assert np.array_equal(T_k, t0 + period * n_k.astype(np.float64))
        wlo, whi = O.windows(t, T_k, window)
        assert np.array_equal(lo, wlo) and np.array_equal(hi, whi)
        # every epoch of the definition and no other: the next one on either side lies outside
        assert K and T_k[0] >= t[0] - window / 2 and T_k[-1] <= t[-1] + window / 2
        assert t0 + period * (n_k[0] - 1) < t[0] - window / 2 and t0 + period * (n_k[-1] + 1) > t[-1] + window / 2
    # (9.0, 15.0, 2.0): epoch 0 at 15 holds no cadence (the axis has none in (10, 20)); ends of t cut the first and last windows
    counts = (whi - wlo + 1).tolist()
    assert 0 in counts
    # a window of exactly one cadence, one of none, and both ends of the axis
    t = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    n_k = np.arange(-1, 10, dtype=np.int64)
    K = len(n_k)
    T_k, lo, hi = np.empty(K), np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
    harness.harness_windows(_p(t), t.size, _p(n_k, _lp), K, 0.5, 0.0, 0.2, _p(T_k), _p(lo, _ip), _p(hi, _ip))
    assert (hi - lo + 1).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert lo[0] == 0 and hi[0] == -1 and lo[-1] == 5 and hi[-1] == 4
    harness.harness_windows(_p(t), t.size, _p(n_k, _lp), K, 0.5, 0.0, 2.0, _p(T_k), _p(lo, _ip), _p(hi, _ip))
    assert lo[0] == 0 and hi[0] == 0 and lo[-1] == 4 and hi[-1] == 4 and int((hi - lo + 1).max()) == 3


def test_the_statement_alone_stays_inside_the_science_bounds():
    """the bounds tests/test_gpu_timing.py asserts on the kernel hold for the numpy statement on all three inputs"""
    for case in O.CASES:
        t, y, sigma = O.main_input(case)
        res = O.transit_times(t, y, sigma, template=O.main_template(), **O.SEARCH)
        report = O.science("statement, " + case, res)
        assert len(res["transit_ind"]) == 12
        if case == "30min":
            full = res["n_window"][res["valid"] == 1]                   # (the window in the gap keeps 6 cadences)
            assert full.min() == 25 and full.max() == 32
        assert report["rms_pull"] < 2


@pytest.mark.parametrize("case,offset", [("30min", 0.0), ("30min", 1.0), ("10min", 0.0)])
def test_whole_transits_within_the_rounding_of_the_statement(harness, case, offset):
    t, y, sigma = O.main_input(case, offset)
    g = O.main_template()
    for kw in (dict(yerr=sigma), dict(yerr=None), dict(yerr=sigma, depth=0.011),
               dict(yerr=sigma * (1 + 0.3 * np.sin(t)), exclude=(t > 3.3) & (t < 3.36))):
        yerr = kw.pop("yerr")
        ref = O.reference(t, y, yerr, template=g, **kw, **O.SEARCH)
        got = host_transit_times(harness, t, y, yerr, g, **kw, **O.SEARCH)
        O.check(f"host core, {case}, offset {offset}, {sorted(kw)}", got, ref)
        # the record's shift and error are the vertex formula on the record's own curve
        shift, err = O.vertex_from_curve(got["curve"], O.shifts(O.SEARCH["max_shift"], O.SEARCH["n_shift"])[0], got["valid"])
        assert np.array_equal(shift, got["shift"], equal_nan=True) and np.array_equal(err, got["time_err"], equal_nan=True)


def test_min_in_transit_and_a_transit_beyond_the_grid(harness):
    t, y, sigma = O.main_input("30min")
    g = O.main_template()
    for mit in (1, 5, 9, 10, 11, 40):
        ref = O.reference(t, y, sigma, template=g, min_in_transit=mit, **O.SEARCH)
        got = host_transit_times(harness, t, y, sigma, g, min_in_transit=mit, **O.SEARCH)
        O.check(f"host core, min_in_transit {mit}", got, ref)
    assert not got["valid"].any()                                       # (a 0.2 d template holds at most 10 cadences of 30 min)
    search = dict(O.SEARCH, max_shift=0.004, n_shift=9, window=0.5)     # the true shifts reach 0.01: most maxima sit on an end
    ref = O.reference(t, y, sigma, template=g, **search)
    got = host_transit_times(harness, t, y, sigma, g, **search)
    O.check("host core, beyond the grid", got, ref)
    edge = got["at_edge"] == 1
    assert edge.sum() >= 6 and np.all(np.abs(got["shift"][edge]) == 0.004) and np.all(np.isnan(got["time_err"][edge]))


def test_abi_of_the_timing_entry_points(harness):
    """every argument check happens on the host, before any launch (the pointers are never followed)"""
    import re

    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib
    from exoplanet_amd import estimators as E

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    caps = [int(consts[k]) for k in ("EXO_TIMING_MAX_WINDOW", "EXO_TIMING_MAX_TEMPLATE", "EXO_TIMING_MAX_SHIFTS")]
    assert caps == [E.MAX_TIMING_WINDOW, E.MAX_TIMING_TEMPLATE, E.MAX_TIMING_SHIFTS] == [4096, 1024, 4097]
    assert caps == [harness.harness_cap(i) for i in range(3)]
    threads = harness.harness_cap(3)
    # the LDS the kernel asks for at the caps fits a CU
    assert harness.harness_lds_bytes(*caps) == 8 * (3 * caps[0] + caps[1] + caps[2] + 2 * threads) + 4 * threads <= 160 * 1024
    assert lib.exo_abi_version() == 21
    INVALID = 1
    names_w = ["t", "n", "epochs", "n_transit", "period", "t0", "window", "linear_time", "lo", "hi", "widest", "stream"]
    ok_w = [8, 100, 8, 5, 2.0, 0.5, 0.6, 8, 8, 8, 8, None]
    names_f = ["t", "y", "ivar", "n_ivar", "n", "n_series", "linear_time", "lo", "hi", "n_transit", "max_window", "duration", "max_shift",
               "n_shift", "window", "tmpl", "n_template", "depth", "n_depth", "min_in_transit", "out", "iout", "curve", "stream"]
    ok_f = [8, 8, None, 0, 100, 3, 8, 8, 8, 5, 64, 0.2, 0.05, 21, 0.6, 8, 16, None, 0, 3, 8, 8, None, None]

    def call(fn, names, ok, **kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)

    nan = float("nan")
    for bad in (dict(t=None), dict(epochs=None), dict(linear_time=None), dict(lo=None), dict(hi=None), dict(widest=None), dict(n=0),
                dict(n=-3), dict(n_transit=0), dict(period=0.0), dict(period=-1.0), dict(period=nan), dict(window=0.0), dict(window=nan),
                dict(t0=nan), dict(t0=float("inf"))):
        assert call(lib.exo_timing_windows_f64, names_w, ok_w, **bad) == INVALID, bad
    for bad in (dict(t=None), dict(y=None), dict(linear_time=None), dict(lo=None), dict(hi=None), dict(tmpl=None), dict(out=None),
                dict(iout=None), dict(n=0), dict(n=-1), dict(n_series=0), dict(n_transit=0), dict(n_shift=20), dict(n_shift=1),
                dict(n_shift=-3), dict(n_shift=caps[2] + 2), dict(duration=0.0), dict(duration=-0.2), dict(duration=nan),
                dict(window=0.0), dict(window=nan), dict(max_shift=-1e-9), dict(max_shift=nan), dict(window=0.29),
                dict(max_window=0), dict(max_window=caps[0] + 1), dict(n_template=0), dict(n_template=caps[1] + 1),
                dict(min_in_transit=0), dict(n_ivar=2, ivar=8), dict(n_ivar=-1, ivar=8), dict(n_ivar=1), dict(n_ivar=3),
                dict(n_depth=2, depth=8), dict(n_depth=-1, depth=8), dict(n_depth=1), dict(n_depth=3)):
        assert call(lib.exo_transit_timing_f64, names_f, ok_f, **bad) == INVALID, bad


def test_python_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    assert {"TimingPlan", "timing_plan", "transit_times", "ttv_estimator"} <= set(E.__all__)
    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.timing_plan(t, 2.0, 0.5, 0.2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.transit_times(t, t, period=2.0, t0=0.5, duration=0.2)
    with pytest.raises(ValueError, match="torch.Tensor"):
        E.transit_times(t.numpy(), t.numpy(), period=2.0, t0=0.5, duration=0.2)
    with pytest.raises(ValueError, match="torch.Tensor"):
        E.timing_plan(t.numpy(), 2.0, 0.5, 0.2)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no CPU fallback"):
            E.ttv_estimator(t.numpy(), t.numpy(), period=2.0, t0=0.5, duration=0.2)
        return
    d = t.cuda()
    for kw, match in ((dict(period=0.0), "period"), (dict(period=None), "period"), (dict(t0=float("nan")), "t0"),
                      (dict(duration=-1.0), "duration"), (dict(max_shift=-0.1), "max_shift"), (dict(n_shift=200), "n_shift"),
                      (dict(n_shift=1), "n_shift"), (dict(n_shift=E.MAX_TIMING_SHIFTS + 2), "n_shift"), (dict(window=0.25), "window")):
        args = dict(period=2.0, t0=0.5, duration=0.2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            E.timing_plan(d, args.pop("period"), args.pop("t0"), args.pop("duration"), **args)
    g = np.ones(8)
    with pytest.raises(ValueError, match="shape"):
        E.transit_times(d, d[:-1], period=2.0, t0=0.5, duration=0.2, template=g)
    with pytest.raises(ValueError, match="exclude"):
        E.transit_times(d, d, period=2.0, t0=0.5, duration=0.2, template=g, exclude=torch.zeros(7, dtype=torch.bool, device=d.device))
    with pytest.raises(ValueError, match="min_in_transit"):
        E.transit_times(d, d, period=2.0, t0=0.5, duration=0.2, template=g, min_in_transit=0)
    with pytest.raises(ValueError, match="template"):
        E.transit_times(d, d, period=2.0, t0=0.5, duration=0.2, template=np.ones(E.MAX_TIMING_TEMPLATE + 1))
    with pytest.raises(ValueError, match="not finite"):
        E.transit_times(d, d, period=2.0, t0=0.5, duration=0.2, template=np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="depth"):
        E.transit_times(d, d, period=2.0, t0=0.5, duration=0.2, template=g, depth=torch.ones(3, dtype=torch.float64, device=d.device))
    with pytest.raises(ValueError, match="non-decreasing"):
        E.timing_plan(d.flip(0) + 0.0, 2.0, 0.5, 0.2)
    with pytest.raises(ValueError, match="plan was made"):
        E.transit_times(d, d, template=g, plan=E.timing_plan(d[:-1], 2.0, 0.5, 0.2))
