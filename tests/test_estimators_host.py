"""CPU: the period-search arithmetic of exoplanet_amd/csrc/exo_estimators_core.hpp compiled for the host
(tests/estimators_harness.cpp) against the numpy restatement of the definitions (tests/estimators_oracle.py), and the host
side of exoplanet_amd.estimators: find_peaks, the two grids, argument errors.  The kernels themselves:
tests/test_gpu_estimators.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimators_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_lp = ctypes.POINTER(ctypes.c_int64)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64, _f64 = ctypes.c_int64, ctypes.c_double


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "estimators_harness.so")
    srcs = [os.path.join(ROOT, "tests", "estimators_harness.cpp"),
            os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_estimators_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_n_bins.restype = _i64
    lib.harness_n_bins.argtypes = [_f64, _f64, ctypes.c_int]
    lib.harness_bin_index.argtypes = [_dp, _i64, _f64, _f64, _i64, _lp]
    lib.harness_bls_search.argtypes = [_dp, _dp, _i64, _ip, ctypes.c_int, _f64, _f64, ctypes.c_int, _f64, _f64, _f64, _i64, _dp]
    lib.harness_ls_sums.argtypes = [_dp, _dp, _dp, _i64, _f64, _f64, _dp]
    lib.harness_ls_kappa.restype = _f64
    lib.harness_ls_kappa.argtypes = [_f64, _f64]
    lib.harness_ls_power.restype = _f64
    lib.harness_ls_power.argtypes = [_dp, _f64, _f64]
    return lib


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def bls_input(seed=721, n=5000):
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, 27, n))
    y = 1e-3 * rs.randn(n)
    y[np.abs((t - 1.0 + 0.5 * 2.345) % 2.345 - 0.5 * 2.345) < 0.1] -= 0.1
    return t, y


def test_bin_indices_match_the_definition(harness):
    """identical on every cadence of every non-fragile period (and the fragile periods are few: the band is 1e-9)"""
    t, _ = bls_input()
    tt = np.ascontiguousarray(t - t.min())
    delta, oversample = 0.01, 10
    n_fragile = 0
    for p in np.concatenate([np.exp(np.linspace(np.log(0.5), np.log(13.5), 300)), [700.0, 2.345, 1.0, 0.64]]):
        n_bins = int(np.ceil(p / delta)) + oversample
        assert harness.harness_n_bins(p, delta, oversample) == n_bins
        q = np.fmod(tt, p) / delta
        want = 1 + np.floor(q).astype(np.int64)
        got = np.empty(tt.size, dtype=np.int64)
        harness.harness_bin_index(_p(tt), tt.size, p, delta, n_bins, _p(got, _lp))
        solid = (np.abs(q - np.round(q)) >= O.FRAGILE_BAND) | (tt == 0)
        n_fragile += int((~solid).sum())
        assert np.array_equal(got[solid], want[solid]), p
        assert got.min() >= 1 and got.max() <= n_bins - oversample
    assert n_fragile <= 2
    # times on exact bin edges (multiples of a delta that is a power of two): the quotient is exact, and so is the index
    tt = np.arange(0, 4096, dtype=np.float64) * 2.0 ** -6
    got = np.empty(tt.size, dtype=np.int64)
    harness.harness_bin_index(_p(tt), tt.size, 8.0, 2.0 ** -6, 512 + 10, _p(got, _lp))
    assert np.array_equal(got, 1 + np.arange(4096) % 512)
    # what is used as an address stays inside the histogram whatever the time
    bad = np.array([np.nan, np.inf, -1.0, 1e300])
    got = np.empty(4, dtype=np.int64)
    harness.harness_bin_index(_p(bad), 4, 3.0, 0.01, 310, _p(got, _lp))
    assert got.min() >= 1 and got.max() <= 310


def search(harness, cy, cw, m, Y, W, objective, p=100.0, delta=0.5, t_min=3.0, n_lane=1):
    cy, cw = np.ascontiguousarray(cy, dtype=np.float64), np.ascontiguousarray(cw, dtype=np.float64)
    m = np.ascontiguousarray(m, dtype=np.int32)
    out = np.full(7, 123.0)
    harness.harness_bls_search(_p(cy), _p(cw), cy.size - 1, _p(m, _ip), m.size, Y, W, objective, p, delta, t_min, n_lane, _p(out))
    return dict(zip(O.FIELDS, out))


def brute(cy, cw, m, Y, W, objective, p=100.0, delta=0.5, t_min=3.0):
    best, arg = -np.inf, None
    for mk in m:
        for s in range(0, len(cy) - 1 - mk + 1):
            box = O.bls_box(np.asarray(cy, float), np.asarray(cw, float), Y, W, np.array([s]), mk)[:, 0]
            obj = box[3 if objective == 0 else 2]
            if not np.isnan(obj) and obj > best:
                best, arg = obj, (s, mk, box)
    if arg is None:
        return dict(zip(O.FIELDS, [-np.inf] + [np.nan] * 6))
    s, mk, box = arg
    return dict(zip(O.FIELDS, [best, *box, mk * delta, np.fmod(s * delta + 0.5 * mk * delta + t_min, p)]))


@pytest.mark.parametrize("n_lane", [1, 3, 64])
def test_search_over_hand_made_prefix_sums(harness, n_lane):
    # bins 1..8: a dip in bins 3-4, an empty bin 6 (w_in = 0 for the one-bin box there)
    hw = np.array([0, 2, 2, 2, 2, 2, 0, 2, 2], dtype=float)
    hy = np.array([0, .1, -.1, -2, -2.2, .1, 0, -.1, .1])
    cy, cw = np.cumsum(hy), np.cumsum(hw)
    Y, W = 1.5 * hy.sum() - 0.3, 1.5 * hw.sum()          # (totals beyond the bins searched: w_out > 0 everywhere)
    for objective in (0, 1):
        got, want = search(harness, cy, cw, [1, 2, 3], Y, W, objective, n_lane=n_lane), brute(cy, cw, [1, 2, 3], Y, W, objective)
        for k in O.FIELDS:
            assert got[k] == pytest.approx(want[k], rel=1e-14, abs=1e-300), (objective, k)
        assert got["duration"] == 1.0 and got["transit_time"] == 2 * 0.5 + 0.5 + 3.0     # s = 2, m = 2
    # w_out = 0: the box that holds every cadence is skipped, the next best is returned
    got = search(harness, cy, cw, [8, 2], hy.sum(), hw.sum(), 0, n_lane=n_lane)
    want = brute(cy, cw, [8, 2], hy.sum(), hw.sum(), 0)
    assert got["duration"] == 1.0 and got["power"] == pytest.approx(want["power"], rel=1e-14)
    # nothing admissible at all: one bin holds everything, every box has w_in = 0 or w_out = 0
    one = np.cumsum([0, 0, 5.0, 0, 0])
    got = search(harness, -one, one, [1, 2], -5.0, 5.0, 0, n_lane=n_lane)
    assert got["power"] == -np.inf and all(np.isnan(got[k]) for k in O.FIELDS[1:])
    # an exact tie: two identical dips; the first (k, s) wins: the narrowest box first, then the earliest start
    hy = np.array([0, 0, -1.0, 0, 0, -1.0, 0, 0])
    hw = np.ones(8)
    hw[0] = 0
    for objective in (0, 1):
        got = search(harness, np.cumsum(hy), np.cumsum(hw), [1, 1, 2], hy.sum(), hw.sum(), objective, n_lane=n_lane)
        assert got["duration"] == 0.5 and got["transit_time"] == 1 * 0.5 + 0.25 + 3.0, got
    # a brightening only: depth < 0.  The likelihood does not see the sign; the signal to noise prefers the least negative box
    hy = np.array([0, 0, 0, 3.0, 0, 0, 0])
    hw = np.array([0, 1, 1, 1, 1, 1, 1.0])
    cy, cw = np.cumsum(hy), np.cumsum(hw)
    like = search(harness, cy, cw, [1], 3.0, 6.0, 0, n_lane=n_lane)
    snr = search(harness, cy, cw, [1], 3.0, 6.0, 1, n_lane=n_lane)
    assert like["depth"] == pytest.approx(-3.0) and like["power"] == pytest.approx(4.5) and like["transit_time"] == 1.25 + 3.0
    assert snr["depth"] == pytest.approx(0.6) and snr["power"] == snr["depth_snr"] > 0 and snr["transit_time"] == 0.25 + 3.0
    for objective in (0, 1):
        got, want = search(harness, cy, cw, [1], 3.0, 6.0, objective, n_lane=n_lane), brute(cy, cw, [1], 3.0, 6.0, objective)
        for k in O.FIELDS:
            assert got[k] == pytest.approx(want[k], rel=1e-14), (objective, k)


def test_search_matches_the_oracle_on_real_prefix_sums(harness):
    t, y = bls_input(n=800)
    durations, oversample = (0.1, 0.2, 0.4), 10
    delta, ms = O.bls_plan(durations, oversample)
    for p in (0.9, 2.345, 7.77):
        for objective in ("likelihood", "snr"):
            want = O.bls_power(t, y, None, [p], durations, oversample, objective)
            cy, cw, Y, W, t_min, _ = O.bls_prefix(t, y, None, p, delta, oversample)
            got = search(harness, cy, cw, ms, Y, W, 0 if objective == "likelihood" else 1, p=p, delta=delta, t_min=t_min, n_lane=7)
            for k in O.FIELDS:
                assert got[k] == pytest.approx(want[k][0], rel=1e-13), (p, objective, k)


def ls_closed_form(harness, t, y, yerr, f, kappa=None):
    y, w = O._weights(y, yerr, np.float64)
    t, w, wy = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(w), np.ascontiguousarray(w * y)
    sums = np.empty(7)
    kappa = harness.harness_ls_kappa(f, t.max() - t.min()) if kappa is None else kappa
    harness.harness_ls_sums(_p(t), _p(w), _p(wy), t.size, f, kappa, _p(sums))
    return harness.harness_ls_power(_p(sums), w.sum(), wy.sum())


def test_lomb_scargle_closed_form_against_least_squares(harness):
    rs = np.random.RandomState(9502)
    t = np.sort(rs.uniform(0, 10, 500))
    y = 4.5 * np.sin(2 * np.pi * t / 2.345) + 7.0
    yerr = 0.5 + rs.uniform(size=t.size)
    freq = np.concatenate([0.02 + 0.0993 * np.arange(60), [1 / 2.345]])
    for e in (None, yerr):
        tc = t - 0.5 * (t.min() + t.max())
        want = O.lomb_scargle_power(tc, y, e, freq, dtype=np.longdouble)
        f64 = O.lomb_scargle_power(tc, y, e, freq)
        tol = max(16 * O.rel_diff(f64, want, scale=float(want.max())), 1e-13)
        got = np.array([ls_closed_form(harness, tc, y, e, f) for f in freq])
        assert O.rel_diff(got, want, scale=float(want.max())) <= tol
        # the constant taken off cos x changes nothing but the rounding
        for kappa in (0.0, 0.7):
            other = np.array([ls_closed_form(harness, tc, y, e, f, kappa) for f in freq[5:]])
            assert O.rel_diff(other, want[5:], scale=float(want.max())) <= tol
        # a pure sine is fitted exactly: chi2 = 0 at its frequency, the power is chi2_0 / 2
        yy, w = O._weights(y, e, np.float64)
        chi2_0 = (w * (yy - (w * yy).sum() / w.sum()) ** 2).sum()
        assert got[-1] == pytest.approx(0.5 * chi2_0, rel=1e-12)
    assert harness.harness_ls_kappa(0.0, 10.0) == 1.0 and harness.harness_ls_kappa(0.05, 10.0) == pytest.approx(2 / np.pi)
    # periods far longer than the baseline, where cos x is all but constant: still the least-squares value
    low = np.array([1e-4, 1e-3, 5e-3, 2e-2])
    want = O.lomb_scargle_power(tc, y, yerr, low, dtype=np.longdouble)
    got = np.array([ls_closed_form(harness, tc, y, yerr, f) for f in low])
    print("low frequencies:", np.abs(got - want) / np.abs(want))
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want))
    # a constant series has no power; a frequency at which the sine column vanishes on an even grid is a rank-2 problem
    assert abs(ls_closed_form(harness, t, np.full(t.size, 3.0), None, 0.7)) < 1e-12
    te = np.arange(64, dtype=np.float64)
    ye = np.cos(np.pi * te) + 0.1 * te
    want = O.lomb_scargle_power(te, ye, None, [0.5])[0]
    assert ls_closed_form(harness, te, ye, None, 0.5) == pytest.approx(want, rel=1e-10)


# ---- the host side of exoplanet_amd.estimators -------------------------------------------------------------------------------

def test_find_peaks_on_a_gaussian():
    from exoplanet_amd.estimators import find_peaks

    freq = np.linspace(0.1, 1.0, 91)
    f0, sig = 0.4321, 0.05
    power = 3.0 * np.exp(-0.5 * (freq - f0) ** 2 / sig ** 2)
    peak = find_peaks(freq, power)
    assert peak["index"] == int(np.argmax(power)) + 1
    assert peak["period"] == pytest.approx(1 / f0, rel=1e-10)
    assert peak["period_uncert"] == pytest.approx(sig / f0 ** 2, rel=1e-10)
    assert peak["log_power"] == pytest.approx(np.log(3.0), abs=1e-10)
    assert all(type(v) in (int, float) for v in peak.values())
    two = power + 1.0 * np.exp(-0.5 * (freq - 0.8) ** 2 / 0.02 ** 2)
    peaks = find_peaks(freq, two, max_peaks=5)
    assert len(peaks) == 2 and peaks[0]["period"] == pytest.approx(1 / f0, rel=1e-3) and peaks[1]["period"] == pytest.approx(1.25, rel=1e-3)
    assert find_peaks(freq, freq, max_peaks=3) == []
    with pytest.raises(ValueError, match="no peaks"):
        find_peaks(freq, freq)


def test_grids_against_hand_computed_values():
    from exoplanet_amd.estimators import bls_autoperiod, lomb_scargle_autofrequency

    t = np.array([3.0, 13.0, 5.0, 8.0])                                 # T = 10
    p = bls_autoperiod(t, [0.5, 0.25])                                  # df = 0.25 / 100, f from 1 (= 1 / (2 * 0.5)) down to 0.2 (= 2 / T)
    assert len(p) == 321 and p[0] == 1.0 and p[-1] == pytest.approx(5.0, rel=1e-12)
    assert p[1] == pytest.approx(1 / (1 - 0.0025), rel=1e-15)
    p = bls_autoperiod(t, 0.25, minimum_period=2.0, maximum_period=4.0, frequency_factor=4.0)     # df = 0.01, f from 0.5 to 0.25
    assert np.allclose(p, 1 / (0.5 - 0.01 * np.arange(26)), rtol=1e-15, atol=0)
    assert np.array_equal(p, O.bls_autoperiod(t, 0.25, 2.0, 4.0, frequency_factor=4.0))
    assert len(bls_autoperiod(t, 0.25, minimum_n_transit=6)) == 1 + round((2 - 0.5) / 0.0025)    # max period T / 5
    f = lomb_scargle_autofrequency(t)                                   # df = 1 / 50, from df / 2 to 5 * 0.5 * 4 / 10 = 1
    assert len(f) == 1 + round((1 - 0.01) / 0.02) and f[0] == pytest.approx(0.01) and f[1] - f[0] == pytest.approx(0.02)
    f = lomb_scargle_autofrequency(t, samples_per_peak=2, minimum_frequency=0.1, maximum_frequency=1.0)
    assert np.allclose(f, 0.1 + 0.05 * np.arange(19), rtol=1e-15)
    with pytest.raises(ValueError):
        bls_autoperiod(np.array([1.0, 1.0]), 0.2)
    with pytest.raises(ValueError):
        bls_autoperiod(t, -0.2)
    with pytest.raises(ValueError):
        bls_autoperiod(t, 0.2, minimum_period=5.0, maximum_period=1.0)


def test_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.bls_power(t, t, periods=[1.0, 2.0], durations=[0.1])
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.lomb_scargle_power(t, t, frequencies=[1.0])
    with pytest.raises(ValueError, match="torch.Tensor"):
        E.bls_power(t.numpy(), t.numpy(), periods=[1.0], durations=[0.1])
    with pytest.raises(ValueError, match="objective"):
        E.bls_power(t, t, periods=[1.0], durations=[0.1], objective="depth")
    # the host arithmetic of a box search refuses what has no meaning
    E.bls_plan([1.0, 2.0], [0.1, 0.2], 10)
    for periods, durations, oversample in (([1.0, -2.0], [0.1], 10), ([1.0, 0.0], [0.1], 10), ([1.0], [0.1, -0.1], 10),
                                           ([1.0], [], 10), ([0.3, 1.0], [0.1, 0.3], 10), ([1.0], [2.0], 10), ([1.0], [0.1], 0),
                                           ([1.0], [0.1], 2.5), ([1.0], [0.01] * 17, 10)):
        with pytest.raises(ValueError):
            E.bls_plan(periods, durations, oversample)
    delta, m, n_bins = E.bls_plan([1.0, 700.0], [0.05, 0.1, 0.2], 10)
    assert delta == 0.005 and list(m) == [10, 20, 40] and list(n_bins) == [210, 140010]
    if torch.cuda.is_available():
        d = t.cuda()
        with pytest.raises(ValueError, match="shape"):
            E.bls_power(d, d[:-1], periods=[1.0], durations=[0.1])
        with pytest.raises(ValueError, match="yerr"):
            E.bls_power(d, d, d[:7], periods=[1.0], durations=[0.1])


def test_abi_of_the_new_entry_points():
    """argument checks on the host, before any launch; the workspace is sized by pure arithmetic"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    lib = _lib.load()
    INVALID, WORKSPACE = 1, 3
    head = 8                                                            # t_min, t_max, (Y, W) per series, padded to 8 doubles
    assert lib.exo_bls_workspace_bytes(1000, 1, 10, 500) == 8 * (head + 3 * 1000)
    assert lib.exo_bls_workspace_bytes(1000, 3, 0, 0) == 8 * (head + 7 * 1000)
    big = lib.exo_bls_workspace_bytes(1000, 1, 10, 5000)                # above the LDS limit: one slab per (period, series) pair
    assert big == 8 * (head + 3 * 1000 + 10 * 2 * 5001)
    assert lib.exo_bls_workspace_bytes(1000, 1, 10 ** 6, 5000) == 8 * (head + 3 * 1000 + 256 * 2 * 5001)
    assert lib.exo_bls_workspace_bytes(0, 1, 10, 500) == -1
    m = (ctypes.c_int32 * 2)(10, 20)
    ok = [8, 8, None, 0, 100, 1, 8, 5, 100, 200, ctypes.addressof(m), 2, 0.01, 10, 0, 8, 8, 1 << 30, None]

    def call(**kw):
        names = ["t", "y", "yerr", "n_yerr", "n", "n_series", "periods", "n_period", "min_bins", "max_bins", "m", "n_dur", "delta",
                 "oversample", "objective", "out", "ws", "ws_bytes", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_bls_power_f64(*args)

    assert call(n_period=0) == 0                                        # nothing to do
    for bad in (dict(t=None), dict(n=0), dict(n_yerr=1), dict(n_yerr=3, yerr=8), dict(n_dur=0), dict(n_dur=17), dict(delta=0.0),
                dict(oversample=0), dict(objective=2), dict(min_bins=300), dict(out=None), dict(ws=None), dict(n_series=0)):
        assert call(**bad) == INVALID, bad
    zero = (ctypes.c_int32 * 2)(10, 0)
    assert call(m=ctypes.addressof(zero)) == INVALID
    assert call(ws_bytes=100) == WORKSPACE
    assert lib.exo_lomb_scargle_power_f64(8, 8, None, 0, 100, 1, 8, 0, 8, 8, 1 << 20, None) == 0
    assert lib.exo_lomb_scargle_power_f64(8, 8, None, 0, 100, 1, None, 5, 8, 8, 1 << 20, None) == INVALID
    assert lib.exo_lomb_scargle_power_f64(8, 8, None, 0, 100, 1, 8, 5, 8, 8, 64, None) == WORKSPACE
