"""CPU: the Keplerian periodogram's arithmetic of exoplanet_amd/csrc/exo_keplerian_core.hpp compiled for the host
(tests/keplerian_harness.cpp) against the numpy statement of DESIGN.md section 22 (tests/keplerian_oracle.py), and the argument
errors of exoplanet_amd.estimators.keplerian_power that need no device.  The kernel itself: tests/test_gpu_keplerian.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keplerian_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i32, _f64 = ctypes.c_int32, ctypes.c_double


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "keplerian_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "keplerian_harness.cpp"), os.path.join(ROOT, "tests", "orbit_lanes.hpp")] + [
        os.path.join(csrc, h) for h in ("exo_keplerian_core.hpp", "exo_orbit_search.hpp", "exo_estimators_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_keplerian.argtypes = [_dp, _dp, _dp, _i32, _ip, ctypes.c_int, _f64, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      _dp, _dp]
    lib.harness_lomb_scargle.restype = _f64
    lib.harness_lomb_scargle.argtypes = [_dp, _dp, _dp, _i32, _f64]
    lib.harness_best.restype = _i32
    lib.harness_best.argtypes = [_dp, _ip, ctypes.c_int]
    return lib


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def columns(t, y, yerr, inst):
    """what the preparation kernel hands the search: the epochs sorted by instrument (stably), t - t_min, w, w y, the offsets"""
    y, w = O.weights(y, yerr, np.float64)
    inst = np.zeros(t.size, dtype=np.int64) if inst is None else np.asarray(inst, dtype=np.int64)
    order = np.argsort(inst, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(inst))]).astype(np.int32)
    c = np.ascontiguousarray
    return c((t - t.min())[order]), c(w[order]), c((w * y)[order]), off


def run(harness, t, y, yerr, inst, freq, ecc, n_phase, n_lane=256):
    tt, w, wy, off = columns(t, y, yerr, inst)
    ecc = np.ascontiguousarray(ecc, dtype=np.float64)
    n_inst, C = off.size - 1, ecc.size * n_phase
    table, record = np.empty((len(freq), C)), np.empty((len(freq), 4 + n_inst))
    for i, f in enumerate(freq):
        harness.harness_keplerian(_p(tt), _p(w), _p(wy), tt.size, _p(off, _ip), n_inst, f, _p(ecc), ecc.size, n_phase, n_lane,
                                  _p(table[i]), _p(record[i]))
    return dict(table=table, power=record[:, 0], candidate=record[:, 1].astype(np.int64), A=record[:, 2], B=record[:, 3],
                const=record[:, 4:])


def statements(inst=True, yerr=True):
    d = O.main_input()
    args = (d["t"], d["y"], d["err"] if yerr else None, d["inst"] if inst else None, d["f"], d["ecc"], d["n_phase"])
    return d, args, O.cached(("main", inst, yerr, "f64"), lambda: O.keplerian(*args)), \
        O.cached(("main", inst, yerr, "ld"), lambda: O.keplerian(*args, dtype=np.longdouble))


def test_the_main_input_is_the_one_described():
    """what the definition's author measured on this input, on the statement itself"""
    d, _, f64, ld = statements()
    assert d["f"].size == 197 and int(np.isfinite(f64["table"][0]).sum()) == 289
    print("smallest gap between the best and the second-best candidate, of the peak: %.2e" % f64["gap"].min())
    assert 5e-5 < f64["gap"].min() < 2e-4
    assert np.array_equal(f64["candidate"], ld["candidate"])
    peak = int(np.argmax(f64["power"]))
    assert f64["ecc"][peak] == pytest.approx(0.6) and f64["candidate"][peak] % 32 == 12      # phi = 0.375
    assert abs(1 / d["f"][peak] - O.MAIN["period"]) < 0.2


@pytest.mark.parametrize("inst", [True, False])
def test_sums_power_coefficients_and_argmax_against_the_statement(harness, inst):
    _, args, f64, ld = statements(inst=inst)
    got = run(harness, *args)
    peak = float(ld["power"].max())
    live = np.isfinite(ld["table"])
    assert np.array_equal(np.isfinite(got["table"]), live)
    tol = O.tolerance(f64["table"][live], ld["table"][live], peak)
    err = O.rel_diff(got["table"][live], ld["table"][live], peak)
    print("every candidate's power: f64 vs longdouble %.1e, tolerance %.1e, core vs longdouble %.1e"
          % (O.rel_diff(f64["table"][live], ld["table"][live], peak), tol, err))
    assert err <= tol
    assert np.array_equal(got["candidate"], ld["candidate"])
    for key, scale in (("power", peak), ("A", float(np.abs(ld["A"]).max())), ("B", float(np.abs(ld["B"]).max())),
                       ("const", float(np.abs(ld["const"]).max()))):
        tol = O.tolerance(f64[key], ld[key], scale)
        err = O.rel_diff(got[key], ld[key], scale)
        print("%s: tolerance %.1e, core vs longdouble %.1e" % (key, tol, err))
        assert err <= tol, key
    # the winner's record is the table's entry: the same walk twice
    assert np.array_equal(got["power"], got["table"][np.arange(len(got["power"])), got["candidate"]])


@pytest.mark.parametrize("n_lane", [1, 7, 64])
def test_the_winner_does_not_depend_on_the_lanes(harness, n_lane):
    d = O.main_input()
    f = d["f"][::40]
    a = run(harness, d["t"], d["y"], d["err"], d["inst"], f, d["ecc"], d["n_phase"], n_lane=n_lane)
    b = run(harness, d["t"], d["y"], d["err"], d["inst"], f, d["ecc"], d["n_phase"], n_lane=256)
    assert np.array_equal(a["candidate"], b["candidate"]) and np.array_equal(a["power"], b["power"])


def test_the_comparison_of_the_argmax(harness):
    def best(power, cand):
        power, cand = np.ascontiguousarray(power, dtype=np.float64), np.ascontiguousarray(cand, dtype=np.int32)
        return harness.harness_best(_p(power), _p(cand, _ip), power.size)

    assert best([1.0, 3.0, 2.0], [5, 6, 7]) == 6
    assert best([3.0, 3.0, 3.0], [9, 4, 6]) == 4 and best([3.0, 3.0, 3.0], [4, 9, 6]) == 4      # equal: the lowest number
    assert best([np.nan, 1.0, np.nan], [0, 8, 1]) == 8                                           # NaN never wins
    assert best([np.nan, np.nan], [0, 1]) == np.iinfo(np.int32).max
    assert best([-np.inf, -np.inf], [3, 2]) == 2


def test_zero_eccentricity_is_lomb_scargle(harness):
    d = O.main_input()
    tt, w, wy, _ = columns(d["t"], d["y"], d["err"], None)
    got = run(harness, d["t"], d["y"], d["err"], None, d["f"], [0.0], 1)
    ls = np.array([harness.harness_lomb_scargle(_p(tt), _p(w), _p(wy), tt.size, f) for f in d["f"]])
    args = (d["t"], d["y"], d["err"], None, d["f"], [0.0], 1)
    f64, ld = O.keplerian(*args), O.keplerian(*args, dtype=np.longdouble)
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    print("ecc = [0]: tolerance %.1e, core vs its Lomb-Scargle path %.1e, core vs longdouble %.1e"
          % (tol, O.rel_diff(got["power"], ls, peak), O.rel_diff(got["power"], ld["power"], peak)))
    assert O.rel_diff(got["power"], ls, peak) <= tol and O.rel_diff(got["power"], ld["power"], peak) <= tol
    assert np.all(got["candidate"] == 0)
    # ... and with 0 in the grid the periodogram is never below it
    _, _, full, _ = statements(inst=False)
    assert np.all(full["power"] >= f64["power"] - tol * peak)


def test_a_noise_free_orbit_on_the_grid_is_fitted_exactly(harness):
    d = O.main_input()
    P = 1 / d["f"][40]
    y = O.rv_model(d["t"], P, 0.6, 1.1, 30.0, d["t"].min() + 12 / 32 * P, (5.0, -12.0), d["inst"])
    got = run(harness, d["t"], y, None, d["inst"], d["f"][40:41], d["ecc"], 32)
    ld = O.keplerian(d["t"], y, None, d["inst"], d["f"][40:41], d["ecc"], 32, dtype=np.longdouble)
    half = 0.5 * float(ld["chi2_0"])
    print("chi2 / chi2_0 left: core %.1e, longdouble statement %.1e" % ((half - got["power"][0]) / half, (half - float(ld["power"][0])) / half))
    assert abs(half - got["power"][0]) <= 1e-10 * half and abs(half - float(ld["power"][0])) <= 1e-10 * half
    assert got["candidate"][0] == 6 * 32 + 12
    A, B = got["A"][0], got["B"][0]
    assert np.hypot(A, B) == pytest.approx(30.0, rel=1e-9) and np.arctan2(-B, A) == pytest.approx(1.1, rel=1e-9)
    assert got["const"][0] - 0.6 * A == pytest.approx([5.0, -12.0], rel=1e-9)


def test_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    f = [0.1, 0.2]
    for bad in ([0.0, 1.0], [-0.1], [0.5, np.nan], [], np.zeros((2, 2)), np.linspace(0, 0.9, 65)):
        with pytest.raises(ValueError, match="ecc"):
            E.keplerian_power(t, t, frequencies=f, ecc=bad)
    for bad in (0, -3, 2.5, 5000):
        with pytest.raises(ValueError, match="n_phase"):
            E.keplerian_power(t, t, frequencies=f, n_phase=bad)
    inst = np.arange(50) % 3
    with pytest.raises(ValueError, match="shape"):
        E.keplerian_power(t, t, frequencies=f, instrument=inst[:-1])
    with pytest.raises(ValueError, match="negative"):
        E.keplerian_power(t, t, frequencies=f, instrument=inst - 1)
    with pytest.raises(ValueError, match="at most 8"):
        E.keplerian_power(t, t, frequencies=f, instrument=np.arange(50) % 9)
    with pytest.raises(ValueError, match="gaps"):
        E.keplerian_power(t, t, frequencies=f, instrument=2 * inst)
    with pytest.raises(ValueError, match="integers"):
        E.keplerian_power(t, t, frequencies=f, instrument=inst + 0.5)
    # what is well formed gets as far as the device: there is no CPU fallback
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.keplerian_power(t, t, frequencies=f, instrument=torch.as_tensor(inst))
    order, off = E._instrument_segments(np.array([1, 0, 2, 0, 1, 1]), 6)
    assert list(order) == [1, 3, 0, 4, 5, 2] and list(off) == [0, 2, 5, 6] and off.dtype == np.int32
    assert E._instrument_segments(None, 6)[0] is None and list(E._instrument_segments(np.array([True, False]), 2)[1]) == [0, 1, 2]


def test_abi_of_the_entry_point():
    """argument checks on the host, before any launch; the workspace is sized by pure arithmetic"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    lib = _lib.load()
    INVALID, WORKSPACE = 1, 3
    assert lib.exo_keplerian_workspace_bytes(100, 1) == 8 * (3 * 100 + 16)
    assert lib.exo_keplerian_workspace_bytes(100, 5) == 8 * (100 + 2 * 5 * 100 + 5 * 16)
    assert lib.exo_keplerian_workspace_bytes(0, 1) == -1 and lib.exo_keplerian_workspace_bytes(100, 0) == -1
    off = (ctypes.c_int32 * 3)(0, 40, 100)
    ecc = (ctypes.c_double * 3)(0.0, 0.5, 0.9)
    names = ["t", "y", "yerr", "n_yerr", "n", "n_series", "off", "n_inst", "freq", "n_freq", "ecc", "n_ecc", "n_phase", "power",
             "cand", "coef", "ws", "ws_bytes", "stream"]
    ok = [8, 8, None, 0, 100, 1, ctypes.addressof(off), 2, 8, 5, ctypes.addressof(ecc), 3, 16, 8, 8, 8, 8, 1 << 20, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_keplerian_power_f64(*args)

    assert call(n_freq=0) == 0                                          # nothing to do
    one = (ctypes.c_double * 3)(0.0, 1.0, 0.5)
    nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.5)
    gap = (ctypes.c_int32 * 3)(0, 0, 100)
    short = (ctypes.c_int32 * 3)(0, 40, 99)
    late = (ctypes.c_int32 * 3)(1, 40, 100)
    for bad in (dict(t=None), dict(y=None), dict(n=0), dict(n_series=0), dict(n_yerr=1), dict(n_yerr=3, yerr=8), dict(off=None),
                dict(n_inst=0), dict(n_inst=9), dict(freq=None), dict(n_freq=-1), dict(ecc=None), dict(n_ecc=0), dict(n_ecc=65),
                dict(n_phase=0), dict(n_phase=4097), dict(power=None), dict(cand=None), dict(coef=None), dict(ws=None),
                dict(ecc=ctypes.addressof(one)), dict(ecc=ctypes.addressof(nan)), dict(off=ctypes.addressof(gap)),
                dict(off=ctypes.addressof(short)), dict(off=ctypes.addressof(late))):
        assert call(**bad) == INVALID, bad
    assert call(ws_bytes=8 * (3 * 100 + 16) - 1) == WORKSPACE
