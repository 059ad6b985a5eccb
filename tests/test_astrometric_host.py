"""CPU: the arithmetic of the astrometric orbit search, exoplanet_amd/csrc/exo_astrometric_core.hpp compiled for the host
(tests/astrometric_harness.cpp), against the numpy statement of DESIGN.md section 23 (tests/astrometric_oracle.py); the
conditions the statement itself has to meet on every fixed input before a kernel is judged by it; and the argument errors of
exoplanet_amd.estimators.astrometric_power that need no device.  The kernel itself: tests/test_gpu_astrometric.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import astrometric_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_i32, _f64 = ctypes.c_int32, ctypes.c_double


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "astrometric_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "astrometric_harness.cpp"), os.path.join(ROOT, "tests", "orbit_lanes.hpp")] + [
        os.path.join(csrc, h) for h in ("exo_astrometric_core.hpp", "exo_orbit_search.hpp", "exo_estimators_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_astrometric.argtypes = [_dp] * 6 + [_i32, _f64, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp]
    lib.harness_campbell.argtypes = [_dp, ctypes.c_int, _dp]
    return lib


def _p(a):
    return a.ctypes.data_as(_dp)


def run(harness, s, freq, ecc, n_phase, n_lane=256):
    """the columns the preparation kernel hands the search (here from the float64 statement), then the core header"""
    col = O.columns(s["rho"], s["rho_err"], s["theta"], s["theta_err"], np.float64)
    c = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    tt = c(s["t"] - s["t"].min())
    cols = [c(col[k]) for k in ("pxx", "pxy", "pyy", "qx", "qy")]
    ecc = c(ecc)
    C = ecc.size * n_phase
    table, pivot, record = np.empty((len(freq), C)), np.empty((len(freq), C)), np.empty((len(freq), 10))
    for i, f in enumerate(freq):
        harness.harness_astrometric(_p(tt), *[_p(a) for a in cols], tt.size, f, _p(ecc), ecc.size, n_phase, n_lane, _p(table[i]),
                                    _p(pivot[i]), _p(record[i]))
    return dict(table=table, pivot=pivot, power=record[:, 0], candidate=record[:, 1].astype(np.int64), beta=record[:, 2:6],
                a_angular=record[:, 6], incl=record[:, 7], omega=record[:, 8], Omega=record[:, 9])


def main_statements():
    d = O.main_input()
    return (d,) + O.statements("main", d, d["f"], d["ecc"], d["n_phase"])


def test_the_main_input_is_the_one_described():
    """what DESIGN.md 23.4 records of this input, measured on the statement itself"""
    d, f64, ld = main_statements()
    live = np.isfinite(ld["table"])
    peak = float(ld["power"].max())
    print("float64 against longdouble over all candidates: %.1e of the peak; winners equal at %d of %d periods; smallest gap "
          "between the best and the second-best candidate: %.1e of the peak"
          % (O.rel_diff(f64["table"][live], ld["table"][live], peak), (f64["candidate"] == ld["candidate"]).sum(), d["f"].size,
             ld["gap"].min()))
    assert d["f"].size == 40 and int(np.isfinite(f64["pivot"][0]).sum()) == 289
    assert np.array_equal(np.isfinite(f64["table"]), live)                     # none live in one arithmetic and dead in the other
    assert np.array_equal(f64["candidate"], ld["candidate"])
    i = int(np.argmax(ld["power"]))
    print("best period %.2f: ecc %.2f, a_angular %.3f, incl %.3f, omega %.3f, Omega %.3f, t_periastron %.3f"
          % (1 / d["f"][i], ld["ecc"][i], ld["a_angular"][i], ld["incl"][i], ld["omega"][i], ld["Omega"][i], ld["t_periastron"][i]))
    assert i == int(np.argmin(np.abs(1 / d["f"] - O.MAIN["period"]))) and ld["ecc"][i] == pytest.approx(0.6)
    assert abs(ld["a_angular"][i] - 0.8) < 0.1 and abs(ld["incl"][i] - 1.0) < 0.2
    assert abs(ld["omega"][i] - 0.7) < 0.2 and abs(ld["Omega"][i] - 2.2) < 0.1


FIXED = ["main"] + list(O.shapes())


@pytest.mark.parametrize("name", FIXED)
def test_the_statement_meets_its_own_conditions(name):
    """Before any kernel is judged: on every fixed input the statement's gap between the best and the second-best candidate
    exceeds 100 tolerances at every frequency (so that no frequency is excused from the winner check -- except where four
    equations meet four unknowns and all candidates tie), no candidate's smallest squared pivot lies within a factor 2 of the
    floor, and none is a candidate in one arithmetic and not in the other."""
    if name == "main":
        d, f64, ld = main_statements()
    else:
        s, f, ecc, n_phase = O.shapes()[name]
        f64, ld = O.statements(name, s, f, ecc, n_phase)
    piv = ld["pivot"][np.isfinite(ld["pivot"])].astype(np.float64)
    piv64 = f64["pivot"][np.isfinite(f64["pivot"])]
    near = lambda p: (p >= 0.5 * O.PIVOT_FLOOR) & (p <= 2 * O.PIVOT_FLOOR)  # noqa: E731
    live = np.isfinite(ld["table"])
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak) if peak > 0 else 1e-13
    print("%s: %d of %d candidates live, smallest squared pivot of a live one %.1e, largest of a dead one %.1e; tolerance %.1e, "
          "smallest gap %.1e" % (name, live.sum(), live.size, piv[piv >= O.PIVOT_FLOOR].min() if live.any() else np.nan,
                                 piv[piv < O.PIVOT_FLOOR].max() if (piv < O.PIVOT_FLOOR).any() else np.nan, tol, ld["gap"].min()))
    assert not near(piv).any() and not near(piv64).any()
    assert np.array_equal(np.isfinite(f64["table"]), live)
    assert np.array_equal(f64["candidate"], ld["candidate"]) or name in O.EXACT_FIT_ONLY
    if name not in O.EXACT_FIT_ONLY:
        assert np.all(ld["gap"] > 100 * tol)


def test_powers_winners_and_records_against_the_statement(harness):
    d, f64, ld = main_statements()
    got = run(harness, d, d["f"], d["ecc"], d["n_phase"])
    peak = float(ld["power"].max())
    live = np.isfinite(ld["table"])
    assert np.array_equal(np.isfinite(got["table"]), live)
    tol = O.tolerance(f64["table"][live], ld["table"][live], peak)
    err = O.rel_diff(got["table"][live], ld["table"][live], peak)
    print("every live candidate's power: f64 vs longdouble %.1e, tolerance %.1e, core vs longdouble %.1e"
          % (O.rel_diff(f64["table"][live], ld["table"][live], peak), tol, err))
    assert err <= tol
    assert np.array_equal(got["candidate"], ld["candidate"])
    scale = float(np.abs(ld["beta"]).max())
    for key, sc in (("power", peak), ("beta", scale)):
        t_k, e_k = O.tolerance(f64[key], ld[key], sc), O.rel_diff(got[key], ld[key], sc)
        print("%s: tolerance %.1e, core vs longdouble %.1e" % (key, t_k, e_k))
        assert e_k <= t_k, key
    # the elements of the record are the conversion of its own constants, and the record's power is the table's entry
    a, incl, om, Om = O.campbell(got["beta"])
    for key, want in (("a_angular", a), ("incl", incl), ("omega", om), ("Omega", Om)):
        assert np.max(np.abs(got[key] - want)) <= 1e-12, key
    assert np.array_equal(got["power"], got["table"][np.arange(len(got["power"])), got["candidate"]])
    # the pivots: the same side of the floor as the statement's, candidate by candidate
    assert np.array_equal(got["pivot"] >= O.PIVOT_FLOOR, ld["pivot"] >= O.PIVOT_FLOOR)


@pytest.mark.parametrize("n_lane", [1, 7, 64])
def test_the_winner_does_not_depend_on_the_lanes(harness, n_lane):
    d = O.main_input()
    f = d["f"][::8]
    a = run(harness, d, f, d["ecc"], d["n_phase"], n_lane=n_lane)
    b = run(harness, d, f, d["ecc"], d["n_phase"], n_lane=256)
    assert np.array_equal(a["candidate"], b["candidate"]) and np.array_equal(a["power"], b["power"])


def test_one_and_two_epochs(harness):
    """one epoch: two equations for four unknowns, no candidate anywhere -- power 0, candidate -1, NaN; two epochs: every
    well-conditioned candidate fits exactly"""
    s, f, ecc, n_phase = O.shapes()["one epoch"]
    got = run(harness, s, f, ecc, n_phase)
    assert np.all(got["power"] == 0.0) and np.all(got["candidate"] == -1) and np.all(np.isnan(got["beta"]))
    assert np.all(np.isnan(got["a_angular"])) and not np.isfinite(got["table"]).any()
    s, f, ecc, n_phase = O.shapes()["two epochs"]
    got = run(harness, s, f, ecc, n_phase)
    _, ld = O.statements("two epochs", s, f, ecc, n_phase)
    half = 0.5 * float(ld["chi2_0"])
    live = np.isfinite(ld["table"])
    assert live.any() and np.array_equal(np.isfinite(got["table"]), live)
    print("two epochs: chi2 left of chi2_0, worst live candidate: %.1e" % np.max(np.abs(half - got["table"][live]) / half))
    assert np.max(np.abs(half - got["table"][live])) <= 1e-10 * half


def test_the_campbell_conversion_round_trip(harness):
    """Elements -> constants by the statement's rotation, -> elements by the core, -> constants again.  The conversion loses
    digits towards face-on orbits: k^2 - m^2 = a^4 sin^4(i) / 4 is the difference of two numbers of size a^4, so a_angular^2 =
    j + k carries an error of order eps a^2 / sin^2 i and incl = acos(m / a^2) one of order eps / sin^3 i.  The bound is 64 eps
    / sin^3 i of a_angular on every constant, on inclinations at least 0.2 rad from 0 and pi."""
    rs = np.random.RandomState(23)
    n = 2000
    a, incl = rs.uniform(0.1, 3.0, n), rs.uniform(0.2, np.pi - 0.2, n)
    om, Om = rs.uniform(-np.pi, np.pi, n), rs.uniform(0, np.pi, n)
    beta = np.ascontiguousarray(O.thiele_innes(a, incl, om, Om))
    out = np.empty((n, 4))
    harness.harness_campbell(_p(beta), n, _p(out))
    back = O.thiele_innes(*out.T, dtype=np.longdouble)
    err = np.max(np.abs(back - beta), axis=1) / a
    bound = 64 * np.finfo(np.float64).eps / np.sin(incl) ** 3
    print("round trip over %d orientations: worst %.1e of a_angular (its bound %.1e), worst ratio to the bound %.2f"
          % (n, err.max(), bound[np.argmax(err)], np.max(err / bound)))
    assert np.all(err <= bound)
    assert np.all((out[:, 3] >= 0) & (out[:, 3] < np.pi)) and np.all((out[:, 2] > -np.pi) & (out[:, 2] <= np.pi))
    # away from the ambiguity the elements themselves come back: Omega was drawn in [0, pi)
    wrap = lambda x: (x + np.pi) % (2 * np.pi) - np.pi  # noqa: E731
    assert np.max(np.abs(out[:, 0] - a) / a) <= bound.max() and np.max(np.abs(out[:, 1] - incl)) <= bound.max()
    inner = (Om > 1e-6) & (Om < np.pi - 1e-6)
    assert np.max(np.abs(wrap(out[:, 2] - om))[inner]) <= 4 * bound.max() and np.max(np.abs(out[:, 3] - Om)[inner]) <= 4 * bound.max()
    # the statement's own conversion is the same function
    a2, i2, om2, Om2 = O.campbell(beta)
    assert np.max(np.abs(out - np.stack([a2, i2, om2, Om2], 1))) <= 4 * bound.max()


def test_a_noise_free_orbit_on_the_grid_is_fitted_exactly(harness):
    d = O.main_input()
    k, j, kp = 16, 6, 12
    P, e = 1 / d["f"][k], d["ecc"][j]
    tp = d["t"].min() + kp / 32 * P
    rho, theta = O.sky_model(d["t"], P, e, tp, 0.8, 1.0, 0.7, 2.2)
    s = dict(d, rho=rho, theta=theta)
    got = run(harness, s, d["f"][k:k + 1], d["ecc"], 32)
    ld = O.statement(s, d["f"][k:k + 1], d["ecc"], 32, dtype=np.longdouble)
    half = 0.5 * float(ld["chi2_0"])
    print("chi2 / chi2_0 left: core %.1e, longdouble statement %.1e" % ((half - got["power"][0]) / half, (half - float(ld["power"][0])) / half))
    assert abs(half - got["power"][0]) <= 1e-10 * half and abs(half - float(ld["power"][0])) <= 1e-10 * half
    assert got["candidate"][0] == j * 32 + kp == ld["candidate"][0]
    errs = [abs(got["a_angular"][0] - 0.8), abs(got["incl"][0] - 1.0), abs(got["omega"][0] - 0.7), abs(got["Omega"][0] - 2.2)]
    print("a_angular, incl, omega, Omega off the truth by %.1e, %.1e, %.1e, %.1e" % tuple(errs))
    assert max(errs) <= 1e-9


def test_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    f = [0.1, 0.2]
    for bad in ([0.0, 1.0], [-0.1], [0.5, np.nan], [], np.zeros((2, 2)), np.linspace(0, 0.9, 65)):
        with pytest.raises(ValueError, match="ecc"):
            E.astrometric_power(t, t, 0.01, t, 0.01, frequencies=f, ecc=bad)
    for bad in (0, -3, 2.5, 5000):
        with pytest.raises(ValueError, match="n_phase"):
            E.astrometric_power(t, t, 0.01, t, 0.01, frequencies=f, n_phase=bad)
    # what is well formed gets as far as the device: there is no CPU fallback
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.astrometric_power(t, t, 0.01, t, 0.01, frequencies=f)
    with pytest.raises(ValueError, match="required"):
        E._astrometric_error("rho_err", None, (1, 50), "cpu")
    assert "astrometric_power" in E.__all__ and "astrometric_estimator" in E.__all__
    with pytest.raises(ValueError, match="descending"):
        E.astrometric_estimator(t, t, 0.01, t, 0.01, periods=[10.0, 20.0, 30.0])


def test_abi_of_the_entry_point():
    """argument checks on the host, before any launch; the workspace is sized by pure arithmetic"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    lib = _lib.load()
    INVALID, WORKSPACE = 1, 3
    assert lib.exo_astrometric_workspace_bytes(100, 1) == 8 * (6 * 100 + 2)
    assert lib.exo_astrometric_workspace_bytes(100, 5) == 8 * (100 + 5 * 5 * 100 + 1 + 5)
    assert lib.exo_astrometric_workspace_bytes(0, 1) == -1 and lib.exo_astrometric_workspace_bytes(100, 0) == -1
    ecc = (ctypes.c_double * 3)(0.0, 0.5, 0.9)
    names = ["t", "rho", "rho_err", "n_rho_err", "theta", "theta_err", "n_theta_err", "n", "n_series", "freq", "n_freq", "ecc",
             "n_ecc", "n_phase", "power", "cand", "coef", "ws", "ws_bytes", "stream"]
    ok = [8, 8, 8, 1, 8, 8, 1, 100, 1, 8, 5, ctypes.addressof(ecc), 3, 16, 8, 8, 8, 8, 1 << 20, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_astrometric_power_f64(*args)

    assert call(n_freq=0) == 0                                          # nothing to do
    one = (ctypes.c_double * 3)(0.0, 1.0, 0.5)
    nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.5)
    for bad in (dict(t=None), dict(rho=None), dict(rho_err=None), dict(theta=None), dict(theta_err=None), dict(n=0),
                dict(n_series=0), dict(n_rho_err=0), dict(n_rho_err=3), dict(n_theta_err=0), dict(n_theta_err=2), dict(freq=None),
                dict(n_freq=-1), dict(ecc=None), dict(n_ecc=0), dict(n_ecc=65), dict(n_phase=0), dict(n_phase=4097),
                dict(power=None), dict(cand=None), dict(coef=None), dict(ws=None), dict(ecc=ctypes.addressof(one)),
                dict(ecc=ctypes.addressof(nan))):
        assert call(**bad) == INVALID, bad
    assert call(ws_bytes=8 * (6 * 100 + 2) - 1) == WORKSPACE
