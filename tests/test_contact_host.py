"""CPU: first / fourth contact and the in-transit windows against the multiprecision fixture tests/golden/contact_mp.npz
(tools/make_contact_golden.py; definition and allowances: tests/contact_cases.py).  Three implementations are held to it:
oracle.numpy_port.contact_points (80-step bisection on libm), exo::contact_solve of exoplanet_amd/csrc/exo_contact.hpp
compiled for the host (tests/contact_harness.cpp: the fast path in sin theta and the Illinois fallback, the lines the
kernels run), and the numpy glue oracle.numpy_port.KeplerianOrbit.in_transit.  Flags exactly, values within the allowance,
the left and right roots on their sides of the conjunction; every test prints worst error / allowance before it asserts.
The kernels themselves: tests/test_gpu_contact.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import contact_cases as K
from oracle import numpy_port as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "contact_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "contact_harness.cpp")] + [os.path.join(csrc, h) for h in ("exo_contact.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.contact_harness.restype = None
    lib.contact_harness.argtypes = [_dp, ctypes.c_int64, _dp, _dp, ctypes.POINTER(ctypes.c_int32)]
    return lib


@pytest.fixture(scope="module")
def g():
    return K.load()


def conjunction_M(inp):
    """mean anomaly of the conjunction f_c = pi/2 - omega, E on the branch continuous with f (float64)"""
    e, cw, sw = inp[:, 1], inp[:, 2], inp[:, 3]
    f = 0.5 * np.pi - np.arctan2(sw, cw)
    E = 2 * np.arctan2(np.sqrt(1 - e) * np.sin(0.5 * f), np.sqrt(1 + e) * np.cos(0.5 * f))
    return E - e * np.sin(E)


def hold(label, g, Ml, Mr, flag, c=None):
    """flags equal; values of every entry with contacts within the allowance; roots on their sides.  Returns worst ratio."""
    assert np.array_equal(flag != 0, g["flag"] != 0), [K.NAMES[i] for i in np.nonzero((flag != 0) != (g["flag"] != 0))[0]]
    ok = K.has_contacts(g)
    got = np.stack([Ml, Mr], axis=-1)
    tol = K.allow_M(g, c)
    assert np.all(np.isfinite(tol[ok])) and np.all(tol[ok] > 0)
    ratio = np.abs(got - g["M"])[ok] / tol[ok]
    k = int(np.argmax(ratio.max(axis=1)))
    K.report(label, entries=ok.sum(), worst_error_over_allowance=ratio, worst_error=np.abs(got - g["M"])[ok], worst_allowance=tol[ok])
    print("   worst entry:", np.array(K.NAMES)[ok][k])
    Mc = conjunction_M(g["inputs"])
    assert np.all(Ml[ok] < Mc[ok]) and np.all(Mc[ok] < Mr[ok])
    assert np.all(got[~ok] == 0.0)
    return float(ratio.max())


def run_harness(lib, inp):
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    n = inp.shape[0]
    Ml, Mr, fl = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
    lib.contact_harness(inp.ctypes.data_as(_dp), n, Ml.ctypes.data_as(_dp), Mr.ctypes.data_as(_dp),
                        fl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return Ml, Mr, fl


def test_fixture_conditions(g):
    """what the fixture must contain, as conditions: the counts, the margins of the flags, every group, both sides of every
    acceptance rule of the fast path, and the path each entry is built for"""
    ok = K.has_contacts(g)
    assert ok.sum() >= 150 and (~ok).sum() >= 20
    assert np.all(g["margin"][~ok] > 1e-9)
    assert np.array_equal(g["ctor"], np.array([K.ctor_inputs(c) for c in K.CASES]))
    assert np.array_equal(g["inputs"], np.array([K.contact_inputs(ct) for ct in g["ctor"]]))
    e, aor, w = g["inputs"][:, 1], g["inputs"][:, 0] / g["ctor"][:, 7], g["ctor"][:, 4]
    ror = g["ctor"][:, 5] / g["ctor"][:, 7]
    for ecc in (0.0, 0.3, 0.9, 0.95, 0.99, 0.995, 0.999):
        for q in K.QUADRANTS + (1.1,):
            assert np.any(ok & (e == ecc) & (w == q)), (ecc, q)
    assert aor[ok].min() < 1.6 and aor[ok].max() >= 500 and ror[ok].min() <= 1e-3 and ror[ok].max() >= 1.2
    assert np.any(ok & (g["inputs"][:, 4] == 0.0)) and np.any(ok & (g["ctor"][:, 2] == 1e-9))
    assert np.any(ok & (g["ctor"][:, 1] > 2.4e6)) and np.any(ok & (np.abs(g["ctor"][:, 1]) < 1))
    assert (np.isfinite(g["win"][:, 2]) & (g["sec"] == 1)).sum() >= 20 and int(g["fallback"].sum()) == 0
    circ = g["circular"] == 1
    assert np.any(circ & np.isfinite(g["circ_hdur"])) and np.any(circ & (g["circ_arg"] < 0)) and np.any(circ & (g["circ_x"] > 1))
    # occultation nearly as long as the period (the nearest thing to the boundary fallback)
    assert np.nanmax((g["win"][:, 3] - g["win"][:, 2]) / g["ctor"][:, 0]) > 0.99
    paths = [K.fast_path(inp) for inp in g["inputs"]]
    seen = set()
    for c, p, has in zip(K.CASES, paths, ok):
        if has:
            seen.update(p)
            if c["path"] == "fast":
                assert p == ("fast", "fast"), (c["name"], p)
            elif c["path"] == "bracket":
                assert "fast" not in p, (c["name"], p)
    print("paths of the entries with contacts:", {k: sum(pp.count(k) for pp, has in zip(paths, ok) if has) for k in sorted(seen)})
    # (no geometry is known that the three sign probes reject: 300 000 random ones with periastron at 1.02 to 3 L, e from 0.3
    # to 0.97, have no converged Newton root that is not the nearest -- DESIGN.md section 2)
    assert {"fast", "S", "wide", "newton", "converge"} <= seen, seen
    # both sides of |sin theta| <= 0.5 lie close to it
    s = np.sin(g["theta"])
    assert np.any(ok[:, None] & (np.abs(s) > 0.5) & (np.abs(s) < 0.52)) and np.any(ok[:, None] & (np.abs(s) < 0.5) & (np.abs(s) > 0.48))


def test_numpy_oracle(g):
    """the oracle sets the allowance's constant (C = 4 x its worst ratio at C = 1, contact_cases.ORACLE_WORST): the measured
    ratio may not exceed the recorded one, or the constant is stale"""
    inp = g["inputs"]
    Ml, Mr, fl = P.contact_points(*[inp[:, k] for k in range(7)])
    ok = K.has_contacts(g)
    ratio1 = (np.abs(np.stack([Ml, Mr], -1) - g["M"])[ok] / K.allow_M(g, 1.0)[ok]).max()
    print(f"numpy_port.contact_points: worst error / allowance at C = 1: {ratio1:.3g} (contact_cases.ORACLE_WORST = {K.ORACLE_WORST})")
    assert 0.5 * K.ORACLE_WORST <= ratio1 <= K.ORACLE_WORST
    assert hold("numpy_port.contact_points", g, Ml, Mr, fl) <= 0.25 + 1e-12


def test_host_build_of_contact_solve(harness, g):
    Ml, Mr, fl = run_harness(harness, g["inputs"])
    assert hold("exo::contact_solve (host build)", g, Ml, Mr, fl) <= 1.0
    # one entry at a time and in reverse order: no state between calls
    Ml2, Mr2, fl2 = run_harness(harness, g["inputs"][::-1])
    assert np.array_equal(Ml2[::-1], Ml) and np.array_equal(Mr2[::-1], Mr) and np.array_equal(fl2[::-1], fl)


def numpy_orbit(g, i):
    P_, t0, b, e, w, r, ms, rs, mpl, sbr = g["ctor"][i]
    kw = dict(period=P_, t0=t0, b=b, m_star=ms, r_star=rs)
    if not g["circular"][i]:
        kw.update(ecc=e, omega=w)
    return P.KeplerianOrbit(**kw), r


@pytest.mark.parametrize("texp", [None, 0.02])
def test_numpy_in_transit_glue(g, texp):
    """oracle.numpy_port.KeplerianOrbit.in_transit (the reference's glue: wrap rules, exposure padding) on the cadences the
    generator placed either side of every contact: the index set of the mp contacts, for the cadences at least 10 allowances
    from a contact -- which excludes none of them"""
    n_ent = excluded = 0
    worst = 0.0
    for i in range(len(K.CASES)):
        t = g["cad_t"][i]
        if not np.isfinite(t[0]):
            continue
        orbit, r = numpy_orbit(g, i)
        got = np.zeros(K.N_CAD, dtype=bool)
        got[orbit.in_transit(t, r=r, texp=texp)] = True
        tr = g["cad_in"][i] == 1          # in_transit knows the transit only
        edge = cad_edge_distance(g, i, transit_only=True)
        h = 0.0 if texp is None else 0.5 * texp
        want = edge > -h                  # signed: + inside the transit window
        tol = K.allow_cadence(g, i, t)
        clear = np.abs(edge + h) >= 10 * tol
        excluded += int((~clear).sum())
        worst = max(worst, float((tol / np.abs(edge + h)).max()))
        assert np.array_equal(got[clear], want[clear]), (K.NAMES[i], np.nonzero(got != want)[0])
        assert texp is not None or np.array_equal(want, tr)
        n_ent += 1
    K.report(f"in_transit(texp={texp})", entries=n_ent, excluded=excluded, worst_allowance_over_distance=worst)
    assert n_ent >= 150 and excluded == 0


def cad_edge_distance(g, i, transit_only=False):
    """signed distance (days) of entry i's cadences to the nearest transit contact: + inside the window"""
    P_, t0 = g["ctor"][i, 0], g["ctor"][i, 1]
    win = g["circ_win"][i] if g["circular"][i] else g["win"][i]
    dt = np.mod(g["cad_t"][i] - t0 + 0.5 * P_, P_) - 0.5 * P_
    return np.minimum(dt - win[0], win[1] - dt)
