"""GPU: the astrometric orbit search (csrc/exo_astrometric.hip) behind exoplanet_amd.estimators.astrometric_power and
astrometric_estimator against the numpy statement of DESIGN.md section 23 (tests/astrometric_oracle.py), by the rule of
DESIGN.md 9.5: what float64 costs the statement itself on a case's own input, relative to the peak, is the unit, and the kernel
gets 16 of them (floor 1e-13) on the power, on the four constants and on the positions they imply at the epochs; the winning
candidate is the statement's (tests/test_astrometric_host.py holds the statement to a gap of 100 tolerances on every input used
here, so no frequency is excused -- except with two epochs, where every candidate fits exactly).  Every check prints its figures
before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import astrometric_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

PARALLAX = 0.05


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def E():
    from exoplanet_amd import estimators

    return estimators


def _err(e):
    return dev(e) if isinstance(e, np.ndarray) else e


def run(s, f, ecc, n_phase, **kw):
    """astrometric_power(return_fit=True) -> host arrays under the statement's names"""
    power, fit = E().astrometric_power(dev(s["t"]), dev(s["rho"]), _err(s["rho_err"]), dev(s["theta"]), _err(s["theta_err"]),
                                       frequencies=f, ecc=ecc, n_phase=n_phase, return_fit=True, **kw)
    out = {k: v.cpu().numpy() for k, v in fit.items()}
    out["power"] = power.cpu().numpy()
    out["beta"] = np.stack([out[k] for k in ("TA", "TB", "TF", "TG")], -1)
    return out


def model_positions(s, f, r):
    """the positions the winners' constants imply at the epochs, (F, 2, N), by the statement's own Kepler solve (longdouble)"""
    out = np.full((len(f), 2, s["t"].size), np.nan, np.longdouble)
    for i in np.flatnonzero(r["candidate"] >= 0):
        out[i] = O.positions(s["t"], 1 / f[i], r["ecc"][i], r["t_periastron"][i], r["beta"][i], np.longdouble)
    return out


def check(name, s, f, got, f64, ld, winners=True):
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    err = O.rel_diff(got["power"], ld["power"], peak)
    same = got["candidate"] == ld["candidate"]
    print("%s: power f64 vs longdouble %.1e, tolerance %.1e, kernel vs longdouble %.1e; winners equal at %d of %d frequencies, "
          "smallest gap %.1e" % (name, O.rel_diff(f64["power"], ld["power"], peak), tol, err, same.sum(), same.size, ld["gap"].min()))
    assert err <= tol, name
    if winners:
        assert np.array_equal(got["candidate"], ld["candidate"]), name
    else:
        assert np.all(ld["gap"][~same] <= tol), name
    found = same & (ld["candidate"] >= 0)
    if not found.any():
        return tol
    scale = float(np.abs(ld["beta"][found]).max())
    t_b = O.tolerance(f64["beta"][found], ld["beta"][found], scale)
    e_b = O.rel_diff(got["beta"][found], ld["beta"][found], scale)
    # the positions: the kernel's constants and the float64 statement's, each through the longdouble Kepler solve
    want = model_positions(s, f, ld)[found]
    t_p = O.tolerance(model_positions(s, f, dict(f64, beta=f64["beta"].astype(np.longdouble)))[found], want, scale)
    e_p = O.rel_diff(model_positions(s, f, dict(ld, beta=got["beta"].astype(np.longdouble)))[found], want, scale)
    print("    constants: tolerance %.1e, kernel vs longdouble %.1e; positions at the epochs: tolerance %.1e, kernel %.1e"
          % (t_b, e_b, t_p, e_p))
    assert e_b <= t_b and e_p <= t_p, name
    assert np.array_equal(got["ecc"][found], ld["ecc"][found])
    assert np.all(np.abs(got["t_periastron"] - ld["t_periastron"])[found] <= 1e-14 * (1 + np.abs(ld["t_periastron"][found])))
    # (chi2 = chi2_0 - 2 power: twice the power's error, and the rounding of chi2_0, a sum of at most 257 positive terms in a tree)
    assert O.rel_diff(got["chi2"][found], ld["chi2"][found], float(ld["chi2_0"])) <= 2 * tol * peak / float(ld["chi2_0"]) + 1e-15
    return tol


def against_the_statement(name, s, f, ecc, n_phase, winners=True):
    f64, ld = O.statements(name, s, f, ecc, n_phase)
    got = run(s, f, ecc, n_phase)
    return got, f64, ld, check(name, s, f, got, f64, ld, winners)


# ---- 1: the main input ---------------------------------------------------------------------------------------------------------

def test_main_input_against_the_statement():
    d = O.main_input()
    got, f64, ld, tol = against_the_statement("main", d, d["f"], d["ecc"], d["n_phase"])
    assert ld["gap"].min() > 100 * tol
    i = int(np.argmax(got["power"]))
    assert i == int(np.argmax(ld["power"])) == int(np.argmin(np.abs(1 / d["f"] - 27.0))) and got["ecc"][i] == d["ecc"][6]
    a, incl, om, Om = O.campbell(got["beta"])                 # the record's elements are the conversion of its own constants
    for key, want in (("a_angular", a), ("incl", incl), ("omega", om), ("Omega", Om)):
        assert np.max(np.abs(got[key] - want)) <= 1e-12, key


# ---- 2: shapes where the kernel can go wrong ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [k for k in O.shapes() if k not in ("one epoch", "isotropic weights")])
def test_shapes(name):
    s, f, ecc, n_phase = O.shapes()[name]
    against_the_statement(name, s, f, ecc, n_phase, winners=name not in O.EXACT_FIT_ONLY)


def test_one_epoch_has_no_candidate():
    s, f, ecc, n_phase = O.shapes()["one epoch"]
    got = run(s, f, ecc, n_phase, parallax=PARALLAX)
    assert np.all(got["power"] == 0.0) and np.all(got["candidate"] == -1)
    for key in ("ecc", "t_periastron", "omega", "Omega", "incl", "a_angular", "a", "TA", "TB", "TF", "TG", "chi2"):
        assert np.all(np.isnan(got[key])), key


def test_isotropic_weights_are_two_independent_fits():
    s, f, ecc, n_phase = O.shapes()["isotropic weights"]
    got, f64, ld, tol = against_the_statement("isotropic weights", s, f, ecc, n_phase)
    x, y, w = s["rho"] * np.cos(s["theta"]), s["rho"] * np.sin(s["theta"]), 1 / s["rho_err"] ** 2
    power, cand = O.isotropic(s["t"], x, y, w, f, ecc, n_phase, dtype=np.longdouble)
    peak = float(power.max())
    p64, _ = O.isotropic(s["t"], x, y, w, f, ecc, n_phase)
    # (the weights are equal up to the rounding of rho_err / rho: the unit is what that and float64 cost the 4 x 4 statement)
    tol2 = max(tol, O.tolerance(p64, power, peak), O.tolerance(f64["power"], power, peak))
    print("isotropic: kernel vs the two 2 x 2 fits %.1e of the peak (tolerance %.1e)" % (O.rel_diff(got["power"], power, peak), tol2))
    assert O.rel_diff(got["power"], power, peak) <= tol2 and np.array_equal(got["candidate"], cand)


def test_error_shapes():
    """scalar, (N,) and (B, N) errors: a batch with per-series errors against its rows with per-epoch errors, bitwise"""
    d = O.main_input()
    rs = np.random.RandomState(3)
    n = d["t"].size
    rho, theta = d["rho"][None] + 0.01 * rs.randn(3, n), d["theta"][None] + 0.01 * rs.randn(3, n)
    re, te = d["rho_err"][None] * rs.uniform(0.8, 1.25, (3, n)), d["theta_err"][None] * rs.uniform(0.8, 1.25, (3, n))
    kw = dict(frequencies=d["f"][::5], ecc=d["ecc"], n_phase=32, return_fit=True)
    t = dev(d["t"])
    power, fit = E().astrometric_power(t, dev(rho), dev(re), dev(theta), dev(te), **kw)
    shared, fit_s = E().astrometric_power(t, dev(rho), dev(re[0]), dev(theta), 0.02, **kw)
    assert tuple(power.shape) == (3, 8) and tuple(fit["TA"].shape) == (3, 8)
    for b in range(3):
        p1, f1 = E().astrometric_power(t, dev(rho[b]), dev(re[b]), dev(theta[b]), dev(te[b]), **kw)
        assert torch.equal(p1, power[b]) and all(torch.equal(f1[k], fit[k][b]) for k in fit), b
        p2, f2 = E().astrometric_power(t, dev(rho[b]), dev(re[0]), dev(theta[b]), dev(np.full(n, 0.02)), **kw)
        assert torch.equal(p2, shared[b]) and all(torch.equal(f2[k], fit_s[k][b]) for k in fit_s), b
    for bad in (dev(re[:, :-1]), dev(re[:2])):
        with pytest.raises(ValueError, match="shape"):
            E().astrometric_power(t, dev(rho), bad, dev(theta), 0.02, **kw)
    with pytest.raises(ValueError, match="theta"):
        E().astrometric_power(t, dev(rho), 0.01, dev(theta[0]), 0.02, **kw)


# ---- 3: reproducibility ---------------------------------------------------------------------------------------------------------

def test_rows_of_a_batch_runs_and_a_far_origin():
    d = O.main_input()
    rs = np.random.RandomState(3)
    n = d["t"].size
    rho, theta = d["rho"][None] + 0.01 * rs.randn(5, n), d["theta"][None] + 0.01 * rs.randn(5, n)
    kw = dict(frequencies=d["f"][::4], ecc=d["ecc"], n_phase=32, return_fit=True)
    t, re, te = dev(d["t"]), dev(d["rho_err"]), dev(d["theta_err"])
    power, fit = E().astrometric_power(t, dev(rho), re, dev(theta), te, **kw)
    again, fit2 = E().astrometric_power(t, dev(rho), re, dev(theta), te, **kw)
    assert tuple(power.shape) == (5, 10)
    assert torch.equal(power, again) and all(torch.equal(fit[k], fit2[k]) for k in fit)
    for b in range(5):
        p1, f1 = E().astrometric_power(t, dev(rho[b]), re, dev(theta[b]), te, **kw)
        assert torch.equal(p1, power[b]) and all(torch.equal(f1[k], fit[k][b]) for k in fit), b
    # the same epochs counted from 2 457 000: t - t_min is formed first, so nothing but the time of periastron moves
    far = d["t"] + 2457000.0
    near = far - 2457000.0                                   # (what the far epochs hold of the near ones, exactly)
    p_far, fit_far = E().astrometric_power(dev(far), dev(d["rho"]), re, dev(d["theta"]), te, **kw)
    p_near, fit_near = E().astrometric_power(dev(near), dev(d["rho"]), re, dev(d["theta"]), te, **kw)
    assert torch.equal(p_far, p_near)
    assert all(torch.equal(fit_far[k], fit_near[k]) for k in fit_far if k != "t_periastron")
    assert float((fit_far["t_periastron"] - 2457000.0 - fit_near["t_periastron"]).abs().max()) <= 1e-9


# ---- 4: a noise-free orbit exactly on the grid ----------------------------------------------------------------------------------

def test_noise_free_orbit_on_the_grid():
    d = O.main_input()
    k, j, kp = 16, 6, 12
    P, e = 1 / d["f"][k], d["ecc"][j]
    tp = d["t"].min() + kp / 32 * P
    rho, theta = O.sky_model(d["t"], P, e, tp, 0.8, 1.0, 0.7, 2.2)
    s = dict(d, rho=rho, theta=theta)
    f = d["f"][k - 2:k + 3]
    f64, ld = O.statements("noise-free", s, f, d["ecc"], 32)
    got = run(s, f, d["ecc"], 32)
    half = 0.5 * float(ld["chi2_0"])
    left, left_ld = (half - got["power"][2]) / half, float((half - ld["power"][2]) / half)
    print("chi2 / chi2_0 left at the orbit's frequency: kernel %.1e, longdouble statement %.1e" % (left, left_ld))
    assert abs(left_ld) <= 1e-10 and abs(left) <= 1e-10
    assert got["candidate"][2] == j * 32 + kp == ld["candidate"][2]
    assert got["ecc"][2] == e and got["t_periastron"][2] == pytest.approx(tp, rel=1e-15)
    errs = [abs(got["a_angular"][2] - 0.8), abs(got["incl"][2] - 1.0), abs(got["omega"][2] - 0.7), abs(got["Omega"][2] - 2.2)]
    print("a_angular, incl, omega, Omega off the truth by %.1e, %.1e, %.1e, %.1e" % tuple(errs))
    assert max(errs) <= 1e-9
    # (at the neighbouring frequencies the fit is an ordinary one: the statement's rule)
    check("noise-free", s, f, got, f64, ld, winners=False)


# ---- 5: the convention, end to end ----------------------------------------------------------------------------------------------

def test_elements_go_straight_into_the_orbit_and_the_likelihood():
    import exoplanet_amd as xo

    d = O.main_input()
    f64, ld = O.statements("main", d, d["f"], d["ecc"], d["n_phase"])
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    scale = float(np.abs(ld["beta"]).max())
    tol_b = O.tolerance(f64["beta"], ld["beta"], scale)
    col = O.columns(d["rho"], d["rho_err"], d["theta"], d["theta_err"], np.longdouble)
    t = dev(d["t"])
    power, fit = E().astrometric_power(t, dev(d["rho"]), dev(d["rho_err"]), dev(d["theta"]), dev(d["theta_err"]), frequencies=d["f"],
                                       ecc=d["ecc"], n_phase=32, parallax=PARALLAX, return_fit=True)
    from exoplanet_amd.orbits.constants import au_per_R_sun

    assert torch.equal(fit["a"], fit["a_angular"] / (PARALLAX * au_per_R_sun)) and au_per_R_sun == pytest.approx(O.AU_PER_R_SUN, rel=1e-12)
    for i in (int(np.argmax(ld["power"])), 3, 33):
        one = lambda key: fit[key][i].reshape(1)                                                    # noqa: E731
        orbit = xo.KeplerianOrbit(period=1 / dev(d["f"][i:i + 1]), t_periastron=one("t_periastron"), ecc=one("ecc"),
                                  omega=one("omega"), Omega=one("Omega"), incl=one("incl"), a=one("a"))
        X, Y, _ = orbit.get_relative_position(t, PARALLAX)
        X, Y = X.reshape(-1).cpu().numpy(), Y.reshape(-1).cpu().numpy()
        beta = np.array([float(fit[key][i]) for key in ("TA", "TB", "TF", "TG")], dtype=np.longdouble)
        wx, wy = O.positions(d["t"], 1 / d["f"][i], float(fit["ecc"][i]), float(fit["t_periastron"][i]), beta, np.longdouble)
        a_ang = float(fit["a_angular"][i])
        e_pos = max(O.rel_diff(X, wx, a_ang), O.rel_diff(Y, wy, a_ang))
        chi2 = O.chi2_of(col, X, Y)
        want = float(ld["chi2_0"]) - 2 * float(power[i])
        ll = orbit.astrometry_log_likelihood(t, dev(d["rho"]), dev(d["rho_err"]), dev(d["theta"]), dev(d["theta_err"]),
                                             parallax=PARALLAX)
        chi2_ll = -2 * float(ll) - float(np.log(2 * np.pi * d["rho_err"] ** 2).sum() + np.log(2 * np.pi * d["theta_err"] ** 2).sum())
        print("frequency %d: the orbit's positions against TA xi + TF eta, TB xi + TG eta: %.1e of a_angular (tolerance %.1e); "
              "their chi2 %.12g against chi2_0 - 2 power %.12g: %.1e of the peak (tolerance %.1e); the unlinearised "
              "-2 log L less its constant: %.12g" % (i, e_pos, tol_b, chi2, want, abs(chi2 - want) / (2 * peak), tol, chi2_ll))
        assert e_pos <= tol_b and abs(chi2 - want) <= 2 * tol * peak


# ---- 6: the estimator -----------------------------------------------------------------------------------------------------------

def test_astrometric_estimator_on_the_main_input():
    d = O.main_input()
    periods = 1 / d["f"]
    res = E().astrometric_estimator(d["t"], d["rho"], d["rho_err"], d["theta"], d["theta_err"], periods=periods, n_phase=32,
                                    parallax=PARALLAX)
    freq, power = res["periodogram"]
    _, ld = O.statements("main", d, d["f"], d["ecc"], d["n_phase"])
    peak = res["peaks"][0]
    print("first peak:", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in peak.items()})
    assert np.array_equal(freq, 1 / periods) and power.shape == freq.shape
    assert peak["period"] == periods[int(np.argmin(np.abs(periods - 27.0)))]
    for key in ("period", "ecc", "t_periastron", "omega", "Omega", "incl", "a_angular", "a", "chi2", "power"):
        assert type(peak[key]) is float, key
    i = peak["index"] - 1
    assert i == int(np.argmax(ld["power"])) and peak["power"] == power[i] and peak["ecc"] == float(ld["ecc"][i])
    # the default grid: 1 / (4 baseline) to N / (4 baseline), ten samples per peak
    res = E().astrometric_estimator(d["t"], d["rho"], d["rho_err"], d["theta"], d["theta_err"], n_phase=16, ecc=[0.0, 0.3, 0.6])
    T = d["t"].max() - d["t"].min()
    want = E().lomb_scargle_autofrequency(d["t"], samples_per_peak=10, minimum_frequency=1 / (4 * T), maximum_frequency=30 / (4 * T))
    assert np.array_equal(res["periodogram"][0], want) and "a" not in res["peaks"][0]
    f64 = O.statement(d, want, [0.0, 0.3, 0.6], 16)
    assert res["peaks"][0]["index"] - 1 == int(np.argmax(f64["power"])) and res["peaks"][0]["period"] == 1 / want[int(np.argmax(f64["power"]))]
