"""GPU: the Keplerian periodogram (csrc/exo_keplerian.hip) behind exoplanet_amd.estimators.keplerian_power and
keplerian_estimator against the numpy statement of DESIGN.md section 22 (tests/keplerian_oracle.py), by the rule of DESIGN.md
9.5: what float64 costs the statement itself on a case's own input, relative to the peak, is the unit, and the kernel gets 16
of them (floor 1e-13) on the power, on A, B and the constants; the winning candidate is exact.  Every check prints its figures
before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keplerian_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256            # epochs staged in LDS at a time (csrc/exo_keplerian.hip, kTile)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def E():
    from exoplanet_amd import estimators

    return estimators


def run(t, y, yerr, inst, f, ecc, n_phase):
    """keplerian_power(return_fit=True) -> host arrays under the statement's names (A, B and the constants from the elements)"""
    yerr = dev(yerr) if isinstance(yerr, np.ndarray) else yerr
    power, fit = E().keplerian_power(dev(t), dev(y), yerr, frequencies=f, ecc=ecc, n_phase=n_phase, instrument=inst, return_fit=True)
    out = {k: v.cpu().numpy() for k, v in fit.items()}
    out["power"] = power.cpu().numpy()
    out["A"], out["B"] = out["K"] * np.cos(out["omega"]), -out["K"] * np.sin(out["omega"])
    out["const"] = out["zero_point"] + (out["ecc"] * out["A"])[..., None]
    return out


def statements(key, *args):
    return O.cached((key, "f64"), lambda: O.keplerian(*args)), O.cached((key, "ld"), lambda: O.keplerian(*args, dtype=np.longdouble))


def check(name, got, f64, ld, exact=False):
    """power everywhere; the winner where the statement has one (`exact`: everywhere -- else a frequency at which the kernel
    names another candidate must be a tie within the tolerance in the statement itself); A, B, the constants and the elements
    where the winners agree"""
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    err = O.rel_diff(got["power"], ld["power"], peak)
    cand = got["candidate"]
    same = cand == ld["candidate"]
    print("%s: power f64 vs longdouble %.1e, tolerance %.1e, kernel vs longdouble %.1e; winners equal at %d of %d frequencies, "
          "smallest gap %.1e" % (name, O.rel_diff(f64["power"], ld["power"], peak), tol, err, same.sum(), same.size, ld["gap"].min()))
    assert err <= tol, name
    if exact:
        assert np.array_equal(cand, ld["candidate"]), name
    assert np.all(ld["gap"][~same] <= tol), (name, cand[~same], ld["candidate"][~same])
    if not same.any():                                       # (three epochs: every candidate fits them exactly, all tie)
        return tol
    for key in ("A", "B", "const", "K", "zero_point"):
        scale = float(np.abs(ld[key]).max())
        t_k = O.tolerance(f64[key][same], ld[key][same], scale)
        e_k = O.rel_diff(got[key][same], ld[key][same], scale)
        print("    %s: tolerance %.1e, kernel vs longdouble %.1e" % (key, t_k, e_k))
        assert e_k <= t_k, (name, key)
    wrap = lambda a, b: np.abs((np.asarray(a, dtype=np.longdouble) - b + np.pi) % (2 * np.pi) - np.pi).astype(np.float64)  # noqa: E731
    t_w = max(16 * float(wrap(f64["omega"], ld["omega"])[same].max()), 1e-13)
    e_w = float(wrap(got["omega"], ld["omega"])[same].max())
    print("    omega: tolerance %.1e, kernel vs longdouble %.1e" % (t_w, e_w))
    assert e_w <= t_w, name
    assert np.array_equal(got["ecc"][same], ld["ecc"][same])
    assert np.all(np.abs(got["t_periastron"] - ld["t_periastron"])[same] <= 1e-14 * (1 + np.abs(ld["t_periastron"][same])))
    return tol


def against_the_statement(name, t, y, yerr, inst, f, ecc, n_phase, exact=False):
    f64, ld = statements(name, t, y, yerr, inst, f, ecc, n_phase)
    got = run(t, y, yerr, inst, f, ecc, n_phase)
    return got, f64, ld, check(name, got, f64, ld, exact)


# ---- 1: the main input ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yerr", ["per_epoch", "scalar", "absent"])
@pytest.mark.parametrize("inst", [True, False])
def test_main_input_against_the_statement(inst, yerr):
    d = O.main_input()
    e = dict(per_epoch=d["err"], scalar=2.0, absent=None)[yerr]
    got, f64, ld, _ = against_the_statement(("main", inst, yerr), d["t"], d["y"], e, d["inst"] if inst else None, d["f"], d["ecc"],
                                            d["n_phase"], exact=True)
    if inst and yerr == "per_epoch":
        assert ld["gap"].min() > 5e-5                                  # (no near-ties: the winners must agree, and do)
        peak = int(np.argmax(got["power"]))
        assert peak == int(np.argmax(ld["power"])) and got["ecc"][peak] == d["ecc"][6]
        assert got["t_periastron"][peak] == pytest.approx(d["t"].min() + 0.375 / d["f"][peak], rel=1e-15)


# ---- 2: a noise-free orbit on the grid -----------------------------------------------------------------------------------------

def test_noise_free_orbit_on_the_grid():
    d = O.main_input()
    P = 1 / d["f"][40]
    y = O.rv_model(d["t"], P, 0.6, 1.1, 30.0, d["t"].min() + 12 / 32 * P, (5.0, -12.0), d["inst"])
    got, f64, ld, _ = against_the_statement("noise-free", d["t"], y, None, d["inst"], d["f"][38:43], d["ecc"], 32)
    half = 0.5 * float(ld["chi2_0"])
    left, left_ld = (half - got["power"][2]) / half, float((half - ld["power"][2]) / half)
    print("chi2 / chi2_0 left at the orbit's frequency: kernel %.1e, longdouble statement %.1e" % (left, left_ld))
    assert abs(left_ld) <= 1e-10 and abs(left) <= 1e-10
    assert got["ecc"][2] == d["ecc"][6] and got["t_periastron"][2] == pytest.approx(d["t"].min() + 12 / 32 * P, rel=1e-15)
    assert got["K"][2] == pytest.approx(30.0, rel=1e-9) and got["omega"][2] == pytest.approx(1.1, rel=1e-9)
    assert got["zero_point"][2] == pytest.approx([5.0, -12.0], rel=1e-9)


# ---- 3: the relation to Lomb-Scargle -------------------------------------------------------------------------------------------

def test_relation_to_lomb_scargle():
    d = O.main_input()
    t, y, err = dev(d["t"]), dev(d["y"]), dev(d["err"])
    f64, ld = statements("circular", d["t"], d["y"], d["err"], None, d["f"], [0.0], 1)
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    ls = E().lomb_scargle_power(t, y, err, frequencies=d["f"]).cpu().numpy()
    circ = E().keplerian_power(t, y, err, frequencies=d["f"], ecc=[0.0]).cpu().numpy()
    full = E().keplerian_power(t, y, err, frequencies=d["f"]).cpu().numpy()                   # (the default grids: 10 x 64)
    print("ecc = [0] against lomb_scargle_power: %.1e of the peak (tolerance %.1e; against the longdouble statement %.1e); "
          "default grid less Lomb-Scargle: min %.1e of the peak, the sinusoid's peak is %.2f of the Keplerian one"
          % (O.rel_diff(circ, ls, peak), tol, O.rel_diff(circ, ld["power"], peak), float((full - ls).min()) / peak, ls.max() / full.max()))
    assert O.rel_diff(circ, ls, peak) <= tol and O.rel_diff(circ, ld["power"], peak) <= tol
    assert np.all(full >= ls - tol * peak)


# ---- 4: the convention, end to end ----------------------------------------------------------------------------------------------

def test_elements_go_straight_into_the_orbit_and_the_likelihood():
    import exoplanet_amd as xo

    d = O.main_input()
    _, ld = statements(("main", True, "per_epoch"), d["t"], d["y"], d["err"], d["inst"], d["f"], d["ecc"], d["n_phase"])
    f64, _ = statements(("main", True, "per_epoch"), d["t"], d["y"], d["err"], d["inst"], d["f"], d["ecc"], d["n_phase"])
    tol = O.tolerance(f64["power"], ld["power"], float(ld["power"].max()))
    chi2_0 = float(ld["chi2_0"])
    t, y, err, inst = dev(d["t"]), dev(d["y"]), dev(d["err"]), dev(d["inst"], torch.int64)
    power, fit = E().keplerian_power(t, y, err, frequencies=d["f"], ecc=d["ecc"], n_phase=32, instrument=d["inst"], return_fit=True)
    for i in (int(np.argmax(ld["power"])), 7, 150):
        one = lambda k: fit[k][i].reshape(1)                                                       # noqa: E731
        orbit = lambda: xo.KeplerianOrbit(period=1 / dev(d["f"][i:i + 1]), ecc=one("ecc"), omega=one("omega"),  # noqa: E731
                                          t_periastron=one("t_periastron"))
        model = fit["zero_point"][i][inst] + orbit().get_radial_velocity(t, K=one("K")).reshape(-1)
        chi2 = float((((y - model) / err) ** 2).sum())
        want = chi2_0 - 2 * float(power[i])
        ll = orbit().rv_log_likelihood(t, y, err, K=one("K"), zero_point=fit["zero_point"][i].reshape(1, -1), instrument=inst)
        chi2_ll = -2 * float(ll) - float(torch.log(2 * np.pi * err ** 2).sum())
        print("frequency %d: chi2 of the orbit's model %.12g, -2 log L less its constant %.12g, chi2_0 - 2 power %.12g; "
              "differences %.1e, %.1e of chi2_0 (tolerance %.1e)"
              % (i, chi2, chi2_ll, want, abs(chi2 - want) / chi2_0, abs(chi2_ll - want) / chi2_0, tol))
        assert abs(chi2 - want) <= tol * chi2_0 and abs(chi2_ll - want) <= tol * chi2_0


# ---- 5: shapes where the kernel can go wrong ------------------------------------------------------------------------------------

def series(n, n_inst=1, seed=11, single=False, first=None):
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, 120, n))
    inst = rs.randint(0, n_inst, n) if n_inst > 1 else None
    if single:                                               # the last instrument owns one epoch only
        inst = np.arange(n) % (n_inst - 1)
        inst[n // 2] = n_inst - 1
    if first is not None:                                    # the first of two instruments owns exactly `first` epochs
        inst = (np.arange(n) >= first).astype(np.int64)
    err = rs.uniform(0.5, 2.0, n)
    zp = 3.0 * rs.randn(n_inst)
    y = O.rv_model(t, 9.7, 0.45, 0.7, 12.0, 3.1, zp, inst) + err * rs.randn(n)
    return t, y, err, inst


F8 = 0.011 + 0.0237 * np.arange(8)
SHAPES = {
    "one tile exactly": (series(TILE, 2), F8, [0.0, 0.45, 0.8], 8),
    "one tile and one epoch": (series(TILE + 1, 3), F8, [0.0, 0.45, 0.8], 8),
    "three epochs": (series(3), F8, [0.0, 0.5], 4),
    "one candidate": (series(40, 2), F8, [0.0], 64),
    "one phase": (series(40, 2), F8, [0.0, 0.3, 0.6], 1),
    "a candidate per lane": (series(40, 2), F8, [0.15, 0.35, 0.55, 0.75], 64),
    "two candidates per lane": (series(40, 2), F8, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], 64),
    "eight instruments, one of a single epoch": (series(40, 8, single=True), F8, [0.0, 0.45], 16),
    "one frequency": (series(40, 2), F8[3:4], [0.0, 0.45, 0.8], 16),
    # (what the search shared with the astrometric one owns, csrc/exo_orbit_search.hpp: 128 lanes of which 63 have no candidate;
    # 64 lanes and three passes; three tiles with a short last one -- a segment folded at a tile's last epoch, and one that
    # stays open across two tile boundaries)
    "65 candidates": (series(40, 2), F8, [0.15, 0.3, 0.45, 0.6, 0.75], 13),
    "192 candidates": (series(40, 2), F8, [0.2, 0.5, 0.8], 64),
    "three tiles, the first instrument one tile exactly": (series(2 * TILE + 5, 2, first=TILE), F8, [0.0, 0.45, 0.8], 8),
    "three tiles, one instrument": (series(2 * TILE + 5), F8, [0.0, 0.45, 0.8], 8),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    (t, y, err, inst), f, ecc, n_phase = SHAPES[name]
    against_the_statement(name, t, y, err, inst, f, ecc, n_phase)


# ---- 6: reproducibility ---------------------------------------------------------------------------------------------------------

def test_rows_of_a_batch_runs_and_a_far_origin():
    d = O.main_input()
    rs = np.random.RandomState(3)
    ys = d["y"][None, :] + rs.randn(5, d["t"].size)
    errs = d["err"][None, :] * rs.uniform(0.8, 1.25, (5, d["t"].size))
    kw = dict(frequencies=d["f"][::4], ecc=d["ecc"], n_phase=32, instrument=d["inst"], return_fit=True)
    t = dev(d["t"])
    power, fit = E().keplerian_power(t, dev(ys), dev(errs), **kw)
    again, fit2 = E().keplerian_power(t, dev(ys), dev(errs), **kw)
    assert tuple(power.shape) == (5, 50) and tuple(fit["zero_point"].shape) == (5, 50, 2)
    assert torch.equal(power, again) and all(torch.equal(fit[k], fit2[k]) for k in fit)
    for b in range(5):
        p1, f1 = E().keplerian_power(t, dev(ys[b]), dev(errs[b]), **kw)
        assert torch.equal(p1, power[b]) and all(torch.equal(f1[k], fit[k][b]) for k in fit), b
    # the same epochs counted from 2 457 000: t - t_min is formed first, so nothing is lost
    far = d["t"] + 2457000.0
    near = far - 2457000.0                                   # (what the far epochs hold of the near ones, exactly)
    f64, ld = statements("far origin", near, d["y"], d["err"], d["inst"], d["f"][::4], d["ecc"], 32)
    peak = float(ld["power"].max())
    tol = O.tolerance(f64["power"], ld["power"], peak)
    p_far, fit_far = E().keplerian_power(dev(far), dev(d["y"]), dev(d["err"]), **kw)
    p_near, fit_near = E().keplerian_power(dev(near), dev(d["y"]), dev(d["err"]), **kw)
    err = O.rel_diff(p_far.cpu().numpy(), p_near.cpu().numpy(), peak)
    print("origin 2 457 000 against origin 0: %.1e of the peak (tolerance %.1e)" % (err, tol))
    assert err <= tol and O.rel_diff(p_far.cpu().numpy(), ld["power"], peak) <= tol
    assert torch.equal(fit_far["ecc"], fit_near["ecc"])
    assert float((fit_far["t_periastron"] - 2457000.0 - fit_near["t_periastron"]).abs().max()) <= 1e-9


# ---- 7: the estimator -----------------------------------------------------------------------------------------------------------

def test_keplerian_estimator_on_the_main_input():
    import exoplanet_amd as xo

    d = O.main_input()
    res = E().keplerian_estimator(d["t"], d["y"], d["err"], n_phase=32, instrument=d["inst"], samples_per_peak=3,
                                  minimum_frequency=d["f"][0], maximum_frequency=d["f"][-1])
    freq, power = res["periodogram"]
    assert np.array_equal(freq, E().lomb_scargle_autofrequency(d["t"], samples_per_peak=3, minimum_frequency=d["f"][0],
                                                               maximum_frequency=d["f"][-1])) and freq.size == 119
    f64, ld = statements("estimator", d["t"], d["y"], d["err"], d["inst"], freq, d["ecc"], 32)
    want = E().find_peaks(freq, np.asarray(f64["power"]) / d["t"].size, max_peaks=2)
    peak, ref = res["peaks"][0], want[0]
    print("first peak: period %.6f (statement %.6f, period_uncert %.4f), ecc %.2f, omega %.4f, K %.3f, t_periastron %.4f, "
          "zero points %s" % (peak["period"], ref["period"], ref["period_uncert"], peak["ecc"], peak["omega"], peak["K"],
                              peak["t_periastron"], peak["zero_point"]))
    assert set(ref) <= set(peak) and peak["index"] == ref["index"]
    assert abs(peak["period"] - ref["period"]) <= ref["period_uncert"]
    i = peak["index"] - 1
    assert i == int(np.argmax(ld["power"])) and peak["power"] == power[i]
    assert peak["ecc"] == float(ld["ecc"][i]) and peak["t_periastron"] == pytest.approx(float(ld["t_periastron"][i]), rel=1e-15)
    for key in ("K", "omega", "zero_point"):                 # (the tolerances of case 1; omega is nowhere near a wrap at the peak)
        scale = float(np.abs(ld[key]).max())
        assert O.rel_diff(peak[key], ld[key][i], scale) <= O.tolerance(f64[key], ld[key], scale), key
    assert all(type(peak[k]) is float for k in ("ecc", "omega", "t_periastron", "K", "power")) and type(peak["zero_point"]) is list
    # the peak's numbers start an RV model as they are
    orbit = xo.KeplerianOrbit(period=dev([1 / freq[i]]), ecc=dev([peak["ecc"]]), omega=dev([peak["omega"]]),
                              t_periastron=dev([peak["t_periastron"]]))
    ll = orbit.rv_log_likelihood(dev(d["t"]), dev(d["y"]), dev(d["err"]), K=dev([peak["K"]]), zero_point=dev([peak["zero_point"]]),
                                 instrument=dev(d["inst"], torch.int64))
    chi2 = -2 * float(ll) - float(np.log(2 * np.pi * d["err"] ** 2).sum())
    assert chi2 == pytest.approx(float(ld["chi2_0"]) - 2 * float(ld["power"][i]), rel=1e-9)
