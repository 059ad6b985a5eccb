"""GPU: the highest peak of the Keplerian periodogram without the periodogram (csrc/exo_keplerian.hip: keplerian_max_kernel)
behind exoplanet_amd.estimators.keplerian_max_power, and the false-alarm probabilities built on it.  The
reference is always the existing route on the same batch: keplerian_power(..., return_fit=True) brought to the host, the first
arg-max along the frequencies, the candidate there, and (-inf, -1, -1) where no power is finite.  Equality is exact: the same
functions in the same order, without contraction."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keplerian_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256            # epochs the periodogram's kernel stages at a time; the maximum's kernel stages half as many


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def E():
    from exoplanet_amd import estimators

    return estimators


def on_device(yerr):
    return dev(yerr) if isinstance(yerr, np.ndarray) else yerr


def reference(t, ys, yerr, inst, f, ecc, n_phase):
    """-> power, frequency_index, candidate, each (B,), from the periodogram of every row"""
    power, fit = E().keplerian_power(dev(t), dev(ys), on_device(yerr), frequencies=f, ecc=ecc, n_phase=n_phase, instrument=inst,
                                     return_fit=True)
    power, cand = power.cpu().numpy().reshape(-1, len(f)), fit["candidate"].cpu().numpy().reshape(-1, len(f))
    rows = np.arange(power.shape[0])
    where = np.argmax(power, axis=1)                         # (the first of equal maxima)
    top, cand = power[rows, where], cand[rows, where]
    none = ~np.isfinite(power).any(axis=1)
    top[none], where[none], cand[none] = -np.inf, -1, -1
    return top, where, cand


def maximum(t, ys, yerr, inst, f, ecc, n_phase, **kw):
    got = E().keplerian_max_power(dev(t), dev(ys), on_device(yerr), frequencies=f, ecc=ecc, n_phase=n_phase, instrument=inst, **kw)
    assert got["power"].dtype == torch.float64 and got["frequency_index"].dtype == got["candidate"].dtype == torch.int64
    return tuple(np.atleast_1d(got[k].cpu().numpy()) for k in ("power", "frequency_index", "candidate"))


def same_levels(got, want):
    return list(got) == list(want) and np.array_equal(list(got.values()), list(want.values()), equal_nan=True)


def same(name, got, want):
    for key, g, w in zip(("power", "frequency_index", "candidate"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, key, g, w)


# ---- 1: group and block boundaries ----------------------------------------------------------------------------------------------

def main_rows(n_series):
    """the main input and its five perturbed rows (tests/test_gpu_keplerian.py), repeated with fresh noise"""
    d = O.main_input()
    rs = np.random.RandomState(3)
    n = d["t"].size
    ys = np.concatenate([d["y"][None], d["y"][None, :] + rs.randn(5, n)])
    errs = np.concatenate([d["err"][None], d["err"][None, :] * rs.uniform(0.8, 1.25, (5, n))])
    pick = np.arange(n_series) % 6
    return d, ys[pick] + (np.arange(n_series) >= 6)[:, None] * rs.randn(n_series, n), errs[pick]


def group():
    return E().KEPLERIAN_MAX_GROUP


BATCHES = {"1": lambda G: 1, "G - 1": lambda G: G - 1, "G": lambda G: G, "G + 1": lambda G: G + 1, "2 G + 3": lambda G: 2 * G + 3}


@pytest.mark.parametrize("n_series", list(BATCHES))
def test_group_and_block_boundaries(n_series):
    B = BATCHES[n_series](group())
    d, ys, errs = main_rows(B)
    args = (d["t"], ys, errs, d["inst"], d["f"], d["ecc"], d["n_phase"])
    want = reference(*args)
    assert np.all(want[1] >= 0) and abs(1 / d["f"][want[1][0]] - O.MAIN["period"]) < 0.2
    for per_block in (1, 3, 7, d["f"].size, None):
        same((B, per_block), maximum(*args, frequencies_per_block=per_block), want)


# ---- 2: the shapes at which the periodogram's kernel can go wrong, each as a batch of three -------------------------------------

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
    y = O.rv_model(t, 9.7, 0.45, 0.7, 12.0, 3.1, zp, inst)
    return t, y + err * rs.randn(3, n), err, inst


def circular():
    t, ys, err, inst = series(40, 2)
    model = O.rv_model(t, 9.7, 0.0, 0.7, 12.0, 3.1, (1.0, -2.0), inst)
    return t, model + 0.05 * (ys - ys.mean(axis=0)), err, inst


F8 = 0.011 + 0.0237 * np.arange(8)
SHAPES = {
    "one tile exactly": (series(TILE, 2), F8, [0.0, 0.45, 0.8], 8),
    "one tile and one epoch": (series(TILE + 1, 3), F8, [0.0, 0.45, 0.8], 8),
    "half a tile and one epoch": (series(TILE // 2 + 1, 2), F8, [0.0, 0.45, 0.8], 8),
    "three epochs": (series(3), F8, [0.0, 0.5], 4),
    "one candidate": (series(40, 2), F8, [0.0], 64),
    "one phase": (series(40, 2), F8, [0.0, 0.3, 0.6], 1),
    "a candidate per lane": (series(40, 2), F8, [0.15, 0.35, 0.55, 0.75], 64),
    "two candidates per lane": (series(40, 2), F8, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], 64),
    "eight instruments, one of a single epoch": (series(40, 8, single=True), F8, [0.0, 0.45], 16),
    "one frequency": (series(40, 2), F8[3:4], [0.0, 0.45, 0.8], 16),
    "65 candidates": (series(40, 2), F8, [0.15, 0.3, 0.45, 0.6, 0.75], 13),
    "192 candidates": (series(40, 2), F8, [0.2, 0.5, 0.8], 64),
    "three tiles, the first instrument one tile exactly": (series(2 * TILE + 5, 2, first=TILE), F8, [0.0, 0.45, 0.8], 8),
    "three tiles, one instrument": (series(2 * TILE + 5), F8, [0.0, 0.45, 0.8], 8),
    # (a circular orbit, so that e = 0 wins in a grid that holds other eccentricities: the periodogram's power is then that of
    # the record's walk, which takes the solver's circular branch, and the maximum must be that one)
    "a circular winner among eccentric candidates": (circular(), np.array([0.05, 1 / 9.7, 0.2]), [0.0, 0.45, 0.8], 8),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    (t, ys, err, inst), f, ecc, n_phase = SHAPES[name]
    want = reference(t, ys, err, inst, f, ecc, n_phase)
    if name.startswith("a circular winner"):
        assert np.all(want[2] == 0) and np.all(want[1] == 1)
    same(name, maximum(t, ys, err, inst, f, ecc, n_phase), want)
    same(name, maximum(t, ys, err, inst, f, ecc, n_phase, frequencies_per_block=3), want)


# ---- 3: yerr in its four forms ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yerr", ["absent", "scalar", "per_epoch", "per_series"])
def test_yerr_forms(yerr):
    d, ys, errs = main_rows(group() + 2)
    e = dict(absent=None, scalar=2.0, per_epoch=d["err"], per_series=errs)[yerr]
    args = (d["t"], ys, e, d["inst"], d["f"][::3], d["ecc"], d["n_phase"])
    same(yerr, maximum(*args), reference(*args))


# ---- 4: exact ties ---------------------------------------------------------------------------------------------------------------

def test_exact_ties_go_to_the_lower_frequency_index():
    d, ys, errs = main_rows(3)
    peak = int(reference(d["t"], ys[:1], errs[:1], d["inst"], d["f"], d["ecc"], d["n_phase"])[1][0])
    f3, f1 = d["f"][peak], d["f"][peak // 2]
    for f, first in (([f3, f1, f3, f3], 0), ([f1, f3, f3], 1), ([f1, f1, f3, f1, f3], 2)):
        args = (d["t"], ys, errs, d["inst"], np.array(f), d["ecc"], d["n_phase"])
        want = reference(*args)
        assert want[1][0] == first
        same(f, maximum(*args), want)
        same(f, maximum(*args, frequencies_per_block=1), want)         # (the tie is decided in the finish kernel)
        same(f, maximum(*args, frequencies_per_block=2), want)


# ---- 5: reproducibility ----------------------------------------------------------------------------------------------------------

def test_two_calls_and_a_row_of_a_batch():
    B = group() + 3
    d, ys, errs = main_rows(B)
    args = (d["t"], ys, errs, d["inst"], d["f"][::4], d["ecc"], d["n_phase"])
    first, again = maximum(*args), maximum(*args)
    same("again", again, first)
    for b in (0, group() - 1, group(), B - 1):
        one = E().keplerian_max_power(dev(d["t"]), dev(ys[b]), dev(errs[b]), frequencies=d["f"][::4], ecc=d["ecc"], n_phase=d["n_phase"],
                                      instrument=d["inst"])
        assert all(v.ndim == 0 for v in one.values())
        assert (float(one["power"]), int(one["frequency_index"]), int(one["candidate"])) == (first[0][b], first[1][b], first[2][b]), b
    # a series that holds a NaN has no power that compares, and no frequency at all gives none either
    ys[1, 5] = np.nan
    got = maximum(*args)
    assert (got[0][1], got[1][1], got[2][1]) == (-np.inf, -1, -1)
    same("beside a NaN row", [np.delete(g, 1) for g in got], [np.delete(g, 1) for g in first])
    same("no frequency", maximum(d["t"], ys, errs, d["inst"], np.array([]), d["ecc"], d["n_phase"]),
         (np.full(B, -np.inf), np.full(B, -1), np.full(B, -1)))


# ---- 6: false_alarm on an explicit table ------------------------------------------------------------------------------------------

def chi2_0(ys, errs, inst):
    w = 1 / errs ** 2
    return sum((w[:, m] * (ys[:, m] - (w[:, m] * ys[:, m]).sum(1, keepdims=True) / w[:, m].sum(1, keepdims=True)) ** 2).sum(1)
               for m in (inst == k for k in np.unique(inst)))


def test_false_alarm_with_an_explicit_table():
    d = O.main_input()
    n, f = d["t"].size, d["f"][::2]
    idx = E().resample_indices(n, 20, instrument=d["inst"], replace=True, seed=1)
    idx[0] = np.arange(n)
    kw = dict(frequencies=f, ecc=d["ecc"], n_phase=d["n_phase"], instrument=d["inst"])
    res = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), resamples=idx, **kw)
    assert np.array_equal(res["resamples"], idx)
    assert res["z"][0] == res["observed"]["z"] and res["max_power"][0] == res["observed"]["max_power"]
    assert res["frequency_index"][0] == res["observed"]["frequency_index"]
    top, where, _ = reference(d["t"], d["y"][idx], d["err"][idx], d["inst"], f, d["ecc"], d["n_phase"])
    assert np.array_equal(res["max_power"].cpu().numpy(), top) and np.array_equal(res["frequency_index"].cpu().numpy(), where)
    own = E().series_chi2_0(dev(d["y"][idx]), dev(d["err"][idx]), d["inst"]).cpu().numpy()
    want = chi2_0(d["y"][idx], d["err"][idx], d["inst"])
    assert np.all(np.abs(own - want) <= 1e-13 * want) and np.ptp(want) > 0.1 * want[0]      # (with replacement it varies)
    z = res["z"].cpu().numpy()
    assert np.array_equal(z, 2 * top / own) and np.all((z >= 0) & (z <= 1))
    assert res["fap"] == (1 + int((z >= z[0]).sum())) / 21
    assert set(res["levels"]) == set(res["power_levels"]) == {0.1, 0.01, 0.001}
    assert res["levels"][0.1] == np.sort(z)[-2] and np.isnan(res["levels"][0.01])
    assert res["power_levels"][0.1] == res["levels"][0.1] * own[0] / 2
    few = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), resamples=idx, chunk=7, power=np.array([top[0], 0.0]), **kw)
    for key in ("z", "max_power", "frequency_index"):
        assert torch.equal(few[key], res[key]), key
    assert np.array_equal(few["fap"], [res["fap"], 1.0])
    a, b = (E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), n_resample=20, seed=9, **kw) for _ in range(2))
    assert np.array_equal(a["resamples"], b["resamples"]) and torch.equal(a["z"], b["z"]) and a["fap"] == b["fap"]
    assert not np.array_equal(a["resamples"], idx)


# ---- 7: the answer on the main input ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("replace", [False, True])
def test_the_planet_is_a_detection_and_white_noise_is_not(replace):
    d = O.main_input()
    kw = dict(frequencies=d["f"], ecc=d["ecc"], n_phase=d["n_phase"], instrument=d["inst"], n_resample=199, replace=replace)
    res = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), **kw)
    z = res["z"].cpu().numpy()
    print("replace=%s: the data's z %.3f, the highest of 199 resamplings %.3f (raw power %.0f against %.0f), levels %s"
          % (replace, float(res["observed"]["z"]), z.max(), float(res["max_power"].max()), float(res["observed"]["max_power"]),
             res["levels"]))
    assert res["fap"] == 1 / 200
    assert z.shape == (199,) and np.all((z >= 0) & (z <= 1)) and 0 <= float(res["observed"]["z"]) <= 1
    assert res["levels"][0.01] == np.sort(z)[-2] and np.isnan(res["levels"][0.001])           # (k = floor(0.01 x 200) = 2)
    noise = np.array([5.0, -12.0])[d["inst"]] + d["err"] * np.random.default_rng(7).standard_normal(40)
    res = E().false_alarm(dev(d["t"]), dev(noise), dev(d["err"]), **kw)
    print("white noise: fap %.3f, z %.3f" % (res["fap"], float(res["observed"]["z"])))
    assert res["fap"] >= 0.5


# ---- 8: the sinusoid ---------------------------------------------------------------------------------------------------------------

def test_lomb_scargle_method():
    d = O.main_input()
    idx = E().resample_indices(40, 30, seed=2)
    res = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), frequencies=d["f"], method="lomb_scargle", resamples=idx, chunk=8)
    power = E().lomb_scargle_power(dev(d["t"]), dev(d["y"][idx]), dev(d["err"][idx]), frequencies=d["f"]).cpu().numpy()
    assert np.array_equal(res["max_power"].cpu().numpy(), power.max(axis=1))
    assert np.array_equal(power[np.arange(30), res["frequency_index"].cpu().numpy()], power.max(axis=1))
    own = E().series_chi2_0(dev(d["y"][idx]), dev(d["err"][idx])).cpu().numpy()
    assert np.array_equal(res["z"].cpu().numpy(), 2 * power.max(axis=1) / own)
    data = E().lomb_scargle_power(dev(d["t"]), dev(d["y"]), dev(d["err"]), frequencies=d["f"]).cpu().numpy()
    assert float(res["observed"]["max_power"]) == data.max() and res["fap"] == (1 + int((res["z"] >= res["observed"]["z"]).sum())) / 31
    with pytest.raises(ValueError, match="instrument must be None"):
        E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), frequencies=d["f"], method="lomb_scargle", instrument=d["inst"])


# ---- 9: the estimators --------------------------------------------------------------------------------------------------------------

def test_estimators_carry_the_probability():
    d = O.main_input()
    kw = dict(n_phase=32, instrument=d["inst"], samples_per_peak=3, minimum_frequency=d["f"][0], maximum_frequency=d["f"][-1])
    plain = E().keplerian_estimator(d["t"], d["y"], d["err"], **kw)
    zero = E().keplerian_estimator(d["t"], d["y"], d["err"], n_resample=0, **kw)
    assert set(plain) == set(zero) == {"periodogram", "peaks"} and all("fap" not in p for p in zero["peaks"])
    assert np.array_equal(plain["periodogram"][0], zero["periodogram"][0]) and np.array_equal(plain["periodogram"][1], zero["periodogram"][1])
    assert plain["peaks"] == zero["peaks"] and set(zero["peaks"][0]) == {
        "index", "log_power", "period", "period_uncert", "ecc", "omega", "t_periastron", "K", "zero_point", "power"}
    res = E().keplerian_estimator(d["t"], d["y"], d["err"], n_resample=99, seed=0, **kw)
    assert set(res) == {"periodogram", "peaks", "power_levels"} and np.array_equal(res["periodogram"][1], plain["periodogram"][1])
    assert [{k: v for k, v in p.items() if k != "fap"} for p in res["peaks"]] == plain["peaks"]
    assert res["peaks"][0]["fap"] == 0.01 and all(0.01 <= p["fap"] <= 1 for p in res["peaks"])
    freq = res["periodogram"][0]
    fa = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), frequencies=freq, n_resample=99, seed=0, n_phase=32, instrument=d["inst"])
    assert same_levels(res["power_levels"], {alpha: v / 40 for alpha, v in fa["power_levels"].items()})
    level = res["power_levels"][0.01]
    print("keplerian_estimator: the peak %.2f, the 1 %% line %.2f, the 10 %% line %.2f" % (res["peaks"][0]["power"], level, res["power_levels"][0.1]))
    assert res["peaks"][0]["power"] > level > res["power_levels"][0.1] > 0 and np.isnan(res["power_levels"][0.001])
    # the sinusoid's estimator likewise
    ls_kw = dict(samples_per_peak=3, minimum_frequency=d["f"][0], maximum_frequency=d["f"][-1])
    plain = E().lomb_scargle_estimator(d["t"], d["y"], d["err"], **ls_kw)
    res = E().lomb_scargle_estimator(d["t"], d["y"], d["err"], n_resample=99, seed=0, **ls_kw)
    assert set(plain) == {"periodogram", "peaks"} and set(res) == {"periodogram", "peaks", "power_levels"}
    assert [{k: v for k, v in p.items() if k != "fap"} for p in res["peaks"]] == plain["peaks"] and np.array_equal(
        res["periodogram"][1], plain["periodogram"][1])
    fa = E().false_alarm(dev(d["t"]), dev(d["y"]), dev(d["err"]), frequencies=freq, method="lomb_scargle", n_resample=99, seed=0)
    assert same_levels(res["power_levels"], {alpha: v / 40 for alpha, v in fa["power_levels"].items()})
    assert all(1 / 100 <= p["fap"] <= 1 for p in res["peaks"])
