"""CPU: the template search (transit least squares) of exoplanet_amd/csrc/exo_estimators_core.hpp compiled for the host
(tests/tls_harness.cpp) against the numpy restatement of DESIGN.md section 18 (tests/tls_oracle.py), its two properties with an
all-ones template, the tie rule, inadmissible windows, and the host side of estimators.tls_power / transit_template and of
exo_tls_power_f64: argument errors that need no device.  The kernels themselves: tests/test_gpu_tls.py.

Tolerances follow DESIGN.md 9.5: 16 x (float64 oracle against longdouble oracle on the same input, at the same maximiser), floor
1e-13, relative to each period's own value; printed before every assertion."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimators_oracle as O  # noqa: E402
import tls_oracle as TO  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64, _f64 = ctypes.c_int64, ctypes.c_double

DURATIONS, OVERSAMPLE = (0.1, 0.2, 0.4), 10


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "tls_harness.so")
    srcs = [os.path.join(ROOT, "tests", "tls_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_estimators_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_tls_window.argtypes = [_dp, _dp, _dp, _i64, _i64, _f64, _f64, _dp]
    lib.harness_tls_search.argtypes = [_dp, _dp, _i64, _ip, _ip, ctypes.c_int, _dp, _f64, _f64, ctypes.c_int, _f64, _f64, _f64, _i64,
                                       _dp]
    lib.harness_box_search.argtypes = [_dp, _dp, _i64, _ip, ctypes.c_int, _f64, _f64, ctypes.c_int, _f64, _f64, _f64, _dp]
    return lib


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


def search(harness, hy, hw, templates, Y, W, objective, p=100.0, delta=0.5, t_min=3.0, n_lane=1):
    hy, hw = _c(hy), _c(hw)
    m = _c([len(g) for g in templates], np.int32)
    off = _c(np.concatenate([[0], np.cumsum(m)]), np.int32)
    g = _c(np.concatenate([np.asarray(x, dtype=np.float64) for x in templates]))
    out = np.full(7, 123.0)
    harness.harness_tls_search(_p(hy), _p(hw), hy.size - 1, _p(m, _ip), _p(off, _ip), m.size, _p(g), Y, W, objective, p, delta, t_min,
                               n_lane, _p(out))
    return dict(zip(O.FIELDS, out))


def box_search(harness, hy, hw, ms, Y, W, objective, p, delta, t_min):
    cy, cw, m = _c(np.cumsum(hy)), _c(np.cumsum(hw)), _c(ms, np.int32)
    out = np.full(7, 123.0)
    harness.harness_box_search(_p(cy), _p(cw), cy.size - 1, _p(m, _ip), m.size, Y, W, objective, p, delta, t_min, _p(out))
    return dict(zip(O.FIELDS, out))


def window(harness, hy, hw, g, s, Y, W):
    hy, hw, g = _c(hy), _c(hw), _c(g)
    out = np.empty(10)
    harness.harness_tls_window(_p(hy), _p(hw), _p(g), s, g.size, Y, W, _p(out))
    return dict(zip(("A", "B", "C", "w_in", "D", "depth", "depth_err", "depth_snr", "log_likelihood", "ok"), out))


@pytest.fixture(scope="module")
def main():
    t, y = TO.main_input()
    delta, ms = O.bls_plan(DURATIONS, OVERSAMPLE)
    return dict(t=t, y=y, periods=TO.main_periods(), delta=delta, ms=ms,
                templates=[TO.transit_template(int(m), TO.TRUE["ror"], TO.TRUE["b"]) for m in ms])


def run_search(harness, main, templates, objective, periods, y=None, n_lane=7):
    y = main["y"] if y is None else y
    got = {k: np.empty(len(periods)) for k in O.FIELDS}
    for i, p in enumerate(periods):
        hy, hw, Y, W, t_min, _ = TO.tls_hist(main["t"], y, None, p, main["delta"], OVERSAMPLE)
        one = search(harness, hy, hw, templates, Y, W, 0 if objective == "likelihood" else 1, p=p, delta=main["delta"], t_min=t_min,
                     n_lane=n_lane)
        for k in O.FIELDS:
            got[k][i] = one[k]
    return got


@pytest.mark.parametrize("objective", ["likelihood", "snr"])
def test_search_and_outputs_match_the_oracle_on_the_main_input(harness, main, objective):
    """tls_search and tls_outputs on the oracle's own float64 histogram of every one of the 203 periods"""
    got = run_search(harness, main, main["templates"], objective, main["periods"])
    TO.check(f"host, main input, {objective}", got, main["t"], main["y"], None, main["periods"], DURATIONS, main["templates"], OVERSAMPLE,
             objective)
    i = int(np.argmax(got["power"]))
    assert abs(main["periods"][i] - 2.345) < 2e-4 and got["duration"][i] == pytest.approx(0.2)


def test_all_ones_templates_give_the_box_search(harness, main):
    """g = 1: with the "snr" objective the whole result is the box search's; with the likelihood (which differs from the box's
    by w_out / W) depth, depth_err and depth_snr of the chosen window are the box's statistics of that window"""
    ones = [np.ones(int(m)) for m in main["ms"]]
    periods = main["periods"][::8]
    want = O.bls_power(main["t"], main["y"], None, periods, DURATIONS, OVERSAMPLE, "snr")
    exact = O.bls_power(main["t"], main["y"], None, periods, DURATIONS, OVERSAMPLE, "snr", dtype=np.longdouble)
    _, _, unit_tls = TO.unit_and_reference(main["t"], main["y"], None, periods, DURATIONS, ones, OVERSAMPLE, "snr")
    unit = max([O.rel_diff(want[k], exact[k]) for k in ("power",) + TO.STATS] + [unit_tls])
    tol = max(TO.FACTOR * unit, TO.FLOOR)
    tls = run_search(harness, main, ones, "snr", periods)
    worst = 0.0
    for i, p in enumerate(periods):
        hy, hw, Y, W, t_min, _ = TO.tls_hist(main["t"], main["y"], None, p, main["delta"], OVERSAMPLE)
        box = box_search(harness, hy, hw, main["ms"], Y, W, 1, p, main["delta"], t_min)
        assert box["duration"] == tls["duration"][i] and box["transit_time"] == tls["transit_time"][i], p
        worst = max([worst] + [abs(tls[k][i] - box[k]) / abs(box[k]) for k in ("power", "depth", "depth_err", "depth_snr")])
        # the eighth key differs by definition: the box's log_likelihood is astropy's approximation w_in depth^2 / 2, the
        # template search's is exact, depth_snr^2 / 2 (smaller by w_out / W)
        worst = max(worst, abs(tls["log_likelihood"][i] - 0.5 * box["depth_snr"] ** 2) / tls["log_likelihood"][i])
        assert tls["log_likelihood"][i] < box["log_likelihood"]
    print(f"[g = 1, snr] {len(periods)} periods, unit {unit:.2e}, tolerance {tol:.2e}, search against the box search {worst:.2e}")
    assert worst <= tol
    like = run_search(harness, main, ones, "likelihood", periods)
    worst = 0.0
    for i, p in enumerate(periods):
        st = O.bls_at(main["t"], main["y"], None, p, DURATIONS, OVERSAMPLE, like["duration"][i], like["transit_time"][i])
        worst = max([worst] + [abs(like[k][i] - st[j]) / abs(st[j]) for j, k in enumerate(("depth", "depth_err", "depth_snr"))])
    print(f"[g = 1, likelihood] depth, depth_err, depth_snr against the box of the same window {worst:.2e}")
    assert worst <= tol


def test_formulas_of_one_window(harness, main):
    """D = B - A^2 / W, depth = (A Y / W - C) / D, depth_err = 1 / sqrt(D), and log_likelihood = depth^2 D / 2 = depth_snr^2 / 2:
    half the drop in chi-squared of the two-parameter fit against a constant, checked by least squares on the bins"""
    hy, hw, Y, W, _, _ = TO.tls_hist(main["t"], main["y"], None, 2.345, main["delta"], OVERSAMPLE)
    g = main["templates"][1]
    n_phase = len(hy) - 1 - OVERSAMPLE
    for s in (0, 37, 95, n_phase - 15):                               # (the last one straddles phase zero by five bins)
        assert s + len(g) <= len(hy) - 1
        w = window(harness, hy, hw, g, s, Y, W)
        idx = s + 1 + np.arange(len(g))
        A, B, C = (g * hw[idx]).sum(), (g * g * hw[idx]).sum(), (g * hy[idx]).sum()
        assert w["ok"] == 1.0
        assert w["A"] == pytest.approx(A, rel=1e-14) and w["B"] == pytest.approx(B, rel=1e-14) and w["C"] == pytest.approx(C, rel=1e-12)
        assert w["w_in"] == pytest.approx(hw[idx].sum(), rel=1e-14) and w["D"] == pytest.approx(B - A * A / W, rel=1e-14)
        assert w["depth_err"] == pytest.approx(1 / np.sqrt(w["D"]), rel=1e-15)
        assert w["log_likelihood"] == pytest.approx(0.5 * w["depth"] ** 2 * w["D"], rel=1e-14)
        assert w["log_likelihood"] == pytest.approx(0.5 * w["depth_snr"] ** 2, rel=1e-14)
        # weighted least squares of the binned means on (1, -g placed in the window): the same depth and the same drop.  The
        # bins of one phase cycle that the window covers, wrapped where it straddles phase zero.
        cols = (idx - 1) % n_phase + 1
        shape = np.zeros(len(hy))
        np.add.at(shape, cols, g)
        ph = slice(1, n_phase + 1)
        good = hw[ph] > 0
        wq, yq, gq = hw[ph][good], hy[ph][good] / hw[ph][good], shape[ph][good]
        M = np.stack([np.ones_like(gq), -gq], axis=1) * np.sqrt(wq)[:, None]
        coef = np.linalg.lstsq(M, np.sqrt(wq) * yq, rcond=None)[0]
        chi2 = lambda r: float((wq * r * r).sum())  # noqa: E731
        drop = chi2(yq - (wq * yq).sum() / wq.sum()) - chi2(yq - coef[0] + coef[1] * gq)
        assert w["depth"] == pytest.approx(coef[1], rel=1e-9) and w["log_likelihood"] == pytest.approx(0.5 * drop, rel=1e-8)


@pytest.mark.parametrize("n_lane", [1, 3, 64])
def test_ties_gaps_and_inadmissible_windows(harness, n_lane):
    # an exact tie: two identical dips under identical templates; the smaller key k (n_bins + 1) + s wins -- the first duration,
    # then the earliest start -- whichever lane found it and in whatever order the lanes are reduced
    hy = np.array([0, 0, -1.0, 0, 0, -1.0, 0, 0])
    hw = np.ones(8)
    hw[0] = 0
    for objective in (0, 1):
        got = search(harness, hy, hw, [[1.0], [1.0], [1.0, 1.0]], hy.sum(), hw.sum(), objective, n_lane=n_lane)
        assert got["duration"] == 0.5 and got["transit_time"] == 1 * 0.5 + 0.25 + 3.0, got
    hy = np.array([0, 0, -.5, -1.0, -.5, 0, 0, -.5, -1.0, -.5, 0, 0])
    hw = np.ones(12)
    hw[0] = 0
    tri = [0.5, 1.0, 0.5]
    for objective in (0, 1):
        got = search(harness, hy, hw, [tri, tri], hy.sum(), hw.sum(), objective, n_lane=n_lane)
        assert got["duration"] == 1.5 and got["transit_time"] == 1 * 0.5 + 0.75 + 3.0, got
        st = TO.tls_windows(hy, hw, hy.sum(), hw.sum(), np.array([1]), tri)[:, 0]
        assert [got[k] for k in TO.STATS] == pytest.approx(list(st), rel=1e-14)
    # a gap: bins without weight.  Windows wholly inside it have w_in = 0 and are skipped, never chosen; against brute force
    hw = np.array([0, 2, 2, 0, 0, 0, 2, 2, 2, 2], dtype=float)
    hy = np.array([0, .1, -.1, 0, 0, 0, -2.0, -2.2, .1, -.1])
    Y, W = 1.5 * hy.sum() - 0.3, 1.5 * hw.sum()
    tpl = [[1.0], [0.6, 1.0], [0.5, 1.0, 0.5]]
    for objective in (0, 1):
        got = search(harness, hy, hw, tpl, Y, W, objective, n_lane=n_lane)
        best = (-np.inf, None)
        for k, g in enumerate(tpl):
            st = TO.tls_windows(hy, hw, Y, W, np.arange(0, 9 - len(g) + 1), g)
            assert np.all(np.isnan(st[:, [s for s in range(9 - len(g) + 1) if hw[s + 1:s + 1 + len(g)].sum() == 0]]))
            obj = np.where(np.isnan(st[3 - objective]), -np.inf, st[3 - objective])
            if obj.max() > best[0]:
                best = (obj.max(), (k, int(np.argmax(obj)), st[:, int(np.argmax(obj))]))
        k, s, st = best[1]
        assert got["power"] == pytest.approx(best[0], rel=1e-14) and got["duration"] == 0.5 * len(tpl[k])
        assert got["transit_time"] == s * 0.5 + 0.25 * len(tpl[k]) + 3.0
        assert [got[k_] for k_ in TO.STATS] == pytest.approx(list(st), rel=1e-14)
    # nothing admissible: one bin holds every cadence, so each window has w_in = 0 or W - w_in = 0
    one = np.array([0, 0, 5.0, 0, 0])
    got = search(harness, -one, one, [[1.0], [1.0, 0.7]], -5.0, 5.0, 0, n_lane=n_lane)
    assert got["power"] == -np.inf and all(np.isnan(got[k]) for k in O.FIELDS[1:])
    # D = 0 with weight outside: a template that vanishes on every weighted bin of its window is no fit
    w = window(harness, np.array([0, -1.0, 0, -1.0]), np.array([0, 1.0, 0, 1.0]), [0.0, 1.0], 0, -2.0, 2.0)
    assert w["w_in"] == 1.0 and w["D"] == 0.0 and w["ok"] == 0.0
    # a template longer than the histogram has no window
    got = search(harness, -one, one, [np.ones(9)], -5.0, 5.0, 0, n_lane=n_lane)
    assert got["power"] == -np.inf


# ---- the host side of exoplanet_amd.estimators ---------------------------------------------------------------------------------

def test_argument_errors():
    import torch

    from exoplanet_amd import estimators as E

    assert {"tls_power", "tls_estimator", "transit_template"} <= set(E.__all__)
    t = torch.linspace(0, 10, 50, dtype=torch.float64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.tls_power(t, t, periods=[1.0, 2.0], durations=[0.1])
    with pytest.raises(ValueError, match="torch.Tensor"):
        E.tls_power(t.numpy(), t.numpy(), periods=[1.0], durations=[0.1])
    with pytest.raises(ValueError, match="'depth'"):
        E.tls_power(t, t, periods=[1.0], durations=[0.1], objective="depth")
    # the template's arguments are checked before a device is looked for, and the message names the value
    for kw, what in ((dict(m=0), "0"), (dict(m=2.5), "2.5"), (dict(m=-3), "-3"), (dict(m=10, ror=0.0), "0.0"),
                     (dict(m=10, ror=-0.1), "-0.1"), (dict(m=10, b=1.0), "1.0"), (dict(m=10, b=-0.2), "-0.2"),
                     (dict(m=10, b=float("nan")), "nan"), (dict(m=10, u=(0.1, 0.2, 0.3)), "0.3")):
        with pytest.raises(ValueError, match=re.escape(what)):
            E.transit_template(**kw)
    # the table of a call: one finite array of m_k entries per duration, EXO_TLS_MAX_TEMPLATE entries in all
    m = np.array([2, 3], dtype=np.int32)
    table, off = E._template_table([[1.0, 0.5], [0.5, 1.0, 0.5]], m, 0.1, 0.0, (0.4, 0.2))
    assert list(table) == [1.0, 0.5, 0.5, 1.0, 0.5] and list(off) == [0, 2, 5] and off.dtype == np.int32
    assert list(E._template_table(np.ones(2), m[:1], 0.1, 0.0, (0.4, 0.2))[1]) == [0, 2]
    for bad, what in (([[1.0, 0.5]], "got 1"), ([[1.0, 0.5], [1.0, 0.5]], r"(3,)"), ([[1.0, np.inf], [1.0, 1.0, 1.0]], "inf"),
                      ([[1.0, 0.5], [1.0, np.nan, 1.0]], "nan"), (np.ones((2, 3)), "(2, 3)")):
        with pytest.raises(ValueError, match=re.escape(what)):
            E._template_table(bad, m, 0.1, 0.0, (0.4, 0.2))
    big = np.array([5000, 5000], dtype=np.int32)
    with pytest.raises(ValueError, match="10000"):
        E._template_table([np.ones(5000), np.ones(5000)], big, 0.1, 0.0, (0.4, 0.2))
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    assert int(re.search(r"#define\s+EXO_TLS_MAX_TEMPLATE\s+(\d+)", text).group(1)) == E.MAX_TEMPLATE


def test_abi_of_exo_tls_power():
    """the argument checks return on the host, before any launch: the pointers are never followed"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    lib = _lib.load()
    INVALID, WORKSPACE = 1, 3
    m = (ctypes.c_int32 * 2)(10, 20)
    off = (ctypes.c_int32 * 3)(0, 10, 30)
    names = ["t", "y", "yerr", "n_yerr", "n", "n_series", "periods", "n_period", "min_bins", "max_bins", "m", "n_dur", "delta",
             "oversample", "objective", "templates", "offsets", "out", "ws", "ws_bytes", "stream"]
    ok = [8, 8, None, 0, 100, 1, 8, 5, 100, 200, ctypes.addressof(m), 2, 0.01, 10, 0, 8, ctypes.addressof(off), 8, 8, 100, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_tls_power_f64(*args)

    # every argument in order: the only thing left to refuse is the workspace (too small here, so nothing is launched)
    assert call() == WORKSPACE
    assert call(n_period=0) == 0                                        # nothing to do
    for bad in (dict(templates=None), dict(offsets=None), dict(t=None), dict(n=0), dict(n_yerr=1), dict(n_dur=0), dict(n_dur=17),
                dict(delta=0.0), dict(oversample=0), dict(objective=2), dict(min_bins=300), dict(out=None), dict(ws=None)):
        assert call(**bad) == INVALID, bad
    for steps in ((0, 10, 29), (0, 11, 30), (1, 10, 30), (-1, 9, 29), (0, 10, 10), (0, 10, 2 ** 31 - 1)):
        wrong = (ctypes.c_int32 * 3)(*steps)
        assert call(offsets=ctypes.addressof(wrong)) == INVALID, steps
    shifted = (ctypes.c_int32 * 3)(5, 15, 35)                           # a table may begin anywhere inside the allocation
    assert call(offsets=ctypes.addressof(shifted)) == WORKSPACE
    zero = (ctypes.c_int32 * 2)(10, 0)
    assert call(m=ctypes.addressof(zero)) == INVALID
    # the cap on the table: EXO_TLS_MAX_TEMPLATE entries in all
    from exoplanet_amd.estimators import MAX_TEMPLATE

    for total, want in ((MAX_TEMPLATE, WORKSPACE), (MAX_TEMPLATE + 1, INVALID)):
        wide = (ctypes.c_int32 * 2)(10, total - 10)
        woff = (ctypes.c_int32 * 3)(0, 10, total)
        assert call(m=ctypes.addressof(wide), offsets=ctypes.addressof(woff)) == want, total
    # sixteen durations are taken, and their seventeen offsets read
    m16 = (ctypes.c_int32 * 16)(*([3] * 16))
    off16 = (ctypes.c_int32 * 17)(*range(0, 51, 3))
    assert call(m=ctypes.addressof(m16), n_dur=16, offsets=ctypes.addressof(off16)) == WORKSPACE
