"""GPU: the per-transit fit (csrc/exo_timing.hip) behind exoplanet_amd.estimators.timing_plan, transit_times and ttv_estimator
against the numpy statement of DESIGN.md section 20 (tests/timing_oracle.py), by the rule of DESIGN.md 9.5: what float64 costs
the statement itself on a case's own input is the unit, the kernel gets 16 of them (floor 1e-13) on the curve, the depth and
its error, and the first-order propagation of that through the vertex formula on the shift and its error; counts, flags, the
epochs and the position of the maximum are exact.  Every check prints its figures before it asserts."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timing_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

LANES = 256           # lanes of the workgroup of one (transit, series) (csrc/exo_timing_core.hpp, EXO_TIMING_THREADS)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def E():
    from exoplanet_amd import estimators

    return estimators


def host(res, row=None):
    """a result of transit_times (return_curve=True) as the host arrays tests/timing_oracle.py's check reads; row: of a batch"""
    out = {}
    for k, v in res.items():
        a = v.cpu().numpy()
        batched = a.ndim == (3 if k == "curve" else 2) and k not in ("transit_ind", "linear_time", "shifts")
        out[k] = a[row] if (batched and row is not None) else a
    return out


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def run(t, y, yerr=None, **kw):
    yerr = dev(yerr) if isinstance(yerr, np.ndarray) else yerr
    for k in ("exclude",):
        if kw.get(k) is not None:
            kw[k] = dev(kw[k], torch.bool)
    if isinstance(kw.get("depth"), np.ndarray):
        kw["depth"] = dev(kw["depth"])
    return E().transit_times(dev(t), dev(y), yerr, return_curve=True, **kw)


def check(name, got, ref):
    """the statement's check, and the record's shift and error against the vertex formula on the record's own curve"""
    rep = O.check(name, got, ref)
    shift, err = O.vertex_from_curve(got["curve"], got["shifts"], got["valid"])
    for mine, want in ((got["shift"], shift), (got["time_err"], err)):
        assert np.array_equal(np.isnan(mine), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(mine[ok] - want[ok]) <= 1e-14 * np.abs(want[ok])), name
    assert np.array_equal(got["shifts"], ref[1]["shifts"])
    return rep


@functools.lru_cache(maxsize=None)
def main(case, offset=0.0):
    return O.main_input(case, offset)


def yerr_of(kind, t, sigma, row=0):
    if kind == "none":
        return None
    if kind == "scalar":
        return sigma
    return sigma * (1 + 0.3 * np.sin(t + row))


@functools.lru_cache(maxsize=None)
def main_reference(case, offset, kind, row=0):
    t, y, sigma = main(case, offset)
    return O.reference(t, y, yerr_of(kind, t, sigma, row), template=O.main_template(), **O.SEARCH)


@pytest.mark.parametrize("case", list(O.CASES))
def test_main_inputs_against_the_statement(case):
    t, y, sigma = main(case)
    g = O.main_template()
    singles = {}
    for kind in ("none", "scalar", "cadence"):
        res = run(t, y, yerr_of(kind, t, sigma), template=g, **O.SEARCH)
        singles[kind] = host(res)
        assert res["shift"].shape == (12,) and res["curve"].shape == (12, 121) and res["valid"].dtype == torch.bool
        check(f"{case}, yerr {kind}", singles[kind], main_reference(case, 0.0, kind))
    O.science(f"{case}, the kernel", singles["scalar"])
    again = host(run(t, y, sigma, template=g, **O.SEARCH))
    assert same(singles["scalar"], again)                               # run to run: bitwise
    # a batch of three series with an error bar per series and cadence: row b is bitwise the single call
    y1 = main(case, 1.0)[1]
    ys = np.stack([y, y1, y[::-1].copy()])
    errs = np.stack([yerr_of("cadence", t, sigma, b) for b in range(3)])
    batch = run(t, ys, errs, template=g, **O.SEARCH)
    assert batch["shift"].shape == (3, 12) and batch["curve"].shape == (3, 12, 121) and batch["transit_ind"].shape == (12,)
    for b in range(3):
        single = host(run(t, ys[b], errs[b], template=g, **O.SEARCH))
        assert same(single, host(batch, b)), b
    check(f"{case}, batch row 0", host(batch, 0), main_reference(case, 0.0, "cadence"))
    # around 1 instead of 0: the mean is removed first, and the unit shows what is left
    check(f"{case}, around 1, batch row 1", host(batch, 1), main_reference(case, 1.0, "cadence", 1))
    one = host(run(t, y1, sigma, template=g, **O.SEARCH))
    check(f"{case}, around 1", one, main_reference(case, 1.0, "scalar"))
    O.science(f"{case}, around 1, the kernel", one)


def test_held_depth():
    t, y, sigma = main("10min")
    g = O.main_template()
    ref = O.reference(t, y, sigma, template=g, depth=0.011, **O.SEARCH)
    got = host(run(t, y, sigma, template=g, depth=0.011, **O.SEARCH))
    check("held depth", got, ref)
    valid = got["valid"]
    assert np.all(np.isnan(got["depth_err"])) and np.all(np.isnan(got["depth_snr"])) and np.all(got["depth"][valid] == 0.011)
    depths = np.array([0.011, 0.009, 0.02])
    batch = run(t, np.stack([y, y, y]), sigma, template=g, depth=depths, **O.SEARCH)
    assert same(got, host(batch, 0))
    for b in (1, 2):
        check(f"held depth, row {b}", host(batch, b), O.reference(t, y, sigma, template=g, depth=float(depths[b]), **O.SEARCH))


def test_exclude_takes_out_one_transit_and_nothing_else():
    t, y, sigma = main("10min")
    g = O.main_template()
    plain = host(run(t, y, sigma, template=g, **O.SEARCH))
    T3 = 1.0 + 2.345 * 3
    mask = np.abs(t - T3) <= 0.33
    got = host(run(t, y, sigma, template=g, exclude=mask, **O.SEARCH))
    k3 = int(np.flatnonzero(plain["transit_ind"] == 3)[0])
    assert plain["valid"][k3] and not got["valid"][k3] and got["n_in"][k3] == 0 and got["n_window"][k3] == plain["n_window"][k3]
    assert np.all(got["curve"][k3] == -np.inf) and np.isnan(got["transit_time"][k3])
    others = np.arange(12) != k3
    for k in plain:
        a, b = (plain[k], got[k]) if k == "shifts" else (plain[k][others], got[k][others])
        assert np.array_equal(a, b, equal_nan=True), k
    check("exclude", got, O.reference(t, y, sigma, template=g, exclude=mask, **O.SEARCH))
    # a mask per series: row 0 masked, row 1 not; no error bars at all with a mask
    batch = run(t, np.stack([y, y]), sigma, template=g, exclude=np.stack([mask, np.zeros_like(mask)]), **O.SEARCH)
    assert same(got, host(batch, 0)) and same(plain, host(batch, 1))
    partial = (t > T3) & (t < T3 + 0.05)                                # some cadences of the transit only
    check("exclude, unit weights", host(run(t, y, None, template=g, exclude=partial, **O.SEARCH)),
          O.reference(t, y, None, template=g, exclude=partial, **O.SEARCH))


def test_smallest_shapes_and_tiny_windows():
    g = O.main_template()
    t, y, sigma = main("10min")
    keep = (t > 0.5) & (t < 1.5)
    search = dict(O.SEARCH, n_shift=3)
    res = run(t[keep], y[keep], sigma, template=g, **search)            # K = 1, B = 1, three shifts
    assert res["shift"].shape == (1,) and res["curve"].shape == (1, 3)
    check("K = 1, M = 3", host(res), O.reference(t[keep], y[keep], sigma, template=g, **search))
    assert run(t[keep], y[keep][None], sigma, template=g, **search)["shift"].shape == (1, 1)
    # windows of three (all inside the template: nothing outside), four (three inside, one outside) and one cadence
    tt = np.array([0.95, 1.0, 1.05, 10.95, 11.0, 11.05, 11.25, 21.0])
    yy = np.array([0.0, -0.01, 0.001, 0.0, -0.01, 0.001, 0.002, -0.01])
    search = dict(period=10.0, t0=1.0, duration=0.2, max_shift=0.01, n_shift=5, window=0.6)
    got = host(run(tt, yy, 0.001, template=g, **search))
    assert got["n_window"].tolist() == [3, 4, 1] and got["valid"].tolist() == [False, True, False]
    check("windows of 3, 4 and 1 cadences", got, O.reference(tt, yy, 0.001, template=g, **search))
    got = host(run(tt, yy, 0.001, template=g, min_in_transit=4, **search))
    assert not got["valid"].any()
    check("min_in_transit 4", got, O.reference(tt, yy, 0.001, template=g, min_in_transit=4, **search))
    # no epoch in range
    for ys, shape in ((yy, (0,)), (np.stack([yy, yy]), (2, 0))):
        res = run(tt, ys, template=g, period=100.0, t0=50.0, duration=0.2)
        assert res["shift"].shape == shape and res["valid"].shape == shape and res["curve"].shape == shape + (201,)
        assert res["transit_ind"].shape == (0,) and res["linear_time"].shape == (0,)


@pytest.mark.parametrize("m", [1, 1024])
def test_template_sizes(m):
    t, y, sigma = main("30min")
    g = np.array([1.0]) if m == 1 else O.main_template(1024)
    check(f"m = {m}", host(run(t, y, sigma, template=g, **O.SEARCH)), O.reference(t, y, sigma, template=g, **O.SEARCH))


@pytest.mark.parametrize("n_shift", [LANES - 1, LANES + 1, 4097])
def test_shift_counts_around_the_lanes_and_at_the_cap(n_shift):
    t, y, sigma = main("30min")
    g = O.main_template()
    search = dict(O.SEARCH, n_shift=n_shift)
    check(f"n_shift = {n_shift}", host(run(t, y, sigma, template=g, **search)), O.reference(t, y, sigma, template=g, **search))


def test_widest_window_and_one_more():
    est = E()
    cap = est.MAX_TIMING_WINDOW
    g = O.main_template()
    search = dict(period=100.0, t0=0.5, duration=0.2, max_shift=0.05, n_shift=21, window=2.0)
    for n in (cap, cap + 1):
        t = np.arange(n) / float(cap)
        x = (t - 0.52) / 0.1
        y = 1e-3 * np.random.RandomState(3).randn(n) - 0.01 * np.clip(1 - x * x, 0, None)
        if n > cap:
            with pytest.raises(ValueError, match=rf"{cap + 1} cadences, more than the {cap}"):
                est.timing_plan(dev(t), **search)
            continue
        plan = est.timing_plan(dev(t), **search)
        assert plan.max_window == cap and type(plan.max_window) is int and plan.transit_ind.tolist() == [0]
        got = host(run(t, y, 1e-3, template=g, **search))
        assert got["n_window"].tolist() == [cap] and got["valid"].all() and not got["at_edge"].any()
        check("a window at the cap", got, O.reference(t, y, 1e-3, template=g, **search))


def test_a_transit_beyond_the_grid_sits_on_its_edge():
    t, y, sigma = main("30min")
    g = O.main_template()
    search = dict(O.SEARCH, max_shift=0.004, n_shift=9, window=0.5)     # the true shifts reach 0.01
    got = host(run(t, y, sigma, template=g, **search))
    check("beyond the grid", got, O.reference(t, y, sigma, template=g, **search))
    edge = got["at_edge"]
    truth = O.true_shift(got["transit_ind"])
    far = got["valid"] & (np.abs(truth) > 0.006)
    assert far.sum() >= 4 and edge[far].all()
    assert np.array_equal(got["shift"][far], 0.004 * np.sign(truth[far])) and np.all(np.isnan(got["time_err"][far]))
    assert np.array_equal(got["transit_time"][far], got["linear_time"][far] + got["shift"][far])


def test_plan_and_graph_capture():
    est = E()
    t, y, sigma = main("10min")
    y2 = main("10min", 1.0)[1][::-1].copy()
    g = O.main_template()
    td, yd = dev(t), dev(y)
    plan = est.timing_plan(td, **O.SEARCH)
    n_k = O.epochs(t, O.SEARCH["period"], O.SEARCH["t0"], O.SEARCH["window"])
    lo, hi = O.windows(t, O.SEARCH["t0"] + O.SEARCH["period"] * n_k, O.SEARCH["window"])
    assert np.array_equal(plan.transit_ind, n_k) and np.array_equal(plan.lo.cpu().numpy(), lo) and np.array_equal(plan.hi.cpu().numpy(), hi)
    assert plan.max_window == int((hi - lo + 1).max()) and np.array_equal(plan.shifts.cpu().numpy(), O.shifts(0.03, 121)[0])
    assert np.array_equal(plan.linear_time.cpu().numpy(), O.SEARCH["t0"] + O.SEARCH["period"] * n_k)
    kw = dict(template=g, return_curve=True, plan=plan)
    eager = host(est.transit_times(td, yd, sigma, **kw))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # (torch wants a warm-up on the capturing stream)
        est.transit_times(td, yd, sigma, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = est.transit_times(td, yd, sigma, **kw)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = host(res)
    assert same(eager, got)
    check("graph replay", got, O.reference(t, y, sigma, template=g, **O.SEARCH))
    yd.copy_(dev(y2))                                                   # new data in the captured input, same graph
    graph.replay()
    torch.cuda.synchronize()
    check("graph replay, new data", host(res), O.reference(t, y2, sigma, template=g, **O.SEARCH))
    with pytest.raises(ValueError, match="plan was made"):
        est.transit_times(td[:-1], yd[:-1], sigma, template=g, plan=plan)


def test_ttv_estimator_hands_over_to_a_ttv_orbit():
    import exoplanet_amd as xo
    from exoplanet_amd.orbits import KeplerianOrbit, TTVOrbit

    est = E()
    t, y, sigma = main("2min")                                          # (out of transit around 0)
    search = {k: v for k, v in O.SEARCH.items() if k not in ("period", "t0", "duration")}
    res = est.ttv_estimator(t, y, sigma, period=2.345, t0=1.0, duration=0.2, ror=0.1, b=0.3, **search)
    timing = res["timing"]
    rep = O.science("ttv_estimator, 2min", timing)
    assert np.array_equal(timing["transit_ind"], np.arange(12)) and res["transit_inds"].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]
    assert res["transit_inds"].dtype == np.int64 and isinstance(res["period"], float) and isinstance(res["t0"], float)
    assert np.array_equal(res["transit_times"], timing["transit_time"][timing["valid"]])
    line = res["t0"] + res["period"] * res["transit_inds"]
    assert np.allclose(res["ttvs"], res["transit_times"] - line, rtol=0, atol=1e-12)
    assert res["ttv_dof"] == 9 and abs(res["period"] - 2.345) < 1e-3 and abs(res["t0"] - 1.0) < 1e-2
    print(f"[ttv_estimator] ttv_chi2 / ttv_dof = {res['ttv_chi2'] / res['ttv_dof']:.1f}, odd_even_sigma = {res['odd_even_sigma']:.2f}, "
          f"depth odd {res['depth_odd']:.5f} even {res['depth_even']:.5f}, period {res['period']:.6f}, t0 {res['t0']:.5f}")
    assert res["ttv_chi2"] / res["ttv_dof"] > 50                        # the sine is 25 time_err tall
    assert abs(res["odd_even_sigma"]) < 4
    assert rep["time_err"][1] < 5e-4
    # n_template and the bins of transit_template agree
    again = est.transit_times(dev(t), dev(y), sigma, template=est.transit_template(256, 0.1, 0.3), **O.SEARCH)
    assert np.array_equal(again["transit_time"].cpu().numpy(), timing["transit_time"], equal_nan=True)
    coarse = est.transit_times(dev(t), dev(y), sigma, n_template=64, ror=0.1, b=0.3, **O.SEARCH)
    by_hand = est.transit_times(dev(t), dev(y), sigma, template=est.transit_template(64, 0.1, 0.3), **O.SEARCH)
    assert np.array_equal(coarse["shift"].cpu().numpy(), by_hand["shift"].cpu().numpy(), equal_nan=True)
    # the hand-over: the measured times describe the light curve better than the refit line does
    td = dev(t)
    star = xo.LimbDarkLightCurve(0.4804, 0.1867)
    ttv_orbit = TTVOrbit(transit_times=[dev(res["transit_times"])], transit_inds=[res["transit_inds"]], b=dev([0.3]),
                         duration=dev([0.2]), ror=dev([0.1]))
    line_orbit = KeplerianOrbit(period=dev([res["period"]]), t0=dev([res["t0"]]), b=dev([0.3]), duration=dev([0.2]), ror=dev([0.1]))
    misfit = []
    for orbit in (ttv_orbit, line_orbit):
        model = star.get_light_curve(orbit=orbit, r=dev([0.1]), t=td).sum(-1).cpu().numpy()
        misfit.append(float(((y - model.reshape(y.shape)) ** 2).sum()))
    print(f"[hand-over] sum (y - model)^2: TTVOrbit {misfit[0]:.6e}, linear ephemeris {misfit[1]:.6e}")
    assert misfit[0] < misfit[1]
