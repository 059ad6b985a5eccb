"""GPU: the running location kernels (csrc/exo_detrend.hip) behind exoplanet_amd.estimators.running_location, flatten and sde
against the brute-force numpy restatement of DESIGN.md section 19 (tests/flatten_oracle.py).  Median and MAD are compared
EXACTLY (selection does no arithmetic beyond single correctly rounded operations); the biweight by the rule of DESIGN.md 9.5:
what float64 costs the oracle itself is the unit, the kernel gets 16 of them."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flatten_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256            # cadences per workgroup (csrc/exo_detrend.hip, kTile)
VARIANTS = ("plain", "ties", "excluded")
WINDOWS = (0.02, 0.3, 1.0)
BREAK = 0.5


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(x):
    return x.cpu().numpy()


def E():
    from exoplanet_amd import estimators

    return estimators


def same(got, want):
    """equal as numbers, NaNs in the same places"""
    return np.array_equal(got, want, equal_nan=True)


@functools.lru_cache(maxsize=None)
def oracle(variant, wl, cval=5.0, n_iter=10, every=1):
    """median, MAD, and the biweight in float64 and in long double, on every `every`-th cadence of the main input"""
    t, y, exclude = O.main_input(variant)
    lo, hi, _ = O.windows(t, wl, break_tolerance=BREAK)
    ex = np.zeros(t.size, dtype=bool) if exclude is None else exclude
    med, mad, bw, bwl = (np.full(t.size, np.nan) for _ in range(4))
    for i in range(0, t.size, every):
        v = y[lo[i]:hi[i] + 1][~ex[lo[i]:hi[i] + 1]]
        if v.size == 0:
            continue
        med[i] = O.median(v)
        mad[i] = O.mad(v, med[i])
        bw[i] = O.biweight(v, med[i], mad[i], cval, n_iter)
        vl = v.astype(np.longdouble)
        ml = O.median(vl)
        bwl[i] = float(O.biweight(vl, ml, O.mad(vl, ml), cval, n_iter))
    return med, mad, bw, bwl, (hi - lo + 1)


def test_main_input_is_what_the_tests_assume():
    t, y, _ = O.main_input()
    assert t.size == 1519 and np.all(np.diff(t) >= 0)
    widths = [oracle("plain", wl)[4] for wl in WINDOWS]
    assert [int(w.max()) for w in widths] == [17, 114, 328] and int(widths[0].min()) == 1
    empty = np.isnan(oracle("excluded", 0.02)[0])
    assert int(empty.sum()) == 117                      # the NaN path is on the table
    # the plan's windows are the oracle's, and the widest comes back as a Python int
    plan = E().location_plan(dev(t), 0.3, break_tolerance=BREAK)
    lo, hi, _ = O.windows(t, 0.3, break_tolerance=BREAK)
    assert np.array_equal(host(plan.lo), lo) and np.array_equal(host(plan.hi), hi) and plan.max_window == 114
    assert type(plan.max_window) is int and not bool(plan.edge.any())


@pytest.mark.parametrize("wl", WINDOWS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_median_and_mad_are_exact(variant, wl):
    t, y, exclude = O.main_input(variant)
    med, mad, _, _, _ = oracle(variant, wl)
    ex = None if exclude is None else dev(exclude, torch.bool)
    got, scale = E().running_location(dev(t), dev(y), wl, method="median", exclude=ex, break_tolerance=BREAK, return_scale=True)
    assert same(host(got), med)
    assert same(host(scale), mad)
    # without the scale the kernel skips the MAD: the same trend
    assert same(host(E().running_location(dev(t), dev(y), wl, method="median", exclude=ex, break_tolerance=BREAK)), med)


def check_biweight(variant, wl, cval, n_iter, every):
    t, y, exclude = O.main_input(variant)
    _, mad, bw, want, _ = oracle(variant, wl, cval, n_iter, every)
    ex = None if exclude is None else dev(exclude, torch.bool)
    got, scale = E().running_location(dev(t), dev(y), wl, exclude=ex, break_tolerance=BREAK, cval=cval, n_iter=n_iter, return_scale=True)
    got, scale = host(got)[::every], host(scale)[::every]
    mad, bw, want = mad[::every], bw[::every], want[::every]
    size = np.abs(y).max()
    assert same(scale, mad) and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    unit = np.abs(bw[ok] - want[ok]).max()
    err = np.abs(got[ok] - want[ok]).max()
    print(f"{variant} {wl} cval={cval} n_iter={n_iter}: unit = {unit / size:.2e} max|y|, kernel - long double = {err / size:.2e} max|y|")
    assert unit <= 1e-12 * size                         # (else: another input, not a wider tolerance)
    assert err <= max(16 * unit, 1e-13 * size)


@pytest.mark.parametrize("wl", WINDOWS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_biweight_within_sixteen_units(variant, wl):
    """measured: unit <= 1.07e-15 max|y| on all nine, and the kernel's error equals it"""
    check_biweight(variant, wl, 5.0, 10, 1)


@pytest.mark.parametrize("cval,n_iter", [(5.0, 1), (5.0, 40), (2.0, 10)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_biweight_other_iteration_counts_and_tuning(variant, cval, n_iter):
    """(every fourth cadence: the long-double oracle of 40 iterations is the slow part)"""
    check_biweight(variant, 0.3, cval, n_iter, 4)


def uniform_case(n, wl, t=None, seed=0):
    rs = np.random.RandomState(1000 + n + seed)
    t = np.arange(n, dtype=np.float64) if t is None else t
    y = np.round(rs.randn(n) * 8) / 8 if seed % 2 else rs.randn(n)
    want, want_scale = O.running_location(t, y, wl, "median")
    got, scale = E().running_location(dev(t), dev(y), wl, method="median", return_scale=True)
    assert same(host(got), want), (n, wl)
    assert same(host(scale), want_scale), (n, wl)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_geometry_sizes_around_the_wave_and_the_tile(n):
    uniform_case(n, 4.0)                                # windows of 5 cadences
    uniform_case(n, 0.0, seed=1)                        # the cadence alone


def test_geometry_windows_wider_than_a_tile():
    n = 2 * TILE + 3                                    # three tiles
    uniform_case(n, 300.0)                              # 301 cadences: wider than a tile
    uniform_case(n, 3.0 * n, seed=1)                    # every window holds the whole series
    # runs of equal times: a window holds whole runs, and window_length = 0 the cadence's own run
    t = np.floor(np.arange(n) / 3.0)
    uniform_case(n, 0.0, t=t)
    uniform_case(n, 2.0, t=t, seed=1)
    lo, hi = E().location_plan(dev(t), 0.0).lo, E().location_plan(dev(t), 0.0).hi
    assert np.array_equal(host(lo), 3 * (np.arange(n) // 3)) and np.array_equal(host(hi), np.minimum(3 * (np.arange(n) // 3) + 2, n - 1))


def test_the_widest_window_allowed_passes_and_one_more_raises():
    cap = E().MAX_WINDOW
    rs = np.random.RandomState(4)
    y = rs.randn(cap + 1)
    t = dev(np.arange(cap + 1, dtype=np.float64))
    plan = E().location_plan(t[:cap], 4.0 * cap)
    assert plan.max_window == cap
    got, scale = E().running_location(t[:cap], dev(y[:cap]), plan=plan, method="median", return_scale=True)
    med = np.median(y[:cap])
    assert np.all(host(got) == med) and np.all(host(scale) == np.median(np.abs(y[:cap] - med)))
    with pytest.raises(ValueError, match=rf"{cap + 1} cadences, more than the {cap}"):
        E().running_location(t, dev(y), 4.0 * cap)
    with pytest.raises(ValueError, match="non-decreasing"):
        E().location_plan(t.flip(0), 1.0)
    # a cadence whose window is wider than the max_window the kernel was promised gets NaN, not a wrong value
    small = E().location_plan(t[:600], 40.0)
    wide = E().location_plan(t[:600], 80.0)
    lied = E().LocationPlan(wide.lo, wide.hi, wide.edge, small.max_window)
    got = host(E().running_location(t[:600], dev(y[:600]), plan=lied, method="median"))
    want, _ = O.running_location(np.arange(600.0), y[:600], 80.0, "median")
    width = host(wide.hi - wide.lo + 1)
    assert np.all(np.isnan(got[width > small.max_window])) and np.isnan(got).sum() < 600
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(got)])


def test_edge_cutoff_and_break_tolerance_give_nan_where_the_definition_says():
    t, y, exclude = O.main_input("excluded")
    for wl, cutoff, brk in ((0.3, 0.1, BREAK), (0.02, 0.0, BREAK), (0.3, 0.25, None), (1.0, 0.1, 0.004)):
        want, want_scale = O.running_location(t, y, wl, "median", exclude=exclude, break_tolerance=brk, edge_cutoff=cutoff)
        lo, hi, edge = O.windows(t, wl, brk, cutoff)
        empty = np.array([not np.any(~exclude[a:b + 1]) for a, b in zip(lo, hi)])
        got, scale = E().running_location(dev(t), dev(y), wl, method="median", exclude=dev(exclude, torch.bool), break_tolerance=brk,
                                          edge_cutoff=cutoff, return_scale=True)
        assert np.array_equal(np.isnan(host(got)), edge | empty) and np.array_equal(np.isnan(host(scale)), edge | empty)
        assert same(host(got), want) and same(host(scale), want_scale)
        assert np.array_equal(host(E().location_plan(dev(t), wl, brk, cutoff).edge), edge)
        if cutoff == 0.25:                               # (the case itself has edges, and interior cadences too)
            assert edge.any() and not edge.all()
        if wl == 0.02:
            assert empty.any() and not edge.any()


def test_batch_rows_are_bitwise_the_single_call_and_runs_repeat():
    t = O.main_input()[0]
    y = np.stack([O.main_input(v)[1] for v in VARIANTS])
    rs = np.random.RandomState(8)
    exclude = rs.rand(3, t.size) < 0.2
    td, yd, xd = dev(t), dev(y), dev(exclude, torch.bool)
    plan = E().location_plan(td, 0.3, break_tolerance=BREAK)
    for method in ("median", "biweight"):
        a, sa = E().running_location(td, yd, plan=plan, method=method, exclude=xd, return_scale=True)
        b, sb = E().running_location(td, yd, plan=plan, method=method, exclude=xd, return_scale=True)
        assert a.shape == (3, t.size) and torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert torch.equal(sa.view(torch.int64), sb.view(torch.int64))
        for r in range(3):
            one, s1 = E().running_location(td, yd[r], plan=plan, method=method, exclude=xd[r], return_scale=True)
            assert one.shape == (t.size,) and torch.equal(one.view(torch.int64), a[r].view(torch.int64))
            assert torch.equal(s1.view(torch.int64), sa[r].view(torch.int64))
        # one exclude row for every series
        shared = E().running_location(td, yd, plan=plan, method=method, exclude=xd[0])
        assert torch.equal(shared[1].view(torch.int64), E().running_location(td, yd[1], plan=plan, method=method, exclude=xd[0]).view(torch.int64))
    want, _ = O.running_location(t, y[2], 0.3, "median", exclude=exclude[2], break_tolerance=BREAK)
    assert same(host(E().running_location(td, yd, plan=plan, method="median", exclude=xd)[2]), want)


def test_a_call_with_a_plan_is_captured_and_replayed():
    t, y1, _ = O.main_input("plain")
    y2 = O.main_input("ties")[1]
    td = dev(t)
    plan = E().location_plan(td, 0.3, break_tolerance=BREAK)
    eager = [E().running_location(td, dev(y), plan=plan) for y in (y1, y2)]
    buf = dev(y1).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = E().running_location(td, buf, plan=plan)
    for y, want in zip((y1, y2), eager):
        buf.copy_(dev(y))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), want.view(torch.int64))


def test_sde_against_numpy():
    rs = np.random.RandomState(31)
    power = 50 + 10 * np.sin(np.arange(600) / 90.0) + rs.randn(600)
    power[417] += 25.0
    power[[3, 300]] = -np.inf
    want = O.sde(power, 151)
    got = E().sde(power, 151)
    assert isinstance(got, np.ndarray) and np.array_equal(np.isnan(got), np.isnan(want)) and list(np.flatnonzero(np.isnan(got))) == [3, 300]
    ok = ~np.isnan(want)
    # the trend is exact; the standard deviation sums 598 terms in another order: a few hundred roundings at the most
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12 * np.abs(want[ok]).max()
    assert int(np.nanargmax(got)) == 417 and got[417] > 8
    again = E().sde(dev(power), 151)
    assert isinstance(again, torch.Tensor) and same(host(again), got)


def test_end_to_end_flatten_then_box_search():
    """variability of 8e-3 over a transit of 2.5e-3: the raw search finds the variability, the flattened one the planet"""
    rs = np.random.RandomState(2718)
    t = np.sort(rs.uniform(0, 20, 3000))
    t = t[(t < 9.0) | (t > 10.5)]
    y = 1 + 8e-3 * np.sin(2 * np.pi * t / 3.1 + 0.4) + 3e-3 * np.sin(2 * np.pi * t / 1.37) + 4e-4 * rs.randn(t.size)
    period, depth = 2.345, 2.5e-3
    y[np.abs((t - 1.0 + 0.5 * period) % period - 0.5 * period) < 0.06] -= depth
    periods = np.sort(np.append(np.exp(np.linspace(np.log(1.0), np.log(5.0), 600)), period))

    def search(series):
        res = E().bls_power(dev(t), dev(series - series.mean()), periods=periods, durations=[0.12])
        k = int(torch.argmax(res["power"]))
        return periods[k], float(res["depth"][k])

    raw, _ = search(y)
    assert abs(raw - period) > 0.01 * period
    for method in ("biweight", "median"):
        flat, trend = E().flatten(t, y, 1.0, method=method, return_trend=True)
        assert isinstance(flat, np.ndarray) and np.array_equal(flat, y / trend)
        found, found_depth = search(flat)
        print(f"{method}: raw peak {raw:.4f} d, flattened peak {found:.4f} d, depth {found_depth:.3e}")
        assert found == period
        assert abs(found_depth - depth) <= 0.1 * depth
