"""GPU: the local-polynomial trend kernel (csrc/exo_trend.hip) behind exoplanet_amd.estimators.running_location and flatten
with order = 1 or 2, against the brute-force numpy restatement of DESIGN.md section 21 (tests/trend_oracle.py), by the rule of
DESIGN.md 9.5 / 19.4: what float64 costs the oracle itself is the unit, the kernel gets 16 of them (floor: 1e-13 max|y|)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flatten_oracle as F  # noqa: E402
import trend_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256            # cadences per workgroup (csrc/exo_trend.hip, kTile)
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


def bits(x):
    return x.view(torch.int64)


def empty_windows(t, wl, exclude, brk, cutoff=0.0):
    """where the definition puts NaN: cut by edge_cutoff, or no participating cadence"""
    lo, hi, edge = F.windows(t, wl, brk, cutoff)
    ex = np.zeros(t.size, dtype=bool) if exclude is None else exclude
    return edge | np.array([not np.any(~ex[a:b + 1]) for a, b in zip(lo, hi)])


def check(label, t, y, wl, order, rescale, exclude=None, brk=None, cutoff=0.0, cval=5.0, n_iter=10, cadences=None):
    """the kernel on every cadence: NaN exactly where the definition says; on `cadences` (None: all): within 16 units of the
    long-double oracle, trend and scale"""
    cadences = np.arange(t.size) if cadences is None else np.asarray(cadences)
    kw = dict(exclude=exclude, break_tolerance=brk, edge_cutoff=cutoff, cval=cval, n_iter=n_iter, rescale=rescale, cadences=cadences)
    f64, s64 = O.running_trend(t, y, wl, order, **kw)
    want, swant = O.running_trend(t, y, wl, order, dtype=np.longdouble, **kw)
    got, scale = E().running_location(dev(t), dev(y), wl, order=order, rescale=rescale, cval=cval, n_iter=n_iter, break_tolerance=brk,
                                      edge_cutoff=cutoff, exclude=None if exclude is None else dev(exclude, torch.bool),
                                      return_scale=True)
    got, scale = host(got), host(scale)
    nan = empty_windows(t, wl, exclude, brk, cutoff)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(scale), nan), label
    assert np.array_equal(np.isnan(want[cadences]).astype(bool), nan[cadences])
    ok = cadences[~nan[cadences]]
    size = np.abs(y).max()
    out = {}
    for name, g, f, w in (("trend", got, f64, want), ("scale", scale, s64, swant)) if ok.size else ():
        unit = np.abs(f[ok] - w[ok]).astype(np.float64)
        err = np.abs(g[ok] - w[ok]).astype(np.float64)
        print(f"{label} order={order} rescale={rescale} cval={cval} n_iter={n_iter} {name}: largest unit = {unit.max() / size:.2e} max|y|, "
              f"largest kernel - long double = {err.max() / size:.2e} max|y|, differs from the float64 oracle at "
              f"{int(np.sum(g[ok] != f[ok]))} of {ok.size}")
        out[name] = (unit, err)
    for name, (unit, err) in out.items():
        assert np.all(err <= np.maximum(16 * unit, 1e-13 * size)), (label, name)
    return got, scale


@functools.lru_cache(maxsize=None)
def main_input(variant):
    return F.main_input(variant)


def some_cadences(t):
    """every third cadence, and those beside the gap, the lone last one and its neighbour"""
    gap = int(np.argmax(np.diff(t[:-1]))) + 1
    return np.unique(np.concatenate([np.arange(0, t.size, 3), [gap - 2, gap - 1, gap, gap + 1, t.size - 2, t.size - 1]]))


def test_main_input_is_what_the_tests_assume():
    t, y, _ = main_input("plain")
    lo, hi, _ = F.windows(t, 1.0, break_tolerance=BREAK)
    assert t.size == 1519 and int((hi - lo + 1).max()) == 328 and hi[-1] == lo[-1] == 1518
    assert int(empty_windows(t, 0.02, main_input("excluded")[2], BREAK).sum()) == 117      # the NaN path is on the table
    assert E().MAX_TREND_WINDOW == 4096


@pytest.mark.parametrize("rescale", (0, 1))
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("wl", WINDOWS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_trend_within_sixteen_units(variant, wl, order, rescale):
    t, y, exclude = main_input(variant)
    check(f"{variant} {wl}", t, y, wl, order, rescale, exclude=exclude, brk=BREAK)           # (every cadence)


@pytest.mark.parametrize("cval,n_iter", [(5.0, 1), (2.0, 10)])
@pytest.mark.parametrize("order", (1, 2))
def test_trend_other_iteration_count_and_tuning(order, cval, n_iter):
    t, y, exclude = main_input("excluded")
    check("excluded 0.3", t, y, 0.3, order, 1, exclude=exclude, brk=BREAK, cval=cval, n_iter=n_iter, cadences=some_cadences(t))


def uniform_case(n, wl, order, seed=0):
    rs = np.random.RandomState(1000 + n + seed)
    t = np.arange(n, dtype=np.float64)
    y = 1 + 1e-2 * np.sin(t / 20.0) + 1e-3 * rs.randn(n)
    if seed % 2:
        y = np.round(y * 2000) / 2000
    return check(f"n={n} window={wl}", t, y, wl, order, 1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_geometry_sizes_around_the_wave_and_the_tile(n):
    uniform_case(n, 8.0, 2)                             # windows of 9 cadences, fewer at the ends
    uniform_case(n, 8.0, 1, seed=1)
    uniform_case(n, 0.0, 2, seed=1)                     # the cadence alone


def test_geometry_windows_wider_than_a_tile():
    n = 2 * TILE + 3                                    # three tiles
    uniform_case(n, 300.0, 2)                           # 301 cadences: wider than a tile
    uniform_case(n, 3.0 * n, 1, seed=1)                 # every window holds the whole series


def test_the_widest_window_allowed_passes_and_one_more_raises():
    cap = E().MAX_TREND_WINDOW
    rs = np.random.RandomState(4)
    th = np.arange(cap + 1, dtype=np.float64)
    y = 1 + 1e-2 * np.sin(th / 700.0) + 1e-3 * rs.randn(cap + 1)
    t = dev(th)
    plan = E().location_plan(t[:cap], 4.0 * cap)
    assert plan.max_window == cap
    got = host(E().running_location(t[:cap], dev(y[:cap]), plan=plan, order=2))
    assert not np.isnan(got).any()
    at = [0, 1, cap // 2, cap - 1]
    f64, _ = O.running_trend(th[:cap], y[:cap], 4.0 * cap, 2, cadences=at)
    want, _ = O.running_trend(th[:cap], y[:cap], 4.0 * cap, 2, cadences=at, dtype=np.longdouble)
    unit, err = np.abs(f64[at] - want[at]).astype(np.float64), np.abs(got[at] - want[at]).astype(np.float64)
    print(f"window of {cap}: largest unit {unit.max():.2e}, largest kernel - long double {err.max():.2e}")
    assert np.all(err <= np.maximum(16 * unit, 1e-13 * np.abs(y).max()))
    with pytest.raises(ValueError, match=rf"{cap + 1} cadences, more than the {cap}"):
        E().running_location(t, dev(y), 4.0 * cap, order=2)
    wide = E().location_plan(t, 4.0 * cap)               # (the location itself still takes it)
    assert wide.max_window == cap + 1
    with pytest.raises(ValueError, match=rf"{cap + 1} cadences, more than the {cap}"):
        E().running_location(t, dev(y), plan=wide, order=1)
    assert not bool(torch.isnan(E().running_location(t, dev(y), plan=wide, method="median")).any())
    # a cadence whose window is wider than the max_window the kernel was promised gets NaN, not a wrong value
    small = E().location_plan(t[:600], 40.0)
    wider = E().location_plan(t[:600], 80.0)
    lied = E().LocationPlan(wider.lo, wider.hi, wider.edge, small.max_window)
    got = host(E().running_location(t[:600], dev(y[:600]), plan=lied, order=2))
    honest = host(E().running_location(t[:600], dev(y[:600]), plan=wider, order=2))
    width = host(wider.hi - wider.lo + 1)
    assert np.all(np.isnan(got[width > small.max_window])) and np.isnan(got).sum() < 600
    assert np.array_equal(got[~np.isnan(got)], honest[~np.isnan(got)])


def test_edge_cutoff_and_break_tolerance_give_nan_where_the_definition_says():
    t, y, exclude = main_input("excluded")
    cadences = some_cadences(t)[::3]
    for wl, cutoff, brk in ((0.3, 0.1, BREAK), (0.02, 0.0, BREAK), (0.3, 0.25, None), (1.0, 0.1, 0.004)):
        got, _ = check(f"window={wl} edge_cutoff={cutoff} break_tolerance={brk}", t, y, wl, 2, 1, exclude=exclude, brk=brk, cutoff=cutoff,
                       cadences=cadences)
        edge = F.windows(t, wl, brk, cutoff)[2]
        if cutoff == 0.25:                               # (the case itself has edges, and interior cadences too)
            assert edge.any() and not edge.all() and np.all(np.isnan(got[edge]))
        if wl == 0.02:
            assert np.isnan(got).any() and not edge.any()


def test_order_zero_through_the_new_keyword_is_the_call_without_it():
    t, y, exclude = main_input("excluded")
    td, yd, xd = dev(t), dev(y), dev(exclude, torch.bool)
    for method in ("median", "biweight"):
        old, old_scale = E().running_location(td, yd, 0.3, method=method, exclude=xd, break_tolerance=BREAK, return_scale=True)
        new, new_scale = E().running_location(td, yd, 0.3, method=method, exclude=xd, break_tolerance=BREAK, return_scale=True, order=0,
                                              rescale=3)
        assert torch.equal(bits(old), bits(new)) and torch.equal(bits(old_scale), bits(new_scale))
    first = E().running_location(td, yd, 0.3, exclude=xd, break_tolerance=BREAK, order=1)
    assert not torch.equal(bits(first), bits(old))      # (and the keyword does reach the other kernel)


def test_batch_rows_are_bitwise_the_single_call_and_runs_repeat():
    t = main_input("plain")[0]
    y = np.stack([main_input(v)[1] for v in VARIANTS])
    rs = np.random.RandomState(8)
    exclude = rs.rand(3, t.size) < 0.2
    td, yd, xd = dev(t), dev(y), dev(exclude, torch.bool)
    plan = E().location_plan(td, 0.3, break_tolerance=BREAK)
    for order in (1, 2):
        a, sa = E().running_location(td, yd, plan=plan, order=order, exclude=xd, return_scale=True)
        b, sb = E().running_location(td, yd, plan=plan, order=order, exclude=xd, return_scale=True)
        assert a.shape == (3, t.size) and torch.equal(bits(a), bits(b)) and torch.equal(bits(sa), bits(sb))
        for r in range(3):
            one, s1 = E().running_location(td, yd[r], plan=plan, order=order, exclude=xd[r], return_scale=True)
            assert one.shape == (t.size,) and torch.equal(bits(one), bits(a[r])) and torch.equal(bits(s1), bits(sa[r]))
        # one exclude row, (N,), for every series
        shared = E().running_location(td, yd, plan=plan, order=order, exclude=xd[0])
        for r in range(3):
            assert torch.equal(bits(shared[r]), bits(E().running_location(td, yd[r], plan=plan, order=order, exclude=xd[0])))
        # without the scale: the same trend
        assert torch.equal(bits(E().running_location(td, yd, plan=plan, order=order, exclude=xd)), bits(a))


def test_a_call_with_a_plan_is_captured_and_replayed():
    t, y1, _ = main_input("plain")
    y2 = main_input("ties")[1]
    td = dev(t)
    plan = E().location_plan(td, 0.3, break_tolerance=BREAK)
    eager = [E().running_location(td, dev(y), plan=plan, order=2) for y in (y1, y2)]
    buf = dev(y1).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = E().running_location(td, buf, plan=plan, order=2)
    for y, want in zip((y1, y2), eager):
        buf.copy_(dev(y))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(want))


def test_end_to_end_flatten_with_a_parabola_then_box_search():
    """the input of DESIGN.md 21.3: ramps after each segment's start, variability of 8e-3 over transits of 2.5e-3"""
    t, y, truth, in_transit = O.science_input()
    period = 2.345
    rms = {}
    for order in (0, 2):
        flat, trend = E().flatten(t, y, 1.5, order=order, break_tolerance=0.5, return_trend=True)
        assert isinstance(flat, np.ndarray) and np.array_equal(flat, y / trend) and not np.isnan(flat).any()
        rms[order] = np.sqrt(np.mean((flat[~in_transit] - (y / truth)[~in_transit]) ** 2))
    res = E().bls_estimator(t, flat, duration=0.12, min_period=1.0, max_period=5.0)
    found = res["peak_info"]["period"]
    print(f"flattened - truly flat, rms out of transit: order 0 {rms[0]:.2e}, order 2 {rms[2]:.2e}; peak at {found:.4f} d, "
          f"depth {res['peak_info']['depth']:.2e}")
    assert abs(found - period) < 0.005 * period
    assert rms[2] < rms[0]
