"""GPU: exoplanet_amd.estimators -- the box-least-squares and Lomb-Scargle kernels against the brute-force numpy restatement
of their definitions (tests/estimators_oracle.py), and the reference's five estimator tests restated on this package.

Tolerances are not constants.  Every comparison computes, on its own input, the largest relative difference between the
oracle run in float64 and in np.longdouble, and allows 16 times that with a floor of 1e-13: the kernels' sums differ from
numpy's only in their order; 16 covers the arrival order of the atomic adds and the wider spread of a tree sum, and the floor
keeps a lucky exact oracle from demanding bit equality.  The box search is compared on `power`; because a near-tie may
legitimately pick another box, the other six outputs are checked for consistency instead: the oracle's statistics of the box
that the returned (period, duration, transit_time) names are the returned ones, and its objective is the returned power.
Periods that the oracle flags as fragile (a cadence within 1e-9 of a bin edge) are left out, at most 1 % of them.

Measured on an MI355X (the figures are printed before each assertion; DESIGN.md section 9.5 records them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimators_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR, FACTOR = 1e-13, 16.0


def T(a, dev):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=dev)


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def bls_input(seed=721, n=5000, span=27.0, period=2.345, depth=0.1, duration=0.2, t0=1.0):
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, span, n))
    y = 1e-3 * rs.randn(n)
    y[np.abs((t - t0 + 0.5 * period) % period - 0.5 * period) < 0.5 * duration] -= depth
    return t, y


def sine_input(seed=9502):
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0, 10, 500))
    return t, 4.5 * np.sin(2 * np.pi * t / 2.345)


def check_bls(name, got, t, y, yerr, periods, durations, oversample, objective, max_fragile=0.01):
    """`got`: host arrays of one series from bls_power.  -> (tolerance, largest error of power)"""
    want = O.bls_power(t, y, yerr, periods, durations, oversample, objective)
    exact = O.bls_power(t, y, yerr, periods, durations, oversample, objective, dtype=np.longdouble)
    keep = ~(want["fragile"] | exact["fragile"])
    finite = np.isfinite(want["power"])
    unit = O.rel_diff(want["power"][keep & finite], exact["power"][keep & finite])
    tol = max(FACTOR * unit, FLOOR)
    err = O.rel_diff(got["power"][keep & finite], want["power"][keep & finite])
    print(f"[{name}] periods {len(periods)}, fragile {int((~keep).sum())}, float64 vs longdouble oracle {unit:.2e}, "
          f"tolerance {tol:.2e}, power error {err:.2e}")
    assert (~keep).sum() <= max_fragile * len(periods)
    assert np.array_equal(np.isfinite(got["power"][keep]), finite[keep])
    assert err <= tol
    worst = 0.0
    row = 3 if objective == "likelihood" else 2
    for i in np.flatnonzero(keep & finite):
        box = O.bls_at(t, y, yerr, periods[i], durations, oversample, got["duration"][i], got["transit_time"][i])
        mine = np.array([got[k][i] for k in ("depth", "depth_err", "depth_snr", "log_likelihood")])
        worst = max(worst, float(np.max(np.abs(mine - box) / np.abs(box))), abs(got["power"][i] - box[row]) / abs(box[row]))
    print(f"[{name}] consistency of the returned box: {worst:.2e}")
    assert worst <= tol
    return tol, err


@pytest.mark.parametrize("objective", ["likelihood", "snr"])
@pytest.mark.parametrize("with_yerr", [False, True])
def test_bls_power_against_the_oracle(dev, objective, with_yerr):
    from exoplanet_amd.estimators import bls_power

    t, y = bls_input()
    yerr = 1e-3 * (0.5 + np.random.RandomState(5).uniform(size=t.size)) if with_yerr else None
    periods = np.exp(np.linspace(np.log(0.5), np.log(13.5), 5000))
    durations = (0.1, 0.2, 0.4)
    got = host(bls_power(T(t, dev), T(y, dev), T(yerr, dev), periods=periods, durations=durations, oversample=10, objective=objective))
    assert got["power"].shape == (5000,) and np.array_equal(got["period"], periods)
    check_bls(f"reference input, {objective}, yerr {with_yerr}", got, t, y, yerr, periods, durations, 10, objective)
    assert abs(periods[np.argmax(got["power"])] - 2.345) < 0.01 * 2.345


def test_bls_large_bin_counts_and_the_switch_of_paths(dev):
    from exoplanet_amd.estimators import bls_plan, bls_power

    t, y = bls_input(seed=11, n=20000, span=1400.0, period=411.7, depth=0.02, duration=0.05, t0=100.0)
    durations = (0.05, 0.1)
    periods = np.linspace(300.0, 700.0, 64)
    assert bls_plan(periods, durations, 10)[2].max() > 140000
    got = host(bls_power(T(t, dev), T(y, dev), periods=periods, durations=durations))
    check_bls("140 000 bins", got, t, y, None, periods, durations, 10, "likelihood")
    # a range across the largest histogram that LDS holds (3835 bins): both kernels in one call, neighbours on either side
    periods = np.linspace(19.0, 19.25, 40)
    n_bins = bls_plan(periods, durations, 10)[2]
    assert n_bins.min() < 3835 < n_bins.max()
    got = host(bls_power(T(t, dev), T(y, dev), periods=periods, durations=durations))
    check_bls("switch of paths", got, t, y, None, periods, durations, 10, "likelihood")


def test_bls_batches_order_gaps_and_degenerate_input(dev):
    from exoplanet_amd.estimators import bls_power

    t, y = bls_input(n=3000)
    rs = np.random.RandomState(2)
    Y = y[None] + 2e-3 * rs.randn(7, t.size)
    E = 1e-3 * (0.5 + rs.uniform(size=(7, t.size)))
    periods = np.exp(np.linspace(np.log(0.5), np.log(13.5), 300))
    kw = dict(periods=periods, durations=(0.1, 0.2, 0.4))
    batch = host(bls_power(T(t, dev), T(Y, dev), T(E, dev), **kw))
    assert batch["power"].shape == (7, 300)
    worst = 0.0
    for b in range(7):
        one = host(bls_power(T(t, dev), T(Y[b], dev), T(E[b], dev), **kw))
        series = {k: (v[b] if v.ndim == 2 else v) for k, v in batch.items()}
        tol, _ = check_bls(f"series {b} of a batch", series, t, Y[b], E[b], periods, kw["durations"], 10, "likelihood")
        worst = max(worst, O.rel_diff(series["power"], one["power"]))
        assert O.rel_diff(series["power"], one["power"]) <= tol
    print(f"[batch] batched vs single calls: {worst:.2e}")
    # a shared (N,) yerr and a scalar one
    shared = host(bls_power(T(t, dev), T(Y, dev), T(E[0], dev), **kw))
    check_bls("shared yerr", {k: (v[3] if v.ndim == 2 else v) for k, v in shared.items()}, t, Y[3], E[0], periods, kw["durations"], 10,
              "likelihood")
    scalar = host(bls_power(T(t, dev), T(Y[0], dev), 2e-3, **kw))
    check_bls("scalar yerr", scalar, t, Y[0], np.full(t.size, 2e-3), periods, kw["durations"], 10, "likelihood")
    # unsorted times
    perm = rs.permutation(t.size)
    shuffled = host(bls_power(T(t[perm], dev), T(Y[0][perm], dev), T(E[0][perm], dev), **kw))
    tol, _ = check_bls("unsorted times", shuffled, t, Y[0], E[0], periods, kw["durations"], 10, "likelihood")
    assert O.rel_diff(shuffled["power"], host(bls_power(T(t, dev), T(Y[0], dev), T(E[0], dev), **kw))["power"]) <= tol
    # a gap as long as a duration in every cycle: boxes of no weight are skipped, never chosen
    tg = np.arange(4000) * 0.0100371 + 1e-4 * rs.uniform(size=4000)      # (not on the bin edges: no fragile periods)
    tg = tg[np.fmod(tg, 2.0) > 0.45]
    yg = 1e-3 * rs.randn(tg.size) - 0.05 * (np.abs(np.fmod(tg, 2.0) - 1.3) < 0.1)
    pg = np.array([1.0, 2.0, 4.0, 3.1])
    got = host(bls_power(T(tg, dev), T(yg, dev), periods=pg, durations=(0.2, 0.4)))
    check_bls("gaps", got, tg, yg, None, pg, (0.2, 0.4), 10, "likelihood")
    assert np.all(np.isfinite(got["power"])) and abs(got["transit_time"][1] - 1.3) < 0.03
    # one cadence: no box leaves weight outside itself
    got = host(bls_power(T([3.0], dev), T([1.0], dev), periods=[1.0, 2.5], durations=[0.1]))
    assert np.all(got["power"] == -np.inf)
    for k in O.FIELDS[1:]:
        assert np.all(np.isnan(got[k])), k


def check_ls(name, got, t, y, yerr, freq, want=None):
    exact = O.lomb_scargle_power(t, y, yerr, freq, dtype=np.longdouble)
    f64 = O.lomb_scargle_power(t, y, yerr, freq)
    peak = float(exact.max())
    unit = O.rel_diff(f64, exact, scale=peak)
    tol = max(FACTOR * unit, FLOOR)
    err = O.rel_diff(got, f64 if want is None else want, scale=peak)
    print(f"[{name}] frequencies {len(freq)}, float64 vs longdouble oracle {unit:.2e} of the peak, tolerance {tol:.2e}, "
          f"error {err:.2e} (against longdouble: {O.rel_diff(got, exact, scale=peak):.2e})")
    assert err <= tol
    return tol


def test_lomb_scargle_power_against_least_squares(dev):
    from exoplanet_amd.estimators import lomb_scargle_autofrequency, lomb_scargle_power

    t, y = sine_input()
    freq = lomb_scargle_autofrequency(t)
    df = 1 / (5 * (t.max() - t.min()))
    assert freq[0] == pytest.approx(0.5 * df) and abs(freq[-1] - 5 * 0.5 * 500 * 5 * df) <= 0.5001 * df
    got = lomb_scargle_power(T(t, dev), T(y, dev), frequencies=freq).cpu().numpy()
    assert got.shape == freq.shape
    check_ls("reference input", got, t, y, None, freq)
    assert abs(1 / freq[np.argmax(got)] - 2.345) < 0.02 * 2.345
    rs = np.random.RandomState(1)
    yerr = 0.3 + rs.uniform(size=t.size)
    yn = y + yerr * rs.randn(t.size) + 11.0
    got = lomb_scargle_power(T(t, dev), T(yn, dev), T(yerr, dev), frequencies=freq).cpu().numpy()
    check_ls("heteroscedastic", got, t, yn, yerr, freq)
    # a time origin of 2 457 000 days.  A float64 oracle on the raw times is only good to ~1e-9 there, and even the longdouble
    # one loses digits in 2 pi f t at 3e8 turns (measured: 2e-12 of the peak).  The power does not depend on the origin, so the
    # yardstick is the longdouble oracle on the same float64 times with the mid-time taken off IN longdouble (exact); the
    # tolerance is that of the centred input.
    far = t + 2457000.0
    far_ld = far.astype(np.longdouble)
    centred = far_ld - (far_ld.min() + far_ld.max()) / 2
    exact = O.lomb_scargle_power(centred, yn, yerr, freq, dtype=np.longdouble)
    got = lomb_scargle_power(T(far, dev), T(yn, dev), T(yerr, dev), frequencies=freq).cpu().numpy()
    check_ls("origin 2 457 000", got, centred.astype(np.float64), yn, yerr, freq, want=exact)
    raw = O.rel_diff(O.lomb_scargle_power(far, yn, yerr, freq[::50]), exact[::50], scale=float(exact.max()))
    print(f"[origin 2 457 000] the float64 oracle on the raw times, for comparison: {raw:.2e}")
    # batched, per-series yerr; each row is the single call, bit for bit (the sums have a fixed order)
    Y = yn[None] + rs.randn(5, t.size)
    E = 0.3 + rs.uniform(size=(5, t.size))
    batch = lomb_scargle_power(T(t, dev), T(Y, dev), T(E, dev), frequencies=freq)
    assert batch.shape == (5, len(freq))
    for b in range(5):
        one = lomb_scargle_power(T(t, dev), T(Y[b], dev), T(E[b], dev), frequencies=freq)
        assert torch.equal(batch[b], one)
        check_ls(f"series {b} of a batch", batch[b].cpu().numpy(), t, Y[b], E[b], freq)


# ---- the reference's tests/estimators_test.py, on this package ---------------------------------------------------------------------

def test_bls_estimator(dev):
    from exoplanet_amd.estimators import bls_estimator

    t, y = bls_input()
    results = bls_estimator(t, y)
    print(f"[bls_estimator] {len(results['bls']['period'])} periods, peak at {results['peaks'][0]['period']:.5f}")
    assert len(results["bls"]["period"]) <= len(t)
    assert np.abs(2.345 - results["peaks"][0]["period"]) / 2.345 < 0.01
    info = results["peak_info"]
    assert set(info) == set(O.FIELDS) | {"period"} and abs(info["depth"] - 0.1) < 0.01 and info["duration"] == pytest.approx(0.2)
    assert abs((info["transit_time"] - 1.0 + 0.5 * 2.345) % 2.345 - 0.5 * 2.345) < 0.05
    # device tensors in, the full grid, the other objective
    full = bls_estimator(T(t, dev), T(y, dev), yerr=1e-3, frequency_factor=1.0, objective="snr")
    assert len(full["bls"]["period"]) > len(t)
    assert np.abs(2.345 - full["peaks"][0]["period"]) / 2.345 < 0.01


def test_lomb_scargle_estimator(dev):
    from exoplanet_amd.estimators import lomb_scargle_estimator

    t, y = sine_input()
    results = lomb_scargle_estimator(t, y, min_period=1, max_period=10, filter_period=10.0)
    print(f"[lomb_scargle_estimator] peak at {results['peaks'][0]['period']:.6f}")
    assert np.abs(2.345 - results["peaks"][0]["period"]) / 2.345 < 0.001
    freq, power = results["periodogram"]
    assert freq.shape == power.shape and freq[0] == pytest.approx(0.1) and abs(freq[-1] - 1.0) <= 0.5001 * (freq[1] - freq[0])
    assert 1 <= len(results["peaks"]) <= 2 and type(results["peaks"][0]["period"]) is float


def test_autocorr_estimator(dev):
    from exoplanet_amd.estimators import autocorr_estimator, autocorr_function

    t = np.linspace(0, 10, 500)
    y = 4.5 * np.sin(2 * np.pi * t / 2.345)
    results = autocorr_estimator(t, y, min_period=0.01, max_period=10, smooth=0.0)
    assert np.abs(2.345 - results["peaks"][0]["period"]) / 2.345 < 0.01
    smoothed = autocorr_estimator(T(t, dev), T(y, dev), min_period=0.05, max_period=10)
    assert np.abs(2.345 - smoothed["peaks"][0]["period"]) / 2.345 < 0.02
    tau, acor = results["autocorr"]
    assert tau.shape == acor.shape and acor[0] == pytest.approx(1.0)
    # the autocorrelation function against its definition
    x = np.random.RandomState(0).randn(100)
    xc = x - x.mean()
    want = np.array([xc[: 100 - k] @ xc[k:] for k in range(100)]) / (xc @ xc)
    np.testing.assert_allclose(autocorr_function(T(x, dev)).cpu().numpy(), want, atol=1e-12)


def test_estimate_semi_amplitude(dev):
    from exoplanet_amd.estimators import estimate_semi_amplitude

    t, y = sine_input()
    assert np.allclose(estimate_semi_amplitude(2.345, t, y), 4.5)
    assert np.allclose(estimate_semi_amplitude(2.345, t, y, yerr=np.ones_like(t), t0s=0.5 * 2.345), 4.5)
    two = y + 1.5 * np.cos(2 * np.pi * t / 0.77)
    assert np.allclose(estimate_semi_amplitude([2.345, 0.77], T(t, dev), T(two, dev)), [4.5, 1.5])


def test_estimate_minimum_mass(dev):
    from exoplanet_amd import KeplerianOrbit
    from exoplanet_amd.estimators import estimate_minimum_mass

    t, _ = sine_input()
    orbit = KeplerianOrbit(period=T(2.345, dev), t0=T(0.5, dev), m_planet=T(0.01, dev), incl=T(0.8, dev))
    y = orbit.get_radial_velocity(T(t, dev)).reshape(-1)
    m1 = float((orbit.m_planet * orbit.sin_incl).reshape(-1)[0])
    m_jup_per_m_sun = 1047.5655                       # (IAU nominal GM_sun / GM_jup)
    m2 = estimate_minimum_mass(2.345, t, y)[0] / m_jup_per_m_sun
    m3 = estimate_minimum_mass(2.345, t, y, t0s=0.5)[0] / m_jup_per_m_sun
    print(f"[minimum mass] {m1:.6f} against {m2:.6f} and {m3:.6f} solar masses")
    assert np.abs((m1 - m2) / m1) < 0.01
    assert np.abs((m1 - m3) / m1) < 0.01


# ---- full size, and the stream -------------------------------------------------------------------------------------------------------

def test_bls_full_size(dev):
    """N = 150 000 two-minute cadences, the unthinned grid (frequency_factor = 1), one series"""
    from exoplanet_amd.estimators import bls_autoperiod, bls_power

    n = 150000
    rs = np.random.RandomState(4)
    t = np.arange(n) * (2.0 / 1440.0) + 1e-4 * rs.uniform(size=n)    # (an even grid is commensurate with the bins: all fragile)
    y = 1e-3 * rs.randn(n)
    y[np.abs((t - 1.0 + 0.5 * 7.3219) % 7.3219 - 0.5 * 7.3219) < 0.1] -= 0.003
    periods = bls_autoperiod(t, 0.2)
    assert len(periods) > 3 * n
    res = bls_power(T(t, dev), T(y, dev), periods=periods, durations=[0.2])
    torch.cuda.synchronize()
    got = host(res)
    assert np.all(np.isfinite(got["power"]))
    best = periods[np.argmax(got["power"])]
    print(f"[full size] {len(periods)} periods, best {best:.5f}")
    assert abs(best - 7.3219) < 0.01 * 7.3219
    idx = np.linspace(0, len(periods) - 1, 256).astype(int)
    check_bls("full size, 256 periods", {k: v[idx] for k, v in got.items()}, t, y, None, periods[idx], [0.2], 10, "likelihood")


def test_captured_in_a_graph(dev):
    """host grids: no device-to-host copy, kernels on the caller's stream only -- capturable after one eager call"""
    from exoplanet_amd.estimators import bls_power, lomb_scargle_autofrequency, lomb_scargle_power

    t, y = bls_input(n=2000)
    periods = np.exp(np.linspace(np.log(0.5), np.log(13.5), 200))
    periods[-1] = 45.0                                                # (one period on the workspace path as well)
    td, yd = T(t, dev), T(y, dev)
    freq = lomb_scargle_autofrequency(t, maximum_frequency=5.0)
    kw = dict(periods=periods, durations=(0.1, 0.2))
    eager, eager_ls = bls_power(td, yd, **kw), lomb_scargle_power(td, yd, frequencies=freq)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                      # (torch wants a warm-up on the capturing stream)
        bls_power(td, yd, **kw), lomb_scargle_power(td, yd, frequencies=freq)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, res_ls = bls_power(td, yd, **kw), lomb_scargle_power(td, yd, frequencies=freq)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    tol, _ = check_bls("graph replay", host(res), t, y, None, periods, kw["durations"], 10, "likelihood")
    assert O.rel_diff(res["power"].cpu().numpy(), eager["power"].cpu().numpy()) <= tol
    assert torch.equal(res_ls, eager_ls)
    # new data in the captured inputs, same graph
    yd.copy_(T(y[::-1].copy(), dev))
    graph.replay()
    torch.cuda.synchronize()
    check_bls("graph replay, new data", host(res), t, y[::-1], None, periods, kw["durations"], 10, "likelihood")
