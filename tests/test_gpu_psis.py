"""GPU: the kernel of csrc/exo_psis.hip (`comparison.loo`, `ops.column_psis`) against the long-double numpy statement of the
definition (tests/psis_oracle.py) with the allowance of tests/test_psis_host.py (16 units of the float64 statement's own
error); the longest tail, strided input, reproducibility, memory; `comparison.loo` with a callable, end to end on a
white-noise transit model.  The arithmetic on the host: tests/test_psis_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psis_oracle as O  # noqa: E402
from test_psis_host import ALLOWANCE, KEYS  # noqa: E402

pytestmark = pytest.mark.gpu

# the host test's sizes, then this kernel's own boundaries: 16 lanes share a column of a 32-column tile (32 of a 16-column
# tile), so a sweep is 16 or 32 rows; a lane keeps 16 (4) loads in flight in the counting passes and 4 in the gather, so an
# unrolled step is 256 (128) rows there and 64 (128) here; 512: the 16-column tile at 16 loads, should it take them; then 5000
SIZES = ((1, 2, 5, 20, 21, 25, 63, 64, 65, 225, 1000, 4000) + (15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513)
         + (5000,))
WIDTHS = (1, 63, 64, 65, 200)


def _matrix(S, N, seed):
    """(S, N): the column families of the oracle, one after the other, each with numbers of its own"""
    rs = np.random.RandomState(seed)
    cols = []
    while len(cols) < N:
        cols += list(O.column_families(S, rs).values())
    return np.ascontiguousarray(np.stack(cols[:N], axis=1))


def _statements(values, M):
    return O.columns(values, M, np.longdouble), O.columns(values, M, np.float64)


def _check(got, ld, f64, label, cols=slice(None), family=None):
    """`family`: which columns share a unit (the default: _matrix's, the ten families one after the other); the units come from
    ALL columns of the statement, whatever `cols` of them the kernel was given"""
    family = np.arange(ld["k"].size) % 10 if family is None else np.asarray(family)

    got = {o: got[k].cpu().numpy() for o, k in KEYS.items()} | {"n_tail": got["n_tail"].cpu().numpy()}

    def ratios(key):
        full = np.array(ld[key], dtype=np.longdouble)                 # (columns the kernel was not given: the statement itself)
        full[cols] = got[key]
        return O.allowance(full, f64[key], ld[key], key, family)[cols]

    assert np.array_equal(got["n_tail"], ld["n_tail"][cols]), (label, got["n_tail"], ld["n_tail"][cols])
    worst = {key: float(ratios(key).max()) for key in O.OUTPUTS}
    print(f"{label}: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})
    for key in O.OUTPUTS:
        ratio = ratios(key)
        assert ratio.max() <= ALLOWANCE, (label, key, int(ratio.argmax()), got[key][int(ratio.argmax())], ld[key][cols][int(ratio.argmax())])


@pytest.fixture(scope="module")
def cases():
    """per S: the (S, 200) array, M and the statement in long double and in float64, computed once"""
    out = {}
    for S in SIZES:
        values = _matrix(S, max(WIDTHS), 1000 + S)
        M = O.tail_length(S)
        out[S] = (values, M) + _statements(values, M)
    return out


@pytest.mark.parametrize("S", SIZES)
def test_kernel_against_the_long_double_statement(dev, cases, S):
    from exoplanet_amd import comparison, ops

    values, M, ld, f64 = cases[S]
    for N in WIDTHS:
        x = torch.as_tensor(np.ascontiguousarray(values[:, :N]), device=dev)
        got = ops.column_psis(x, max(M, 1))
        assert got["n_tail"].dtype == torch.int32 and all(a.shape == (N,) for a in got.values())
        _check(got, ld, f64, f"kernel, S = {S}, N = {N}", slice(0, N))
    res = comparison.loo(torch.as_tensor(values[:, :7], device=dev))            # (the seven regular families)
    assert torch.equal(res["elpd_i"].view(torch.int64), ops.column_psis(x[:, :7], max(M, 1))["elpd"].view(torch.int64))
    assert res["elpd_loo"] == pytest.approx(float(np.sum(ld["elpd"][:7])), rel=1e-12) and res["n_data"] == 7
    assert res["n_high_k"] == int(np.sum(ld["k"][:7] > 0.7))


@pytest.mark.parametrize("S,M", [(33, 600), (129, 600), (513, 600), (1500, 600), (1500, 1024)])
def test_tails_of_more_than_512_take_the_16_column_tile(dev, S, M):
    """M is the caller's: above 512 the tile is 16 columns wide with 32 lanes a column; M + 1 > S clamps the cut-off to the
    smallest ratio, and the tail is every draw above it"""
    from exoplanet_amd import ops

    values = _matrix(S, 40, 3000 + S)
    ld, f64 = _statements(values, M)
    assert ld["n_tail"].max() == min(M, S - 1)
    _check(ops.column_psis(torch.as_tensor(values, device=dev), M), ld, f64, f"kernel, S = {S}, M = {M}")


def test_the_longest_tail(dev):
    """S = 116 000 draws: M = 1022 of the 1024 values a column's tail may hold"""
    from exoplanet_amd import comparison

    S = 116000
    rs = np.random.RandomState(9)
    fam = O.column_families(S, rs)
    values = np.ascontiguousarray(np.stack([fam[k] for k in ("normal model", "Student-t outlier", "near -1e6, spread 1e-3",
                                                            "one far draw")], axis=1))
    M = O.tail_length(S)
    assert M == 1022
    ld, f64 = _statements(values, M)
    assert ld["n_tail"].max() == 1022
    res = comparison.loo(torch.as_tensor(values, device=dev))
    _check({"elpd": res["elpd_i"], "k": res["pareto_k"], "lppd": res["lppd_i"], "var": res["p_waic_i"], "n_tail": res["n_tail"]},
           ld, f64, "kernel, S = 116000")
    with pytest.raises(ValueError, match="n_draws"):
        comparison.loo(torch.zeros(120000, 1, dtype=torch.float64, device=dev))


def test_strided_input_is_taken_as_it_is(dev, cases):
    from exoplanet_amd import comparison, ops

    values, M, ld, f64 = cases[1000]
    N = values.shape[1]
    tall = torch.full((1000 + 40, N + 5), 7.0, dtype=torch.float64, device=dev)   # (a number that would show)
    tall[:1000, :N] = torch.as_tensor(values, device=dev)
    view = tall[:1000, :N]
    assert not view.is_contiguous()
    want = ops.column_psis(torch.as_tensor(values, device=dev), M)
    got = ops.column_psis(view, M)
    _check(got, ld, f64, "kernel, a view of a taller and wider buffer")
    assert all(torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)) for k in KEYS.values())
    spread = torch.full((3 * 1000, N), 7.0, dtype=torch.float64, device=dev)
    spread[::3] = torch.as_tensor(values, device=dev)
    got = ops.column_psis(spread[::3], M)
    assert all(torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)) for k in KEYS.values())
    v4, _, ld4, f4 = cases[4000]
    cube = comparison.loo(torch.as_tensor(v4, device=dev).reshape(1000, 4, N))                # (n_draws, chains, N)
    _check({"elpd": cube["elpd_i"], "k": cube["pareto_k"], "lppd": cube["lppd_i"], "var": cube["p_waic_i"], "n_tail": cube["n_tail"]},
           ld4, f4, "kernel, (n_draws, chains, N)")


def test_two_calls_give_identical_bits(dev, cases):
    from exoplanet_amd import ops

    values, M = cases[5000][:2]
    x = torch.as_tensor(values, device=dev)
    a, b = ops.column_psis(x, M), ops.column_psis(x, M)
    for key in a:
        assert torch.equal(a[key].view(torch.int64) if a[key].dtype == torch.float64 else a[key],
                           b[key].view(torch.int64) if b[key].dtype == torch.float64 else b[key]), key


def test_outputs_are_untouched_beyond_the_columns_and_no_temporary_is_made(dev, cases):
    from exoplanet_amd import ops

    values, M = cases[225][:2]
    N = 65
    x = torch.as_tensor(np.ascontiguousarray(values[:, :N]), device=dev)
    outs = [torch.full((N + 64,), -7.0, dtype=torch.float64, device=dev) for _ in range(4)]
    tails = torch.full((N + 64,), -7, dtype=torch.int32, device=dev)
    ops._call("exo_column_psis_f64", dev, ops._ptr(x), 225, N, N, M, *[ops._ptr(o) for o in outs], ops._ptr(tails), ops._stream(x))
    torch.cuda.synchronize()
    want = ops.column_psis(x, M)
    for o, key in zip(outs, ("elpd", "k", "lppd", "var")):
        assert bool((o[N:] == -7.0).all()) and torch.equal(o[:N].view(torch.int64), want[key].view(torch.int64)), key
    assert bool((tails[N:] == -7).all()) and torch.equal(tails[:N], want["n_tail"])
    S, N = 2048, 4096
    big = torch.randn(S, N, dtype=torch.float64, device=dev)                                 # 64 MiB
    ops.column_psis(big, 136)                                                                # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    ops.column_psis(big, 136)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= 4 * N * 8 + N * 4 + (1 << 20)


def test_loo_end_to_end_on_a_white_noise_transit_model(dev):
    import exoplanet_amd as xo
    from exoplanet_amd import comparison
    from exoplanet_amd import distributions as xd

    period0, t00, sigma = 3.5, 1.0, 1e-3
    space = xd.ParameterSpace(period=xd.normal(period0, 1e-3), t0=xd.normal(t00, 1e-2), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), device=dev)
    z0 = space.unconstrain(1, period=period0, t0=t00, r=0.1, b=0.3)
    gen = torch.Generator(device=dev).manual_seed(11)
    z = z0.reshape(1, 1, -1) + 0.005 * torch.randn(256, 2, space.n_free, dtype=torch.float64, device=dev, generator=gen)
    trace = xo.Trace(z, {}, None, None, 0, "nuts")
    grid = torch.linspace(t00 - 0.3, t00 + 0.3, 1000, dtype=torch.float64, device=dev)
    lc = xo.LimbDarkLightCurve(0.3, 0.2)

    def curve(period, t0, r, b):
        return lc.get_light_curve(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=grid, total=True)

    with torch.no_grad():
        theta0, _ = space.constrain(z0.reshape(1, -1))
        y = curve(**{k: theta0[k] for k in space.names})[0] + sigma * torch.randn(1000, dtype=torch.float64, device=dev, generator=gen)
    chunks = []

    def log_likelihood(period, t0, r, b):
        chunks.append(int(period.shape[0]))
        return comparison.normal_log_likelihood(y, curve(period, t0, r, b), sigma)

    res = comparison.loo(log_likelihood, trace, space, chunk=200)
    assert chunks == [200, 200, 112] and res["n_draws"] == 512 and res["n_data"] == 1000
    with torch.no_grad():
        theta, _ = space.constrain(z.reshape(512, -1))
        ll = log_likelihood(**{k: theta[k] for k in space.names}).cpu().numpy()
    ld, f64 = _statements(ll, O.tail_length(512))
    _check({"elpd": res["elpd_i"], "k": res["pareto_k"], "lppd": res["lppd_i"], "var": res["p_waic_i"], "n_tail": res["n_tail"]},
           ld, f64, "loo with a callable", family=np.zeros(1000, dtype=int))
    assert res["p_loo"] > 0 and np.isfinite(res["elpd_loo"]) and res["se"] > 0
    w = comparison.waic(log_likelihood, trace, space, chunk=512)
    assert torch.equal(w["lppd_i"].view(torch.int64), res["lppd_i"].view(torch.int64)) and w["p_waic"] > 0
