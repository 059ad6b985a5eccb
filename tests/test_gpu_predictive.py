"""GPU: the kernel of csrc/exo_predictive.hip (`predictive.quantiles`, `ops.column_quantiles`) against the numpy statement of
the definition (tests/predictive_oracle.py), exactly; strided input, counts, reproducibility, memory; `predictive.bands` end
to end on a transit model.  The arithmetic on the host: tests/test_predictive_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predictive_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

# the issue's sizes, then this kernel's own boundaries: a workgroup sweeps 4, 16 or 64 rows at a time and a lane keeps 8 loads
# in flight (32, 128, 512 rows per unrolled step); from 512 rows on 16 waves (8 for more than four quantiles) share a tile,
# below that 4
SIZES = (1, 2, 3, 63, 64, 65, 257, 1025, 5000) + (4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 511, 512, 513)
WIDTHS = (1, 63, 64, 65, 200)
P16 = (0, 100, 50, 16, 84, 2.5, 97.5, 15.865, 5, 95, 1, 99, 33.3, 66.7, 0.1, 99.9)
PERCENTS = {1: (50,), 3: (16, 50, 84), 16: P16}


def _matrix(S, N, seed):
    """(S, N): the column families of the oracle, one after the other, each with numbers of its own"""
    rs = np.random.RandomState(seed)
    cols = []
    while len(cols) < N:
        cols += list(O.column_families(S, rs).values())
    return np.stack(cols[:N], axis=1)


@pytest.fixture(scope="module")
def cases():
    """per S: the (S, 200) array and its sixteen quantiles, computed once"""
    out = {}
    for S in SIZES:
        values = _matrix(S, max(WIDTHS), 1000 + S)
        out[S] = (values,) + O.quantiles(values, P16)
    return out


@pytest.mark.parametrize("S", SIZES)
def test_kernel_equals_the_oracle_exactly(dev, cases, S):
    from exoplanet_amd import predictive

    values, want, want_count = cases[S]
    for N in WIDTHS:
        x = torch.as_tensor(np.ascontiguousarray(values[:, :N]), device=dev)
        for Q, percent in PERCENTS.items():
            got, count = predictive.quantiles(x, percent, return_count=True)
            rows = [P16.index(p) for p in percent]
            assert got.shape == (Q, N) and count.dtype == torch.int32
            assert O.same(got.cpu().numpy(), want[rows][:, :N]), (S, N, Q)
            assert np.array_equal(count.cpu().numpy(), want_count[:N]), (S, N, Q)


def test_strided_input_is_taken_as_it_is(dev, cases):
    from exoplanet_amd import predictive

    values, want, want_count = cases[1025]
    N = values.shape[1]
    rows = [P16.index(p) for p in (16, 50, 84)]
    tall = torch.full((1025 + 40, N + 5), 7.0, dtype=torch.float64, device=dev)
    tall[:1025, :N] = torch.as_tensor(values, device=dev)
    view = tall[:1025, :N]                                            # buf[:S] of a taller and wider buffer
    assert not view.is_contiguous()
    assert O.same(predictive.quantiles(view).cpu().numpy(), want[rows])
    spread = torch.full((3 * 1025, N), 7.0, dtype=torch.float64, device=dev)
    spread[::3] = torch.as_tensor(values, device=dev)
    assert O.same(predictive.quantiles(spread[::3]).cpu().numpy(), want[rows])               # curves[::3]
    v5, w5, _ = cases[5000]
    cube = torch.as_tensor(v5, device=dev).reshape(1250, 4, N)                               # (n_draws, chains, N)
    assert O.same(predictive.quantiles(cube).cpu().numpy(), w5[rows])


def test_wide_tiles_and_a_grid_that_walks_its_tiles(dev):
    """From 256 tiles of 64 columns on (N > 16320) a wave reads 64 adjacent columns, below that 16; a grid smaller than the
    number of tiles (tiles in flight kept to 192 MiB, at least 256 workgroups) walks them."""
    from exoplanet_amd import predictive

    rs = np.random.RandomState(77)
    for S, N in ((65, 16320), (65, 16321), (600, 16321)):
        values = np.round(rs.randn(S, N), 2)
        got = predictive.quantiles(torch.as_tensor(values, device=dev), (16, 50, 84, 2.5))
        assert O.same(got.cpu().numpy(), O.quantiles_dense(values, (16, 50, 84, 2.5))), (S, N)
    # 257 tiles of 1600 x 64 doubles each (0.78 MiB): more than 192 MiB in all, so 256 workgroups take 257 tiles
    S, N = 1600, 16448
    x = torch.randn(S, N, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    got = predictive.quantiles(x, (16, 50, 84))
    assert O.same(got.cpu().numpy(), O.quantiles_dense(x.cpu().numpy(), (16, 50, 84)))


def test_two_calls_give_identical_bits(dev, cases):
    from exoplanet_amd import predictive

    x = torch.as_tensor(cases[5000][0], device=dev)
    a, ca = predictive.quantiles(x, P16, return_count=True)
    b, cb = predictive.quantiles(x, P16, return_count=True)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ca, cb)


def test_no_temporary_of_the_input_size(dev):
    from exoplanet_amd import predictive

    S, N, Q = 2048, 4096, 3
    x = torch.randn(S, N, dtype=torch.float64, device=dev)                                   # 64 MiB
    predictive.quantiles(x, return_count=True)                                               # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    q, count = predictive.quantiles(x, return_count=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise <= Q * N * 8 + N * 4 + (1 << 20), rise


def test_bands_end_to_end_on_a_transit_model(dev):
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd
    from exoplanet_amd import predictive

    period0, t00 = 3.5, 1.0
    space = xd.ParameterSpace(period=xd.normal(period0, 1e-3), t0=xd.normal(t00, 1e-2), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), device=dev)
    z0 = space.unconstrain(1, period=period0, t0=t00, r=0.1, b=0.3)
    gen = torch.Generator(device=dev).manual_seed(11)
    z = z0.reshape(1, 1, -1) + 0.02 * torch.randn(300, 2, space.n_free, dtype=torch.float64, device=dev, generator=gen)
    trace = xo.Trace(z, {}, None, None, 0, "nuts")
    grid = torch.linspace(t00 - 0.15, t00 + 0.15, 200, dtype=torch.float64, device=dev)
    lc = xo.LimbDarkLightCurve(0.3, 0.2)
    chunks = []

    def model(period, t0, r, b):
        chunks.append(int(period.shape[0]))
        return lc.get_light_curve(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=grid, total=True)

    res = predictive.bands(model, trace, space, chunk=128, mean=True)
    assert chunks == [128] * 4 + [88] and res["n_draws"] == 600
    with torch.no_grad():
        theta, _ = space.constrain(z.reshape(600, -1))
        curves = model(**{k: theta[k] for k in space.names})
    want, want_count = predictive.quantiles(curves, return_count=True)
    assert res["quantiles"].shape == (3, 200)
    assert torch.equal(res["quantiles"].view(torch.int64), want.view(torch.int64)) and torch.equal(res["n_valid"], want_count)
    assert O.same(want.cpu().numpy(), O.quantiles(curves.cpu().numpy(), (16, 50, 84))[0])
    median = res["quantiles"][1]
    assert float(median[100]) < -5e-3 and abs(float(median[0])) < 1e-6 and bool((res["quantiles"][0] <= res["quantiles"][2]).all())
    assert torch.isfinite(res["mean"]).all()
