"""GPU: exoplanet_amd.sample on the device -- NUTS with the native tree kernels and the replayed leaf on the 3-d Gaussian of
tests/test_gpu_sampling.py: the recorded chain is bit for bit the manual loop's, and its summary says it has converged; and one
run end to end on the injected transit of tests/test_gpu_optimize.py: ParameterSpace, optimize, sample, summary."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nuts(dev, D=64, seed=123):
    from exoplanet_amd.sampling import NUTS
    from test_gpu_sampling import _gauss_logp

    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(D, 2, dtype=torch.float64, device=dev, generator=g)
    y = torch.randn(D, 1, dtype=torch.float64, device=dev, generator=g)
    smp = NUTS(_gauss_logp(dev), [x, y], step_size=0.3, max_depth=6, generator=g)
    assert smp._native is not None and smp._graph is not None
    return smp


def test_sample_is_the_manual_loop_and_its_summary_says_converged(dev):
    import exoplanet_amd as xo

    a, b = _nuts(dev), _nuts(dev)
    trace = xo.sample(a, draws=100, tune=100, target_accept=0.8)
    b.warmup(100, target_accept=0.8)
    rows, energy = [], []
    for _ in range(100):
        b.step()
        rows.append(torch.cat([b.params[0], b.params[1]], dim=1).clone())
        energy.append(b.last_energy.clone())
    assert trace.draws.shape == (100, 64, 3) and trace.draws.is_cuda
    assert torch.equal(trace.draws, torch.stack(rows)) and torch.equal(trace.stats["energy"], torch.stack(energy))
    assert torch.equal(trace.eps, b.eps)
    assert torch.equal(trace.stats["diverging"].sum(0).to(torch.float64), a.n_divergent)
    assert torch.equal(trace.stats["depth"].sum(0), a.sum_depth)
    table = xo.diagnostics.summary(trace)
    print(table)
    assert table.names == ["x[0]", "x[1]", "x[2]"]
    assert bool((table["r_hat"] < 1.05).all())
    for k in ("ess_bulk", "ess_tail"):
        assert bool((torch.isfinite(table[k]) & (table[k] > 0)).all()), k
    assert table.n_divergent == 0 and bool((table.bfmi > 0.3).all()) and 1.5 < table.mean_depth < 5.0


def test_end_to_end_on_an_injected_transit(dev):
    """ParameterSpace -> optimize -> sample -> summary on the 16 chains x 8000 cadences of tests/test_gpu_optimize.py"""
    import exoplanet_amd as xo
    from test_gpu_optimize import TRUTH, transit_model

    model = transit_model(dev)
    space, logp = model["space"], model["logp"]
    z = xo.optimize(logp, [model["z0"]])
    nuts = xo.NUTS(logp, z, step_size=1e-3, max_depth=6, generator=torch.Generator(device=dev).manual_seed(9))
    trace = xo.sample(nuts, draws=150, tune=300, target_accept=0.9, adapt_mass=True)
    theta = trace.constrain(space)
    names = ["t0", "r", "b", "mean", "log_jitter"]
    assert trace.draws.shape == (150, 16, 5) and all(theta[k].shape == (150, 16, 1) for k in names)
    assert theta["log_prior"].shape == (150, 16)
    table = xo.diagnostics.summary({k: theta[k] for k in names}, trace.stats)
    print(table)
    assert table.names == names
    for k in table.columns:
        assert table[k].shape == (5,) and bool(torch.isfinite(table[k]).all()), k
    assert bool(torch.isfinite(trace.draws).all()) and all(bool(torch.isfinite(v.double()).all()) for v in trace.stats.values())
    assert bool((table["r_hat"] < 1.1).all())
    i = names.index("r")
    assert abs(float(table["mean"][i]) - TRUTH["r"]) < 5 * float(table["sd"][i])
