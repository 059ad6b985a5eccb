"""CPU: exoplanet_amd.sample -- the recorded run of an HMC / NUTS sampler -- on the Gaussian target of tests/test_sampling.py:
the chain is bit for bit the one of as many plain step() calls from the same generator seed, the trace has the documented
shapes and dtypes, the recorded statistics are the samplers' own, and Trace.constrain goes through a ParameterSpace."""
import pytest
import torch

import exoplanet_amd as xo
from exoplanet_amd import distributions as xd
from exoplanet_amd.sampling import HMC, NUTS, Trace, sample

D = 16
MU = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
SD = torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)


def logp(x, s):          # two parameter blocks: a vector and a scalar per chain
    return (-0.5 * ((x - MU) / SD) ** 2).sum(-1) - 0.5 * (s[:, 0] / 3.0) ** 2


def make(kind, seed=1):
    x = torch.zeros(D, 3, dtype=torch.float64)
    s = torch.zeros(D, 1, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    if kind == "hmc":
        return HMC(logp, [x, s], step_size=0.35, n_leapfrog=6, mass=[1.0 / SD**2, 1.0 / 9.0], generator=g)
    return NUTS(logp, [x, s], step_size=0.4, max_depth=5, mass=[1.0 / SD**2, 1.0 / 9.0], generator=g)


@pytest.mark.parametrize("kind", ["hmc", "nuts"])
def test_sample_is_the_manual_loop_bit_for_bit(kind):
    n = 25
    a, b = make(kind), make(kind)
    trace = sample(a, draws=n)
    rows, logps, energies, rets = [], [], [], []
    for _ in range(n):
        rets.append(b.step().clone())
        rows.append(torch.cat([p.reshape(D, -1) for p in b.params], dim=1).clone())
        logps.append(b.last_logp.clone())
        energies.append(b.last_energy.clone())
    assert isinstance(trace, Trace) and len(trace) == n and trace.sampler == kind and trace.n_tune == 0
    assert trace.draws.shape == (n, D, 4) and trace.draws.dtype == torch.float64
    assert torch.equal(trace.draws, torch.stack(rows))
    for p, q in zip(a.params, b.params):
        assert torch.equal(p, q)
    # ... and the generator is where the manual loop left it
    assert torch.equal(a.generator.get_state(), b.generator.get_state())
    extra = "accepted" if kind == "hmc" else "depth"
    assert set(trace.stats) == {"logp", "energy", "accept_prob", "diverging", extra}
    for k, v in trace.stats.items():
        assert v.shape == (n, D), k
        assert v.dtype == (torch.bool if k in ("diverging", "accepted") else torch.float64), k
    assert torch.equal(trace.stats["logp"], torch.stack(logps)) and torch.equal(trace.stats["energy"], torch.stack(energies))
    assert torch.equal(trace.stats[extra], torch.stack(rets))
    assert torch.equal(trace.eps, a.eps) and all(torch.equal(m, w) for m, w in zip(trace.mass, a.mass))
    if kind == "nuts":
        assert torch.equal(trace.stats["diverging"].sum(0).to(torch.float64), a.n_divergent)
        assert float(trace.stats["depth"].min()) >= 1
    # what was recorded is where the chain is: logp of the draws
    assert torch.allclose(trace.stats["logp"][-1], logp(*a.params), rtol=1e-12, atol=1e-12)


def test_tune_runs_the_samplers_own_warmup():
    a, b = make("nuts", seed=4), make("nuts", seed=4)
    trace = sample(a, draws=10, tune=30, target_accept=0.9, adapt_mass=True)
    b.warmup(30, target_accept=0.9, adapt_mass=True)
    assert torch.equal(trace.eps, b.eps) and all(torch.equal(m, w) for m, w in zip(trace.mass, b.mass))
    for _ in range(10):
        b.step()
    assert torch.equal(trace.draws[-1], torch.cat([p.reshape(D, -1) for p in b.params], dim=1))
    assert trace.n_tune == 30 and a.n_steps == 10
    assert torch.equal(trace.stats["diverging"].sum(0).to(torch.float64), a.n_divergent)
    with pytest.raises(TypeError):
        sample(object(), draws=3)
    with pytest.raises(ValueError):
        sample(a, draws=-1)
    assert len(sample(a, draws=0)) == 0


def test_hmc_energy_is_the_hamiltonian_at_the_start_of_the_transition():
    hmc = make("hmc", seed=9)
    hmc.step()
    twin = torch.Generator().manual_seed(0)
    for _ in range(3):
        lp_before = logp(*hmc.params).clone()
        twin.set_state(hmc.generator.get_state())
        mflat = torch.cat([m.reshape(D, -1) for m in hmc.mass], dim=1)
        p0 = torch.randn(D, 4, dtype=torch.float64, generator=twin) * torch.sqrt(mflat)     # the momenta step() draws next
        hmc.step()
        want = -lp_before + (0.5 * p0 * p0 / mflat).sum(1)
        assert torch.allclose(hmc.last_energy, want, rtol=1e-13, atol=1e-13)
        assert hmc.last_energy.shape == (D,) and not bool(hmc.last_diverged.any())


def test_trace_constrain_goes_through_the_parameter_space():
    space = xd.ParameterSpace(r=xd.uniform(0.01, 0.3), mean=xd.normal(0.0, 1.0))
    target = space.wrap(lambda r, mean: -0.5 * ((r[:, 0] - 0.1) / 0.02) ** 2 - 0.5 * mean[:, 0] ** 2)
    z0 = space.unconstrain(D, r=0.1, mean=0.0)
    nuts = NUTS(target, [z0], step_size=0.3, max_depth=5, generator=torch.Generator().manual_seed(2))
    trace = xo.sample(nuts, draws=40, tune=40)
    theta = trace.constrain(space)
    want, want_lp = space.constrain(trace.draws.reshape(40 * D, -1))
    assert set(theta) == set(want) | {"log_prior"}
    for k, v in want.items():
        assert theta[k].shape == (40, D) + tuple(v.shape[1:]) and torch.equal(theta[k].reshape(v.shape), v)
    assert torch.equal(theta["log_prior"], want_lp.reshape(40, D))
    assert bool(((theta["r"] > 0.01) & (theta["r"] < 0.3)).all())
    table = xo.diagnostics.summary({k: v for k, v in theta.items() if k != "log_prior"}, trace.stats)
    assert table.names == ["r", "mean"] and bool(torch.isfinite(table["r_hat"]).all()) and bool((table["ess_bulk"] > 0).all())
    by_column = xo.diagnostics.summary(trace)
    assert by_column.names == ["x[0]", "x[1]"] and by_column.n_divergent == int(trace.stats["diverging"].sum())
