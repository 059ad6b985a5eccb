"""GPU: the dense metric of `HMC` / `NUTS` with the native tree kernels and the captured leaf -- Q = c + X L^T and G_x = G_q L as
two launches of exo_metric_apply_f64 inside the hipGraph --: the invariance of tests/test_sampling_dense.py on the device (with
an eager twin and a metric changed in place between transitions), the adaptation in windows at 64 chains, and the package's own
white-noise transit model with period and reference epoch almost collinear."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows_times(M):
    """x -> x M^T by a broadcast product and a sum: nothing of a BLAS is captured with the leaf"""
    return lambda x: (x.unsqueeze(1) * M.unsqueeze(0)).sum(-1)


@pytest.mark.parametrize("n,condition,step,max_depth", K.CASES)
def test_nuts_invariance_with_native_kernels_and_the_captured_leaf(dev, n, condition, step, max_depth):
    """A: the metric, graphed; A2: the same, eager; B: the parent's unit-mass sampler on the whitened target, which reads A's
    `chol` and `center` in place.  Before transition 12 the metric changes through `set_metric`: the captured leaves follow."""
    from exoplanet_amd.sampling import NUTS

    C, c, x0 = K.setup(n, condition, device=dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(K.SEED)  # noqa: E731
    L0 = torch.linalg.cholesky(C.cpu()).to(dev)
    q0 = c + x0 @ L0.T
    A = NUTS(K.logp, [q0.clone()], step, max_depth=max_depth, cov=C, center=c, generator=gen())
    A2 = NUTS(K.logp, [q0.clone()], step, max_depth=max_depth, cov=C, center=c, generator=gen(), graph=False)
    B = NUTS(lambda x: K.logp(A.center + _rows_times(A.chol)(x)), [x0.clone()], step, max_depth=max_depth, generator=gen())
    assert A._native is not None and A._graph is not None and A2._graph is None and B._graph is not None
    graph, ptrs = A._graph, (A.cov.data_ptr(), A.chol.data_ptr(), A.center.data_ptr())
    C2 = K.covariance(n, condition, seed=6).to(dev) * 1.5
    c2 = c + 0.05

    def between(i):
        if i != 0:
            assert torch.equal(A2.step(), A.last_depth)                  # (the eager twin makes the transition A just made)
        assert float((A.params[0] - A2.params[0]).abs().max()) <= 1e-10 * float(A.params[0].abs().max())
        if i == 12:
            A.set_metric(C2, center=c2)
            A2.set_metric(C2, center=c2)
            # (B goes on from the same points: its x under the new metric, and no cached gradient of the old one)
            B.params[0].copy_(torch.linalg.solve_triangular(A.chol, (A.params[0] - A.center).T, upper=False).T)
            B._lp = B._g = None

    worst_q, worst_a, n_div = K.compare(A, B, A.center, A.chol, between=between)
    between(-1)
    print(f"n = {n}: positions {worst_q:.2e}, accept_prob {worst_a:.2e}, {n_div} divergences, mean depth "
          f"{float(A.mean_depth().mean()):.2f}")
    assert A._graph is graph and ptrs == (A.cov.data_ptr(), A.chol.data_ptr(), A.center.data_ptr())     # no re-capture
    assert torch.equal(A.cov, C2) and A.n_leapfrog == B.n_leapfrog == A2.n_leapfrog


@pytest.mark.parametrize("n,condition,step,max_depth", K.CASES[1:3])
def test_hmc_invariance_with_the_captured_trajectory(dev, n, condition, step, max_depth):
    from exoplanet_amd.sampling import HMC

    C, c, x0 = K.setup(n, condition, device=dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(K.SEED)  # noqa: E731
    L = torch.linalg.cholesky(C.cpu()).to(dev)
    A = HMC(K.logp, [c + x0 @ L.T], step, 4, cov=C, center=c, generator=gen())
    B = HMC(lambda x: K.logp(c + _rows_times(L)(x)), [x0.clone()], step, 4, generator=gen())
    assert A._graph is not None and torch.equal(A.chol, L)
    worst_q, worst_a, _ = K.compare(A, B, c, L, nuts=False)
    print(f"n = {n}: positions {worst_q:.2e}, accept_prob {worst_a:.2e}, accept rate {float(A.accept_rate().mean()):.2f}")


def test_dense_adaptation_at_64_chains(dev):
    """tests/test_sampling_dense.py's adaptation test on the device, 64 chains (6400 draws: an entry's Monte-Carlo standard
    error is 1.3 to 1.8 % of sqrt(C_ii C_jj), the bound is 10 %)"""
    from exoplanet_amd.sampling import NUTS, sample

    n, chains = 8, 64
    C = K.covariance(n, 1e4).to(dev)
    times_P = _rows_times(torch.linalg.inv(C.cpu()).to(dev))

    def adapted(logp, adapt_mass):
        g = torch.Generator(device=dev).manual_seed(1)
        x = 0.1 * torch.randn(chains, n, dtype=torch.float64, device=dev, generator=g)
        smp = NUTS(logp, [x], 0.1, generator=g)
        assert smp._native is not None and smp._graph is not None
        return smp, sample(smp, draws=100, tune=300, adapt_mass=adapt_mass)

    smp, trace = adapted(lambda q: -0.5 * (times_P(q) * q).sum(1), "dense")
    iso, iso_trace = adapted(lambda q: -0.5 * (q * q).sum(1), False)
    iso_dense, _ = adapted(lambda q: -0.5 * (q * q).sum(1), "dense")
    leaves, leaves_iso, leaves_iso_dense = (s.n_leapfrog / s.n_steps for s in (smp, iso, iso_dense))
    got = torch.cov(trace.draws.reshape(-1, n).T)
    scale = torch.sqrt(torch.outer(torch.diag(C), torch.diag(C)))
    print(f"leaves per transition: dense {leaves:.2f}, isotropic yardstick {leaves_iso:.2f}, isotropic through the windows "
          f"{leaves_iso_dense:.2f}; sample covariance: worst entry at {float(((got - C).abs() / scale).max()):.3f} of "
          f"sqrt(C_ii C_jj); status {int(smp.metric_status)}")
    assert leaves <= 1.5 * min(leaves_iso, leaves_iso_dense)
    assert int(trace.stats["diverging"].sum()) == 0 and int(smp.metric_status) == 0
    assert bool(((got - C).abs() <= 0.1 * scale).all())
    assert bool(torch.isfinite(trace.cov).all()) and torch.equal(trace.cov, trace.cov.T) and bool(torch.isfinite(trace.center).all())
    assert iso_trace.cov is None and iso_trace.center is None


def test_transit_model_with_a_far_reference_epoch(dev):
    """The README's white-noise transit model -- period, epoch, r, b, mean, log_jitter; 2000 cadences of 10 minutes with four
    transits, 64 chains -- with the reference epoch 200 periods before the data: the transit times fix t0 + 200 period, so the
    two are almost collinear.  `adapt_mass=True` against `"dense"`, tune = 300, 100 draws.

    Measured on the MI355X: 127.00 leaves per transition with the diagonal metric (the depth limit), 7.00 with the dense one
    (ratio 18.1), no divergences in either, posterior means apart by at most 1.62 standard errors; the learnt metric's
    correlation of period and t0 is -0.999984.  (With Stan's shrinkage in absolute units, 1e-3 * 5 / (N + 5) added to every
    variance, both runs ended at 127 leaves: the posterior variances of period and mean are 1e-9 and 1e-10 in this model's
    units, and the floor of 1e-6 was the metric in those directions.  DESIGN.md 27.6.)"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    n_cad, chains, period, epochs = 2000, 64, 3.5, 200
    t_mid, sigma = 1.0, 5e-4
    rng = np.random.default_rng(5)
    t = torch.arange(n_cad, dtype=torch.float64, device=dev) * (10.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    lc = xo.LimbDarkLightCurve(0.3, 0.2)
    ref = t_mid - epochs * period
    with torch.no_grad():
        f0 = lc.get_light_curve(orbit=xo.KeplerianOrbit(period=T(period), t0=T(ref), b=T(0.3)), r=T(0.1), t=t)[:, 0]
    assert float(f0.min()) < -5e-3
    y = f0 + sigma * torch.as_tensor(rng.normal(size=n_cad), device=dev)
    space = xd.ParameterSpace(period=xd.normal(period, 1e-2), t0=xd.normal(ref, 5.0), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), mean=xd.normal(0.0, 1e-2),
                              log_jitter=xd.normal(math.log(3e-4), 2.0), device=dev)

    def loglike(period, t0, r, b, mean, log_jitter):
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y, yerr=4e-4,
                                             mean=mean, jitter=torch.exp(log_jitter))

    logp = space.wrap(loglike)
    col = lambda v: torch.tensor(v).reshape(chains, 1)  # noqa: E731
    p0 = period + 2e-5 * rng.normal(size=chains)
    z0 = space.unconstrain(chains, period=col(p0), t0=col(t_mid - epochs * p0 + 2e-4 * rng.normal(size=chains)),
                           r=col(0.1 * (1 + 0.01 * rng.normal(size=chains))),
                           b=col(np.clip(0.3 + 0.05 * rng.normal(size=chains), 0.05, 0.6)), mean=col(1e-5 * rng.normal(size=chains)),
                           log_jitter=col(math.log(3e-4) + 0.05 * rng.normal(size=chains)))
    runs = {}
    for adapt in (True, "dense"):
        nuts = xo.NUTS(logp, [z0.clone()], step_size=1e-3, max_depth=7, generator=torch.Generator(device=dev).manual_seed(3))
        trace = xo.sample(nuts, draws=100, tune=300, target_accept=0.9, adapt_mass=adapt)
        runs[adapt] = dict(leaves=nuts.n_leapfrog / nuts.n_steps, div=int(trace.stats["diverging"].sum()),
                           mean=trace.draws.mean((0, 1)), mcse=xo.diagnostics.mcse_mean(trace.draws), trace=trace)
    diag, dense = runs[True], runs["dense"]
    err = (diag["mean"] - dense["mean"]).abs() / torch.sqrt(diag["mcse"] ** 2 + dense["mcse"] ** 2)
    C = dense["trace"].cov
    corr = float(C[0, 1] / torch.sqrt(C[0, 0] * C[1, 1]))
    print(f"leaves per transition: diagonal {diag['leaves']:.2f}, dense {dense['leaves']:.2f} (ratio "
          f"{diag['leaves'] / dense['leaves']:.2f}); divergences {diag['div']} / {dense['div']}; means apart by "
          f"{[round(float(e), 2) for e in err]} standard errors; corr(period, t0) in the metric {corr:.8f}; status "
          f"{int(nuts.metric_status)}")
    assert bool(torch.isfinite(err).all()) and bool((err <= 4.0).all())
    assert dense["div"] <= diag["div"]
    assert dense["leaves"] < diag["leaves"]
    assert int(nuts.metric_status) == 0 and diag["trace"].cov is None
