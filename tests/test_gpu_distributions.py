"""GPU: the two kernels of exoplanet_amd/csrc/exo_priors.hip behind ParameterSpace.constrain -- against the multiprecision
fixture, against the composed torch statement on a four-planet space, hipGraph replay against the eager call, and end to
end: box search -> ParameterSpace -> NUTS on the white-noise likelihood, and the prior-only statistical cases of
tests/test_distributions_host.py with the native tree kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import priors_cases as C  # noqa: E402
import priors_check as K  # noqa: E402

from exoplanet_amd import distributions as xd  # noqa: E402

pytestmark = pytest.mark.gpu

# The kernels against the fixture, measured on an MI355X: at most 7.7e-15, in the same array as on the
# host (the gradient of the kipping13(fixed=False) log prior with respect to log alpha; vaneylen19(fixed=False): 7.0e-15), every
# other array of every case below 1e-15; the torch path on the host: 8.9e-15.  Asserted where the host test asserts: 4x the larger
# (floor: 8 ulp).
TOL = max(4 * 8.9e-15, 8 * K.ULP)
REL_TOL = max(4 * 2.0e-15, 8 * K.ULP)       # the host test's bound (host core: 2.0e-15 values, 1.5e-15 Jacobian)


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_kernels_against_the_multiprecision_fixture(dev, case):
    data = K.golden()
    space = C.build(xd, case)
    e = K.errors(case, K.kernel_path(space, data[case + "/z"], dev), data)
    print(case, "kernels", {k: "%.2e" % v for k, v in e.items()})
    assert max(e.values()) <= TOL, e
    # ... and the values and their Jacobian relatively, entry by entry, however small (see tests/test_distributions_host.py)
    got = K.kernel_path(space, data[case + "/z"], dev)
    r = {"values": K.rel_err(got[0], data[case + "/values"]), "jacobian": K.rel_err(got[3], data[case + "/jacobian"])}
    print(case, "kernels, relative", {k: "%.2e" % v for k, v in r.items()})
    assert max(r.values()) <= REL_TOL, r


def four_planets():
    """four planets x {period, t0, r, b, ecc, omega} + limb darkening: 26 parameters on 30 coordinates (an angle has two);
    the eccentricities come from three different priors"""
    return xd.ParameterSpace(period=xd.lognormal(1.5, 0.5, shape=4), t0=xd.normal(1.0, 0.1, shape=4), r=xd.uniform(0.01, 0.3, shape=4),
                             b=xd.impact_parameter("r", shape=4), ecc=xd.kipping13(shape=2), ecc2=xd.vaneylen19(upper=0.7),
                             ecc3=xd.kipping13(long=False, lower=0.05, upper=0.9), omega=xd.angle(shape=4), u=xd.quad_limb_dark())


def test_kernels_against_the_torch_path_on_a_four_planet_space(dev):
    space = four_planets()
    assert space.n_free == 30 and len(space.names) == 10 and sum(c for _, c in space.outputs) == 26
    gen = torch.Generator(device=dev).manual_seed(26)
    z = 2.0 * torch.randn(1024, space.n_free, dtype=torch.float64, device=dev, generator=gen)
    z[:, :4] = 1.5 + 0.5 * torch.randn(1024, 4, dtype=torch.float64, device=dev, generator=gen)
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    th_a, lp_a = space.constrain(za)
    th_b, lp_b = space.constrain_composed(zb)
    assert list(th_a) == list(th_b) == [k for k, _ in space.outputs]
    worst = {"log_prior": K.err(lp_a.detach().cpu().numpy(), lp_b.detach().cpu().numpy())}
    for k in th_a:
        assert th_a[k].shape == th_b[k].shape == (1024, dict(space.outputs)[k]) and th_a[k].is_contiguous()
        worst[k] = K.err(th_a[k].detach().cpu().numpy(), th_b[k].detach().cpu().numpy())
    # random cotangents for everything; then with some missing (no zero-filled stand-ins: set_materialize_grads(False))
    cots = {k: torch.randn(v.shape, dtype=torch.float64, device=dev, generator=gen) for k, v in th_a.items()}
    glp = torch.randn(1024, dtype=torch.float64, device=dev, generator=gen)
    for n_case, keep in enumerate((list(th_a), ["r", "u2", "omega"], [])):
        for use_lp in (True, False):
            if not keep and not use_lp:
                continue
            grads = []
            for th, lp, zz in ((th_a, lp_a, za), (th_b, lp_b, zb)):
                outs = [th[k] for k in keep] + ([lp] if use_lp else [])
                gs = [cots[k] for k in keep] + ([glp] if use_lp else [])
                grads.append(torch.autograd.grad(outs, zz, grad_outputs=gs, retain_graph=True)[0].cpu().numpy())
            worst["gz %d %s" % (n_case, use_lp)] = K.err(grads[0], grads[1])
    print({k: "%.2e" % v for k, v in worst.items()})
    assert max(worst.values()) <= TOL, worst
    # closed supports on the device too (the compiler contracts multiply-adds there)
    g = torch.linspace(-36, 36, 289, dtype=torch.float64, device=dev)
    pair = torch.stack(torch.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    with torch.no_grad():
        th, lp = xd.ParameterSpace(h=xd.unit_disk()).constrain(pair)
        assert bool((th["x"] ** 2 + th["y"] ** 2 <= 1).all()) and bool(torch.isfinite(lp).all())
        th, lp = xd.ParameterSpace(u=xd.quad_limb_dark()).constrain(pair)
        assert bool((th["u1"] >= 0).all()) and bool((th["u1"] + th["u2"] <= 1).all()) and bool((th["u1"] + 2 * th["u2"] >= 0).all())
        th, lp = xd.ParameterSpace(r=xd.uniform(0.01, 0.3), b=xd.impact_parameter("r"), e=xd.kipping13(lower=0.3, upper=0.4, shape=2)).constrain(
            torch.cat([pair, pair], 1))
        assert bool((th["b"] >= 0).all()) and bool((th["b"] <= 1 + th["r"]).all()) and bool(((th["e"] >= 0.3) & (th["e"] <= 0.4)).all())
    with pytest.raises(ValueError):
        space.constrain(z[:, :5])


@pytest.mark.parametrize("D", [1, 63, 64, 65, 1024])
def test_graph_replay_equals_the_eager_call_bit_for_bit(dev, D):
    from exoplanet_amd import GraphedStep

    space = four_planets()
    w = torch.linspace(0.5, 1.5, 4, dtype=torch.float64, device=dev)

    def logp(period, t0, r, b, ecc, ecc2, ecc3, omega, u1, u2):      # a stand-in likelihood that uses every parameter
        return -((period * w).sum(1) + (t0 * r).sum(1) + (b * torch.cos(omega)).sum(1) + ecc.sum(1) * ecc2[:, 0] + ecc3[:, 0] * u1[:, 0] + u2[:, 0])

    wrapped = space.wrap(logp)

    def value_and_grad(z):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            lp = wrapped(zz)
            (g,) = torch.autograd.grad(lp, zz, grad_outputs=torch.ones_like(lp))
        return lp.detach(), g

    gen = torch.Generator(device=dev).manual_seed(D)
    draw = lambda: torch.randn(D, space.n_free, dtype=torch.float64, device=dev, generator=gen)  # noqa: E731
    step = GraphedStep(value_and_grad, draw())
    for _ in range(3):
        z = draw()
        lp_e, g_e = value_and_grad(z)
        lp_g, g_g = step(z)
        assert torch.equal(lp_e, lp_g) and torch.equal(g_e, g_g)
        assert bool(torch.isfinite(lp_e).all()) and bool(torch.isfinite(g_e).all())


def test_box_search_to_parameter_space_to_nuts(dev):
    """the README example: the box search's peak starts a NUTS run over a ParameterSpace on the white-noise likelihood"""
    import exoplanet_amd as xo
    from exoplanet_amd import estimators

    rng = np.random.default_rng(61)
    N, D = 8000, 128
    t = torch.arange(N, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    with torch.no_grad():
        f0 = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=xo.KeplerianOrbit(period=T(3.5), t0=T(1.0), b=T(0.3)), r=T(0.1), t=t)[:, 0]
    sigma = 5e-4
    y = f0 + sigma * torch.as_tensor(rng.normal(size=N), device=dev)
    found = estimators.bls_estimator(t, y, yerr=sigma, duration=[0.1, 0.2], min_period=2.0, max_period=6.0)
    period0, t00 = found["peak_info"]["period"], found["peak_info"]["transit_time"]
    epoch = 1.0 + 3.5 * round((t00 - 1.0) / 3.5)               # the search reports one of the transits, not necessarily the first
    assert abs(period0 - 3.5) < 0.05 and abs(t00 - epoch) < 0.02
    space = xd.ParameterSpace(period=xd.normal(period0, 0.05), t0=xd.normal(t00, 0.02), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              u=xd.quad_limb_dark(), device=dev)
    assert space.n_free == 6

    def logp(period, t0, r, b, u1, u2):
        lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y, yerr=sigma)

    g = np.random.default_rng(62)
    z0 = space.unconstrain(D, period=period0, t0=torch.tensor(t00 + 2e-3 * g.normal(size=D)), r=torch.tensor(0.1 * (1 + 0.05 * g.normal(size=D))),
                           b=0.3, u1=0.3, u2=0.2)
    assert z0.device.type == "cuda" and z0.shape == (D, 6)
    nuts = xo.NUTS(space.wrap(logp), [z0], step_size=1e-3, max_depth=6, generator=torch.Generator(device=dev).manual_seed(9))
    nuts.warmup(150, adapt_mass=True)
    assert bool(nuts.last_adapt_ok.all())                       # no chain stuck outside the support
    draws = []
    for _ in range(60):
        nuts.step()
        draws.append(nuts.params[0].clone())
    assert bool(nuts.last_adapt_ok.all())
    with torch.no_grad():
        theta, lp = space.constrain(torch.cat(draws))
    th = {k: v.cpu().numpy() for k, v in theta.items()}
    assert np.isfinite(lp.cpu().numpy()).all()
    assert (th["r"] >= 0.01).all() and (th["r"] <= 0.3).all() and (th["b"] >= 0).all() and (th["b"] <= 1 + th["r"]).all()
    assert (th["u1"] >= 0).all() and (th["u1"] + th["u2"] <= 1).all() and (th["u1"] + 2 * th["u2"] >= 0).all()
    print("posterior means: period %.6f t0 %.6f r %.5f b %.3f" % tuple(th[k].mean() for k in ("period", "t0", "r", "b")),
          "mean depth %.2f" % float(nuts.mean_depth().mean()))
    # the tolerances of tests/test_gpu_sampling.py for the same likelihood (t0, r); the period: one part in a thousand of the
    # 3.5 days, which the two transits in the series resolve a hundred times better
    assert abs(th["t0"].mean() - epoch) < 1e-3 and abs(th["r"].mean() - 0.1) < 8e-3 and abs(th["period"].mean() - 3.5) < 3.5e-3


@pytest.mark.parametrize("case", sorted(K.ks_cases(xd)))
def test_what_is_sampled_with_the_native_tree_kernels(dev, case):
    """the prior-only cases of the host test once more: 1024 chains, the native NUTS kernels, the fused prior kernels"""
    from scipy.stats import kstest

    space, logp_fn, statistics, bounds, *start = K.ks_cases(xd)[case]
    theta, nuts, ok_after_warmup = K.sample(xd, space, logp_fn, D=1024, seed=19910626, device=dev, warm=150, keep=40, start=start[0] if start else None)
    assert nuts._native is not None and ok_after_warmup and bool(nuts.last_adapt_ok.all())
    for k, (lo, hi) in bounds.items():
        assert (theta[k] >= lo).all() and (theta[k] <= hi).all(), k
    for stat, cdf in statistics:
        s = kstest(stat(theta), cdf).statistic
        print(case, "KS distance %.4f" % s, "divergences", float(nuts.n_divergent.sum()))
        assert s < K.KS_BOUND
