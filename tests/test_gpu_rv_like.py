"""GPU: the radial-velocity likelihood (exo_rv_loglike_vjp_f64 through ops.rv_loglike and KeplerianOrbit.rv_log_likelihood)
-- against the multiprecision fixture tests/golden/rv_like_mp.npz with the tolerances of tests/rv_like_cases.py, against the
composed route written out here (get_radial_velocity, float64 torch, autograd; tolerances: the figures of
tests/test_gpu_noise.py -- value 1e-10 x max |want|, every leaf gradient 1e-8 x max |composed|), bit-reproducibility and
independence of the batch, the instrument without epochs, a bad eccentricity, hipGraph replay, a joint light-curve + RV
model under NUTS, and the refusals."""
import math

import numpy as np
import pytest
import torch

import rv_like_cases as K

pytestmark = pytest.mark.gpu


def T(a, dev, grad=False):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev).requires_grad_(grad)


def npy(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g():
    return K.load()


def fixture_call(c, dev, params=None, grad=True):
    """ops.rv_loglike on the inputs of a fixture system (jitter = sqrt(jit2): the op squares it) -> outputs as numpy, with
    d loglike / d jit2 recovered from d / d jitter = 2 jitter d / d jit2"""
    from exoplanet_amd import ops

    leaves = dict(params=T(c.params if params is None else params, dev, grad))
    if c.trend.shape[1]:
        leaves["trend"] = T(c.trend, dev, grad)
    if c.offset is not None:
        leaves["offset"] = T(c.offset, dev, grad)
    if c.jit2 is not None:
        leaves["jitter"] = T(np.sqrt(c.jit2), dev, grad)
    inst = torch.as_tensor(c.inst, device=dev) if c.n_inst > 1 else None
    rv_err = T(np.sqrt(c.var), dev) if c.var.size > 1 else float(np.sqrt(c.var[0]))
    kw = {k: v for k, v in leaves.items() if k != "params"}
    ll = ops.rv_loglike(T(c.t, dev), leaves["params"], T(c.rv, dev), rv_err, t_ref=c.tref, instrument=inst, **kw)
    got = dict(loglike=npy(ll))
    if grad:
        grads = dict(zip(leaves, torch.autograd.grad(ll.sum(), list(leaves.values()))))
        got["gparams"] = npy(grads["params"])
        if "trend" in grads:
            got["gtrend"] = npy(grads["trend"])
        if "offset" in grads:
            got["goffset"] = npy(grads["offset"])
        if "jitter" in grads:
            got["gjit2"] = npy(grads["jitter"]) / (2 * np.sqrt(c.jit2))
    return got


@pytest.mark.parametrize("name", K.SYSTEMS)
def test_fixture(dev, g, name):
    c = K.case(g, name)
    got = fixture_call(c, dev)
    # rv_err = sqrt(var) and jitter = sqrt(jit2) are squared again by the op: the variances it sees are var and jit2 to one
    # rounding each, far inside the floor of the tolerance.  (A null offset / jit2 has no leaf to differentiate: those
    # gradients of systems a and e are held by the host test alone.)
    assert "gparams" in got and (c.offset is None) == ("goffset" not in got) and (c.jit2 is None) == ("gjit2" not in got)
    K.check("kernel", c, got)


def _orbit_kwargs(form, dev, D=3):
    rng = np.random.default_rng(17)
    if form == "mass":      # one system, no draw dimension
        return dict(m_star=1.3, r_star=1.0, t0=T([0.5, 3.1], dev, True), period=T([100.0, 37.3], dev, True), ecc=T([0.1, 0.45], dev, True),
                    omega=T([0.5, -2.0], dev, True), incl=T([0.25 * np.pi, 1.3], dev, True), m_planet=T([0.1, 0.02], dev, True))
    kw = dict(period=T(np.array([12.3, 41.0]) * (1 + 1e-3 * rng.normal(size=(D, 2))), dev, True),
              t0=T(np.array([1.0, 7.5]) + 0.01 * rng.normal(size=(D, 2)), dev, True), b=T(np.full((D, 2), 0.3), dev))
    if form == "K":
        kw.update(ecc=T(np.array([0.2, 0.55]) + 0.01 * rng.normal(size=(D, 2)), dev, True),
                  omega=T(np.array([0.7, -1.9]) + 0.02 * rng.normal(size=(D, 2)), dev, True))
    return kw


def composed_loglike(orbit, t, rv, rv_err, K_amp, zero_point, trend, t_ref, jitter, inst):
    """the tutorials' model op by op: get_radial_velocity summed over the planets + trend + zero point, Normal log-density"""
    m = orbit.get_radial_velocity(t, K=K_amp).sum(-1)
    m = m.reshape(-1, t.numel())
    tau = t - t_ref
    for k in range(trend.shape[-1]):
        m = m + trend.reshape(-1, trend.shape[-1])[:, k:k + 1] * tau ** k

    def per_epoch(x):
        if not isinstance(x, torch.Tensor):
            return x
        x = x.reshape(-1, 1) if x.dim() < 2 else x
        return x[:, inst.long()] if x.shape[1] > 1 else x

    m = m + per_epoch(zero_point)
    s2 = rv_err ** 2 + per_epoch(jitter) ** 2 + torch.zeros_like(m)
    r = rv - m
    return -0.5 * (r * r / s2 + torch.log(2 * math.pi * s2)).sum(-1)


@pytest.mark.parametrize("kind", ["number", "per_draw", "per_instrument"])
@pytest.mark.parametrize("form", ["K", "mass", "circular"])
def test_method_equals_the_composed_route(dev, form, kind):
    import exoplanet_amd as xo

    D, N = 3, 97
    rng = np.random.default_rng(23)
    t = T(np.sort(rng.uniform(0.0, 120.0, N)), dev)
    inst = torch.as_tensor(rng.integers(0, 3, N), device=dev)
    rv_err = T(rng.uniform(0.3, 0.7, N), dev)
    base = _orbit_kwargs(form, dev)
    K_amp = None if form == "mass" else T(np.array([3.0, 11.0]) * (1 + 0.02 * rng.normal(size=(D, 2))), dev, True)
    with torch.no_grad():
        truth = xo.KeplerianOrbit(**base).get_radial_velocity(t, K=K_amp).sum(-1).reshape(-1, N)[0]
    rv = truth + 0.4 + 0.5 * T(rng.normal(size=N), dev)
    if kind == "number":
        zero_point, jitter, extra = 0.4, 0.3, {}
    elif kind == "per_draw":
        zero_point, jitter = T(0.4 + 0.1 * rng.normal(size=D), dev, True), T(0.3 + 0.05 * rng.uniform(size=D), dev, True)
        extra = dict(zero_point=zero_point, jitter=jitter)
    else:
        zero_point, jitter = T(0.4 + 0.3 * rng.normal(size=(D, 3)), dev, True), T(0.3 + 0.1 * rng.uniform(size=(D, 3)), dev, True)
        extra = dict(zero_point=zero_point, jitter=jitter)
    trend = T(np.array([0.1, 2e-3, -3e-5]) * (1 + 0.1 * rng.normal(size=(D, 3))), dev, True)
    t_ref = 60.0
    leaves = {k: v for k, v in base.items() if isinstance(v, torch.Tensor) and v.requires_grad}
    leaves.update(extra, trend=trend, **({} if K_amp is None else dict(K=K_amp)))
    out = []
    for route in ("fused", "composed"):
        orbit = xo.KeplerianOrbit(**base)
        if route == "fused":
            ll = orbit.rv_log_likelihood(t, rv, rv_err, K=K_amp, zero_point=zero_point, trend=trend, t_ref=t_ref, jitter=jitter,
                                         instrument=inst if kind == "per_instrument" else None)
        else:
            ll = composed_loglike(orbit, t, rv, rv_err, K_amp, zero_point, trend, t_ref, jitter, inst)
        assert tuple(ll.shape) == (D,)
        out.append((ll.detach(), torch.autograd.grad(ll.sum(), list(leaves.values()))))
    (ll_f, g_f), (ll_c, g_c) = out
    err = float((ll_f - ll_c).abs().max()) / float(ll_c.abs().max())
    print(f"{form}/{kind}: value error / max |want| = {err:.3g}")
    worst = {}
    for name, a, b in zip(leaves, g_f, g_c):
        worst[name] = float((a - b).abs().max()) / float(b.abs().max())
    print(f"{form}/{kind}: gradient error / max |composed| = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert err <= 1e-10
    assert all(v <= 1e-8 for v in worst.values()), worst


def test_default_reference_time_is_the_middle_of_the_series(dev):
    import exoplanet_amd as xo

    t = T(np.linspace(10.0, 50.0, 41), dev)
    orbit = lambda: xo.KeplerianOrbit(period=T([9.0], dev), t0=T([1.0], dev), b=T([0.2], dev))  # noqa: E731
    rv, trend, Kamp = T(np.sin(np.arange(41.0)), dev), T([0.2, 0.01], dev), T([2.0], dev)
    a = orbit().rv_log_likelihood(t, rv, 0.5, K=Kamp, trend=trend)
    b = orbit().rv_log_likelihood(t, rv, 0.5, K=Kamp, trend=trend, t_ref=30.0)
    assert tuple(a.shape) == () and torch.equal(a, b)


def test_reproducible_and_independent_of_the_batch(dev, g):
    """two identical calls are bitwise equal; a draw of a 5-draw batch equals its own 1-draw call, bit for bit (both widths
    of the workgroup, and the series that crosses a tile)"""
    for name in ("c", "e", "f"):
        c = K.case(g, name)
        params = np.concatenate([c.params, c.params[:2] * (1 + 1e-4)])           # five draws
        five = lambda x: None if x is None else np.concatenate([x, x[:2] * 1.01])  # noqa: E731
        c.trend, c.offset, c.jit2 = five(c.trend), five(c.offset), five(c.jit2)
        c.params = params
        first, second = fixture_call(c, dev), fixture_call(c, dev)
        for k in first:
            assert np.array_equal(first[k], second[k], equal_nan=True), (name, k)
        for d in range(5):
            one = K.case(g, name)
            one.params, one.trend = c.params[d:d + 1], c.trend[d:d + 1]
            one.offset = None if c.offset is None else c.offset[d:d + 1]
            one.jit2 = None if c.jit2 is None else c.jit2[d:d + 1]
            alone = fixture_call(one, dev)
            for k in alone:
                assert np.array_equal(alone[k][0], first[k][d]), (name, d, k)


def test_empty_instrument_has_zero_gradients(dev, g):
    c = K.case(g, "c")                       # three instruments, none of the epochs is the third's
    got = fixture_call(c, dev)
    assert np.all(got["goffset"][:, 2] == 0.0) and np.all(got["gjit2"][:, 2] == 0.0)
    assert np.all(got["goffset"][:, :2] != 0.0)


def test_bad_eccentricity_is_nan_in_that_draw_only(dev, g):
    c = K.case(g, "d")
    params = c.params.copy()
    params[1, 0, 2] = 1.2
    got = fixture_call(c, dev, params=params)
    for k, v in got.items():
        assert np.isnan(v[1]).any() and np.isfinite(v[[0, 2]]).all(), k
    assert np.isnan(got["loglike"][1]) and np.isnan(got["gparams"][1, 0]).all()


def _two_instrument_model(dev, D, N, seed):
    """(value_and_grad, draw) of a two-instrument model with per-epoch error bars over (draws, 10) leaves"""
    import exoplanet_amd as xo

    rng = np.random.default_rng(seed)
    t = T(np.sort(rng.uniform(0.0, 80.0, N)), dev)
    rv, rv_err = T(3.0 * rng.normal(size=N), dev), T(rng.uniform(0.3, 0.7, N), dev)
    inst = torch.as_tensor(rng.integers(0, 2, N), device=dev)

    def value_and_grad(z):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            orbit = xo.KeplerianOrbit(period=zz[:, 0:1], t0=zz[:, 1:2], b=torch.full_like(zz[:, 0:1], 0.2), ecc=zz[:, 2:3], omega=zz[:, 3:4])
            ll = orbit.rv_log_likelihood(t, rv, rv_err, K=zz[:, 4:5], zero_point=zz[:, 5:7], trend=zz[:, 7:9], t_ref=40.0,
                                         jitter=torch.exp(zz[:, 9:10]), instrument=inst)
            (gz,) = torch.autograd.grad(ll, zz, grad_outputs=torch.ones_like(ll))
        return ll.detach(), gz

    def draw():
        return T(np.array([11.0, 2.0, 0.3, 0.8, 4.0, 0.2, -0.3, 0.1, 1e-3, math.log(0.4)]) * (1 + 0.02 * rng.normal(size=(D, 10))), dev)

    return value_and_grad, draw


def test_graph_replay_matches_eager(dev):
    """one capture of value and gradient (a single chain of launches), replayed twice with changed leaves"""
    import exoplanet_amd as xo

    value_and_grad, draw = _two_instrument_model(dev, D=8, N=150, seed=29)
    z0 = draw()
    step = xo.GraphedStep(value_and_grad, z0)
    for _ in range(2):
        z = draw()
        ll_e, g_e = value_and_grad(z)
        ll_g, g_g = step(z)
        assert bool(torch.isfinite(ll_e).all()) and bool(torch.isfinite(g_e).all())
        assert float((ll_g - ll_e).abs().max()) <= 1e-12 * float(ll_e.abs().max())
        assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())


def test_a_captured_series_outlives_the_cache(dev):
    """a graph holds the per-series arrays (tau, the variances, the int32 instruments) by address: after more other series
    than the cache keeps -- all of them still alive, and the freed blocks of their size overwritten with NaN -- the arrays are
    still the ones the graph was captured with, and a replay still equals eager"""
    import exoplanet_amd as xo
    from exoplanet_amd import ops

    D, N = 4, 20
    value_and_grad, draw = _two_instrument_model(dev, D, N, seed=31)
    z = draw()
    ll_0, g_0 = value_and_grad(z)
    before = set(ops._RV_SERIES.pinned)
    step = xo.GraphedStep(value_and_grad, z)
    held = {k: [x.data_ptr() for x in e.value[:3]] for k, e in ops._RV_SERIES.pinned.items() if k not in before}
    assert len(held) == 1      # this capture's series, pinned by it
    others = [_two_instrument_model(dev, D, N, seed=40 + seed) for seed in range(6)]      # the cache keeps four
    for other, other_draw in others:
        other(other_draw())
    nan = [torch.full((n,), math.nan, dtype=torch.float64, device=dev) for n in (N, N, N // 2, N // 2) for _ in range(4)]
    for k, ptrs in held.items():
        assert [x.data_ptr() for x in ops._RV_SERIES.pinned[k].value[:3]] == ptrs
    ll_e, g_e = value_and_grad(z)
    ll_g, g_g = step(z)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ll_e).all()) and bool(torch.isfinite(g_e).all())
    assert float((ll_e - ll_0).abs().max()) <= 1e-12 * float(ll_0.abs().max())      # (eager, before the other series and after)
    assert float((g_e - g_0).abs().max()) <= 1e-12 * float(g_0.abs().max())
    assert float((ll_g - ll_e).abs().max()) <= 1e-12 * float(ll_e.abs().max())
    assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())
    assert len(others) == 6 and all(bool(torch.isnan(x).all()) for x in nan)


def test_joint_light_curve_and_rv_model_under_nuts(dev):
    """the README's joint model: logp = white-noise light-curve likelihood + RV likelihood over one ParameterSpace; the sum
    equals the two computed separately, and five NUTS steps of eight chains keep finite energies"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    D, N, NRV = 8, 200, 20
    rng = np.random.default_rng(31)
    t = T(np.linspace(0.0, 10.0, N), dev)
    with torch.no_grad():
        o = xo.KeplerianOrbit(period=T([3.5], dev), t0=T([1.0], dev), b=T([0.3], dev))
        y = 1.0 + xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=o, r=T([0.1], dev), t=t).sum(-1) + 2e-4 * T(rng.normal(size=N), dev)
        t_rv = T(np.sort(rng.uniform(0.0, 50.0, NRV)), dev)
        rv = o.get_radial_velocity(t_rv, K=T([5.0], dev)).reshape(-1) + 0.7 + 0.5 * T(rng.normal(size=NRV), dev)
    rv_err = T(rng.uniform(0.3, 0.6, NRV), dev)
    space = xd.ParameterSpace(period=xd.normal(3.5, 0.01), t0=xd.normal(1.0, 0.01), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              u=xd.quad_limb_dark(), K=xd.lognormal(math.log(5.0), 0.5), zero_point=xd.normal(0.0, 5.0),
                              log_jitter=xd.normal(math.log(0.3), 1.0), device=dev)

    def transit_part(period, t0, r, b, u1, u2, K, zero_point, log_jitter):
        lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y, yerr=2e-4, mean=1.0)

    def rv_part(period, t0, r, b, u1, u2, K, zero_point, log_jitter):
        return xo.KeplerianOrbit(period=period, t0=t0, b=b).rv_log_likelihood(t_rv, rv, rv_err, K=K, zero_point=zero_point,
                                                                               jitter=torch.exp(log_jitter))

    def logp(period, t0, r, b, u1, u2, K, zero_point, log_jitter):
        orbit = xo.KeplerianOrbit(period=period, t0=t0, b=b)
        lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
        return (lc.white_noise_log_likelihood(orbit=orbit, r=r, t=t, y=y, yerr=2e-4, mean=1.0)
                + orbit.rv_log_likelihood(t_rv, rv, rv_err, K=K, zero_point=zero_point, jitter=torch.exp(log_jitter)))

    z0 = space.unconstrain(D, period=3.5, t0=torch.tensor(1.0 + 1e-3 * rng.normal(size=D)), r=torch.tensor(0.1 * (1 + 0.02 * rng.normal(size=D))),
                           b=0.3, u1=0.3, u2=0.2, K=torch.tensor(5.0 * (1 + 0.05 * rng.normal(size=D))),
                           zero_point=torch.tensor(0.7 + 0.1 * rng.normal(size=D)), log_jitter=torch.tensor(math.log(0.3) + 0.1 * rng.normal(size=D)))
    with torch.no_grad():
        theta, lp_prior = space.constrain(z0)
        joint = space.wrap(logp)(z0)
        parts = space.wrap(transit_part)(z0) + space.wrap(rv_part)(z0) - lp_prior      # (each wrapped part adds the prior once)
    assert tuple(joint.shape) == (D,) and bool(torch.isfinite(joint).all())
    assert float((joint - parts).abs().max()) <= 1e-12 * float(joint.abs().max())
    nuts = xo.NUTS(space.wrap(logp), [z0.clone()], step_size=1e-3, max_depth=4, generator=torch.Generator(device=dev).manual_seed(3))
    for _ in range(5):
        nuts.step()
        assert bool(torch.isfinite(nuts.last_logp).all()) and bool(torch.isfinite(nuts._st["H0"]).all())
        assert bool(torch.isfinite(nuts.last_accept_prob).all()) and bool(nuts.last_adapt_ok.all())


def test_refusals(dev):
    import exoplanet_amd as xo
    from exoplanet_amd import ops

    t = T(np.linspace(0.0, 30.0, 25), dev)
    rv = T(np.cos(np.arange(25.0)), dev)
    ttv = xo.orbits.TTVOrbit(period=T([3.5], dev), t0=T([1.0], dev), b=T([0.2], dev), ttvs=[T(np.zeros(12), dev)])
    with pytest.raises(NotImplementedError):
        ttv.rv_log_likelihood(t, rv, 0.5, K=T([2.0], dev))
    orbit = xo.KeplerianOrbit(period=T(np.full((4, 1), 9.0), dev), t0=T(np.full((4, 1), 1.0), dev), b=T(np.full((4, 1), 0.2), dev))
    with pytest.raises(ValueError):
        orbit.rv_log_likelihood(t, rv, 0.5, K=T(np.full((4, 1), 2.0), dev), zero_point=T(np.zeros(3), dev))
    with pytest.raises(ValueError):
        orbit.rv_log_likelihood(t, rv, 0.5, K=T(np.full((4, 1), 2.0), dev), jitter=T(np.full((5, 2), 0.1), dev),
                                instrument=torch.zeros(25, dtype=torch.int64, device=dev))
    # the op itself refuses data that requires grad; the method takes the composed route and returns the whole gradient
    params = T([[[0.7, 1.0, 0.1, 1.0, 0.0, 2.0]]], dev)
    with pytest.raises(NotImplementedError):
        ops.rv_loglike(t, params, rv.clone().requires_grad_(True), 0.5)
    rv_g = rv.clone().requires_grad_(True)
    Kamp = T(np.full((4, 1), 2.0), dev, True)
    ll = orbit.rv_log_likelihood(t, rv_g, 0.5, K=Kamp, zero_point=0.1)
    g_rv, g_K = torch.autograd.grad(ll.sum(), [rv_g, Kamp])
    ll_f = orbit.rv_log_likelihood(t, rv, 0.5, K=Kamp, zero_point=0.1)
    (g_K_f,) = torch.autograd.grad(ll_f.sum(), [Kamp])
    assert float((ll - ll_f).detach().abs().max()) <= 1e-10 * float(ll_f.detach().abs().max())
    assert float((g_K - g_K_f).abs().max()) <= 1e-8 * float(g_K_f.abs().max()) and float(g_rv.abs().max()) > 0
