"""GPU: the astrometric likelihood (exo_astrometry_loglike_vjp_f64 through ops.astrometry_loglike and
KeplerianOrbit.astrometry_log_likelihood) -- against the multiprecision fixture tests/golden/astrometry_mp.npz with the
tolerances of tests/astrometry_cases.py, against the composed route written out here (get_relative_angles, float64 torch with
the tutorial's wrap, autograd; tolerances: the figures of tests/test_gpu_rv_like.py -- value 1e-10 x max |want|, every leaf
gradient 1e-8 x max |composed|), the 2 pi convention of the data, bit-reproducibility and independence of the batch, a bad
eccentricity, hipGraph replay, a joint RV + astrometry model under NUTS, and the refusals."""
import math

import numpy as np
import pytest
import torch

import astrometry_cases as K

pytestmark = pytest.mark.gpu


def T(a, dev, grad=False):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev).requires_grad_(grad)


def npy(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g():
    return K.load()


def fixture_call(c, dev, params=None, grad=True):
    """ops.astrometry_loglike on the inputs of a fixture system (jitter = sqrt(jit2): the op squares it) -> outputs as numpy,
    with d loglike / d jit2 recovered from d / d jitter = 2 jitter d / d jit2"""
    from exoplanet_amd import ops

    leaves = dict(params=T(c.params if params is None else params, dev, grad))
    if c.jit2_rho is not None:
        leaves["rho_jitter"] = T(np.sqrt(c.jit2_rho), dev, grad)
    if c.jit2_theta is not None:
        leaves["theta_jitter"] = T(np.sqrt(c.jit2_theta), dev, grad)
    err = lambda var: T(np.sqrt(var), dev) if var.size > 1 else float(np.sqrt(var[0]))  # noqa: E731
    kw = {k: v for k, v in leaves.items() if k != "params"}
    ll = ops.astrometry_loglike(T(c.t, dev), leaves["params"], T(c.rho, dev), err(c.var_rho), T(c.theta, dev), err(c.var_theta), **kw)
    got = dict(loglike=npy(ll))
    if grad:
        grads = dict(zip(leaves, torch.autograd.grad(ll.sum(), list(leaves.values()))))
        got["gparams"] = npy(grads["params"])
        if "rho_jitter" in grads:
            got["gjit2_rho"] = npy(grads["rho_jitter"]) / (2 * np.sqrt(c.jit2_rho))
        if "theta_jitter" in grads:
            got["gjit2_theta"] = npy(grads["theta_jitter"]) / (2 * np.sqrt(c.jit2_theta))
    return got


def entry_call(c, dev, outputs=K.OUTPUTS):
    """exo_astrometry_loglike_vjp_f64 itself on the inputs of a fixture system, exactly as the fixture states them: the
    variances and jit2 as stored (no square root and square in between), a null pointer where the fixture has no jit2, and a
    buffer for every output named in ``outputs`` -- the gradient of a jitter that was passed as null included"""
    from exoplanet_amd import ops

    D, N = c.params.shape[0], c.t.size
    dev_or_null = lambda a: None if a is None else T(a, dev)  # noqa: E731
    t, rho, cn, sn = T(c.t, dev), T(c.rho, dev), T(np.cos(c.theta), dev), T(np.sin(c.theta), dev)
    var_rho, var_theta, params = T(c.var_rho, dev), T(c.var_theta, dev), T(c.params, dev)
    jit2_rho, jit2_theta = dev_or_null(c.jit2_rho), dev_or_null(c.jit2_theta)
    shape = dict(loglike=(D,), gparams=(D, ops.OV_NPAR), gjit2_rho=(D,), gjit2_theta=(D,))
    out = {k: torch.full(shape[k], float("nan"), dtype=torch.float64, device=dev) for k in outputs}
    ops._call("exo_astrometry_loglike_vjp_f64", t.device, ops._ptr(t), ops._ptr(rho), ops._ptr(cn), ops._ptr(sn), ops._ptr(var_rho),
              var_rho.numel(), ops._ptr(var_theta), var_theta.numel(), N, ops._ptr(params), D, ops._ptr(jit2_rho),
              ops._ptr(jit2_theta), *[ops._ptr(out.get(k)) for k in K.OUTPUTS], ops._stream(t))
    torch.cuda.synchronize(t.device)
    return {k: npy(v) for k, v in out.items()}


@pytest.mark.parametrize("name", K.SYSTEMS)
def test_fixture(dev, g, name):
    """every system and every output: the entry point on the fixture's own inputs (all four outputs, the gradients of the
    jitters also where jit2 is a null pointer), then the same system through ops.astrometry_loglike"""
    c = K.case(g, name)
    direct = entry_call(c, dev)
    assert set(direct) == set(K.OUTPUTS) and all(np.isfinite(v).all() for v in direct.values())
    K.check("entry point", c, direct)
    # a null gradient output is not written and changes nothing else; without gparams the reverse arithmetic is skipped and
    # the value and the jitters' gradients are the same, bit for bit
    for outputs in (("loglike",), ("loglike", "gjit2_rho", "gjit2_theta"), ("loglike", "gparams")):
        part = entry_call(c, dev, outputs)
        for k in outputs:
            assert np.array_equal(part[k], direct[k]), (outputs, k)
    got = fixture_call(c, dev)
    # err = sqrt(var) and jitter = sqrt(jit2) are squared again by the op: the variances it sees are var and jit2 to one
    # rounding each, far inside the floor of the tolerance.  (A null jit2 has no leaf to differentiate: the op allocates no
    # output for it; the direct call above holds that gradient.)
    assert "gparams" in got and (c.jit2_rho is None) == ("gjit2_rho" not in got) and (c.jit2_theta is None) == ("gjit2_theta" not in got)
    K.check("op", c, got)
    assert np.array_equal(fixture_call(c, dev, grad=False)["loglike"], got["loglike"])


def test_an_empty_series(dev, g):
    """n_cad == 0 with draws: the sums are empty -- a value of 0 and gradients of 0 in every draw, as the header states"""
    c = K.case(g, "c")
    for k in ("t", "rho", "theta"):
        setattr(c, k, np.empty(0))
    c.var_rho, c.var_theta = c.var_rho[:1], c.var_theta[:1]      # (n_var == 1: no other length agrees with n_cad == 0)
    got = entry_call(c, dev)
    for k in K.OUTPUTS:
        assert np.all(got[k] == 0.0), k


D_METHOD, N_METHOD = 5, 45


def _orbit_kwargs(form, dev):
    D = D_METHOD
    rng = np.random.default_rng(41)
    P = 2 if form == "planet1" else 1
    col = lambda base, rel=0.0, ab=0.0: T(np.asarray(base, dtype=np.float64)[:P] * (1 + rel * rng.normal(size=(D, P)))  # noqa: E731
                                          + ab * rng.normal(size=(D, P)), dev, True)
    kw = dict(period=col([9131.0, 2800.0], 1e-3), incl=col([1.266, 0.8], ab=0.02), a=col([0.3, 0.12], 0.03))
    if form == "circular":
        kw["t0"] = col([1100.0, 300.0], ab=5.0)
    else:
        kw.update(t_periastron=col([1100.0, 300.0], ab=5.0), ecc=col([0.3, 0.5], ab=0.01), omega=col([1.9, -0.7], ab=0.03))
    if form != "no_Omega":
        kw["Omega"] = col([2.4, 0.4], ab=0.03)
    return kw


def composed_loglike(orbit, t, rho, rho_err, theta, theta_err, parallax, rho_jitter, theta_jitter, planet):
    """the tutorial's model op by op: get_relative_angles, the wrapped angle difference, two Normal log-densities"""
    rho_m, theta_m = orbit.get_relative_angles(t, parallax=parallax)
    if planet is not None:
        rho_m, theta_m = rho_m[..., planet], theta_m[..., planet]
    diff = theta_m - theta
    delta = torch.atan2(torch.sin(diff), torch.cos(diff))
    col = lambda x: x.reshape(-1, 1) if isinstance(x, torch.Tensor) else x  # noqa: E731
    s2r = rho_err ** 2 + (0.0 if rho_jitter is None else col(rho_jitter) ** 2) + torch.zeros_like(rho_m)
    s2t = theta_err ** 2 + (0.0 if theta_jitter is None else col(theta_jitter) ** 2) + torch.zeros_like(rho_m)
    r = rho - rho_m
    return -0.5 * (r * r / s2r + torch.log(2 * math.pi * s2r) + delta * delta / s2t + torch.log(2 * math.pi * s2t)).sum(-1)


@pytest.mark.parametrize("jitters", ["none", "number", "per_draw"])
@pytest.mark.parametrize("form", ["plain", "parallax_number", "parallax_leaf", "circular", "no_Omega", "planet1"])
def test_method_equals_the_composed_route(dev, form, jitters):
    import exoplanet_amd as xo

    D, N = D_METHOD, N_METHOD
    rng = np.random.default_rng(43)
    t = T(np.sort(rng.uniform(0.0, 8000.0, N)), dev)
    rho_err, theta_err = T(rng.uniform(0.01, 0.02, N), dev), T(rng.uniform(0.02, 0.05, N), dev)
    base = _orbit_kwargs(form, dev)
    planet = 1 if form == "planet1" else None
    parallax = {"parallax_number": 0.8, "parallax_leaf": T(0.8 * (1 + 0.02 * rng.normal(size=D)), dev, True)}.get(form)
    par_col = parallax.reshape(-1, 1) if isinstance(parallax, torch.Tensor) else parallax      # (draws, 1) against (draws, planets)
    with torch.no_grad():      # the data: draw 0, position angles in [0, 2 pi), plus noise of the size of the error bars
        rho0, theta0 = xo.KeplerianOrbit(**base).get_relative_angles(t, parallax=par_col)
        pick = (lambda x: x[0, :, planet]) if planet is not None else (lambda x: x[0])
        rho_err = rho_err * (1.0 if parallax is None else 0.8 * xo.orbits.constants.au_per_R_sun)      # (in the units of rho)
        rho = pick(rho0) + rho_err * T(rng.normal(size=N), dev)
        theta = torch.remainder(pick(theta0) + theta_err * T(rng.normal(size=N), dev), 2 * math.pi)
    if jitters == "none":
        rho_jitter = theta_jitter = None
        extra = {}
    elif jitters == "number":
        rho_jitter, theta_jitter, extra = 0.3 * float(rho_err.mean()), 0.01, {}
    else:
        rho_jitter = T(0.3 * float(rho_err.mean()) * (1 + 0.1 * rng.uniform(size=D)), dev, True)
        theta_jitter = T(0.01 * (1 + 0.1 * rng.uniform(size=D)), dev, True)
        extra = dict(rho_jitter=rho_jitter, theta_jitter=theta_jitter)
    leaves = dict(base, **extra, **(dict(parallax=parallax) if isinstance(parallax, torch.Tensor) else {}))
    out = []
    for route in ("fused", "composed"):
        orbit = xo.KeplerianOrbit(**base)
        if route == "fused":
            ll = orbit.astrometry_log_likelihood(t, rho, rho_err, theta, theta_err, parallax=parallax, rho_jitter=rho_jitter,
                                                 theta_jitter=theta_jitter, planet=planet)
        else:
            ll = composed_loglike(orbit, t, rho, rho_err, theta, theta_err, par_col, rho_jitter, theta_jitter, planet)
        assert tuple(ll.shape) == (D,)
        out.append((ll.detach(), torch.autograd.grad(ll.sum(), list(leaves.values()))))
    (ll_f, g_f), (ll_c, g_c) = out
    err = float((ll_f - ll_c).abs().max()) / float(ll_c.abs().max())
    print(f"{form}/{jitters}: value error / max |want| = {err:.3g}")
    worst = {}
    for name, a, b in zip(leaves, g_f, g_c):
        if planet is not None and name not in extra:      # the other companion has no data: its gradients are exactly 0
            assert float(a[:, 1 - planet].abs().max()) == 0.0
        worst[name] = float((a - b).abs().max()) / float(b.abs().max())
    print(f"{form}/{jitters}: gradient error / max |composed| = " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert err <= 1e-10
    assert all(v <= 1e-8 for v in worst.values()), worst


def _tutorial_inputs(dev, D=5, N=45, seed=47):
    """a (D, 9) array of (period, t_periastron, ecc, omega, Omega, cos i, a, log rho jitter, log theta jitter) and a series"""
    import exoplanet_amd as xo

    rng = np.random.default_rng(seed)
    t = T(np.sort(rng.uniform(0.0, 8000.0, N)), dev)
    rho_err, theta_err = T(rng.uniform(0.01, 0.02, N), dev), T(rng.uniform(0.02, 0.05, N), dev)
    centre = np.array([9131.0, 1100.0, 0.3, 1.9, 2.4, 0.3, 0.3, math.log(0.01), math.log(0.02)])
    draw = lambda: T(centre * (1 + 0.01 * rng.normal(size=(D, centre.size))), dev)  # noqa: E731

    def orbit_of(z):
        return xo.KeplerianOrbit(period=z[:, 0:1], t_periastron=z[:, 1:2], ecc=z[:, 2:3], omega=z[:, 3:4], Omega=z[:, 4:5],
                                 incl=torch.acos(z[:, 5:6]), a=z[:, 6:7])

    with torch.no_grad():
        rho0, theta0 = orbit_of(T(centre[None, :], dev)).get_relative_angles(t)
        rho = rho0.reshape(-1) + rho_err * T(rng.normal(size=N), dev)
        theta = torch.remainder(theta0.reshape(-1) + theta_err * T(rng.normal(size=N), dev), 2 * math.pi)

    def value_and_grad(z, theta_obs=theta):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            ll = orbit_of(zz).astrometry_log_likelihood(t, rho, rho_err, theta_obs, theta_err, rho_jitter=torch.exp(zz[:, 7]),
                                                        theta_jitter=torch.exp(zz[:, 8]))
            (gz,) = torch.autograd.grad(ll, zz, grad_outputs=torch.ones_like(ll))
        return ll.detach(), gz

    return value_and_grad, draw, theta


def test_any_two_pi_convention_of_the_data(dev):
    """theta + 2 pi and theta - 4 pi: the same value and gradients, up to the rounding of cos / sin of the shifted data"""
    value_and_grad, draw, theta = _tutorial_inputs(dev)
    z = draw()
    ll, gz = value_and_grad(z)
    assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(gz).all()) and float(gz.abs().min()) > 0
    for shift in (2 * math.pi, -4 * math.pi):
        ll_s, gz_s = value_and_grad(z, theta + shift)
        ev = float((ll_s - ll).abs().max()) / float(ll.abs().max())
        eg = float((gz_s - gz).abs().max()) / float(gz.abs().max())
        print(f"theta {shift:+.3f}: value {ev:.3g}, gradient {eg:.3g} (relative to the largest)")
        assert ev <= 1e-12 and eg <= 1e-12


def test_reproducible_and_independent_of_the_batch(dev, g):
    """two identical calls are bitwise equal; a draw of a 5-draw batch equals its own 1-draw call, bit for bit (both widths
    of the workgroup)"""
    widths = set()
    for name in ("b", "c", "d"):
        c = K.case(g, name)
        widths.add(64 if c.t.size <= K.NARROW_CAD else K.WIDE)
        five = lambda x, f: None if x is None else np.concatenate([x, x[:2] * f])  # noqa: E731
        c.params, c.jit2_rho, c.jit2_theta = five(c.params, 1 + 1e-4), five(c.jit2_rho, 1.01), five(c.jit2_theta, 1.01)
        first, second = fixture_call(c, dev), fixture_call(c, dev)
        for k in first:
            assert np.isfinite(first[k]).all() and np.array_equal(first[k], second[k]), (name, k)
        for d in range(5):
            one = K.case(g, name)
            one.params = c.params[d:d + 1]
            one.jit2_rho = None if c.jit2_rho is None else c.jit2_rho[d:d + 1]
            one.jit2_theta = None if c.jit2_theta is None else c.jit2_theta[d:d + 1]
            alone = fixture_call(one, dev)
            for k in alone:
                assert np.array_equal(alone[k][0], first[k][d]), (name, d, k)
    assert widths == {64, K.WIDE}


def test_bad_eccentricity_is_nan_in_that_draw_only(dev, g):
    for name in ("b", "c"):
        c = K.case(g, name)
        params = c.params.copy()
        params[1, 2] = 1.2
        got = fixture_call(c, dev, params=params)
        for k, v in got.items():
            assert np.isnan(v[1]).all() and np.isfinite(v[[0, 2]]).all(), (name, k)


def test_graph_replay_matches_eager(dev):
    """one capture of value and gradient (a single chain of launches), replayed twice with changed leaves"""
    import exoplanet_amd as xo

    value_and_grad, draw, _ = _tutorial_inputs(dev, D=8, N=150, seed=53)
    step = xo.GraphedStep(value_and_grad, draw())
    for _ in range(2):
        z = draw()
        ll_e, g_e = value_and_grad(z)
        ll_g, g_g = step(z)
        assert bool(torch.isfinite(ll_e).all()) and bool(torch.isfinite(g_e).all())
        assert float((ll_g - ll_e).abs().max()) <= 1e-12 * float(ll_e.abs().max())
        assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())


def test_a_captured_series_outlives_the_cache(dev):
    """a graph holds the per-series arrays (cos theta, sin theta, the variances) by address: after more other series than the
    cache keeps, they are still the ones the graph was captured with, and a replay still equals eager"""
    import exoplanet_amd as xo
    from exoplanet_amd import ops

    value_and_grad, draw, _ = _tutorial_inputs(dev, D=4, N=45, seed=61)
    z = draw()
    step = xo.GraphedStep(value_and_grad, z)
    held = {k: [x.data_ptr() for x in e.value] for k, e in ops._AST_SERIES.pinned.items()}
    assert held
    for seed in range(6):                                  # six other series: the cache keeps four
        other, other_draw, _ = _tutorial_inputs(dev, D=4, N=45, seed=70 + seed)
        other(other_draw())
    for k, ptrs in held.items():
        assert [x.data_ptr() for x in ops._AST_SERIES.pinned[k].value] == ptrs
    ll_e, g_e = value_and_grad(z)
    ll_g, g_g = step(z)
    assert float((ll_g - ll_e).abs().max()) <= 1e-12 * float(ll_e.abs().max())
    assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())


def test_joint_rv_and_astrometry_model_under_nuts(dev):
    """the README's joint model: logp = RV likelihood + astrometric likelihood on ONE orbit over one ParameterSpace; the sum
    equals the two computed separately, and five NUTS steps of eight chains keep finite energies"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    D, NRV, NAST = 8, 20, 45
    rng = np.random.default_rng(59)
    t_rv, t_ast = T(np.sort(rng.uniform(0.0, 3000.0, NRV)), dev), T(np.sort(rng.uniform(0.0, 8000.0, NAST)), dev)
    truth = dict(period=9131.0, tp=1100.0, ecc=0.3, omega=1.9, Omega=2.4, cosi=0.3, a=0.3, K=5.0)

    def orbit_of(period, tp, ecc, omega, Omega, cosi, a):
        return xo.KeplerianOrbit(period=period, t_periastron=tp, ecc=ecc, omega=omega, Omega=Omega, incl=torch.acos(cosi), a=a)

    with torch.no_grad():
        o = orbit_of(*[T([truth[k]], dev) for k in ("period", "tp", "ecc", "omega", "Omega", "cosi", "a")])
        rv = o.get_radial_velocity(t_rv, K=T([truth["K"]], dev)).reshape(-1) + 0.5 * T(rng.normal(size=NRV), dev)
        rho0, theta0 = o.get_relative_angles(t_ast)
        rho_err, theta_err = T(rng.uniform(0.01, 0.02, NAST), dev), T(rng.uniform(0.02, 0.05, NAST), dev)
        rho = rho0.reshape(-1) + rho_err * T(rng.normal(size=NAST), dev)
        theta = torch.remainder(theta0.reshape(-1) + theta_err * T(rng.normal(size=NAST), dev), 2 * math.pi)
    rv_err = T(rng.uniform(0.3, 0.6, NRV), dev)
    space = xd.ParameterSpace(period=xd.normal(9131.0, 50.0), tp=xd.normal(1100.0, 50.0), ecc=xd.uniform(0.0, 0.9), omega=xd.angle(),
                              Omega=xd.angle(), cosi=xd.uniform(0.0, 1.0), a=xd.lognormal(math.log(0.3), 0.5),
                              K=xd.lognormal(math.log(5.0), 0.5), log_rv_s=xd.normal(math.log(0.3), 1.0),
                              log_rho_s=xd.normal(math.log(0.01), 1.0), log_theta_s=xd.normal(math.log(0.02), 1.0), device=dev)

    def rv_part(period, tp, ecc, omega, Omega, cosi, a, K, log_rv_s, log_rho_s, log_theta_s):
        return orbit_of(period, tp, ecc, omega, Omega, cosi, a).rv_log_likelihood(t_rv, rv, rv_err, K=K, jitter=torch.exp(log_rv_s))

    def ast_part(period, tp, ecc, omega, Omega, cosi, a, K, log_rv_s, log_rho_s, log_theta_s):
        return orbit_of(period, tp, ecc, omega, Omega, cosi, a).astrometry_log_likelihood(
            t_ast, rho, rho_err, theta, theta_err, rho_jitter=torch.exp(log_rho_s), theta_jitter=torch.exp(log_theta_s))

    def logp(period, tp, ecc, omega, Omega, cosi, a, K, log_rv_s, log_rho_s, log_theta_s):
        orbit = orbit_of(period, tp, ecc, omega, Omega, cosi, a)
        return (orbit.rv_log_likelihood(t_rv, rv, rv_err, K=K, jitter=torch.exp(log_rv_s))
                + orbit.astrometry_log_likelihood(t_ast, rho, rho_err, theta, theta_err, rho_jitter=torch.exp(log_rho_s),
                                                  theta_jitter=torch.exp(log_theta_s)))

    col = lambda v, rel: torch.tensor(v * (1 + rel * rng.normal(size=(D, 1))))  # noqa: E731
    z0 = space.unconstrain(D, period=truth["period"], tp=col(truth["tp"], 1e-3), ecc=col(truth["ecc"], 0.02), omega=truth["omega"],
                           Omega=truth["Omega"], cosi=col(truth["cosi"], 0.02), a=col(truth["a"], 0.02), K=col(truth["K"], 0.05),
                           log_rv_s=math.log(0.3), log_rho_s=math.log(0.01), log_theta_s=math.log(0.02))
    with torch.no_grad():
        _, lp_prior = space.constrain(z0)
        joint = space.wrap(logp)(z0)
        parts = space.wrap(rv_part)(z0) + space.wrap(ast_part)(z0) - lp_prior      # (each wrapped part adds the prior once)
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

    N = 25
    t = T(np.linspace(0.0, 30.0, N), dev)
    rho, theta = T(0.3 + 0.01 * np.cos(np.arange(N)), dev), T(np.linspace(0.1, 6.0, N), dev)
    ttv = xo.orbits.TTVOrbit(period=T([3.5], dev), t0=T([1.0], dev), b=T([0.2], dev), ttvs=[T(np.zeros(12), dev)])
    with pytest.raises(NotImplementedError):
        ttv.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02)
    two = xo.KeplerianOrbit(period=T([9.0, 21.0], dev), t0=T([1.0, 2.0], dev), b=T([0.2, 0.1], dev))
    with pytest.raises(ValueError):
        two.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02)                    # whose data?
    with pytest.raises(ValueError):
        two.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, planet=2)
    assert tuple(two.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, planet=1).shape) == ()
    full = lambda v: T(np.full((4, 1), v), dev)  # noqa: E731
    orbit = xo.KeplerianOrbit(period=full(9.0), t0=full(1.0), incl=full(1.1), a=full(0.3))
    with pytest.raises(ValueError):
        orbit.astrometry_log_likelihood(t.reshape(5, 5), rho, 0.01, theta, 0.02)    # 2-D t
    with pytest.raises(ValueError):
        orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, rho_jitter=T(np.full(3, 0.01), dev))
    with pytest.raises(ValueError):
        orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, parallax=T(np.full(5, 0.04), dev))
    # per draw means (draws,) or (draws, 1): a wider array is refused, also where its size happens to be the draw count
    for wide in (np.full((4, 2), 0.01), np.full((2, 2), 0.01)):
        with pytest.raises(ValueError):
            orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, rho_jitter=T(wide, dev))
        with pytest.raises(ValueError):
            orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, theta_jitter=T(wide, dev))
        with pytest.raises(ValueError):
            orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, parallax=T(wide, dev))
        with pytest.raises(ValueError):
            ops.astrometry_loglike(t, T(np.tile([0.7, 1.0, 0.1, 1.0, 0.0, 0.4, 0.9165, -0.3, 1.0, 0.0], (4, 1)), dev), rho, 0.01,
                                   theta, 0.02, rho_jitter=T(wide, dev))
    column = orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, rho_jitter=T(np.full((4, 1), 0.01), dev))
    assert torch.equal(column, orbit.astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, rho_jitter=T(np.full(4, 0.01), dev)))
    # the op itself refuses data that requires grad; the method takes the composed route and returns the whole gradient
    params = T([[0.7, 1.0, 0.1, 1.0, 0.0, 0.4, 0.9165, -0.3, 1.0, 0.0]], dev)
    with pytest.raises(NotImplementedError):
        ops.astrometry_loglike(t, params, rho.clone().requires_grad_(True), 0.01, theta, 0.02)
    with pytest.raises(NotImplementedError):
        ops.astrometry_loglike(t, params, rho, 0.01, theta.clone().requires_grad_(True), 0.02)
    rho_g, theta_g = rho.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    a = full(0.3).requires_grad_(True)
    orbit = lambda: xo.KeplerianOrbit(period=full(9.0), t0=full(1.0), incl=full(1.1), a=a)  # noqa: E731
    ll = orbit().astrometry_log_likelihood(t, rho_g, 0.01, theta_g, 0.02, rho_jitter=0.005)
    g_rho, g_theta, g_a = torch.autograd.grad(ll.sum(), [rho_g, theta_g, a])
    ll_f = orbit().astrometry_log_likelihood(t, rho, 0.01, theta, 0.02, rho_jitter=0.005)
    (g_a_f,) = torch.autograd.grad(ll_f.sum(), [a])
    assert tuple(ll.shape) == tuple(ll_f.shape) == (4,)
    assert float((ll - ll_f).detach().abs().max()) <= 1e-10 * float(ll_f.detach().abs().max())
    assert float((g_a - g_a_f).abs().max()) <= 1e-8 * float(g_a_f.abs().max())
    assert float(g_rho.abs().max()) > 0 and float(g_theta.abs().max()) > 0
