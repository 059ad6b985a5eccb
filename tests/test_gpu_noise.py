"""GPU: the white-noise likelihood with a sampled mean and a jitter on the fused path (exo_transit_noise[_ttv]_vjp_f64 +
exo_white_noise_terms_f64, through LimbDarkLightCurve.white_noise_log_likelihood) against the DENSE route written out here:
get_light_curve(total=True), the Gaussian log-likelihood in float64 torch, autograd for every gradient.  Never the fused code
against itself.

Tolerances, from tests/test_gpu_chi2.py: log-likelihood 1e-10 x max |want|; orbit / limb-darkening leaves 1e-8 x max |dense|;
the gradients of `mean` and `jitter` 1e-12 x the sum of the absolute terms of the sum they come from; graph replay against
eager 1e-12."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, N = 6, 8000
SIGMA = 3e-4


def _t(dev, t1=30.0):
    return torch.linspace(0.0, t1, N, dtype=torch.float64, device=dev)


def _leaf(v, rng, dev, shape=(D, 1), rel=1e-3):
    return torch.tensor(np.asarray(v) * (1 + rel * rng.normal(size=shape)), dtype=torch.float64, device=dev, requires_grad=True)


class System:
    """one of the issue's routes: its leaves, how an orbit is built from them, and the keywords of the light curve"""

    def __init__(self, name, dev, draws=D):
        import exoplanet_amd as xo

        rng = np.random.default_rng(sum(map(ord, name)))
        self.xo, self.name, self.kw, self.t, self.ttvs = xo, name, {}, _t(dev), None
        P = 3 if name == "three_planets" else 1
        sh = (draws, P)
        if P == 3:
            # commensurate periods and aligned t0 (tests/test_gpu_chi2.py:46-47): planets transit at the same time again and again
            period, t0 = np.array([3.0, 6.0, 4.5]), np.array([1.5, 1.5, 1.52])
            self.leaves = dict(period=_leaf(period, rng, dev, sh, 1e-4), t0=_leaf(t0, rng, dev, sh, 1e-3),
                               b=_leaf([0.3, 0.5, 0.1], rng, dev, sh), ecc=_leaf([0.1, 0.2, 0.3], rng, dev, sh),
                               omega=_leaf([0.5, -1.0, 2.0], rng, dev, sh), r=_leaf([0.1, 0.06, 0.08], rng, dev, sh))
        elif name in ("ttv", "record_ttv", "ttv_exposure"):
            self.t = _t(dev, 40.0)
            self.leaves = dict(period=_leaf(3.3, rng, dev, sh), t0=_leaf(0.9, rng, dev, sh), b=_leaf(0.3, rng, dev, sh),
                               r=_leaf(0.08, rng, dev, sh))
            self.ttvs = torch.tensor(0.01 * rng.normal(size=(draws, 12)), dtype=torch.float64, device=dev, requires_grad=True)
        else:
            self.leaves = dict(period=_leaf(3.5, rng, dev, sh), t0=_leaf(1.0, rng, dev, sh), b=_leaf(0.3, rng, dev, sh),
                               ecc=_leaf(0.2, rng, dev, sh), omega=_leaf(1.1, rng, dev, sh), r=_leaf(0.1, rng, dev, sh))
        if name.startswith("record"):
            # a stellar density: not the standard parameterisation, so the column form declines and the likelihood goes
            # through the records (ops.white_noise_loglike)
            self.leaves["rho_star"] = _leaf(1.3, rng, dev, (draws, 1), 1e-2)
        self.u1, self.u2 = _leaf(0.3, rng, dev, (draws,), 1e-2), _leaf(0.2, rng, dev, (draws,), 1e-2)
        if name.endswith("exposure"):
            self.kw = dict(texp=0.02, oversample=5)
        elif name == "in_transit":
            self.kw = dict(use_in_transit=True)
        elif name == "light_delay":
            self.kw = dict(light_delay=True)
        rs = np.random.default_rng(3)
        with torch.no_grad():
            truth = self.dense_flux(row=0).reshape(-1)
        self.y = (1.0 + truth + SIGMA * torch.as_tensor(rs.normal(size=N), device=dev)).contiguous()
        self.yerr_cad = torch.as_tensor(SIGMA * (1 + 0.3 * rs.uniform(size=N)), device=dev)
        self.mean_d = torch.as_tensor(1 + 1e-4 * rs.normal(size=(D, 1)), device=dev)
        self.jitter_d = torch.as_tensor(2e-4 * rs.uniform(0.5, 1.5, size=(D, 1)), device=dev)
        self.yerr_d = torch.as_tensor(SIGMA * rs.uniform(0.8, 1.2, size=(D, 1)), device=dev)

    def params(self):
        return list(self.leaves.values()) + [self.u1, self.u2] + ([self.ttvs] if self.ttvs is not None else [])

    def names(self):
        return list(self.leaves) + ["u1", "u2"] + (["ttvs"] if self.ttvs is not None else [])

    def orbit(self, row=None):
        sel = (lambda x: x) if row is None else (lambda x: x[row:row + 1])
        L = {k: sel(v) for k, v in self.leaves.items() if k != "r"}
        if self.ttvs is not None:
            return self.xo.orbits.TTVOrbit(ttvs=[sel(self.ttvs)], **L)
        return self.xo.KeplerianOrbit(**L)

    def star(self, row=None):
        if row is None:
            return self.xo.LimbDarkLightCurve(self.u1, self.u2)
        return self.xo.LimbDarkLightCurve(self.u1[row:row + 1], self.u2[row:row + 1])

    def r(self, row=None):
        return self.leaves["r"] if row is None else self.leaves["r"][row:row + 1]

    def dense_flux(self, row=None, per_planet=False):
        kw = dict(self.kw)
        kw.setdefault("use_in_transit", False)
        lc = self.star(row).get_light_curve(orbit=self.orbit(row), r=self.r(row), t=self.t, **kw)
        return lc if per_planet else lc.sum(-1).reshape(-1, N)

    def fused(self, mean, yerr, jitter, row=None):
        return self.star(row).white_noise_log_likelihood(orbit=self.orbit(row), r=self.r(row), t=self.t, y=self.y, yerr=yerr,
                                                         mean=mean, jitter=jitter, **self.kw)

    def dense(self, mean, yerr, jitter, row=None):
        """(loglike (D,), the absolute-term sums of d/dmean (D,), d/djitter (D,) and d/dyerr (D,)) of the dense route"""
        f = self.dense_flux(row)
        m = mean if isinstance(mean, torch.Tensor) else torch.tensor(float(mean), dtype=torch.float64, device=f.device)
        var = torch.as_tensor(yerr, dtype=torch.float64, device=f.device) ** 2
        if jitter is not None:
            var = var + torch.as_tensor(jitter, dtype=torch.float64, device=f.device).reshape(-1, 1) ** 2
        res = self.y - m.reshape(-1, 1) - f
        var = torch.broadcast_to(var, res.shape)
        ll = -0.5 * (res * res / var).sum(-1) - 0.5 * torch.log(var).sum(-1) - 0.5 * N * math.log(2 * math.pi)
        with torch.no_grad():
            s_mean = (res / var).abs().sum(-1)
            s_sig = ((res / var) ** 2 + 1 / var).sum(-1)
            s_jit = None if jitter is None else torch.as_tensor(jitter, dtype=torch.float64, device=f.device).reshape(-1) * s_sig
            s_yerr = yerr.detach().reshape(-1) * s_sig if isinstance(yerr, torch.Tensor) and yerr.requires_grad else None
        return ll, s_mean, s_jit, s_yerr


SYSTEMS = ["one_planet", "three_planets", "exposure", "ttv", "in_transit", "light_delay"]
# (mean, yerr, jitter) of the issue's table
COMBOS = {
    "mean_d-scalar-none": ("per_draw", "scalar", None),
    "number-cadence-jitter_d": ("number", "cadence", "per_draw"),
    "mean_d-cadence-jitter_d": ("per_draw", "cadence", "per_draw"),
    "mean_d-scalar-jitter_d": ("per_draw", "scalar", "per_draw"),
    "mean_11-scalar-none": ("broadcast", "scalar", None),
}
_systems = {}


def system(name, dev, draws=D):
    """built once and shared: the leaves are never modified"""
    if (name, draws) not in _systems:
        _systems[name, draws] = System(name, dev, draws)
    return _systems[name, draws]


def noise_args(s, combo, grad=True):
    mk, yk, jk = COMBOS[combo] if isinstance(combo, str) else combo
    mean = {"per_draw": s.mean_d, "number": 1.0 + 5e-5, "broadcast": s.mean_d[:1].reshape(1, 1), "vector": s.mean_d.reshape(-1),
            "zero_d": s.mean_d[0, 0]}[mk]
    if isinstance(mean, torch.Tensor):
        mean = mean.clone().requires_grad_(grad)
    yerr = {"scalar": SIGMA, "cadence": s.yerr_cad, "per_draw": s.yerr_d.clone().requires_grad_(grad)}[yk]
    jitter = {None: None, "per_draw": s.jitter_d, "vector": s.jitter_d.reshape(-1), "zero_d": s.jitter_d[0, 0], "number": 2e-4}[jk]
    if isinstance(jitter, torch.Tensor):
        jitter = jitter.clone().requires_grad_(grad)
    return mean, yerr, jitter


def compare(s, mean, yerr, jitter, row=None):
    """fused against dense: value, every leaf, mean, jitter and per-draw error bars"""
    leaves = [p for p in s.params()]
    extra = [x for x in (mean, jitter, yerr) if isinstance(x, torch.Tensor) and x.requires_grad]
    ll = s.fused(mean, yerr, jitter, row).reshape(-1)
    want, s_mean, s_jit, s_yerr = s.dense(mean, yerr, jitter, row)
    assert ll.shape == want.shape
    err = float((ll.detach() - want.detach()).abs().max()) / float(want.detach().abs().max())
    wgt = torch.as_tensor(np.random.default_rng(1).normal(size=tuple(ll.shape)), device=ll.device)
    ga = torch.autograd.grad((ll * wgt).sum(), leaves + extra)
    gb = torch.autograd.grad((want * wgt).sum(), leaves + extra)
    report = {"ll": err}
    for n, a, b in zip(s.names(), ga, gb):
        assert float(b.abs().max()) > 0, n
        report[n] = float((a - b).abs().max()) / float(b.abs().max())
    for x, a, b in zip(extra, ga[len(leaves):], gb[len(leaves):]):
        which = "mean" if x is mean else "jitter" if x is jitter else "yerr"
        scale = (s_mean if x is mean else s_jit if x is jitter else s_yerr) * wgt.abs()
        scale = scale.sum() if x.numel() == 1 and scale.numel() > 1 else scale.reshape(a.shape)
        assert a.shape == x.shape
        report["g" + which] = float(((a - b).abs() / scale).max())
    print(s.name, {k: "%.1e" % v for k, v in report.items()})
    assert report["ll"] <= 1e-10
    for n in s.names():
        assert report[n] <= 1e-8, n
    for k in ("gmean", "gjitter", "gyerr"):
        assert report.get(k, 0.0) <= 1e-12, k
    return ll


RECORD_SYSTEMS = ["record", "record_ttv"]


@pytest.mark.parametrize("combo", ["mean_d-cadence-jitter_d", "mean_d-scalar-none", "number-cadence-jitter_d"])
@pytest.mark.parametrize("name", RECORD_SYSTEMS)
def test_record_form_matches_the_dense_route(dev, name, combo):
    """an orbit outside the standard parameterisation (a stellar density): the column form declines, and the value, every
    leaf (the density among them), mean, jitter and the timing shifts come from ops.white_noise_loglike's own Function"""
    s = system(name, dev)
    orbit = s.orbit()
    assert not orbit._standard
    assert s.star()._loglike_from_columns(orbit, s.r(), s.t, s.y, SIGMA, 1.0, None, 7, 0, False, False, name == "record_ttv") is None
    compare(s, *noise_args(s, combo))


# shapes and kinds of `mean` / `yerr` / `jitter` beyond the table above
SHAPES = {
    "vector-cadence-vector": ("vector", "cadence", "vector"),
    "zero_d-cadence-zero_d": ("zero_d", "cadence", "zero_d"),
    "zero_d-scalar-none": ("zero_d", "scalar", None),
    "per_draw-cadence-number": ("per_draw", "cadence", "number"),
    "number-scalar-number": ("number", "scalar", "number"),
    "per_draw-per_draw-per_draw": ("per_draw", "per_draw", "per_draw"),
    "vector-per_draw-none": ("vector", "per_draw", None),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["one_planet", "record_ttv"])
def test_accepted_shapes_of_mean_yerr_and_jitter(dev, name, shape):
    """(D,) and 0-d tensors, a number `jitter`, and per-draw error bars (differentiable) under a per-draw mean / jitter,
    on the column form and on the record form"""
    s = system(name, dev)
    compare(s, *noise_args(s, SHAPES[shape]))


@pytest.mark.parametrize("yk", ["cadence", "scalar", "per_draw"])
@pytest.mark.parametrize("name", ["one_planet", "ttv", "record", "record_ttv"])
def test_one_system_with_many_noise_draws(dev, name, yk):
    """one parameter set and D draws of mean / jitter (/ error bars): the result has D rows, the gradient of a parameter
    sums over them"""
    s = system(name, dev, draws=1)
    mean, yerr, jitter = noise_args(s, ("per_draw", yk, "per_draw"))
    ll = compare(s, mean, yerr, jitter)
    assert ll.shape == (D,)


def test_constant_one_element_mean_keeps_its_route_and_the_fallback_takes_vectors(dev):
    s1, s = system("one_planet", dev, draws=1), system("one_planet", dev)
    with torch.no_grad():
        # one system, many error bars, `mean` a constant one-element tensor: the result has the error bars' draws
        m = torch.tensor(1.0 + 5e-5, dtype=torch.float64, device=dev)
        for mean in (m, m.reshape(1)):
            got = s1.fused(mean, s1.yerr_d, None)
            want = s1.fused(1.0 + 5e-5, s1.yerr_d, None)
            assert got.shape == want.shape and got.numel() == D
            assert float(((got - want) / want).abs().max()) <= 1e-12
        # the dense fallback (here: `y` requires grad) reads a (D,) mean / jitter as per draw, like the fused route
        mean, yerr, jitter = noise_args(s, ("vector", "cadence", "vector"), grad=False)
        fused = s.fused(mean, yerr, jitter)
    y = s.y.clone().requires_grad_(True)
    dense = s.star().white_noise_log_likelihood(orbit=s.orbit(), r=s.r(), t=s.t, y=y, yerr=yerr, mean=mean, jitter=jitter)
    assert dense.shape == fused.shape == (D,)
    assert float((dense.detach() - fused).abs().max()) <= 1e-10 * float(fused.abs().max())


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("name", SYSTEMS)
def test_fused_likelihood_matches_the_dense_route(dev, name, combo):
    s = system(name, dev)
    if name == "three_planets":
        with torch.no_grad():
            per = s.dense_flux(per_planet=True)
        both = (per != 0).sum(-1)
        assert int((both > 1).sum()) > 50, "no simultaneous transits in the test system"
    compare(s, *noise_args(s, combo))


def oracle_loglike(s, row, mean, yerr, jitter):
    """the log-likelihood of one draw from oracle/numpy_port.py's light curve of that draw's parameters"""
    from oracle import numpy_port as P

    leaf = {k: v[row].detach().cpu().numpy() for k, v in s.leaves.items()}
    r = leaf.pop("r")
    if s.ttvs is not None:
        orbit = P.TTVOrbit(ttvs=[s.ttvs[row].detach().cpu().numpy()], **leaf)
    else:
        orbit = P.KeplerianOrbit(**leaf)
    kw = dict(s.kw)
    kw.setdefault("use_in_transit", False)
    f = P.LimbDarkLightCurve(float(s.u1[row].detach()), float(s.u2[row].detach())).get_light_curve(orbit=orbit, r=r, t=s.t.cpu().numpy(), **kw).sum(-1)
    var = np.broadcast_to(np.asarray(yerr.cpu() if isinstance(yerr, torch.Tensor) else yerr) ** 2 + jitter ** 2, f.shape)
    res = s.y.cpu().numpy() - mean - f
    return -0.5 * (res * res / var).sum() - 0.5 * np.log(var).sum() - 0.5 * N * math.log(2 * math.pi)


# (system, draws): the routes of the likelihood's launches on both sides of "a block finishes its own draw" (>= 512 draws)
# that the tests above leave out -- one evaluation per solved cadence with timing tables / light delay, three sweeps without
# and with timing tables
ROUTES = [("one_planet", 512), ("ttv", 512), ("light_delay", 512), ("three_planets", 512), ("exposure", 512),
          ("ttv_exposure", 3), ("ttv_exposure", 512)]


@pytest.mark.parametrize("sampled", [False, True], ids=["fixed", "sampled"])
@pytest.mark.parametrize("name,draws", ROUTES)
def test_likelihood_routes_by_batch_size(dev, name, draws, sampled):
    """a fixed mean and no jitter (exo_transit_chi2[_ttv]_vjp_f64) and a sampled mean and jitter (exo_transit_noise[_ttv]_vjp_f64)
    against the dense route, and the first and last draw's value against the oracle's light curve"""
    s = system(name, dev, draws)
    rs = np.random.default_rng(17)
    if sampled:
        mean = torch.as_tensor(1 + 1e-4 * rs.normal(size=(draws, 1)), device=dev).requires_grad_(True)
        jitter = torch.as_tensor(2e-4 * rs.uniform(0.5, 1.5, size=(draws, 1)), device=dev).requires_grad_(True)
    else:
        mean, jitter = 1.0 + 5e-5, None
    ll = compare(s, mean, s.yerr_cad, jitter).detach()
    for row in (0, draws - 1):
        m, j = (float(mean[row]), float(jitter[row])) if sampled else (mean, 0.0)
        want = oracle_loglike(s, row, m, s.yerr_cad, j)
        assert abs(float(ll[row]) - want) <= 1e-10 * abs(want), (row, float(ll[row]), want)


@pytest.mark.parametrize("name", ["one_planet", "three_planets", "ttv"])
def test_one_draw_reproducible_and_batch_rows(dev, name):
    """D = 1; two identical calls give the same bits; a row of the batch equals the single-draw call bit for bit"""
    s = system(name, dev)
    combo = ("per_draw", "cadence", "per_draw")
    mean, yerr, jitter = noise_args(s, combo)
    compare(s, mean[2:3], yerr, jitter[2:3], row=2)
    with torch.no_grad():
        a = s.fused(mean, yerr, jitter)
        b = s.fused(mean, yerr, jitter)
        one = s.fused(mean[2:3], yerr, jitter[2:3], row=2)
    assert torch.equal(a, b)
    assert torch.equal(a[2:3].reshape(-1), one.reshape(-1))
    # ... and the gradients of the batch's row
    ll = s.fused(mean, yerr, jitter)
    ga = torch.autograd.grad(ll[2], s.params() + [mean, jitter])
    l1 = s.fused(mean[2:3], yerr, jitter[2:3], row=2)
    gb = torch.autograd.grad(l1.sum(), s.params() + [mean, jitter])
    for x, z in zip(ga, gb):
        assert torch.equal(x[2], z[2])


@pytest.mark.parametrize("yk", ["scalar", "cadence"])
def test_zero_jitter_and_constant_mean_reproduce_the_number_mean_call(dev, yk):
    s = system("one_planet", dev)
    yerr = SIGMA if yk == "scalar" else s.yerr_cad
    with torch.no_grad():
        today = s.fused(1.0 + 5e-5, yerr, None)
        const = torch.full((D, 1), 1.0 + 5e-5, dtype=torch.float64, device=dev)
        for jitter in (None, 0.0, torch.zeros(D, 1, dtype=torch.float64, device=dev)):
            got = s.fused(const, yerr, jitter)
            assert float(((got - today) / today).abs().max()) <= 1e-12


def test_parameter_space_with_mean_and_log_jitter_in_a_graph(dev):
    """the README's model: ParameterSpace.wrap(logp) with `mean` and `log_jitter` blocks; one GraphedStep replay equals
    eager, value and gradient"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    s = system("one_planet", dev)
    space = xd.ParameterSpace(period=xd.normal(3.5, 0.01), t0=xd.normal(1.0, 0.01), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), u=xd.quad_limb_dark(), mean=xd.normal(1.0, 1e-2),
                              log_jitter=xd.normal(math.log(SIGMA), 2.0), device=dev)

    def logp(period, t0, r, b, u1, u2, mean, log_jitter):
        lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=s.t, y=s.y, yerr=s.yerr_cad,
                                             mean=mean, jitter=torch.exp(log_jitter))

    wrapped = space.wrap(logp)

    def value_and_grad(z):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            lp = wrapped(zz)
            (g,) = torch.autograd.grad(lp, zz, grad_outputs=torch.ones_like(lp))
        return lp.detach(), g

    g = np.random.default_rng(8)
    z0 = space.unconstrain(D, period=3.5, t0=torch.tensor(1.0 + 1e-3 * g.normal(size=D)), r=torch.tensor(0.1 * (1 + 0.02 * g.normal(size=D))),
                           b=0.3, u1=0.3, u2=0.2, mean=torch.tensor(1 + 1e-4 * g.normal(size=D)),
                           log_jitter=torch.tensor(math.log(2e-4) + 0.2 * g.normal(size=D)))
    lp_e, g_e = value_and_grad(z0)
    assert bool(torch.isfinite(lp_e).all()) and bool(torch.isfinite(g_e).all()) and float(g_e[:, -2:].abs().min()) > 0
    step = xo.GraphedStep(value_and_grad, z0)
    lp_g, g_g = step(z0)
    assert float((lp_g - lp_e).abs().max()) <= 1e-12 * float(lp_e.abs().max())
    assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())
    # the dense route for the same model: the value and the whole gradient with respect to z
    def dense_logp(period, t0, r, b, u1, u2, mean, log_jitter):
        f = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1)).get_light_curve(
            orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=s.t, use_in_transit=False).sum(-1).reshape(-1, N)
        var = s.yerr_cad ** 2 + torch.exp(2 * log_jitter)
        res = s.y - mean - f
        return -0.5 * (res * res / var).sum(-1) - 0.5 * torch.log(var).sum(-1) - 0.5 * N * math.log(2 * math.pi)

    zz = z0.detach().requires_grad_(True)
    lp_d = space.wrap(dense_logp)(zz)
    (g_d,) = torch.autograd.grad(lp_d.sum(), zz)
    assert float((lp_d.detach() - lp_e).abs().max()) <= 1e-10 * float(lp_d.abs().max())
    assert float((g_d - g_e).abs().max()) <= 1e-8 * float(g_d.abs().max())


def test_a_captured_series_outlives_the_cache(dev):
    """a graph holds the per-series arrays (the variances, the per-series sums) by address: after more other series than the
    cache keeps -- all of them still alive, and the freed blocks of their size overwritten with NaN -- the arrays are still
    the ones the graph was captured with, and a replay still equals eager (per-cadence yerr, sampled mean and jitter)"""
    import exoplanet_amd as xo
    from exoplanet_amd import ops

    s = system("one_planet", dev)
    fixed = {k: v.detach() for k, v in s.leaves.items()}
    u1, u2 = s.u1.detach(), s.u2.detach()

    def model(y, yerr):
        def value_and_grad(z):
            with torch.enable_grad():
                zz = z.detach().requires_grad_(True)
                orbit = xo.KeplerianOrbit(period=zz[:, 0:1], t0=zz[:, 1:2], b=fixed["b"], ecc=fixed["ecc"], omega=fixed["omega"])
                ll = xo.LimbDarkLightCurve(u1, u2).white_noise_log_likelihood(
                    orbit=orbit, r=fixed["r"], t=s.t, y=y, yerr=yerr, mean=zz[:, 2:3], jitter=torch.exp(zz[:, 3:4]))
                (g,) = torch.autograd.grad(ll, zz, grad_outputs=torch.ones_like(ll))
            return ll.detach(), g
        return value_and_grad

    rng = np.random.default_rng(12)
    z = torch.as_tensor(np.array([3.5, 1.0, 1.0, math.log(2e-4)]) * (1 + 1e-4 * rng.normal(size=(D, 4))), device=dev)
    value_and_grad = model(s.y.clone(), s.yerr_cad.clone())      # (copies: no earlier capture has pinned this series)
    ll_0, g_0 = value_and_grad(z)
    before = set(ops._NZ_DATA.pinned)
    step = xo.GraphedStep(value_and_grad, z)
    held = {k: (e.value.var.data_ptr(), [x.data_ptr() for x in e.value.series.values()]) for k, e in ops._NZ_DATA.pinned.items()
            if k not in before}
    assert len(held) == 1      # this capture's series, pinned by it
    others = [(s.y + 1e-6 * (k + 1), s.yerr_cad * (1.0 + 0.01 * (k + 1))) for k in range(6)]      # the cache keeps four
    for y, yerr in others:
        model(y, yerr)(z)
    nan = [torch.full((n,), math.nan, dtype=torch.float64, device=dev) for n in (N, ops._NOISE_SERIES) for _ in range(6)]
    for k, (var, series) in held.items():
        e = ops._NZ_DATA.pinned[k].value
        assert e.var.data_ptr() == var and [x.data_ptr() for x in e.series.values()][:len(series)] == series
    ll_e, g_e = value_and_grad(z)
    ll_g, g_g = step(z)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ll_e).all()) and bool(torch.isfinite(g_e).all()) and float(g_e[:, -2:].abs().min()) > 0
    assert float((ll_e - ll_0).abs().max()) <= 1e-12 * float(ll_0.abs().max())      # (eager, before the other series and after)
    assert float((g_e - g_0).abs().max()) <= 1e-12 * float(g_0.abs().max())
    assert float((ll_g - ll_e).abs().max()) <= 1e-12 * float(ll_e.abs().max())
    assert float((g_g - g_e).abs().max()) <= 1e-12 * float(g_e.abs().max())
    assert len(others) == 6 and all(bool(torch.isnan(x).all()) for x in nan)


def test_mismatched_draws_and_data_that_requires_grad(dev):
    from exoplanet_amd import ops
    from oracle import numpy_port as P
    from test_gpu_transit import make_record

    s = system("one_planet", dev)
    mean, yerr, jitter = noise_args(s, ("per_draw", "cadence", "per_draw"), grad=False)
    with pytest.raises(ValueError, match=r"`mean` holds 4 draws, the parameters 6"):
        s.fused(mean[:4], yerr, jitter)
    with pytest.raises(ValueError, match=r"`jitter` holds 5 draws, the parameters 6"):
        s.fused(mean, yerr, jitter[:5])
    # ops level: y and a per-cadence yerr that require grad are refused, with or without the new arguments
    orbit = P.KeplerianOrbit(period=np.array([3.5]), t0=np.array([1.0]), b=np.array([0.3]), ecc=np.array([0.2]), omega=np.array([0.5]))
    rec = torch.as_tensor(np.repeat(make_record(orbit, np.array([0.1])), D, 0), device=dev)
    c = torch.as_tensor(np.repeat(P.get_cl(0.3, 0.2)[None], D, 0), device=dev)
    for kw in (dict(mean=1.0), dict(mean=mean, jitter=jitter)):
        with pytest.raises(NotImplementedError, match="`y` requires grad"):
            ops.white_noise_loglike(s.t, rec, c, s.y.clone().requires_grad_(True), s.yerr_cad, **kw)
        with pytest.raises(NotImplementedError, match="`yerr` requires grad"):
            ops.white_noise_loglike(s.t, rec, c, s.y, s.yerr_cad.clone().requires_grad_(True), **kw)
    # ... and the record form computes what the column form does for the same system
    import exoplanet_amd as xo

    col = lambda v: torch.full((D, 1), v, dtype=torch.float64, device=dev)  # noqa: E731
    star = xo.LimbDarkLightCurve(col(0.3).reshape(-1), col(0.2).reshape(-1))
    with torch.no_grad():
        a = ops.white_noise_loglike(s.t, rec, c, s.y, s.yerr_cad, mean=mean, jitter=jitter)
        b = star.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=col(3.5), t0=col(1.0), b=col(0.3), ecc=col(0.2), omega=col(0.5)),
                                            r=col(0.1), t=s.t, y=s.y, yerr=s.yerr_cad, mean=mean, jitter=jitter)
    assert a.shape == b.shape == (D,)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
