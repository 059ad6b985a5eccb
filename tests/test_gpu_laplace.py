"""GPU: the two entries of csrc/exo_laplace.hip (exo_laplace_points_f64, exo_laplace_factor_f64) against the long-double numpy
statement (tests/laplace_oracle.py) with the allowance of tests/test_laplace_host.py (16 units of the float64 statement's own
error), and against the host build of the same core (tests/laplace_harness.cpp), whose bits they are to give: both form every
sum in one stated order without fused multiply-adds, and the logarithm is written out.  Also D = 65 (the grid index beyond one
wave's worth of chains), the failing chains, reproducibility, capture and replay; `xo.laplace(native=True)` against
``native=False`` on the analytic target; and the README's white-noise transit model from `optimize` to `NUTS` and `bands`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import laplace_oracle as O  # noqa: E402
from test_laplace_host import (ALLOWANCE, LD, Target, _batch_with, _module, build_harness, check, harness_factor,  # noqa: E402
                               harness_points)

pytestmark = pytest.mark.gpu
OUTPUTS = O.FLOATS + ("status",)


def _call(name, dev, *args):
    from exoplanet_amd import _lib

    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def device_factor(dev, grad, dx, logp, free, order):
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    grad, dx, logp = T(grad), T(dx), T(logp)              # (every argument is held by a name until the call is enqueued)
    D, _, n = grad.shape
    m = len(free)
    F = torch.as_tensor(list(free), dtype=torch.int32, device=dev)
    new = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)  # noqa: E731
    out = dict(hess=new(D, m, m), cov=new(D, m, m), sd=new(D, m), logdet=new(D), log_evidence=new(D), asymmetry=new(D),
               fd_error=new(D), status=torch.full((D,), -1, dtype=torch.int32, device=dev))
    _call("exo_laplace_factor_f64", dev, grad.data_ptr(), dx.data_ptr(), logp.data_ptr(), D, n, F.data_ptr(), m, order,
          *(out[k].data_ptr() for k in ("hess", "cov", "sd", "logdet", "log_evidence", "asymmetry", "fd_error", "status")))
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def device_points(dev, x, free, scale, hess, delta, order):
    T = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    x, scale, hess = T(x), T(scale), T(hess)
    D, n = x.shape
    m = len(free)
    F = torch.as_tensor(list(free), dtype=torch.int32, device=dev)
    pts = torch.full((D, order * m, n), 7.0, dtype=torch.float64, device=dev)
    dx = torch.full((D, order * m), 7.0, dtype=torch.float64, device=dev)
    _call("exo_laplace_points_f64", dev, x.data_ptr(), D, n, F.data_ptr(), m, None if scale is None else scale.data_ptr(),
          int(scale is not None and scale.dim() == 2), None if hess is None else hess.data_ptr(), delta, order, pts.data_ptr(),
          dx.data_ptr())
    torch.cuda.synchronize(dev)
    return pts.cpu().numpy(), dx.cpu().numpy()


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def cases():
    """the host test's cases with the statement in long double and in float64, computed once"""
    return [(c, O.statement(c, LD), O.statement(c, np.float64)) for c in O.cases()]


def test_factor_against_the_statement_and_the_host_build(dev, harness, cases):
    worst, differ = {}, []
    for c, ld, f64 in cases:
        got = device_factor(dev, c["grad"], c["dx"], c["logp"], c["free"], c["order"])
        for key, r in check(got, ld, f64, ("kernel", c["n"], c["m"], c["D"], c["order"], c["condition"])).items():
            worst[key] = max(worst.get(key, 0.0), r)
        host = harness_factor(harness, c["grad"], c["dx"], c["logp"], c["free"], c["order"])
        differ += [(c["n"], c["D"], c["order"], key) for key in OUTPUTS if not np.array_equal(got[key], host[key], equal_nan=True)]
    print("kernel: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})
    print("outputs whose bits differ from the host build's:", differ or "none")
    assert not differ
    assert any(c["D"] == 65 for c, _, _ in cases)


def test_points_are_the_host_build_s_bits(dev, harness):
    rng = np.random.RandomState(11)
    for D, n, free in ((3, 7, list(O.MASKED)), (65, 64, list(range(64))), (1, 1, [0])):
        m = len(free)
        x = rng.standard_normal((D, n)) * 10.0 ** rng.uniform(-5, 2, size=n)
        x[0, free[-1]] = 0.0
        hess = np.stack([np.diag(10.0 ** rng.uniform(-4, 10, size=m)) for _ in range(D)])
        hess[D // 2, m // 2, m // 2], hess[D - 1, 0, 0] = -1.0, np.nan
        for order in (2, 4):
            for scale in (None, 10.0 ** rng.uniform(-5, 2, size=n), 10.0 ** rng.uniform(-5, 2, size=(D, n))):
                for H in (None, hess):
                    got_p, got_dx = device_points(dev, x, free, scale, H, 1e-3, order)
                    want_p, want_dx = harness_points(harness, x, free, scale, H, 1e-3, order)
                    assert np.array_equal(got_p, want_p) and np.array_equal(got_dx, want_dx), (D, n, order)
                    st_p, st_dx = O.points(x, free, scale, H, 1e-3, order, np.float64)
                    assert np.array_equal(got_p, st_p) and np.array_equal(got_dx, st_dx), (D, n, order)


def test_run_to_run_bit_identical(dev, cases):
    for c, _, _ in cases[-4:]:
        a, b = (device_factor(dev, c["grad"], c["dx"], c["logp"], c["free"], c["order"]) for _ in range(2))
        for key in OUTPUTS:
            assert np.array_equal(a[key], b[key], equal_nan=True), (c["n"], c["D"], key)


@pytest.mark.parametrize("failing", O.failing_chains(), ids=lambda f: f[0])
def test_a_failing_chain_fails_alone(dev, harness, failing):
    grad, dx, logp, good = _batch_with(failing)
    got = device_factor(dev, grad, dx, logp, [0, 1], 2)
    alone = device_factor(dev, good["grad"], good["dx"], logp[[0, 2]], [0, 1], 2)
    host = harness_factor(harness, grad, dx, logp, [0, 1], 2)
    assert list(got["status"]) == [O.OK, failing[1], O.OK]
    for key in ("cov", "sd", "logdet", "log_evidence"):
        assert np.isnan(got[key][1]).all(), key
    for key in OUTPUTS:
        assert np.array_equal(got[key], host[key], equal_nan=True), key           # hess, asymmetry, fd_error of the failed chain too
        assert np.array_equal(got[key][[0, 2]], alone[key], equal_nan=True), key


@pytest.mark.parametrize("order", [2, 4])
def test_public_laplace_native_against_the_host_build_and_the_torch_statement(dev, harness, order):
    """the analytic target on the device: what the kernels return is bitwise the host build's on the same gradient rows; the
    torch statement (native=False) and the kernels are within the allowance of the long-double statement on theirs"""
    import exoplanet_amd as xo

    target = Target()
    x = np.tile(target.zstar, (3, 1))
    x[1] += 1e-3 * target.sigma
    x[2] -= 2e-3 * target.sigma
    z = torch.as_tensor(x, device=dev)
    free = list(range(target.n))
    pilot = xo.laplace(target.logp_torch, [z], order=order, delta=1e-3, passes=1)
    runs = {native: xo.laplace(target.logp_torch, [z], order=order, delta=1e-3, native=native) for native in (True, False)}
    nat = runs[True]
    assert nat.status.tolist() == [0, 0, 0]
    # the stencils: pilot and final pass
    p1, d1 = harness_points(harness, x, free, None, None, 1e-3, order)
    assert np.array_equal(pilot._points.cpu().numpy(), p1) and np.array_equal(pilot._dx.cpu().numpy(), d1)
    p2, d2 = harness_points(harness, x, free, None, pilot.hess.cpu().numpy(), 1e-3, order)
    assert np.array_equal(nat._points.cpu().numpy(), p2) and np.array_equal(nat._dx.cpu().numpy(), d2)
    worst = {}
    for native, lap in runs.items():
        grad, dx, logp = (a.cpu().numpy() for a in (lap._grad, lap._dx, lap.logp))
        got = {k: getattr(lap, k).cpu().numpy() for k in OUTPUTS}
        ld, f64 = O.factor(grad, dx, logp, free, order, LD), O.factor(grad, dx, logp, free, order, np.float64)
        worst[native] = max(check(got, ld, f64, ("native", native, order)).values())
        if native:
            host = harness_factor(harness, grad, dx, logp, free, order)
            for key in OUTPUTS:
                assert np.array_equal(got[key], host[key], equal_nan=True), key
    print(f"order {order}: worst ratio, kernels {worst[True]:.2f}, torch statement on the device {worst[False]:.2f}")


def test_capture_and_replay(dev):
    """the points and the factor kernels, with the target's gradient between them, captured once and replayed: the eager bits"""
    from exoplanet_amd import GraphedStep

    L = _module()
    target = Target()
    a, w, c, b = (torch.as_tensor(v, device=dev) for v in (target.a, target.w, target.c, target.b))
    F = torch.arange(target.n, dtype=torch.int32, device=dev)
    order, D, n = 4, 5, target.n
    keys = ("hess", "cov", "sd", "logdet", "log_evidence", "asymmetry", "fd_error", "status")

    def fn(x):
        new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        pts, dx = new(D, order * n, n), new(D, order * n)
        L._points_native(x, F, None, None, 1e-3, order, pts, dx)
        u = pts - c                                                              # (D, rows, n); elementwise, no library call
        e = w * torch.exp((u[:, :, None, :] * a).sum(-1))                        # (D, rows, K)
        grad = -((e[:, :, :, None] * a).sum(2) - b)
        logp = -(e[:, 0].sum(1) - (u[:, 0] * b).sum(1))
        out = dict(hess=new(D, n, n), cov=new(D, n, n), sd=new(D, n), logdet=new(D), log_evidence=new(D), asymmetry=new(D),
                   fd_error=new(D), status=new(D, dtype=torch.int32))
        L._factor_native(grad, dx, logp, F, order, out)
        return tuple(out[k] for k in keys)

    rng = np.random.RandomState(2)
    x0 = torch.as_tensor(target.zstar + 1e-3 * target.sigma * rng.standard_normal((D, n)), device=dev)
    x1 = torch.as_tensor(target.zstar + 1e-3 * target.sigma * rng.standard_normal((D, n)), device=dev)
    step = GraphedStep(fn, x0.clone())
    for x in (x1, x0):
        eager = [v.clone() for v in fn(x)]
        replay = step(x)
        torch.cuda.synchronize(dev)
        assert eager[-1].tolist() == [0] * D
        for key, e, r in zip(keys, eager, replay):
            assert torch.equal(e, r), key


# ---- the README's white-noise transit model ------------------------------------------------------------------------------------
N_CAD, CHAINS, SIGMA = 4096, 4, 5e-4


@pytest.fixture(scope="module")
def transit(dev):
    """4096 cadences of 2 minutes, one planet (two transits), per-cadence error bars and a jitter, 4 chains brought to the mode
    by `optimize` in the README's two stages"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    rng = np.random.default_rng(81)
    t = torch.arange(N_CAD, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    with torch.no_grad():
        f0 = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=xo.KeplerianOrbit(period=T(3.5), t0=T(1.0), b=T(0.3)), r=T(0.1),
                                                             t=t)[:, 0]
    assert float(f0.min()) < -5e-3
    yerr = torch.as_tensor(3e-4 * (1.0 + 0.3 * rng.uniform(size=N_CAD)), device=dev)
    y = 1.0 + f0 + SIGMA * torch.as_tensor(rng.normal(size=N_CAD), device=dev)
    space = xd.ParameterSpace(period=xd.normal(3.5, 1e-3), t0=xd.normal(1.0, 1e-2), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), u=xd.quad_limb_dark(), mean=xd.normal(1.0, 1e-2),
                              log_jitter=xd.normal(math.log(4e-4), 2.0), device=dev)
    logp = lambda period, t0, r, b, u1, u2, mean, log_jitter: xo.LimbDarkLightCurve(  # noqa: E731
        u1.squeeze(-1), u2.squeeze(-1)).white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y,
                                                                   yerr=yerr, mean=mean, jitter=torch.exp(log_jitter))
    col = lambda v: torch.tensor(v).reshape(CHAINS, 1)  # noqa: E731
    z0 = space.unconstrain(CHAINS, period=col(3.5 + 1e-5 * rng.normal(size=CHAINS)), t0=col(1.0 + 3e-4 * rng.normal(size=CHAINS)),
                           r=col(0.1 * (1 + 0.01 * rng.normal(size=CHAINS))), b=col(0.3 + 0.03 * rng.normal(size=CHAINS)),
                           u1=col(0.3 + 0.01 * rng.normal(size=CHAINS)), u2=col(0.2 + 0.01 * rng.normal(size=CHAINS)),
                           mean=col(1.0 + 1e-5 * rng.normal(size=CHAINS)), log_jitter=col(math.log(4e-4) + 0.05 * rng.normal(size=CHAINS)))
    wrapped = space.wrap(logp)
    z = xo.optimize(wrapped, [z0], free=[space.free_mask(["t0", "r", "b"])])
    z = xo.optimize(wrapped, z)
    lap = xo.laplace(wrapped, z)
    return dict(space=space, logp=wrapped, z=z, lap=lap, t=t, y=y, yerr=yerr)


def test_transit_model_statuses_and_the_mean_s_curvature(dev, transit):
    """logp is exactly quadratic in `mean` (an identity coordinate with a normal prior), so hess[mean, mean] = sum_i 1 / (yerr_i^2 +
    jitter^2) + 1 / sd_prior^2 but for rounding.  The bound: the gradient with respect to mean is a sum of the N + 1 terms w_i (y_i
    - mean), minus the in-transit terms w_i f_i, and the prior's; summed in any order in float64 its error is at most (N + 16) eps
    times the sum of the terms' magnitudes, B; the difference of two such gradients over dx_+ - dx_- errs by at most 2 B / (dx_+ -
    dx_-), and the weights, the division and the symmetrisation add a few eps of H itself (16 eps allowed)."""
    import exoplanet_amd as xo

    lap, space = transit["lap"], transit["space"]
    print("laplace on the transit model: status", lap.status.tolist(), "asymmetry", lap.asymmetry.tolist(), "logp", lap.logp.tolist())
    assert lap.status.tolist() == [0] * CHAINS
    k = int(torch.nonzero(space.free_mask(["mean"]))[0])
    theta, _ = space.constrain(lap.center)
    with torch.no_grad():
        f = xo.LimbDarkLightCurve(theta["u1"].squeeze(-1), theta["u2"].squeeze(-1)).get_light_curve(
            orbit=xo.KeplerianOrbit(period=theta["period"], t0=theta["t0"], b=theta["b"]), r=theta["r"], t=transit["t"], total=True)
    f = f.reshape(CHAINS, N_CAD).cpu().numpy().astype(LD)
    y, yerr = (transit[key].cpu().numpy().astype(LD) for key in ("y", "yerr"))
    mean = lap.center[:, k].cpu().numpy()
    jitter = torch.exp(lap.center[:, int(torch.nonzero(space.free_mask(["log_jitter"]))[0])]).cpu().numpy().astype(LD)
    h = transit["lap"].delta / np.sqrt(lap.hess[:, k, k].cpu().numpy())            # dx_+ - dx_- = 2 h but for one rounding of x + h
    for d in range(CHAINS):
        w = 1.0 / (yerr ** 2 + jitter[d] ** 2)
        want = w.sum() + LD(1.0) / LD(1e-2) ** 2
        B = (N_CAD + 16) * O.EPS * ((w * np.abs(y - mean[d])).sum() + (w * np.abs(f[d])).sum() + abs(mean[d] - 1.0) / 1e-4)
        bound = 2.0 * B / (2.0 * h[d] * (1.0 - 1e-6)) + 16 * O.EPS * want
        got = LD(float(lap.hess[d, k, k]))
        print(f"chain {d}: hess[mean, mean] = {float(got):.10e}, closed form {float(want):.10e}, error {float(abs(got - want)):.3e}, "
              f"bound {float(bound):.3e}")
        assert abs(got - want) <= bound
        assert bound <= 1e-4 * want                                                # (the bound says something)
        assert float(lap.cov[d, k, k]) >= 1.0 / float(lap.hess[d, k, k])


def test_transit_model_to_nuts_and_bands(dev, transit):
    import exoplanet_amd as xo

    lap, space = transit["lap"], transit["space"]
    cov, center = lap.metric(lap.best())
    nuts = xo.NUTS(transit["logp"], [t.clone() for t in transit["z"]], step_size=0.1, cov=cov, center=center,
                   generator=torch.Generator(device=dev).manual_seed(4))
    nuts.step()
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(nuts.params[0]).all())
    phase = torch.linspace(-0.2, 0.2, 101, dtype=torch.float64, device=dev)
    fold = lambda period, t0, r, b, u1, u2, **_: xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1)).get_light_curve(  # noqa: E731
        orbit=xo.KeplerianOrbit(period=period, t0=0 * t0, b=b), r=r, t=phase, total=True)
    rows = lap.draws(256, generator=torch.Generator(device=dev).manual_seed(5))
    band = xo.predictive.bands(fold, rows, space)["quantiles"]
    assert tuple(band.shape) == (3, 101) and bool(torch.isfinite(band).all())
    assert float(band[1].min()) < -5e-3 and bool((band[0] <= band[2]).all())
    res = lap.importance(1024, generator=torch.Generator(device=dev).manual_seed(6))
    print("importance on the transit model: pareto_k %.3f, log_evidence_is %.3f, Laplace %.3f"
          % (float(res["pareto_k"]), float(res["log_evidence_is"]), float(lap.log_evidence[lap.best()])))
    assert math.isfinite(float(res["pareto_k"])) and math.isfinite(float(res["log_evidence_is"]))
