"""Times of the Laplace approximation on the device and the sweep of its step `delta` (28.5), on the
README's white-noise transit model (8 parameters): the points kernel, the factor kernel and the whole `xo.laplace` call from
the chains' modes, at D = 1024 with n = 8; the two kernels alone at D = 64 with n = 64 (gradient rows of a synthetic Hessian:
the README's model has 8 parameters); beside them, with --nuts, what producing a dense metric costs today:
``sample(nuts, draws=0, tune=500, adapt_mass="dense")`` on the same model.  Device events around `reps` calls, the median of
three rounds after a warm-up; the warm-up run of the sampler is timed once, by the host clock around a synchronise.

    python tools/time_laplace.py [--chains 1024] [--cadences 150000] [--reps 64] [--sweep] [--nuts]
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, rounds=3, warmup=2):
    """milliseconds per call: the median of `rounds` event-timed batches of `reps` calls"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def model(dev, chains, cadences, seed=1):
    """the README's model and `chains` starting points around the truth"""
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(cadences, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    period0, t00, sigma = 3.5, 1.0, 5e-4
    with torch.no_grad():
        f0 = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=xo.KeplerianOrbit(period=T(period0), t0=T(t00), b=T(0.3)),
                                                             r=T(0.1), t=t)[:, 0]
    y = 1.0 + f0 + sigma * torch.randn(cadences, dtype=torch.float64, device=dev, generator=g)
    space = xd.ParameterSpace(period=xd.normal(period0, 1e-3), t0=xd.normal(t00, 1e-2), r=xd.uniform(0.01, 0.3),
                              b=xd.impact_parameter(ror="r"), u=xd.quad_limb_dark(), mean=xd.normal(1.0, 1e-2),
                              log_jitter=xd.normal(math.log(sigma), 2.0), device=dev)
    logp = lambda period, t0, r, b, u1, u2, mean, log_jitter: xo.LimbDarkLightCurve(  # noqa: E731
        u1.squeeze(-1), u2.squeeze(-1)).white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y,
                                                                    yerr=3e-4, mean=mean, jitter=torch.exp(log_jitter))
    z0 = space.unconstrain(chains, period=period0, t0=t00, r=0.1, b=0.3, u1=0.3, u2=0.2, mean=1.0, log_jitter=math.log(sigma))
    z0 = z0 + 1e-4 * torch.randn(z0.shape, dtype=z0.dtype, device=dev, generator=g)
    return space, space.wrap(logp), z0


def modes(space, logp, z0):
    import exoplanet_amd as xo

    z = xo.optimize(logp, [z0], free=[space.free_mask(["t0", "r", "b"])])
    return xo.optimize(logp, z)


def kernel_times(dev, D, n, order, reps):
    """the two entries alone on the gradient rows of a synthetic positive definite Hessian"""
    from exoplanet_amd.laplace import _factor_native, _points_native

    g = torch.Generator(device=dev).manual_seed(2)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    A = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    H = A @ A.T + n * torch.eye(n, dtype=torch.float64, device=dev)
    x = torch.randn((D, n), dtype=torch.float64, device=dev, generator=g)
    F = torch.arange(n, dtype=torch.int32, device=dev)
    points, dx = new(D, order * n, n), new(D, order * n)
    out = dict(hess=new(D, n, n), cov=new(D, n, n), sd=new(D, n), logdet=new(D), log_evidence=new(D), asymmetry=new(D),
               fd_error=new(D), status=new(D, dtype=torch.int32))
    t_points = timed(lambda: _points_native(x, F, None, None, 1e-3, order, points, dx), reps)
    grad = -(points - x[:, None, :]) @ H                     # the gradient of -0.5 (q - x) H (q - x) at the points
    logp = torch.zeros(D, dtype=torch.float64, device=dev)
    t_factor = timed(lambda: _factor_native(grad, dx, logp, F, order, out), reps)
    torch.cuda.synchronize(dev)
    assert out["status"].tolist() == [0] * D
    return t_points, t_factor


def sweep(dev, cadences):
    """hess of the README's model at delta = 1e-1 .. 1e-6, both orders, 4 chains at their modes, against the plateau of the
    order-4 results: the mean of the two neighbouring decades that agree best.  Errors are of the matrix scaled to a unit
    diagonal, the largest entry over the chains."""
    import exoplanet_amd as xo

    space, logp, z0 = model(dev, 4, cadences)
    z = modes(space, logp, z0)
    decades = [10.0 ** -e for e in range(1, 7)]
    res = {(order, d): xo.laplace(logp, z, order=order, delta=d) for order in (2, 4) for d in decades}
    ref = res[(4, 1e-3)].hess
    s = 1.0 / torch.sqrt(torch.diagonal(ref, dim1=1, dim2=2))
    scaled = lambda lap: lap.hess * s[:, :, None] * s[:, None, :]  # noqa: E731
    gaps = [float((scaled(res[(4, a)]) - scaled(res[(4, b)])).abs().max()) for a, b in zip(decades, decades[1:])]
    k = min(range(len(gaps)), key=gaps.__getitem__)
    plateau = 0.5 * (scaled(res[(4, decades[k])]) + scaled(res[(4, decades[k + 1])]))
    print(f"sweep, {cadences} cadences, 4 chains: the order-4 results of delta = {decades[k]:g} and {decades[k + 1]:g} agree to "
          f"{gaps[k]:.1e} (the plateau); status of every run {sorted({int(v) for lap in res.values() for v in lap.status.tolist()})}")
    for order in (2, 4):
        print(f"  order {order}: " + ", ".join(f"{d:g}: {float((scaled(res[(order, d)]) - plateau).abs().max()):.1e}" for d in decades))
    print("  asymmetry, order 2: " + ", ".join(f"{d:g}: {float(res[(2, d)].asymmetry.max()):.1e}" for d in decades))
    print("  fd_error, order 4: " + ", ".join(f"{d:g}: {float(res[(4, d)].fd_error.max()):.1e}" for d in decades))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--cadences", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--sweep", action="store_true", help="the sweep of delta instead of the times")
    ap.add_argument("--nuts", action="store_true", help="the dense warm-up of NUTS instead of the times")
    args = ap.parse_args()
    import exoplanet_amd as xo

    dev = torch.device("cuda:0")
    if args.sweep:
        return sweep(dev, args.cadences)
    space, logp, z0 = model(dev, args.chains, args.cadences)
    if args.nuts:
        nuts = xo.NUTS(logp, modes(space, logp, z0), step_size=1e-3, generator=torch.Generator(device=dev).manual_seed(1))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        xo.sample(nuts, draws=0, tune=500, adapt_mass="dense")
        torch.cuda.synchronize(dev)
        print(f"sample(nuts, draws=0, tune=500, adapt_mass='dense'), D = {args.chains}, {args.cadences} cadences: "
              f"{time.perf_counter() - t0:.1f} s, {nuts.n_leapfrog / max(nuts.n_steps, 1):.1f} leaves per transition")
        return
    z = modes(space, logp, z0)
    for order in (2, 4):
        whole = timed(lambda: xo.laplace(logp, z, order=order), max(args.reps // 16, 1), warmup=1)
        lap = xo.laplace(logp, z, order=order)
        rows = int(lap.n_eval[0]) * args.chains
        tp, tf = kernel_times(dev, args.chains, 8, order, args.reps)
        print(f"order {order}, D = {args.chains}, n = 8, {args.cadences} cadences: xo.laplace {whole:.2f} ms ({rows} rows of value + "
              f"gradient, statuses ok: {int((lap.status == 0).sum())} of {args.chains}); points kernel {1e3 * tp:.1f} us, factor kernel "
              f"{1e3 * tf:.1f} us")
        tp, tf = kernel_times(dev, 64, 64, order, args.reps)
        print(f"order {order}, D = 64, n = 64 (synthetic rows): points kernel {1e3 * tp:.1f} us, factor kernel {1e3 * tf:.1f} us")


if __name__ == "__main__":
    main()
