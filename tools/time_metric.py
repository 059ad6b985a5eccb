"""Times of the dense metric on the device: the captured NUTS leaf of the README's white-noise transit
model (8 parameters, 150 000 cadences, 1024 chains) without a metric and with one -- the two added launches of
exo_metric_apply_f64 --, and the three entries alone at n = 8 and n = 64, D = 1024.  Device events around `reps` replays or
launches, the median of three rounds after a warm-up.

    python tools/time_metric.py [--chains 1024] [--cadences 150000] [--reps 256]
"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


BLOCK = 64


def timed(fn, reps, rounds=3, warmup=5):
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


def leaf_times(dev, chains, cadences, reps):
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    g = torch.Generator(device=dev).manual_seed(1)
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
    n = z0.shape[1]
    out = {}
    # the identity as the metric: x is q, so both samplers walk the same points and the likelihood does the same work (its time
    # depends on where the chains are); steps small enough that the chains stay where they started
    for name, kw in (("no metric", {}), ("dense metric", dict(cov=torch.eye(n, dtype=torch.float64)))):
        nuts = xo.NUTS(space.wrap(logp), [z0.clone()], step_size=1e-5, max_depth=8,
                       generator=torch.Generator(device=dev).manual_seed(1), **kw)
        nuts.step()                                   # (fills the tree's buffers with a real state)

        # the leaves of doubling 6 of a transition: 64 of them, inside the tree's checkpoints and random numbers at max_depth = 8
        def block(nuts=nuts):
            nuts._st["active"].fill_(True)
            nuts._begin_doubling()
            for _ in range(BLOCK):
                nuts._graph()

        out[name] = timed(block, max(reps // BLOCK, 1), warmup=1) / BLOCK
    return n, out


def entry_times(dev, D, n, reps):
    from exoplanet_amd import _lib

    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    new = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev)  # noqa: E731
    A = new(n, n)
    cov = A @ A.T + n * torch.eye(n, dtype=torch.float64, device=dev)
    chol, center, rows, res = torch.linalg.cholesky(cov).contiguous(), new(n), new(D, n), new(D, n)
    s1, s2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, n, dtype=torch.float64, device=dev)
    count, status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}
    for mode, name in enumerate(("apply forward", "apply transposed", "apply solve")):
        out[name] = timed(lambda: _lib.check(lib.exo_metric_apply_f64(chol.data_ptr(), center.data_ptr(), rows.data_ptr(),
                                                                      res.data_ptr(), D, n, mode, stream()), name), reps)
    out["accumulate"] = timed(lambda: _lib.check(lib.exo_metric_accumulate_f64(rows.data_ptr(), D, n, center.data_ptr(), s1.data_ptr(),
                                                                              s2.data_ptr(), count.data_ptr(), stream()),
                                                 "accumulate"), reps)
    out["update"] = timed(lambda: _lib.check(lib.exo_metric_update_f64(s1.data_ptr(), s2.data_ptr(), count.data_ptr(),
                                                                      center.data_ptr(), n, cov.data_ptr(), chol.data_ptr(),
                                                                      res.data_ptr(), status.data_ptr(), stream()), "update"), reps)
    torch.cuda.synchronize(dev)
    assert int(status) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--cadences", type=int, default=150000)
    ap.add_argument("--reps", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, leaf = leaf_times(dev, args.chains, args.cadences, args.reps)
    base, dense = leaf["no metric"], leaf["dense metric"]
    print(f"NUTS leaf, D = {args.chains}, n = {n}, {args.cadences} cadences: {base:.4f} ms without a metric, {dense:.4f} ms with one "
          f"(+{100.0 * (dense / base - 1.0):.1f} %)")
    for n in (8, 64):
        times = entry_times(dev, args.chains, n, args.reps)
        print(f"entries alone, D = {args.chains}, n = {n}: " + ", ".join(f"{k} {1e3 * v:.1f} us" for k, v in times.items()))


if __name__ == "__main__":
    main()
