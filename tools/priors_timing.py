#!/usr/bin/env python
"""What a ParameterSpace costs inside a sampler's leaf: one value + gradient evaluation of

  (a) the white-noise likelihood alone, on unconstrained tensors (the sampler without priors),
  (b) the same behind ``space.wrap`` on the device (the two kernels of csrc/exo_priors.hip),
  (c) the same behind the composed torch statement (``space.constrain_composed``),

each captured as a hipGraph exactly as the samplers evaluate it (flat array -> views -> logp -> gradient -> flat array), timed
with device events around windows of replays of at least ``--window`` seconds, the three legs alternated inside one process,
median of ``--repeats`` windows.  Shapes: ``readme`` (one planet, 6 coordinates) and ``four`` (four planets, 26 parameters on
30 coordinates).  Prints one JSON line per shape.

``--trace LEG``: instead, run ``--evals`` EAGER evaluations of one leg and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/priors_timing.py --shape four --trace b): kernels per evaluation = calls / evals.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exoplanet_amd as xo  # noqa: E402
from exoplanet_amd import distributions as xd  # noqa: E402


def setup(shape, n_cad, D, dev):
    """-> (likelihood of the constrained parameters by keyword, space, z0 (D, n_free), the leg-(a) parameter list)"""
    rng = np.random.default_rng(7)
    t = torch.arange(n_cad, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    P = 1 if shape == "readme" else 4
    span = float(t[-1])
    period = np.array([3.5, 5.2, 8.1, 12.3][:P])
    t0 = np.array([1.0, 2.2, 3.1, 4.7][:P])
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)  # noqa: E731
    with torch.no_grad():
        orbit = xo.KeplerianOrbit(period=T(period), t0=T(t0), b=T([0.3, 0.4, 0.2, 0.5][:P]))
        y = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=orbit, r=T([0.1, 0.05, 0.07, 0.04][:P]), t=t).sum(-1)
        y = y + 5e-4 * torch.as_tensor(rng.normal(size=n_cad), device=dev)
    assert span > period.max()

    if shape == "readme":
        def like(period, t0, r, b, u1, u2):
            lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
            return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y, yerr=5e-4)

        space = xd.ParameterSpace(period=xd.normal(3.5, 1e-3), t0=xd.normal(1.0, 1e-2), r=xd.uniform(0.01, 0.3),
                                  b=xd.impact_parameter(ror="r"), u=xd.quad_limb_dark(), device=dev)
        start = dict(period=3.5, t0=1.0, r=0.1, b=0.3, u1=0.3, u2=0.2)
    else:
        def like(period, t0, r, b, ecc, omega, u1, u2):
            lc = xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1))
            orbit = xo.KeplerianOrbit(period=period, t0=t0, b=b, ecc=ecc, omega=omega)
            return lc.white_noise_log_likelihood(orbit=orbit, r=r, t=t, y=y, yerr=5e-4)

        space = xd.ParameterSpace(period=xd.normal(0.0, 1e-3, shape=4), t0=xd.normal(0.0, 1e-2, shape=4), r=xd.uniform(0.01, 0.3, shape=4),
                                  b=xd.impact_parameter(ror="r", shape=4), ecc=xd.kipping13(shape=4), omega=xd.angle(shape=4),
                                  u=xd.quad_limb_dark(), device=dev)
        # (the normal blocks are offsets from the ephemeris: one prior width per block)
        inner = like
        period_c, t0_c = T(period), T(t0)
        like = lambda period, t0, **kw: inner(period + period_c, t0 + t0_c, **kw)  # noqa: E731
        start = dict(period=0.0, t0=0.0, r=[0.1, 0.05, 0.07, 0.04], b=[0.3, 0.4, 0.2, 0.5], ecc=0.05, omega=0.5, u1=0.3, u2=0.2)
    jitter = {k: torch.as_tensor(np.asarray(v, dtype=float) * (1 + 1e-3 * rng.normal(size=(D, 1)))) for k, v in start.items()}
    z0 = space.unconstrain(D, **jitter)
    with torch.no_grad():
        theta, _ = space.constrain(z0)
    return like, space, z0, [theta[k].clone() for k in space.names]


def flat_evaluation(logp_fn, sizes):
    """one value + gradient evaluation the way the samplers make it: (D, n) -> views -> logp -> gradient -> (D, n)"""
    def fn(q):
        with torch.enable_grad():
            parts = list(torch.split(q.detach().requires_grad_(True), sizes, dim=1))
            lp = logp_fn(*parts)
            grads = torch.autograd.grad(lp, parts, grad_outputs=torch.ones_like(lp))
        return lp.detach(), torch.cat([g.detach() for g in grads], dim=1)
    return fn


def legs(shape, n_cad, D, dev):
    like, space, z0, theta0 = setup(shape, n_cad, D, dev)
    names = space.names
    sizes = [int(x.shape[1]) for x in theta0]
    a = flat_evaluation(lambda *parts: like(**dict(zip(names, parts))), sizes)
    b = flat_evaluation(space.wrap(like), [space.n_free])

    def composed(z):
        theta, log_prior = space.constrain_composed(z)
        return like(**{k: theta[k] for k in names}) + log_prior

    c = flat_evaluation(composed, [space.n_free])
    return {"a": (a, torch.cat(theta0, 1).contiguous()), "b": (b, z0), "c": (c, z0)}, space


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["readme", "four", "both"], default="both")
    ap.add_argument("--cadences", type=int, default=150000)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", choices=["a", "b", "c"])
    ap.add_argument("--evals", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in (["readme", "four"] if args.shape == "both" else [args.shape]):
        fns, space = legs(shape, args.cadences, args.chains, dev)
        if args.trace:
            fn, q = fns[args.trace]
            for _ in range(args.evals):
                fn(q)
            torch.cuda.synchronize()
            print(json.dumps({"shape": shape, "leg": args.trace, "eager_evaluations": args.evals}))
            continue
        graphs = {k: xo.GraphedStep(fn, q.clone()) for k, (fn, q) in fns.items()}
        values = {k: float(g()[0].sum()) for k, g in graphs.items()}
        assert abs(values["b"] - values["c"]) <= 1e-9 * abs(values["c"]), values
        n_rep = {}
        for k, g in graphs.items():                      # replays per window, from a warmed-up estimate
            for _ in range(20):
                g()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                g()
            e1.record()
            torch.cuda.synchronize()
            n_rep[k] = max(int(args.window / (e0.elapsed_time(e1) / 50 * 1e-3)) + 1, 50)
        ms = {k: [] for k in graphs}
        for _ in range(args.repeats):
            for k, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_rep[k]):
                    g()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / n_rep[k])
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({"shape": shape, "cadences": args.cadences, "chains": args.chains, "n_free": space.n_free,
                          "ms_per_evaluation": med, "all_ms": ms, "spread_a_ms": max(ms["a"]) - min(ms["a"]),
                          "b_minus_a_us": 1e3 * (med["b"] - med["a"]), "c_minus_a_us": 1e3 * (med["c"] - med["a"]),
                          "replays_per_window": n_rep}), flush=True)


if __name__ == "__main__":
    main()
