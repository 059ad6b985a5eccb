#!/usr/bin/env python
"""Times one tick of the batched L-BFGS (exoplanet_amd.optimize.LBFGS: a value + gradient evaluation of every chain and the
per-chain decision) on the white-noise likelihood of a transit through a ParameterSpace of t0, r, b, mean and log_jitter, four
ways in the same process, alternately:

  graph   the native decision kernel, the tick replayed as a hipGraph
  eager   the native decision kernel, launched eagerly
  torch   the torch statement of the decision (what runs off the device), eagerly
  leaf    a graphed NUTS leaf on the same likelihood (two small launches around the same evaluation)

Device events around enough calls for >= --seconds per measurement, after a warm-up; --repeats measurements per cell, median
[min .. max].  The chains' tolerances are set to zero so that every chain keeps running while it is timed.  Also reported:
evaluations to convergence (default tolerances) of the two-stage MAP from starts a few standard deviations off.

    python tools/time_optimize.py [--chains 1024] [--cadences 150000] [--repeats 5] [--max-linesearch 20] [--out table.md]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exoplanet_amd as xo  # noqa: E402
from exoplanet_amd import distributions as xd  # noqa: E402
from exoplanet_amd.optimize import LBFGS  # noqa: E402


def model(n_cad, D, dev):
    rng = np.random.default_rng(n_cad)
    t = torch.arange(n_cad, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    lc = xo.LimbDarkLightCurve(0.3, 0.2)
    with torch.no_grad():
        f0 = lc.get_light_curve(orbit=xo.KeplerianOrbit(period=T(3.5), t0=T(1.0), b=T(0.3)), r=T(0.1), t=t)[:, 0]
    y = f0 + 5e-4 * torch.as_tensor(rng.normal(size=n_cad), device=dev)
    space = xd.ParameterSpace(t0=xd.normal(1.0, 0.1), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              mean=xd.normal(0.0, 1e-2), log_jitter=xd.normal(math.log(4e-4), 2.0), device=dev)

    def loglike(t0, r, b, mean, log_jitter):
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=3.5, t0=t0, b=b), r=r, t=t, y=y, yerr=3e-4, mean=mean,
                                             jitter=torch.exp(log_jitter))

    col = lambda v: torch.tensor(v).reshape(D, 1)  # noqa: E731
    s = math.sqrt(8000.0 / n_cad)                   # the posterior narrows with the number of cadences
    z0 = space.unconstrain(D, t0=col(1.0 + 6e-4 * s * rng.normal(size=D)), r=col(0.1 * (1 + 0.015 * s * rng.normal(size=D))),
                           b=col(np.clip(0.3 + 0.1 * s * rng.normal(size=D), 0.05, 0.6)), mean=col(2e-5 * s * rng.normal(size=D)),
                           log_jitter=col(math.log(4e-4) + 0.05 * s * rng.normal(size=D)))
    return space, space.wrap(loglike), z0


def ms_per_call(fn, min_seconds):
    for _ in range(2):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 2
    while True:
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= 1e3 * min_seconds:
            return ms / n
        n = max(2 * n, int(math.ceil(1.2 * n * 1e3 * min_seconds / max(ms, 1e-3))))


BLOCK = 64        # what is timed is a block: a fresh start and BLOCK ticks (BLOCK + 1 evaluations), or the BLOCK leaves of a doubling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--cadences", type=int, default=150000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--max-linesearch", type=int, default=20, help="of the convergence runs (the ticks that are timed never stop)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_optimize.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    space, logp, z0 = model(a.cadences, a.chains, dev)

    # evaluations to convergence of the two stages, default tolerances
    z1, i1 = xo.optimize(logp, [z0], free=[space.free_mask(["t0", "r"])], return_info=True, max_linesearch=a.max_linesearch)
    z2, i2 = xo.optimize(logp, z1, return_info=True, max_linesearch=a.max_linesearch)
    conv = dict(max_linesearch=a.max_linesearch, stage_one_status_counts=torch.bincount(i1["status"].cpu(), minlength=5).tolist(),
                stage_one_never_moved=int((i1["n_iter"] == 0).sum()),
                stage_one_evals=[int(i1["n_eval"].min()), int(i1["n_eval"].max())],
                stage_two_evals=[int(i2["n_eval"].min()), int(i2["n_eval"].max())],
                status_counts=torch.bincount(i2["status"].cpu(), minlength=5).tolist(),
                logp_spread=float(i2["logp"].max() - i2["logp"].min()))
    print(json.dumps(conv), flush=True)

    calls, units = {}, {}
    for name, kw in (("graph", {}), ("eager", dict(graph=False)), ("torch", dict(native=False))):
        opt = LBFGS(logp, [z0.clone()], ftol=0.0, gtol=0.0, **kw)

        def block(opt=opt, tick=opt._graph if opt._graph is not None else opt._tick):
            opt._start()                                # (every block climbs from the same points: the chains are running)
            for _ in range(BLOCK):
                tick()

        calls[name], units[name] = block, BLOCK + 1
    # the leaves of doubling 6 of a transition (64 of them: inside the tree's checkpoints and random numbers at max_depth = 8)
    nuts = xo.NUTS(logp, [z0.clone()], step_size=1e-3, max_depth=8, generator=torch.Generator(device=dev).manual_seed(1))
    nuts.step()

    def leaves():
        nuts._st["active"].fill_(True)
        nuts._begin_doubling()
        for _ in range(BLOCK):
            nuts._graph()

    calls["leaf"], units["leaf"] = leaves, BLOCK
    times = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, call in calls.items():                   # alternately
            times[k].append(ms_per_call(call, a.seconds) / units[k])
    row = dict(chains=a.chains, cadences=a.cadences)
    for k, v in times.items():
        row[k] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    print(json.dumps(row), flush=True)
    fmt = lambda c: f"{c['median']:.3f} [{c['min']:.3f} .. {c['max']:.3f}]"  # noqa: E731
    table = "\n".join(["| chains | cadences | graphed tick, ms | eager tick, ms | torch statement, ms | graphed NUTS leaf, ms |",
                       "|---|---|---|---|---|---|",
                       f"| {a.chains} | {a.cadences} | {fmt(row['graph'])} | {fmt(row['eager'])} | {fmt(row['torch'])} | {fmt(row['leaf'])} |"])
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n" + json.dumps(conv) + "\n")


if __name__ == "__main__":
    main()
