#!/usr/bin/env python
"""What a sampled mean and a jitter cost the white-noise likelihood: one value + gradient evaluation (every leaf) of

  (a) today's call: a number ``mean``, a scalar ``yerr`` -- timed TWICE (a, a2), so its own run-to-run spread is on record,
  (b) a per-draw ``mean`` and a per-draw ``jitter`` with a scalar ``yerr`` (per-series sums, O(1) per draw),
  (c) a per-draw ``mean``, a per-cadence ``yerr`` and a per-draw ``jitter`` (the (draw, cadence) pass over the data terms),
  (d) the dense route for the inputs of (c): get_light_curve(total=True) + torch, what the package did with them before,

at the flagship shape (C2: one planet, e = 0.3, two-minute cadence), each captured as a hipGraph the way the samplers evaluate
it and timed with device events around windows of replays of at least ``--window`` seconds, median of ``--repeats`` windows.
Every leg runs in a child process of its own under its own time limit (``--leg X`` runs one inline); one JSON line per leg and
a summary line.  ``--trace LEG``: ``--evals`` eager evaluations of one leg and nothing else, for
``rocprofv3 --kernel-trace --stats -- python tools/white_noise_timing.py --trace b``.  Leg (a) uses nothing newer than
``white_noise_log_likelihood(mean=number)``: the same file times it on an older checkout."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exoplanet_amd as xo  # noqa: E402

LEGS = ["a", "a2", "b", "c", "d"]
LIMIT_S = {"a": 120, "a2": 120, "b": 120, "c": 120, "d": 240}


def setup(leg, n_cad, D, dev):
    """-> (fn(*leaves) -> (ll, *gradients), leaves)"""
    rng = np.random.default_rng(0)
    t = torch.arange(n_cad, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    base = dict(period=3.5, t0=1.0, b=0.3, ecc=0.3, omega=1.1, r=0.1, u1=0.3, u2=0.2)
    leaves = {k: torch.tensor(v * (1 + 1e-3 * rng.normal(size=(D,) if k[0] == "u" else (D, 1))), dtype=torch.float64, device=dev)
              for k, v in base.items()}
    sigma = 5e-4
    with torch.no_grad():
        orbit = xo.KeplerianOrbit(**{k: leaves[k][:1] for k in ("period", "t0", "b", "ecc", "omega")})
        y = 1.0 + xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=orbit, r=leaves["r"][:1], t=t).sum(-1).reshape(-1)
        y = (y + sigma * torch.as_tensor(rng.normal(size=n_cad), device=dev)).contiguous()
    yerr_cad = torch.as_tensor(sigma * (1 + 0.3 * rng.uniform(size=n_cad)), device=dev)
    if leg in ("b", "c", "d"):
        leaves["mean"] = torch.as_tensor(1 + 1e-4 * rng.normal(size=(D, 1)), device=dev)
        leaves["log_jitter"] = torch.as_tensor(np.log(2e-4 * rng.uniform(0.5, 1.5, size=(D, 1))), device=dev)
    names = list(leaves)

    def loglike(L):
        orbit = xo.KeplerianOrbit(period=L["period"], t0=L["t0"], b=L["b"], ecc=L["ecc"], omega=L["omega"])
        star = xo.LimbDarkLightCurve(L["u1"], L["u2"])
        if leg in ("a", "a2"):
            return star.white_noise_log_likelihood(orbit=orbit, r=L["r"], t=t, y=y, yerr=sigma, mean=1.0)
        if leg in ("b", "c"):
            return star.white_noise_log_likelihood(orbit=orbit, r=L["r"], t=t, y=y, yerr=sigma if leg == "b" else yerr_cad,
                                                   mean=L["mean"], jitter=torch.exp(L["log_jitter"]))
        f = star.get_light_curve(orbit=orbit, r=L["r"], t=t, total=True)
        var = yerr_cad ** 2 + torch.exp(2 * L["log_jitter"])
        res = y - L["mean"] - f
        return -0.5 * (res * res / var).sum(-1) - 0.5 * torch.log(var).sum(-1) - 0.5 * n_cad * math.log(2 * math.pi)

    def fn(*vals):
        with torch.enable_grad():
            vals = [v.detach().requires_grad_(True) for v in vals]
            ll = loglike(dict(zip(names, vals)))
            grads = torch.autograd.grad(ll.sum(), vals)
        return (ll.detach(),) + grads

    return fn, list(leaves.values())


def run_leg(args, leg):
    dev = torch.device("cuda:0")
    fn, leaves = setup(leg, args.cadences, args.chains, dev)
    if args.trace:
        for _ in range(args.evals):
            fn(*leaves)
        torch.cuda.synchronize()
        return {"leg": leg, "eager_evaluations": args.evals}
    g = xo.GraphedStep(fn, *leaves)
    value = float(g()[0].sum())
    for _ in range(10):
        g()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        g()
    e1.record()
    torch.cuda.synchronize()
    n_rep = max(int(args.window / (e0.elapsed_time(e1) / 20 * 1e-3)) + 1, 20)
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n_rep):
            g()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / n_rep)
    return {"leg": leg, "cadences": args.cadences, "chains": args.chains, "ms": float(np.median(ms)), "all_ms": ms,
            "replays_per_window": n_rep, "sum_loglike": value}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cadences", type=int, default=150000)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", choices=LEGS, help="run this leg in this process")
    ap.add_argument("--trace", choices=LEGS)
    ap.add_argument("--evals", type=int, default=20)
    args = ap.parse_args()
    if args.leg or args.trace:
        print(json.dumps(run_leg(args, args.leg or args.trace)), flush=True)
        return 0
    out = {}
    for leg in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--cadences", str(args.cadences), "--chains", str(args.chains),
               "--window", str(args.window), "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S[leg])
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": leg, "error": "time limit"}), flush=True)
            return 1     # nothing more on the GPU after a leg that did not come back
        if r.returncode != 0:
            print(json.dumps({"leg": leg, "error": r.stderr[-2000:], "rc": r.returncode}), flush=True)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        out[leg] = json.loads(line)
    ms = {k: v["ms"] for k, v in out.items()}
    summary = {"cadences": args.cadences, "chains": args.chains, "ms": ms}
    if "a" in ms and "a2" in ms:
        every = out["a"]["all_ms"] + out["a2"]["all_ms"]
        summary["a_spread_ms"] = max(every) - min(every)
    for k, ref in (("b", "a"), ("c", "b"), ("d", "c")):
        if k in ms and ref in ms:
            summary[f"{k}_minus_{ref}_us"] = 1e3 * (ms[k] - ms[ref])
    if "d" in ms and "c" in ms:
        summary["d_over_c"] = ms["d"] / ms["c"]
    print(json.dumps(summary), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
