#!/usr/bin/env python
"""Times one step (value + gradient with respect to every sampled parameter) of the tutorials' radial-velocity model --
zero point + linear trend + sum over planets of get_radial_velocity(t, K), sigma^2 = rv_err^2 + exp(2 log_jitter), Normal --
for a batch of draws, two ways in the same process, alternately:

  fused     KeplerianOrbit.rv_log_likelihood (one launch for the likelihood and all its gradients: exo_rv_loglike_vjp_f64)
  composed  get_radial_velocity + float64 torch + autograd (the only route before that kernel existed)

each both eager and as a replayed hipGraph (GraphedStep).  Device events around enough calls for >= 0.5 s per measurement,
after a warm-up; `--repeats` measurements per cell, reported as median [min .. max].  The two routes are compared on the same
inputs before anything is timed.

    python tools/time_rv_like.py [--draws 1024] [--repeats 5] [--out table.md]
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


def model(route, n_cad, P, D, dev):
    rng = np.random.default_rng(1000 * P + n_cad)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    t = T(np.sort(rng.uniform(0.0, 50.0 * max(1, n_cad // 20) ** 0.5, n_cad)))
    rv, rv_err = T(5.0 * rng.normal(size=n_cad)), T(rng.uniform(0.3, 0.7, n_cad))
    t_ref = 0.5 * float(t.min() + t.max())
    b = T(np.full((D, P), 0.2))
    centre = np.concatenate([10.0 * 2.7 ** np.arange(P), 2.0 + np.arange(P), np.full(P, 0.3), 0.8 - np.arange(P), 5.0 / (1 + np.arange(P)),
                             [0.3, math.log(0.4), 0.1, 1e-3]])
    z0 = T(centre * (1 + 0.01 * rng.normal(size=(D, centre.size))))

    def value_and_grad(z):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            period, t0, ecc, omega, K = (zz[:, k * P:(k + 1) * P] for k in range(5))
            zero_point, log_jitter, trend = zz[:, 5 * P:5 * P + 1], zz[:, 5 * P + 1:5 * P + 2], zz[:, 5 * P + 2:5 * P + 4]
            orbit = xo.KeplerianOrbit(period=period, t0=t0, b=b, ecc=ecc, omega=omega)
            if route == "fused":
                ll = orbit.rv_log_likelihood(t, rv, rv_err, K=K, zero_point=zero_point, trend=trend, t_ref=t_ref, jitter=torch.exp(log_jitter))
            else:
                tau = t - t_ref
                m = orbit.get_radial_velocity(t, K=K).reshape(D, n_cad, P).sum(-1) + zero_point + trend[:, 0:1] + trend[:, 1:2] * tau
                s2 = rv_err ** 2 + torch.exp(2 * log_jitter)
                r = rv - m
                ll = -0.5 * (r * r / s2 + torch.log(2 * math.pi * s2)).sum(-1)
            (g,) = torch.autograd.grad(ll, zz, grad_outputs=torch.ones_like(ll))
        return ll.detach(), g

    return value_and_grad, z0


def ms_per_call(fn, min_seconds):
    for _ in range(5):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 10
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rv_like.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rows = []
    for n_cad in (20, 200, 2000):
        for P in (1, 2):
            fns = {r: model(r, n_cad, P, a.draws, dev) for r in ("fused", "composed")}
            (ll_f, g_f), (ll_c, g_c) = (fn(z) for fn, z in fns.values())
            agree = (float((ll_f - ll_c).abs().max() / ll_c.abs().max()), float((g_f - g_c).abs().max() / g_c.abs().max()))
            assert agree[0] <= 1e-10 and agree[1] <= 1e-8, (n_cad, P, agree)
            for mode in ("eager", "graph"):
                if mode == "eager":
                    calls = {r: (lambda fn=fn, z=z: fn(z)) for r, (fn, z) in fns.items()}
                else:
                    calls = {r: xo.GraphedStep(fn, z) for r, (fn, z) in fns.items()}
                times = {r: [] for r in calls}
                for _ in range(a.repeats):
                    for r, call in calls.items():          # alternately
                        times[r].append(ms_per_call(call, a.seconds))
                row = dict(n_cad=n_cad, n_planet=P, draws=a.draws, mode=mode, agree_value=agree[0], agree_grad=agree[1])
                for r, v in times.items():
                    row[r] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
                rows.append(row)
                print(json.dumps(row), flush=True)
    fmt = lambda c: f"{c['median']:.3f} [{c['min']:.3f} .. {c['max']:.3f}]"  # noqa: E731
    lines = ["| n_cad | planets | mode | fused, ms | composed, ms | composed / fused |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n_cad']} | {r['n_planet']} | {r['mode']} | {fmt(r['fused'])} | {fmt(r['composed'])} | "
                     f"{r['composed']['median'] / r['fused']['median']:.1f} |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
