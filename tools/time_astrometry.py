#!/usr/bin/env python
"""Times one step (value + gradient with respect to every sampled parameter: period, t_periastron, ecc, omega, Omega, cos i,
a and both log jitters) of the tutorial's astrometric model -- separation and position angle from get_relative_angles, the
angle difference wrapped through sin / cos / atan2, sigma^2 = err^2 + exp(2 log_jitter) for each, two Normals -- for a batch
of draws, two ways in the same process, alternately:

  fused     KeplerianOrbit.astrometry_log_likelihood (one launch for the likelihood and all its gradients:
            exo_astrometry_loglike_vjp_f64)
  composed  get_relative_angles + float64 torch + autograd (the only route before that kernel existed)

each both eager and as a replayed hipGraph (GraphedStep).  Device events around enough calls for >= 0.5 s per measurement,
after a warm-up; `--repeats` measurements per cell, reported as median [min .. max].  The two routes are compared on the same
inputs before anything is timed.

    python tools/time_astrometry.py [--draws 1024] [--repeats 5] [--out table.md]
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


def model(route, n_cad, D, dev):
    rng = np.random.default_rng(n_cad)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)  # noqa: E731
    t = T(np.sort(rng.uniform(0.0, 8000.0, n_cad)))
    rho_err, theta_err = T(rng.uniform(0.01, 0.02, n_cad)), T(rng.uniform(0.02, 0.05, n_cad))
    centre = np.array([9131.0, 1100.0, 0.3, 1.9, 2.4, 0.3, 0.3, math.log(0.01), math.log(0.02)])
    with torch.no_grad():      # the data: the model at the centre, position angles in [0, 2 pi), plus noise
        o = xo.KeplerianOrbit(period=T(centre[0:1]), t_periastron=T(centre[1:2]), ecc=T(centre[2:3]), omega=T(centre[3:4]),
                              Omega=T(centre[4:5]), incl=T(np.arccos(centre[5:6])), a=T(centre[6:7]))
        rho0, theta0 = o.get_relative_angles(t)
        rho = rho0.reshape(-1) + rho_err * T(rng.normal(size=n_cad))
        theta = torch.remainder(theta0.reshape(-1) + theta_err * T(rng.normal(size=n_cad)), 2 * math.pi)
    z0 = T(centre * (1 + 0.01 * rng.normal(size=(D, centre.size))))

    def value_and_grad(z):
        with torch.enable_grad():
            zz = z.detach().requires_grad_(True)
            period, tp, ecc, omega, Omega, cosi, a, log_rho_s, log_theta_s = (zz[:, k:k + 1] for k in range(9))
            orbit = xo.KeplerianOrbit(period=period, t_periastron=tp, ecc=ecc, omega=omega, Omega=Omega, incl=torch.acos(cosi), a=a)
            if route == "fused":
                ll = orbit.astrometry_log_likelihood(t, rho, rho_err, theta, theta_err, rho_jitter=torch.exp(log_rho_s),
                                                     theta_jitter=torch.exp(log_theta_s))
            else:
                rho_m, theta_m = orbit.get_relative_angles(t)
                rho_m, theta_m = rho_m.reshape(D, n_cad), theta_m.reshape(D, n_cad)
                diff = theta_m - theta
                delta = torch.atan2(torch.sin(diff), torch.cos(diff))
                s2r, s2t = rho_err ** 2 + torch.exp(2 * log_rho_s), theta_err ** 2 + torch.exp(2 * log_theta_s)
                r = rho - rho_m
                ll = -0.5 * (r * r / s2r + torch.log(2 * math.pi * s2r) + delta * delta / s2t + torch.log(2 * math.pi * s2t)).sum(-1)
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
        raise SystemExit("time_astrometry.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rows = []
    for n_cad in (45, 500, 5000):
        fns = {r: model(r, n_cad, a.draws, dev) for r in ("fused", "composed")}
        (ll_f, g_f), (ll_c, g_c) = (fn(z) for fn, z in fns.values())
        agree = (float((ll_f - ll_c).abs().max() / ll_c.abs().max()), float((g_f - g_c).abs().max() / g_c.abs().max()))
        assert agree[0] <= 1e-10 and agree[1] <= 1e-8, (n_cad, agree)
        for mode in ("eager", "graph"):
            if mode == "eager":
                calls = {r: (lambda fn=fn, z=z: fn(z)) for r, (fn, z) in fns.items()}
            else:
                calls = {r: xo.GraphedStep(fn, z) for r, (fn, z) in fns.items()}
            times = {r: [] for r in calls}
            for _ in range(a.repeats):
                for r, call in calls.items():          # alternately
                    times[r].append(ms_per_call(call, a.seconds))
            row = dict(n_cad=n_cad, draws=a.draws, mode=mode, agree_value=agree[0], agree_grad=agree[1])
            for r, v in times.items():
                row[r] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    fmt = lambda c: f"{c['median']:.3f} [{c['min']:.3f} .. {c['max']:.3f}]"  # noqa: E731
    lines = ["| n_cad | mode | fused, ms | composed, ms | composed / fused |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n_cad']} | {r['mode']} | {fmt(r['fused'])} | {fmt(r['composed'])} | "
                     f"{r['composed']['median'] / r['fused']['median']:.1f} |")
    table = "\n".join(lines)
    print(table)
    if a.out:
        with open(a.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
