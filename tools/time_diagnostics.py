#!/usr/bin/env python
"""Times what DESIGN.md section 16.5 reports, every stage in a child process of its own under its own time limit (a stage that
fails or runs out of time ends the run: nothing more is started on the device after it):

  summary   `diagnostics.summary` of --draws x --chains x --params on the device, split by device events into the sorts, the
            preparation + rank passes, the autocovariance blocks + finish, and the assembly; beside it the torch statement on
            the same device tensor
  host      the torch statement on the host's cores (--threads), on the same numbers
  record    100 `NUTS.step()` calls by hand against `sample(draws=100)` on the white-noise transit model of the README, from
            the same seed: what recording costs

Median of --repeats.  The series are AR(1) with phi from 0 to 0.9 across the parameters, so the truncation ends in the first
lag block for some and runs over several for others.

    python tools/time_diagnostics.py [--draws 1000] [--chains 1024] [--params 16] [--repeats 3] [--out table.md]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = dict(summary=300, host=420, record=300)        # seconds


def series(a, device):
    g = torch.Generator().manual_seed(11)
    e = torch.randn(a.draws + 100, a.chains, a.params, dtype=torch.float64, generator=g)
    phi = torch.linspace(0.0, 0.9, a.params, dtype=torch.float64)
    x = torch.zeros_like(e)
    for n in range(1, e.shape[0]):
        x[n] = phi * x[n - 1] + e[n]
    return x[100:].contiguous().to(device)


def stage_summary(a):
    from exoplanet_amd import diagnostics as dg
    from exoplanet_amd import ops

    dev = torch.device("cuda:0")
    x = series(a, dev)
    N, C, P = x.shape
    L, M = N // 2, 2 * C
    split, total = {}, []
    for rep in range(a.repeats + 1):                      # (the first run warms up)
        info = {}
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        xs = torch.cat([x[:L], x[N - L:]], dim=1).permute(2, 0, 1).contiguous()
        full = None if N % 2 == 0 else x.permute(2, 0, 1).reshape(P, N * C).contiguous()
        ops.chain_diagnostics(xs, full, M, timings=info)
        t1.record()
        torch.cuda.synchronize()
        if rep == 0:
            continue
        total.append(t0.elapsed_time(t1))
        ev = info["events"]
        for (_, e0), (name, e1) in zip(ev[:-1], ev[1:]):
            split.setdefault(name, []).append(e0.elapsed_time(e1))
    res = dict(stage="summary", draws=N, chains=C, params=P, lag_blocks=info["lag_blocks"], device_ms=float(np.median(total)),
               split_ms={k: float(np.median(v)) for k, v in split.items()})
    torch_ms = []
    for rep in range(a.repeats + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ref = dg._torch_statement(x)
        t1.record()
        torch.cuda.synchronize()
        if rep:
            torch_ms.append(t0.elapsed_time(t1))
    got = dg._compute(x)[0]
    res["torch_on_device_ms"] = float(np.median(torch_ms))
    res["largest_relative_difference"] = max(float(((got[k] - ref[k]).abs() / ref[k].abs()).max()) for k in ("ess_bulk", "ess_tail", "r_hat"))
    res["max_t_equal"] = all(bool(torch.equal(got[k], ref[k])) for k in ("max_t_bulk", "max_t_low", "max_t_high", "max_t_mean"))
    return res


def stage_host(a):
    from exoplanet_amd import diagnostics as dg

    torch.set_num_threads(a.threads)
    x = series(a, "cpu")
    times = []
    for _ in range(max(a.repeats // 3, 1)):
        t0 = time.perf_counter()
        dg._torch_statement(x)
        times.append(1e3 * (time.perf_counter() - t0))
    return dict(stage="host", threads=a.threads, torch_on_host_ms=float(np.median(times)))


def stage_record(a):
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(61)
    n_cad, D, sigma = 20000, 1024, 5e-4
    t = torch.arange(n_cad, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    with torch.no_grad():
        f0 = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=xo.KeplerianOrbit(period=T(3.5), t0=T(1.0), b=T(0.3)), r=T(0.1), t=t)[:, 0]
    y = 1.0 + f0 + sigma * torch.as_tensor(rng.normal(size=n_cad), device=dev)
    space = xd.ParameterSpace(period=xd.normal(3.5, 1e-3), t0=xd.normal(1.0, 1e-2), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              u=xd.quad_limb_dark(), mean=xd.normal(1.0, 1e-2), log_jitter=xd.normal(math.log(sigma), 2.0), device=dev)

    def logp(period, t0, r, b, u1, u2, mean, log_jitter):
        return xo.LimbDarkLightCurve(u1.squeeze(-1), u2.squeeze(-1)).white_noise_log_likelihood(
            orbit=xo.KeplerianOrbit(period=period, t0=t0, b=b), r=r, t=t, y=y, yerr=3e-4, mean=mean, jitter=torch.exp(log_jitter))

    z0 = space.unconstrain(D, period=3.5, t0=1.0, r=0.1, b=0.3, u1=0.3, u2=0.2, mean=1.0, log_jitter=math.log(4e-4))

    def sampler():
        nuts = xo.NUTS(space.wrap(logp), [z0.clone()], step_size=1e-3, max_depth=6, generator=torch.Generator(device=dev).manual_seed(9))
        nuts.warmup(100, adapt_mass=True)
        return nuts

    by_hand, recorded, leaves = [], [], []
    for rep in range(a.repeats + 1):
        for which in ("hand", "sample"):
            nuts = sampler()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = nuts.n_leapfrog
            t0.record()
            if which == "hand":
                for _ in range(100):
                    nuts.step()
            else:
                xo.sample(nuts, draws=100)
            t1.record()
            torch.cuda.synchronize()
            if rep:
                (by_hand if which == "hand" else recorded).append(t0.elapsed_time(t1) / 100)
                leaves.append(nuts.n_leapfrog - before)
    assert len(set(leaves)) == 1, leaves                       # the same chain both ways
    h, r = float(np.median(by_hand)), float(np.median(recorded))
    return dict(stage="record", chains=D, n_cad=n_cad, leaves_per_step=leaves[0] / 100, step_by_hand_ms=h, step_recorded_ms=r,
                overhead_percent=100.0 * (r - h) / h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--params", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--stages", default="summary,host,record")
    ap.add_argument("--stage", default=None, help="(internal) run one stage in this process and print its JSON line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stage:
        if a.stage != "host" and not torch.cuda.is_available():
            raise SystemExit("time_diagnostics.py measures on the GPU; there is none here")
        print(json.dumps(dict(summary=stage_summary, host=stage_host, record=stage_record)[a.stage](a)), flush=True)
        return
    rows = []
    for stage in a.stages.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage] + [f"--{k}={getattr(a, k)}" for k in
                                                                                ("draws", "chains", "params", "repeats", "threads")]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[stage])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"stage {stage} ran out of its {LIMITS[stage]} s: stopping here")
        if out.returncode != 0:
            raise SystemExit(f"stage {stage} ended with status {out.returncode}: stopping here\n{out.stdout}{out.stderr}")
        rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
