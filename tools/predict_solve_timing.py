"""Wall times of GaussianProcess.predict and apply_inverse at the bench's series length with the solve by
exo_celerite_solve_f64 (what the package does) and, for comparison, by the route it took before -- minus the gradient of the
likelihood with respect to the residual -- on the likelihood's sequential kernels and on its time-parallel plan; the old
route is put in place of gp.celerite._inverse by this tool alone.  One process, the routes alternating.  N = 150 000
(two-minute cadence), D = 4, one SHO term (J = 2) and three (J = 6); predict at the data times, at M = 10 000 new times,
and with return_var.  Eager calls, a device synchronisation around each, median [min, max] of --reps after one warm-up
call.  One JSON line per shape.

    python tools/predict_solve_timing.py [--reps R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from exoplanet_amd.gp import GaussianProcess, celerite  # noqa: E402
from predict_var_timing import kernel  # noqa: E402


def likelihood_route(n_chunks):
    """what _inverse was before the solve entry point: one forward and one reverse pass of the likelihood on that plan"""
    def inverse(t, resid, diag, real, cplx, kind):
        with torch.enable_grad():
            r = resid.detach().requires_grad_(True)
            ll = celerite.celerite_loglike(t.detach(), r, diag.detach().contiguous(), real.detach(), cplx.detach(),
                                           pair_kind=kind, n_chunks=n_chunks)
            (g,) = torch.autograd.grad(ll.sum(), r)
        return -g
    return inverse


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return [round(statistics.median(out), 3), round(min(out), 3), round(max(out), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, D = 150000, 4
    t = torch.arange(n, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    tq = torch.linspace(-1.0, float(t[-1]) + 1.0, 10000, dtype=torch.float64, device=dev)
    rows = []
    solve = celerite._inverse
    for J in (2, 6):
        gp = GaussianProcess(kernel(J, D, dev), t=t, yerr=1e-3)
        y = 1e-3 * torch.randn(D, n, dtype=torch.float64, device=dev)
        calls = {"apply_inverse": lambda: gp.apply_inverse(y), "predict_data": lambda: gp.predict(y),
                 "predict_new": lambda: gp.predict(y, tq), "predict_new_var": lambda: gp.predict(y, tq, return_var=True)}
        for name, fn in calls.items():
            row = {"J": J, "D": D, "N": n, "call": name}
            for route, label in ((solve, "solve_ms"), (likelihood_route(1), "sequential_ms"),
                                 (likelihood_route(0), "time_parallel_ms")):
                celerite._inverse = route
                row[label] = timed(fn, a.reps)
            celerite._inverse = solve
            row["ratio"] = round(row["solve_ms"][0] / row["time_parallel_ms"][0], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
