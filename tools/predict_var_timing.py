"""Wall times of GaussianProcess.predict(return_var=True) at the bench's series length, with apply_inverse at the same shape
beside it (the mean's share: predict runs it first).  Eager calls, a device synchronisation around each, the median of
--reps after one warm-up call.  N = 150 000 (two-minute cadence), J = 2 (one SHO term: C3's kernel) and J = 6 (three:
C5's), t=None (M = N) and M = 10 000 new times, D in {1, 64, 1024}.  One JSON line per shape.

    python tools/predict_var_timing.py [--reps R] [--draws 1,64,1024] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_var_timing.py --reps 1 --draws 64
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from exoplanet_amd.gp import GaussianProcess, terms  # noqa: E402


def kernel(J, D, dev):
    rng = np.random.default_rng(J)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    sho = lambda sigma, rho, Q: terms.SHOTerm(sigma=T(sigma * (1 + 0.1 * rng.random(D))), rho=T(rho * (1 + 0.1 * rng.random(D))),
                                              Q=T(Q + 0 * rng.random(D)))
    if J == 2:
        return sho(1e-3, 5.0, 0.7)
    return sho(1e-3, 5.0, 0.7) + sho(5e-4, 1.0, 1.0) + sho(3e-4, 0.3, 2.0)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", default="1,64,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 150000
    t = torch.arange(n, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    rows = []
    for J in (2, 6):
        for D in [int(x) for x in a.draws.split(",")]:
            gp = GaussianProcess(kernel(J, D, dev), t=t, yerr=1e-3)
            y = 1e-3 * torch.randn(D, n, dtype=torch.float64, device=dev)
            t_inv = timed(lambda: gp.apply_inverse(y), a.reps)
            for M in (None, 10000):
                tq = None if M is None else torch.linspace(-1.0, float(t[-1]) + 1.0, M, dtype=torch.float64, device=dev)
                t_var = timed(lambda: gp.predict(y, tq, return_var=True), a.reps)
                row = {"J": J, "D": D, "N": n, "M": n if M is None else M, "predict_var_ms": round(1e3 * t_var, 3),
                       "apply_inverse_ms": round(1e3 * t_inv, 3), "var_share_ms": round(1e3 * (t_var - t_inv), 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del gp, y
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
