"""Device-event times of estimators.bls_power and estimators.lomb_scargle_power at N = 20 000 / 65 000 / 150 000 two-minute
cadences, B = 1 and B = 64 series.  The box search runs the bls_autoperiod grid at frequency_factor = 1 (duration 0.2 d,
oversample 10); the periodogram runs --ls-freq frequencies (its cost is N x F whatever the grid).  The median of --reps after
one warm-up call, one JSON line per shape, with the cadence-period pairs per second; --numpy also times the numpy restatement
of tests/estimators_oracle.py on --numpy-periods periods (context only: one CPU thread).

    python tools/estimators_timing.py [--reps R] [--sizes 20000,65000,150000] [--series 1,64] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/estimators_timing.py --reps 1 --sizes 65000 --series 1
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

from exoplanet_amd import estimators as E  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="20000,65000,150000")
    ap.add_argument("--series", default="1,64")
    ap.add_argument("--ls-freq", type=int, default=100000)
    ap.add_argument("--max-pairs", type=float, default=2e12, help="skip a box search above this many cadence-period-series triples")
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--numpy-periods", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        t = np.arange(n) * (2.0 / 1440.0)
        rs = np.random.RandomState(n)
        periods = E.bls_autoperiod(t, 0.2)
        freq = np.linspace(0.01, 50.0, a.ls_freq)
        n_bins = E.bls_plan(periods, [0.2], 10)[2]
        for B in [int(x) for x in a.series.split(",")]:
            y = 1e-3 * rs.randn(B, n)
            y[:, np.abs((t - 1.0 + 1.75) % 3.5 - 1.75) < 0.1] -= 0.002
            td, yd = torch.as_tensor(t, device=dev), torch.as_tensor(y, device=dev)
            row = dict(n=n, series=B, periods=len(periods), max_bins=int(n_bins.max()), periods_in_workspace=int((n_bins > 3835).sum()))
            if float(n) * len(periods) * B <= a.max_pairs:
                s = timed(lambda: E.bls_power(td, yd, periods=periods, durations=[0.2]), a.reps)
                row.update(bls_s=s, bls_pairs_per_s=n * len(periods) * B / s)
            s = timed(lambda: E.lomb_scargle_power(td, yd, frequencies=freq), a.reps)
            row.update(ls_frequencies=len(freq), ls_s=s, ls_pairs_per_s=n * len(freq) * B / s)
            if a.numpy and B == 1:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import estimators_oracle as O

                idx = np.linspace(0, len(periods) - 1, a.numpy_periods).astype(int)
                t0 = time.perf_counter()
                O.bls_power(t, y[0], None, periods[idx], [0.2])
                row.update(numpy_bls_pairs_per_s=n * len(idx) / (time.perf_counter() - t0))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
