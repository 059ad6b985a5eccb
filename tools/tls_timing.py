"""Device-event times of estimators.tls_power beside estimators.bls_power on the rows of DESIGN.md 9.4 (two-minute cadence, the
bls_autoperiod grid at frequency_factor = 1, oversample 10, duration 0.2 d), and one row per size with durations 0.1, 0.2 and
0.4 d.  The method of tools/estimators_timing.py: the median of --reps after one warm-up call; one JSON line per shape with
both times, their ratio and the multiply-adds of the correlation (4 sum_k m_k (n_bins - m_k + 1) per period and series).

    python tools/tls_timing.py [--reps R] [--sizes 20000,65000] [--series 1,64] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from estimators_timing import timed  # noqa: E402
from exoplanet_amd import estimators as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="20000,65000")
    ap.add_argument("--series", default="1,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        t = np.arange(n) * (2.0 / 1440.0)
        rs = np.random.RandomState(n)
        for durations, series in (([0.2], [int(x) for x in a.series.split(",")]), ([0.1, 0.2, 0.4], [1])):
            periods = E.bls_autoperiod(t, durations)
            _, m, n_bins = E.bls_plan(periods, durations, 10)
            templates = [E.transit_template(int(mk)) for mk in m]
            fma = 4.0 * sum(float(mk) * float(np.maximum(n_bins - mk + 1, 0).sum()) for mk in m)
            for B in series:
                y = 1e-3 * rs.randn(B, n)
                y[:, np.abs((t - 1.0 + 1.75) % 3.5 - 1.75) < 0.1] -= 0.002
                td, yd = torch.as_tensor(t, device=dev), torch.as_tensor(y, device=dev)
                bls = timed(lambda: E.bls_power(td, yd, periods=periods, durations=durations), a.reps)
                tls = timed(lambda: E.tls_power(td, yd, periods=periods, durations=durations, templates=templates), a.reps)
                row = dict(n=n, series=B, durations=durations, m=[int(x) for x in m], periods=len(periods), max_bins=int(n_bins.max()),
                           periods_in_workspace=int((n_bins > 3835).sum()), bls_s=bls, tls_s=tls, ratio=tls / bls,
                           pairs=float(n) * len(periods) * B, search_fma=fma * B)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
