"""Device-event times of estimators.astrometric_power at N epochs x F frequencies x (--ecc x --phases) candidates, beside
estimators.keplerian_power at the same N, F and candidates (one instrument).  The median of --reps after one warm-up call, one
JSON line per shape, with the Kepler solves per second (N x F x the live candidates); --numpy also times the numpy statement
of tests/astrometric_oracle.py in float64 on --numpy-freq frequencies of the same series (context only: one CPU thread) and
extrapolates it to F, which is an extrapolation and is labelled as one.

    python tools/astrometric_timing.py [--reps R] [--shapes 50x20000,500x5000] [--ecc 10] [--phases 64] [--numpy] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import astrometric_oracle as O  # noqa: E402
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
    ap.add_argument("--shapes", default="50x20000,500x5000", help="epochs x frequencies, comma separated")
    ap.add_argument("--ecc", type=int, default=10)
    ap.add_argument("--phases", type=int, default=64)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--numpy-freq", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ecc = np.linspace(0.0, 0.9, a.ecc)
    live = 1 + (a.ecc - 1) * a.phases                        # (e = 0 is one candidate whatever the phase)
    rows = []
    for shape in a.shapes.split(","):
        n, n_freq = (int(x) for x in shape.split("x"))
        s = O.series(n, n, span=1000.0, period=270.0)
        freq = np.linspace(0.0005, 0.05, n_freq)
        td, rd, red, thd, ted = (torch.as_tensor(s[k], device=dev) for k in ("t", "rho", "rho_err", "theta", "theta_err"))
        row = dict(n=n, frequencies=n_freq, ecc=a.ecc, phases=a.phases)
        sec = timed(lambda: E.astrometric_power(td, rd, red, thd, ted, frequencies=freq, ecc=ecc, n_phase=a.phases), a.reps)
        row.update(astrometric_s=sec, kepler_solves_per_s=float(n) * n_freq * live / sec)
        sec = timed(lambda: E.keplerian_power(td, rd, red, frequencies=freq, ecc=ecc, n_phase=a.phases), a.reps)
        row.update(keplerian_s=sec)
        if a.numpy:
            few = freq[np.linspace(0, n_freq - 1, a.numpy_freq).astype(int)]
            t0 = time.perf_counter()
            O.statement(s, few, ecc, a.phases)
            dt = time.perf_counter() - t0
            row.update(numpy_frequencies=len(few), numpy_s=dt, numpy_extrapolated_to_all_frequencies_s=dt / len(few) * n_freq)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
