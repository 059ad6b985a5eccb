"""Device-event times of estimators.running_location (the plan given, so kernels only) and of estimators.location_plan on a
two-minute cadence: N = 150 000 cadences, a 0.5 d window (361 cadences), one series and 64, the median and the biweight at
n_iter = 10.  The method of tools/estimators_timing.py: the median of --reps after one warm-up call.  Beside each, the time of
the host build of the same core header (tests/flatten_harness.cpp, g++ -O2) on --threads threads over one series, times the
number of series.  One JSON line per row; DESIGN.md 19.5 holds the figures.  With --order 1 or 2: the local-polynomial trend
(csrc/exo_trend.hip, rescale = 1) in place of the two locations, beside the host build of tests/trend_harness.cpp; DESIGN.md 21.5.

    python tools/flatten_timing.py [--reps R] [--sizes 150000] [--series 1,64] [--window 0.5] [--threads 16] [--order 0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from estimators_timing import timed  # noqa: E402
from exoplanet_amd import estimators as E  # noqa: E402
from test_flatten_host import _dp, _ip, build_harness  # noqa: E402
from test_trend_host import build_harness as build_trend_harness  # noqa: E402


def cpu_seconds(harness, y, lo, hi, method, threads, t=None, order=0):
    """one series through the host build of exo_detrend_core.hpp, the cadences split evenly over `threads` threads"""
    n = y.size
    trend = np.empty(n)
    edges = np.linspace(0, n, threads + 1).astype(np.int64)
    if order:
        run = lambda k: harness.trend_harness_running(t.ctypes.data_as(_dp), y.ctypes.data_as(_dp), None, lo.ctypes.data_as(_ip),  # noqa: E731
                                                      hi.ctypes.data_as(_ip), int(edges[k]), int(edges[k + 1]), order, 5.0, 10, 1,
                                                      trend.ctypes.data_as(_dp), None)
    else:
        run = lambda k: harness.harness_running_location(y.ctypes.data_as(_dp), None, lo.ctypes.data_as(_ip), hi.ctypes.data_as(_ip),  # noqa: E731
                                                         int(edges[k]), int(edges[k + 1]), method, 5.0, 10, trend.ctypes.data_as(_dp), None)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(run, range(threads)))
    return time.perf_counter() - t0, trend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="150000")
    ap.add_argument("--series", default="1,64")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--order", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    harness = None if a.no_cpu else (build_trend_harness() if a.order else build_harness())
    extra = dict(order=a.order, rescale=1) if a.order else {}
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        t = np.arange(n) * (2.0 / 1440.0)
        rs = np.random.RandomState(n)
        td = torch.as_tensor(t, device=dev)
        plan_s = timed(lambda: E.location_plan(td, a.window), a.reps)          # (includes its one read-back)
        plan = E.location_plan(td, a.window)
        lo, hi = plan.lo.cpu().numpy(), plan.hi.cpu().numpy()
        for B in [int(x) for x in a.series.split(",")]:
            y = 1 + 5e-3 * np.sin(2 * np.pi * t / 1.7) + 1e-3 * rs.randn(B, n)
            yd = torch.as_tensor(y, device=dev)
            for method in ("biweight",) if a.order else ("median", "biweight"):
                gpu = timed(lambda: E.running_location(td, yd, plan=plan, method=method, **extra), a.reps)
                row = dict(n=n, series=B, window=a.window, max_window=plan.max_window, method=method, n_iter=10, plan_s=plan_s, gpu_s=gpu,
                           window_values=float((hi - lo + 1).sum()) * B, **extra)
                if harness is not None:
                    one, trend = cpu_seconds(harness, np.ascontiguousarray(y[0]), lo, hi, E._METHODS[method], a.threads, t, a.order)
                    got = E.running_location(td, yd[0], plan=plan, method=method, **extra).cpu().numpy()
                    row.update(cpu_threads=a.threads, cpu_s_one_series=one, cpu_s=one * B, speedup=one * B / gpu,
                               max_abs_diff_from_host_build=float(np.nanmax(np.abs(got - trend))))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
