"""Device-event times of estimators.transit_times (the plan given, so kernels only) and of estimators.timing_plan for a 3-day planet
in four years of one-minute data: 480 transits x 401 shifts x ~950-cadence windows, one series and 16.  The method of
tools/estimators_timing.py: the median of --reps after one warm-up call.  Beside each, the time of the host build of the same
core header (tests/timing_harness.cpp, g++ -O2 -ffp-contract=off) for the same call on ONE core -- measured on one series, times
the number of series -- and the largest difference between the two results.  One JSON line per row; DESIGN.md 20.5 holds the
figures.

    python tools/time_transit_times.py [--reps R] [--series 1,16] [--shifts 401] [--years 4] [--no-cpu] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from estimators_timing import timed  # noqa: E402
from exoplanet_amd import estimators as E  # noqa: E402
from test_timing_host import _dp, _ip, build_harness  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--series", default="1,16")
    ap.add_argument("--shifts", type=int, default=401)
    ap.add_argument("--years", type=float, default=4.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    harness = None if a.no_cpu else build_harness()
    period, t0, duration = 3.0437, 1.3, 0.165                           # window = 4 durations = 0.66 d = 950 cadences
    n = int(a.years * 365.25 * 1440)
    t = np.arange(n) / 1440.0
    rs = np.random.RandomState(7)
    x = ((t - t0 + 0.5 * period) % period - 0.5 * period) / (0.5 * duration)
    signal = -0.01 * np.clip(1 - x * x, 0, None) ** 0.5
    td = torch.as_tensor(t, device=dev)
    g = E.transit_template(256, 0.1, 0.3)
    kw = dict(period=period, t0=t0, duration=duration, n_shift=a.shifts)
    plan_s = timed(lambda: E.timing_plan(td, **kw), a.reps)             # (includes its read-backs)
    plan = E.timing_plan(td, **kw)
    lo, hi = plan.lo.cpu().numpy(), plan.hi.cpu().numpy()
    T_k = plan.linear_time.cpu().numpy()
    K = len(plan.transit_ind)
    rows = []
    for B in [int(v) for v in a.series.split(",")]:
        y = signal + 1e-3 * rs.randn(B, n)
        yd = torch.as_tensor(y, device=dev)
        gpu = timed(lambda: E.transit_times(td, yd, 1e-3, template=g, plan=plan), a.reps)
        row = dict(cadences=n, series=B, transits=K, shifts=a.shifts, max_window=plan.max_window, template=256, plan_s=plan_s, gpu_s=gpu,
                   fits_per_s=K * B * a.shifts / gpu)
        if harness is not None:
            out, iout = np.empty((7, 1, K)), np.empty((4, 1, K), dtype=np.int32)
            y0 = np.ascontiguousarray(y[0])
            ivar = np.full(n, 1.0 / 1e-3 ** 2)
            one = harness.harness_all(t.ctypes.data_as(_dp), y0.ctypes.data_as(_dp), ivar.ctypes.data_as(_dp), n, 1, T_k.ctypes.data_as(_dp),
                                      lo.ctypes.data_as(_ip), hi.ctypes.data_as(_ip), K, duration, plan.max_shift, a.shifts,
                                      g.ctypes.data_as(_dp), g.size, 3, out.ctypes.data_as(_dp), iout.ctypes.data_as(_ip))
            res = E.transit_times(td, yd[0], 1e-3, template=g, plan=plan)
            diff = max(float(np.nanmax(np.abs(res[k].cpu().numpy() - out[i, 0]))) for i, k in enumerate(E.TIMING_FIELDS))
            row.update(cpu_s_one_series_one_core=one, cpu_s=one * B, speedup=one * B / gpu, max_abs_diff_from_host_build=diff,
                       valid=int(res["valid"].sum()), at_edge=int(res["at_edge"].sum()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
