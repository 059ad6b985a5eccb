"""Device-event times of estimators.keplerian_max_power on a batch of --series resampled series at N epochs x F frequencies x
(--ecc x --phases) candidates, beside the route it replaces: estimators.keplerian_power on the same batch and the row maximum
(--route; its (B, F) outputs need 20 bytes per series and frequency and more for the coefficients, so it runs in slices of
--route-slice series whose times are added).  The median of --reps after one warm-up call, one JSON line per shape, with the
workgroups of the new kernel, a digest of its results and whether the two routes agree bit for bit.  EXOPLANET_AMD_LIB selects
another build of the library (a group width other than the shipped one: -DEXO_KEP_MAX_GROUP=G on exo_keplerian.hip; --group G tells the tool, which only
reports it).

    python tools/false_alarm_timing.py [--reps R] [--shapes 200x100000,2000x20000] [--series 128] [--route] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

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
    ap.add_argument("--shapes", default="200x100000,2000x20000", help="epochs x frequencies, comma separated")
    ap.add_argument("--series", type=int, default=128)
    ap.add_argument("--ecc", type=int, default=10)
    ap.add_argument("--phases", type=int, default=64)
    ap.add_argument("--instruments", type=int, default=2)
    ap.add_argument("--group", type=int, default=E.KEPLERIAN_MAX_GROUP)
    ap.add_argument("--per-block", type=int, default=None)
    ap.add_argument("--route", action="store_true")
    ap.add_argument("--route-slice", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ecc = np.linspace(0.0, 0.9, a.ecc)
    rows = []
    for shape in a.shapes.split(","):
        n, n_freq = (int(x) for x in shape.split("x"))
        rs = np.random.RandomState(n)
        t = np.sort(rs.uniform(0.0, 1000.0, n))
        inst = rs.randint(0, a.instruments, n)
        inst[:a.instruments] = np.arange(a.instruments)
        err = rs.uniform(1.0, 3.0, n)
        y = 30.0 * np.sin(2 * np.pi * t / 17.3) + err * rs.randn(n)
        freq = np.linspace(0.001, 1.0, n_freq)
        idx = torch.as_tensor(E.resample_indices(n, a.series, instrument=inst, seed=0), device=dev)
        td, yd, ed = (torch.as_tensor(x, device=dev) for x in (t, y, err))
        ys, es = yd[idx], ed[idx]
        kw = dict(frequencies=freq, ecc=ecc, n_phase=a.phases, instrument=inst)
        groups = -(-a.series // a.group)
        per_block = a.per_block or max(1, n_freq // -(-16384 // groups))        # (the host's choice, csrc/exo_keplerian.hip)
        row = dict(n=n, frequencies=n_freq, series=a.series, ecc=a.ecc, phases=a.phases, instruments=a.instruments, group=a.group,
                   frequencies_per_block=per_block, workgroups=groups * -(-n_freq // per_block))
        got = {}

        def new():
            got.update(E.keplerian_max_power(td, ys, es, frequencies_per_block=a.per_block, **kw))

        row.update(max_s=timed(new, a.reps))
        # (equal digests: bitwise equal results, whatever the build and the block length)
        row.update(digest=hashlib.sha1(b"".join(got[k].cpu().numpy().tobytes() for k in sorted(got))).hexdigest()[:16])
        if a.route:
            top = torch.empty(a.series, dtype=torch.float64, device=dev)

            def route():
                for b in range(0, a.series, a.route_slice):
                    top[b:b + a.route_slice] = E.keplerian_power(td, ys[b:b + a.route_slice], es[b:b + a.route_slice], **kw).max(dim=1).values

            row.update(route_s=timed(route, a.reps))
            row.update(speedup=row["route_s"] / row["max_s"], bitwise_equal=bool(torch.equal(top, got["power"])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
