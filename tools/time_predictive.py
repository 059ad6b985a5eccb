"""Device-event times of predictive.quantiles (Q = 3: 16 / 50 / 84) at the two shapes of a posterior band -- S = 2000 draws x
N = 150 000 cadences and S = 100 000 draws x N = 1000 phases -- on model-like curves 1 - depth * profile + 1e-4 * noise, beside the
torch route on the same device: torch.sort(values, dim=0).values, the three gathers and the interpolation.  The median of
--reps after one warm-up call, one JSON line per shape, with the passes over the array (from the spread of the keys of a
column: 1 + ceil(ceil(log2(keys between its minimum and maximum)) / 2) + 1 -- three quantiles settle two bits per pass --, the
widest column of a 64- or 16-column tile deciding) and the bytes per second those passes amount to.  The two results are compared bit for bit.

    python tools/time_predictive.py [--reps R] [--shapes 2000x150000,100000x1000] [--kernel-only] [--out FILE]

--kernel-only leaves the torch route out (A/B of two builds of the library, EXOPLANET_AMD_LIB).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from exoplanet_amd import predictive  # noqa: E402

PERCENT = (16, 50, 84)


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


def curves(S, N, dev):
    """S draws of a transit-like profile on N points: depth and width differ from draw to draw, noise of 1e-4 on top"""
    gen = torch.Generator(device=dev).manual_seed(S + N)
    x = torch.linspace(-1.0, 1.0, N, dtype=torch.float64, device=dev)
    out = torch.empty((S, N), dtype=torch.float64, device=dev)
    for lo in range(0, S, 1000):                                    # (in chunks: no second array of the full size)
        n = min(1000, S - lo)
        depth = 0.01 * (1.0 + 0.05 * torch.randn(n, 1, dtype=torch.float64, device=dev, generator=gen))
        width = 0.1 * (1.0 + 0.05 * torch.randn(n, 1, dtype=torch.float64, device=dev, generator=gen))
        profile = torch.clamp(1.0 - (x[None, :] / width) ** 2, min=0.0).sqrt()
        out[lo:lo + n] = 1.0 - depth * profile + 1e-4 * torch.randn(n, N, dtype=torch.float64, device=dev, generator=gen)
    return out


def torch_route(values):
    """the yardstick: a full sort along the draws, then the definition's gathers and interpolation"""
    sv = torch.sort(values, dim=0).values
    m = sv.shape[0]
    rows = []
    for p in PERCENT:
        lo, rem = divmod((m - 1) * p, 100)
        a = sv[lo]
        rows.append(a.clone() if rem == 0 else a + (rem / 100.0) * (sv[lo + 1] - a))
    return torch.stack(rows)


BITS_PER_PASS = 2          # csrc/exo_predictive.hip, bits_per_pass<3>


def passes(values, tile):
    """passes over a tile of `tile` columns, averaged over the tiles: the first, the search of its widest column, the last"""
    lo, hi = values.min(0).values, values.max(0).values
    key = lambda v: torch.where(v >= 0, v.view(torch.int64), torch.iinfo(torch.int64).min - v.view(torch.int64))  # noqa: E731
    span = (key(hi) - key(lo)).to(torch.float64)                     # (approximate above 2^53: the logarithm does not care)
    bits = torch.ceil(torch.log2(span + 1.0))
    n = bits.numel()
    pad = (-n) % tile
    bits = torch.cat([bits, bits.new_zeros(pad)]).reshape(-1, tile).max(1).values
    return 2.0 + float(torch.ceil(bits / BITS_PER_PASS).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="2000x150000,100000x1000", help="draws x points, comma separated")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes.split(","):
        S, N = (int(v) for v in shape.split("x"))
        values = curves(S, N, dev)
        t_kernel = timed(lambda: predictive.quantiles(values, PERCENT), a.reps)
        t_torch, same = None, None
        if not a.kernel_only:
            got = predictive.quantiles(values, PERCENT)
            want = torch_route(values)
            same = bool(torch.equal(got.view(torch.int64), want.view(torch.int64)))
            del got, want
            t_torch = timed(lambda: torch_route(values), a.reps)
        tile = 64 if math.ceil(N / 64) >= 256 else 16
        n_pass = passes(values, tile)
        row = dict(draws=S, points=N, quantiles=len(PERCENT), kernel_s=t_kernel, torch_sort_route_s=t_torch,
                   kernel_over_torch=t_kernel / t_torch if t_torch else None, identical_bits=same, passes=n_pass,
                   bytes_per_s=n_pass * S * N * 8 / t_kernel)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del values
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
