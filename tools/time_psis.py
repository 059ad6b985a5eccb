"""Device-event times of the PSIS-LOO / WAIC kernel (`ops.column_psis`, what `comparison.loo` calls) on the pointwise
log-likelihood of model-like curves -- S draws x N cadences: 2000 x 150 000, 4000 x 150 000 and 100 000 x 1000 -- beside the
two routes it is measured against on the same array and device: the module's torch statement (`torch.sort` along the draws
and the vectorised fit, a block of columns at a time: the only route without the kernel) and `predictive.quantiles` with the
one percent whose rank is the cut-off's (the floor the counting passes set).  The median of --reps after one warm-up call,
one JSON line per shape, with the passes over the array (1 + ceil(ceil(log2(keys between a column's minimum and maximum))
/ 3) + 1, the widest column of a tile deciding) and the share of the kernel's time in the tail work: one minus the time of
the same kernel with a tail of one value (the same passes; no sort, no fit -- where both take the same tile width).

    python tools/time_psis.py [--reps R] [--shapes 2000x150000,4000x150000,100000x1000] [--kernel-only] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from exoplanet_amd import comparison, ops  # noqa: E402
from time_predictive import curves, timed  # noqa: E402

BITS_PER_PASS = 3          # csrc/exo_psis_core.hpp, kBits


def log_likelihood(S, N, dev):
    """the pointwise normal log-likelihood of S model-like curves against one noisy realisation of their mean, in place"""
    ll = curves(S, N, dev)
    y = ll[: min(S, 1000)].mean(0) + 1e-4 * torch.randn(N, dtype=torch.float64, device=dev,
                                                       generator=torch.Generator(device=dev).manual_seed(1))
    for lo in range(0, S, 1000):
        ll[lo:lo + 1000] = comparison.normal_log_likelihood(y, ll[lo:lo + 1000], 1e-4)
    return ll


def passes(values, tile):
    """passes over a tile of `tile` columns, averaged over the tiles: the first, the search of its widest column, the gather"""
    lo, hi = values.min(0).values, values.max(0).values
    key = lambda v: torch.where(v >= 0, v.view(torch.int64), torch.iinfo(torch.int64).min - v.view(torch.int64))  # noqa: E731
    # (in float64: a column with values of both signs spans more keys than an int64 holds; the logarithm does not care)
    bits = torch.ceil(torch.log2(key(hi).to(torch.float64) - key(lo).to(torch.float64) + 1.0))
    pad = (-bits.numel()) % tile
    bits = torch.cat([bits, bits.new_zeros(pad)]).reshape(-1, tile).max(1).values
    return 2.0 + float(torch.ceil(bits / BITS_PER_PASS).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="2000x150000,4000x150000,100000x1000", help="draws x points, comma separated")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes.split(","):
        S, N = (int(v) for v in shape.split("x"))
        values = log_likelihood(S, N, dev)
        M = comparison.tail_length(S)
        t_kernel = timed(lambda: ops.column_psis(values, M), a.reps)
        # (a tail of one value takes the 32-column tile: the same passes only where the full tail takes it too)
        t_no_tail = timed(lambda: ops.column_psis(values, 1), a.reps) if M <= 512 else None
        t_quantile = timed(lambda: ops.column_quantiles(values, [M], [S - 1]), a.reps)
        t_torch, worst = None, None
        if not a.kernel_only:
            got, want = ops.column_psis(values, M), comparison._torch_statement(values, M)
            worst = {k: float((got[k] - want[k]).abs().nan_to_num(0.0, 0.0, 0.0).max()) for k in ("elpd", "k", "lppd", "var")}
            worst["n_tail_equal"] = bool(torch.equal(got["n_tail"], want["n_tail"]))
            del got, want
            t_torch = timed(lambda: comparison._torch_statement(values, M), a.reps)
        n_pass = passes(values, 32 if M <= 512 else 16)
        row = dict(draws=S, points=N, tail=M, kernel_s=t_kernel, kernel_tail_of_one_s=t_no_tail, tail_share=1.0 - t_no_tail / t_kernel if t_no_tail else None,
                   quantile_s=t_quantile, kernel_over_quantile=t_kernel / t_quantile, torch_statement_s=t_torch,
                   torch_over_kernel=t_torch / t_kernel if t_torch else None, max_abs_difference=worst, passes=n_pass,
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
