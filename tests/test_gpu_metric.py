"""GPU: the three entries of csrc/exo_metric.hip (exo_metric_apply_f64, exo_metric_accumulate_f64, exo_metric_update_f64)
against the long-double numpy statement (tests/metric_oracle.py) with the allowance of tests/test_metric_host.py (16 units of
the float64 statement's own error), and against the host build of the same core (tests/metric_harness.cpp), whose bits they
are to give: both form every sum in one stated order without fused multiply-adds.  Also D = 130 (three workgroups of the
apply kernel, three tiles of the sums), the failing updates, in-place application, sums that continue, reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_oracle as O  # noqa: E402
from test_metric_host import _failing_windows, build_harness, check, run_harness  # noqa: E402

pytestmark = pytest.mark.gpu


def _call(name, dev, *args):
    from exoplanet_amd import _lib

    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def run_device(c, dev):
    """the five operations of a case through the entries"""
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    n, D = c["n"], c["D"]
    chol, center, shift = T(c["chol"]), T(c["center"]), T(c["shift"])
    out = {}
    for key, src, mode in (("forward", "x", O.FORWARD), ("transposed", "gq", O.TRANSPOSED), ("solve", "q", O.SOLVE)):
        rows, res = T(c[src]), torch.full((D, n), 7.0, dtype=torch.float64, device=dev)
        _call("exo_metric_apply_f64", dev, chol.data_ptr(), center.data_ptr(), rows.data_ptr(), res.data_ptr(), D, n, mode)
        out[key] = res
    s1, s2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, n, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    window = T(c["window"])         # (every argument is held by a name until the call is enqueued)
    _call("exo_metric_accumulate_f64", dev, window.data_ptr(), D, n, shift.data_ptr(), s1.data_ptr(), s2.data_ptr(),
          count.data_ptr())
    out["sum1"], out["sum2"] = s1, s2
    cov, fac = (torch.full((n, n), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
    m, status = torch.full((n,), 7.0, dtype=torch.float64, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
    in1, in2, kept = T(c["sum1"]), T(c["sum2"]), torch.tensor([c["count"]], dtype=torch.int64, device=dev)
    _call("exo_metric_update_f64", dev, in1.data_ptr(), in2.data_ptr(), kept.data_ptr(), shift.data_ptr(), n, cov.data_ptr(),
          fac.data_ptr(), m.data_ptr(), status.data_ptr())
    out["cov"], out["chol"], out["center"] = cov, fac, m
    torch.cuda.synchronize(dev)
    assert int(status) == 0
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["count"] = int(count)
    return out


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def cases():
    """the host test's cases and D = 130, with the statement in long double and in float64, computed once"""
    return [(c, O.statements(c, np.longdouble), O.statements(c, np.float64)) for c in O.cases(O.SIZES_D + (130,))]


def test_entries_against_the_statement_and_the_host_build(dev, harness, cases):
    worst = {}
    for c, ld, f64 in cases:
        label = ("kernels", c["n"], c["D"], c["condition"])
        got = run_device(c, dev)
        for key, r in check(got, ld, f64, label).items():
            worst[key] = max(worst.get(key, 0.0), r)
    print("kernels: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})
    differ = []
    for c, _, _ in cases:
        got, host = run_device(c, dev), run_harness(harness, c)
        differ += [(c["n"], c["D"], key) for key in O.FLOATS + ("count",) if not np.array_equal(got[key], host[key])]
    print("outputs whose bits differ from the host build's:", differ or "none")
    assert not differ


def test_run_to_run_bit_identical(dev, cases):
    for c, _, _ in cases[-6:]:
        a, b = run_device(c, dev), run_device(c, dev)
        for key in O.FLOATS:
            assert np.array_equal(a[key], b[key]), (c["n"], c["D"], key)


def test_in_place_and_continued_sums(dev, harness, cases):
    """`out` may be `in`; a second batch of rows goes on from the sums of the first, as the rows of ONE call would"""
    c = next(c for c, _, _ in cases if c["n"] == 33 and c["D"] == 130)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    n, D = c["n"], c["D"]
    chol, center = T(c["chol"]), T(c["center"])
    for src, mode in (("x", O.FORWARD), ("gq", O.TRANSPOSED), ("q", O.SOLVE)):
        rows, res = T(c[src]), torch.empty(D, n, dtype=torch.float64, device=dev)
        _call("exo_metric_apply_f64", dev, chol.data_ptr(), center.data_ptr(), rows.data_ptr(), res.data_ptr(), D, n, mode)
        _call("exo_metric_apply_f64", dev, chol.data_ptr(), center.data_ptr(), rows.data_ptr(), rows.data_ptr(), D, n, mode)
        assert torch.equal(rows, res)
    sums = []
    for pieces in ((slice(0, D),), (slice(0, 70), slice(70, D))):
        s1, s2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, n, dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        shift = T(c["shift"])
        for sl in pieces:
            w = T(c["window"][sl])
            _call("exo_metric_accumulate_f64", dev, w.data_ptr(), w.shape[0], n, shift.data_ptr(), s1.data_ptr(),
                  s2.data_ptr(), count.data_ptr())
        sums.append((s1, s2, count))
    assert all(torch.equal(a, b) for a, b in zip(*sums))
    assert int(sums[0][2]) == D - 2


@pytest.mark.parametrize("window", [w for w in _failing_windows() if w[5] == 1], ids=lambda w: w[0])
def test_failing_updates_leave_the_metric_alone(dev, window):
    """(the entry always shrinks: the host test's windows that fail with the shrinkage)"""
    _, s1, s2, count, shift, _, want = window
    T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    n = s1.shape[0]
    cov, fac, m = torch.full((n, n), 7.0, device=dev, dtype=torch.float64), torch.full((n, n), 8.0, device=dev, dtype=torch.float64), \
        torch.full((n,), 9.0, device=dev, dtype=torch.float64)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    in1, in2, kept, s = T(s1), T(s2), torch.tensor([count], dtype=torch.int64, device=dev), T(shift)
    _call("exo_metric_update_f64", dev, in1.data_ptr(), in2.data_ptr(), kept.data_ptr(), s.data_ptr(), n, cov.data_ptr(),
          fac.data_ptr(), m.data_ptr(), status.data_ptr())
    assert int(status) == want
    assert bool((cov == 7.0).all()) and bool((fac == 8.0).all()) and bool((m == 9.0).all())


def test_a_pivot_that_is_not_positive(dev):
    """sums no window produces -- a negative second moment -- end at the pivot: status 3, nothing written"""
    n = 4
    s1 = torch.zeros(n, dtype=torch.float64, device=dev)
    s2 = torch.diag(torch.tensor([10.0, 10.0, -10.0, 10.0], dtype=torch.float64, device=dev)).contiguous()
    cov, fac, m = (torch.full(shape, 7.0, device=dev, dtype=torch.float64) for shape in ((n, n), (n, n), (n,)))
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    kept = torch.tensor([10], dtype=torch.int64, device=dev)
    _call("exo_metric_update_f64", dev, s1.data_ptr(), s2.data_ptr(), kept.data_ptr(), s1.data_ptr(), n, cov.data_ptr(),
          fac.data_ptr(), m.data_ptr(), status.data_ptr())
    assert int(status) == 3
    assert bool((cov == 7.0).all()) and bool((fac == 7.0).all()) and bool((m == 7.0).all())
