"""CPU: the arithmetic of exoplanet_amd/csrc/exo_metric_core.hpp compiled for the host (tests/metric_harness.cpp) and the torch
statement that runs for CPU tensors (exoplanet_amd/sampling.py), against the long-double numpy statement of the five
operations of the dense metric (tests/metric_oracle.py); the updates that must fail; Stan's window schedule; the argument checks
of the C entry points.  The kernels themselves: tests/test_gpu_metric.py.

The yardstick is measured (tests/metric_oracle.py, `ratio`): one unit is the error of the FLOAT64 numpy statement against long
double, at least one eps of the output's scale, and the allowance is 16 units.  Worst ratios measured: host
core 1.1 (the factor), torch statement 3.4 (the solve)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
ALLOWANCE = 16.0


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "metric_harness.so")
    srcs = [os.path.join(ROOT, "tests", "metric_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_metric_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_apply.argtypes = [_dp, _dp, _dp, _dp, _i64, _i32, _i32]
    lib.harness_accumulate.argtypes = [_dp, _i64, _i32, _dp, _dp, _dp, ctypes.POINTER(_i64)]
    lib.harness_update.argtypes = [_dp, _dp, _i64, _dp, _i32, _i32, _dp, _dp, _dp]
    return lib


def _p(a):
    return a.ctypes.data_as(_dp)


def run_harness(lib, c):
    """the five operations of a case through the host build"""
    n, D = c["n"], c["D"]
    out = {}
    for key, src, mode in (("forward", "x", O.FORWARD), ("transposed", "gq", O.TRANSPOSED), ("solve", "q", O.SOLVE)):
        out[key] = np.full((D, n), 7.0)
        assert lib.harness_apply(_p(c["chol"]), _p(c["center"]), _p(np.ascontiguousarray(c[src])), _p(out[key]), D, n, mode) == 0
    out["sum1"], out["sum2"], count = np.zeros(n), np.zeros((n, n)), _i64(0)
    assert lib.harness_accumulate(_p(np.ascontiguousarray(c["window"])), D, n, _p(c["shift"]), _p(out["sum1"]), _p(out["sum2"]),
                                  ctypes.byref(count)) == 0
    out["count"] = count.value
    out["cov"], out["chol"], out["center"] = np.full((n, n), 7.0), np.full((n, n), 7.0), np.full(n, 7.0)
    assert lib.harness_update(_p(c["sum1"]), _p(c["sum2"]), c["count"], _p(c["shift"]), n, 1, _p(out["cov"]), _p(out["chol"]),
                              _p(out["center"])) == 0
    return out


def run_torch(c):
    """... and through the torch statement of exoplanet_amd/sampling.py"""
    from exoplanet_amd import sampling as S

    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731
    n = c["n"]
    out = {}
    for key, src, mode in (("forward", "x", S.METRIC_FORWARD), ("transposed", "gq", S.METRIC_TRANSPOSED),
                           ("solve", "q", S.METRIC_SOLVE)):
        out[key] = S._metric_apply_torch(T(c["chol"]), T(c["center"]), T(c[src]), mode).numpy()
    s1, s2, count = torch.zeros(n, dtype=torch.float64), torch.zeros(n, n, dtype=torch.float64), torch.zeros(1, dtype=torch.int64)
    S._metric_accumulate_torch(T(c["window"]), T(c["shift"]), s1, s2, count)
    out["sum1"], out["sum2"], out["count"] = s1.numpy(), s2.numpy(), int(count)
    cov, chol, center = torch.full((n, n), 7.0, dtype=torch.float64), torch.full((n, n), 7.0, dtype=torch.float64), T(np.full(n, 7.0))
    assert S._metric_update_torch(T(c["sum1"]), T(c["sum2"]), torch.tensor([c["count"]]), T(c["shift"]), cov, chol, center) == 0
    out["cov"], out["chol"], out["center"] = cov.numpy(), chol.numpy(), center.numpy()
    return out


def check(got, ld, f64, label):
    """every output of a case within the allowance; the count and the untouched triangles exactly"""
    assert got["count"] == ld["count"], label
    assert np.array_equal(np.triu(got["sum2"], 1), np.zeros_like(got["sum2"])), label       # (the sums' upper triangle: not touched)
    assert np.array_equal(np.triu(got["chol"], 1), np.zeros_like(got["chol"])), label
    assert np.array_equal(got["cov"], got["cov"].T), label
    worst = {key: O.ratio(np.tril(got[key]) if key == "chol" else got[key], f64[key], ld[key]) for key in O.FLOATS}
    for key, r in worst.items():
        assert r <= ALLOWANCE, (label, key, r)
    return worst


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def cases():
    """per (n, D): the inputs, the statement in long double and in float64, computed once"""
    return [(c, O.statements(c, np.longdouble), O.statements(c, np.float64)) for c in O.cases()]


def test_cases_cover_the_sizes_and_conditions(cases):
    assert {(c["n"], c["D"]) for c, _, _ in cases} == {(n, D) for n in O.SIZES_N for D in O.SIZES_D}
    assert {c["condition"] for c, _, _ in cases} == set(O.CONDITIONS)
    for c, ld, _ in cases:
        # the window's mean is 1e4 times its spread; rows with a NaN and an infinity are in it where there are rows to spare
        kept = c["window"][np.isfinite(c["window"]).all(1)]
        assert np.abs(kept.mean(0)).min() >= 1e4 * kept.std(0).max() * 0.3
        assert ld["count"] == (c["D"] - 2 if c["D"] >= 3 else c["D"])


@pytest.mark.parametrize("which", ["host core", "torch statement"])
def test_against_long_double(harness, cases, which):
    worst = {}
    for c, ld, f64 in cases:
        got = run_harness(harness, c) if which == "host core" else run_torch(c)
        w = check(got, ld, f64, (which, c["n"], c["D"], c["condition"]))
        for key, r in w.items():
            worst[key] = max(worst.get(key, 0.0), r)
    print(f"{which}: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})


def _failing_windows():
    """(label, sum1, sum2, count, shift, shrink, status): N = 1; a NaN sum; a window in which one parameter never left the shift
    -- whole numbers, so that its zero variance is exact -- with the shrinkage switched off, and with it: the shrinkage is
    relative to the parameter's own variance and has nothing to add to zero"""
    n = 5
    rng = np.random.RandomState(3)
    rows = rng.randint(-4, 5, size=(12, n)).astype(np.float64)
    rows[:, 2] = 0.0
    s1, s2, count = O.accumulate(rows, np.zeros(n), np.float64)
    nan1 = s1.copy()
    nan1[1] = np.nan
    one1, one2, _ = O.accumulate(rows[:1], np.zeros(n), np.float64)
    return [("one row", one1, one2, 1, np.zeros(n), 1, 1), ("a NaN sum", nan1, s2, count, np.zeros(n), 1, 2),
            ("a parameter that never moved, no shrinkage", s1, s2, count, np.zeros(n), 0, 3),
            ("a parameter that never moved", s1, s2, count, np.zeros(n), 1, 3)]


@pytest.mark.parametrize("window", _failing_windows(), ids=lambda w: w[0])
def test_failing_updates_leave_the_metric_alone(harness, window):
    from exoplanet_amd import sampling as S

    _, s1, s2, count, shift, shrink, status = window
    n = s1.shape[0]
    cov, chol, center = np.full((n, n), 7.0), np.full((n, n), 8.0), np.full(n, 9.0)
    assert harness.harness_update(_p(s1), _p(s2), count, _p(shift), n, shrink, _p(cov), _p(chol), _p(center)) == status
    assert (cov == 7.0).all() and (chol == 8.0).all() and (center == 9.0).all()
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
    tcov, tchol, tcenter = T(cov).clone(), T(chol).clone(), T(center).clone()
    assert S._metric_update_torch(T(s1), T(s2), torch.tensor([count]), T(shift), tcov, tchol, tcenter, shrink=bool(shrink)) == status
    assert bool((tcov == 7.0).all()) and bool((tchol == 8.0).all()) and bool((tcenter == 9.0).all())
    assert O.update(s1, s2, count, shift, np.longdouble, shrink=bool(shrink))[0] == status


def test_fewer_rows_than_parameters_is_a_metric_with_the_shrinkage(harness):
    """three rows of five parameters that all move: S has rank two, N / (N + 5) S + 1e-3 * 5 / (N + 5) diag(S) is positive definite"""
    n = 5
    rows = np.random.RandomState(4).randint(-4, 5, size=(3, n)).astype(np.float64)
    assert (rows.std(0) > 0).all()
    s1, s2, count = O.accumulate(rows, np.zeros(n), np.float64)
    cov, chol, center = np.full((n, n), 7.0), np.full((n, n), 8.0), np.full(n, 9.0)
    assert harness.harness_update(_p(s1), _p(s2), count, _p(np.zeros(n)), n, 1, _p(cov), _p(chol), _p(center)) == 0
    assert np.allclose(chol @ chol.T, cov, rtol=1e-12, atol=0) and np.array_equal(center, rows.mean(0))
    S = np.cov(rows.T)
    assert np.allclose(np.diag(cov), np.diag(S) * (3.0 / 8.0 + 1e-3 * 5.0 / 8.0), rtol=1e-14)
    assert np.allclose(cov - np.diag(np.diag(cov)), (S - np.diag(np.diag(S))) * 3.0 / 8.0, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("tune", [20, 100, 149, 150, 500, 1000])
def test_schedule(tune):
    from exoplanet_amd.sampling import adaptation_windows

    w = adaptation_windows(tune)
    init, term = (75, 50) if tune >= 150 else (int(0.15 * tune), int(0.1 * tune))
    assert w[0][0] == init and w[-1][1] == tune - term                              # inside the buffers, and filling them
    assert all(a[1] == b[0] for a, b in zip(w, w[1:]))                              # contiguous
    widths = [b - a for a, b in w]
    assert all(x > 0 for x in widths)
    assert all(y == 2 * x for x, y in zip(widths[:-2], widths[1:-1]))               # each doubles ...
    if len(w) > 1:
        assert widths[-1] >= 2 * widths[-2] and widths[-1] < 2 * widths[-2] + 4 * widths[-2]   # ... the last is stretched at most
    if tune >= 150:
        assert widths[0] == 25 or len(w) == 1
    else:
        assert len(w) == 1


def test_schedule_known_values_and_refusal():
    from exoplanet_amd.sampling import adaptation_windows

    assert adaptation_windows(500) == [(75, 100), (100, 150), (150, 250), (250, 450)]
    assert adaptation_windows(150) == [(75, 100)]
    assert adaptation_windows(100) == [(15, 90)]
    with pytest.raises(ValueError):
        adaptation_windows(19)


def test_entry_points_reject_bad_arguments():
    """on the host, before any launch (no GPU needed: the pointers are never followed)"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib
    from exoplanet_amd import sampling as S

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    import re

    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert int(consts["EXO_METRIC_MAX_N"]) == S.MAX_METRIC_N == 64
    assert [int(consts[f"EXO_METRIC_{k}"]) for k in ("FORWARD", "TRANSPOSED", "SOLVE")] == [S.METRIC_FORWARD, S.METRIC_TRANSPOSED,
                                                                                           S.METRIC_SOLVE]
    INVALID, p = 1, 0x1000
    assert lib.exo_metric_apply_f64(p, p, p, p, 4, 0, 0, None) == INVALID
    assert lib.exo_metric_apply_f64(p, p, p, p, 4, 65, 0, None) == INVALID
    assert lib.exo_metric_apply_f64(p, p, p, p, 4, 8, 3, None) == INVALID
    assert lib.exo_metric_apply_f64(p, p, p, p, -1, 8, 0, None) == INVALID
    assert lib.exo_metric_apply_f64(p, None, p, p, 4, 8, 0, None) == INVALID          # the forward map needs the centre
    assert lib.exo_metric_apply_f64(None, p, p, p, 4, 8, 1, None) == INVALID
    assert lib.exo_metric_apply_f64(None, None, None, None, 0, 8, 1, None) == 0       # no rows: nothing to do
    assert lib.exo_metric_accumulate_f64(p, 4, 65, p, p, p, p, None) == INVALID
    assert lib.exo_metric_accumulate_f64(p, 4, 8, p, p, p, None, None) == INVALID
    assert lib.exo_metric_accumulate_f64(None, 0, 8, None, None, None, None, None) == 0
    assert lib.exo_metric_update_f64(p, p, p, p, 0, p, p, p, p, None) == INVALID
    assert lib.exo_metric_update_f64(p, p, p, p, 8, p, p, p, None, None) == INVALID
