"""CPU: the per-column arithmetic of exoplanet_amd/csrc/exo_predictive_core.hpp compiled for the host
(tests/predictive_harness.cpp) against the numpy statement of the definition (tests/predictive_oracle.py), the torch statement
that runs for CPU tensors, the argument checks of the C entry point and `bands` on a toy model.  The kernel itself:
tests/test_gpu_predictive.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predictive_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_lp = ctypes.POINTER(ctypes.c_int64)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64 = ctypes.c_int64

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 1000)
PERCENTS = (0, 100, 50, 16, 84, 2.5, 97.5, 15.865)


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "predictive_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "predictive_harness.cpp"), os.path.join(csrc, "exo_predictive_core.hpp"),
            os.path.join(csrc, "exo_detrend_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_rank.argtypes = [_i64, _i64, _i64, _lp, _lp]
    lib.harness_column_quantiles.argtypes = [_dp, _i64, _i64, _i64, _lp, _lp, ctypes.c_int, _dp, _ip, _ip]
    return lib


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def run_harness(harness, values, percent, pad=0):
    """values (S, N) through the host build, its rows N + pad doubles apart -> (Q, N), counts, passes"""
    S, N = values.shape
    buf = np.full((S, N + pad), 7.0)           # (what lies between the rows is a number that would show)
    buf[:, :N] = values
    fr = [O.fraction(p) for p in percent]
    num, den = np.array([a for a, _ in fr], dtype=np.int64), np.array([b for _, b in fr], dtype=np.int64)
    out, count, passes = np.empty((len(percent), N)), np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    assert harness.harness_column_quantiles(buf.ctypes.data_as(_dp), S, N, N + pad, num.ctypes.data_as(_lp), den.ctypes.data_as(_lp),
                                            len(percent), out.ctypes.data_as(_dp), count.ctypes.data_as(_ip),
                                            passes.ctypes.data_as(_ip)) == 0
    return out, count, passes


def families(S, seed):
    fam = O.column_families(S, np.random.RandomState(seed))
    return list(fam), np.stack(list(fam.values()), axis=1)


@pytest.mark.parametrize("S", SIZES)
def test_core_equals_the_oracle_exactly(harness, S):
    names, values = families(S, 100 + S)
    want, want_count = O.quantiles(values, PERCENTS)
    for pad in (0, 3):
        for percent in (PERCENTS, PERCENTS[:3], (50,), tuple(PERCENTS) * 2):
            got, count, passes = run_harness(harness, values, percent, pad)
            ref = np.concatenate([want] * 2)[:len(percent)] if len(percent) > len(PERCENTS) else want[:len(percent)]
            if percent == (50,):
                ref = want[2:3]
            for j, name in enumerate(names):
                assert O.same(got[:, j], ref[:, j]), (S, pad, name, percent, got[:, j], ref[:, j])
            assert np.array_equal(count, want_count)
            # one pass for the count and the extremes, at most 64 of bisection, one for the next order statistics
            assert passes.min() >= 1 and passes.max() <= 66
    k = names.index("one value")
    assert passes[k] <= 2                          # a constant column: no bisection at all
    k = names.index("model-like")
    if S >= 64:
        assert passes[k] <= 48, passes[k]          # values that share sign, exponent and leading mantissa bits


def test_whole_number_percents_equal_the_diagnostics_rule(harness):
    from exoplanet_amd import diagnostics

    rs = np.random.RandomState(3)
    for S in SIZES:
        values = np.stack([rs.randn(S), np.round(3 * rs.randn(S)) / 4, 1e-310 * rs.randn(S)], axis=1)
        percent = (0, 5, 16, 50, 84, 95, 100)
        got, _, _ = run_harness(harness, values, percent)
        sv = torch.sort(torch.as_tensor(values).T.contiguous(), dim=1).values
        for q, p in enumerate(percent):
            assert O.same(got[q], (diagnostics._quantile_sorted(sv, p) + 0.0).numpy()), (S, p)


def test_rank_rule_and_the_reading_of_a_percent(harness):
    from exoplanet_amd import predictive

    assert predictive._fraction(2.5) == (1, 40) and O.fraction(2.5) == (1, 40)
    assert predictive._fraction(15.865) == (3173, 20000)
    assert predictive._fraction(0) == (0, 1) and predictive._fraction(100) == (1, 1) and predictive._fraction("84") == (21, 25)
    for bad in (-1, 100.5, float("nan"), float("inf"), "x", 1e-12):
        with pytest.raises(ValueError):
            predictive._fraction(bad)
    with pytest.raises(ValueError):
        predictive._fractions([])
    lo, rem = _i64(), _i64()
    for m, a, b in [(1, 1, 2), (2, 1, 2), (1000, 1, 40), (2 ** 31 - 1, 10 ** 9 - 1, 10 ** 9), (65, 3173, 20000), (5, 1, 1), (5, 0, 1)]:
        harness.harness_rank(m, a, b, ctypes.byref(lo), ctypes.byref(rem))
        assert (lo.value, rem.value) == divmod((m - 1) * a, b)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """the pointers are never followed: each of these calls returns before a launch"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib, ops

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    assert "#define EXO_QUANTILE_MAX_Q 16" in text and ops.QUANTILE_MAX_Q == 16
    OK, INVALID = 0, 1
    x, out, cnt = 0x1000, 0x2000, 0x3000
    L = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731

    def call(x=x, S=10, N=8, stride=8, num=L(1, 1, 21), den=L(2, 40, 25), n_q=3, out=out, cnt=cnt):
        return lib.exo_column_quantiles_f64(x, S, N, stride, None if num is None else ctypes.addressof(num),
                                            None if den is None else ctypes.addressof(den), n_q, out, cnt, None)

    assert call(N=0) == OK and call(n_q=0) == OK                    # nothing to do
    assert call(N=0, x=None, out=None, cnt=None) == OK
    assert call(x=None) == INVALID and call(out=None) == INVALID and call(num=None) == INVALID and call(den=None) == INVALID
    assert call(S=-1) == INVALID and call(N=-1) == INVALID and call(n_q=-1) == INVALID
    assert call(stride=7) == INVALID
    assert call(n_q=17, num=L(*[1] * 17), den=L(*[2] * 17)) == INVALID
    assert call(den=L(2, 0, 25)) == INVALID and call(den=L(2, -40, 25)) == INVALID
    assert call(num=L(1, -1, 21)) == INVALID and call(num=L(1, 41, 21)) == INVALID
    assert call(den=L(2, 10 ** 9 + 1, 25)) == INVALID
    assert call(S=2 ** 31) == INVALID
    # (a bad fraction past n_q is not read)
    assert call(N=0, num=L(1, 1, 99), den=L(2, 40, 25), n_q=2) == OK


def test_ops_reject_what_the_kernel_cannot_take():
    from exoplanet_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.column_quantiles(torch.zeros(4, 3, dtype=torch.float64), [1], [2])
    with pytest.raises(ValueError):
        ops.column_quantiles(torch.zeros(4, dtype=torch.float64), [1], [2])


@pytest.mark.parametrize("S", SIZES)
def test_quantiles_on_cpu_tensors_take_the_torch_statement(S):
    from exoplanet_amd import predictive

    names, values = families(S, 200 + S)
    want, want_count = O.quantiles(values, PERCENTS)
    got, count = predictive.quantiles(torch.as_tensor(values), PERCENTS, return_count=True)
    assert got.shape == (len(PERCENTS), len(names)) and count.dtype == torch.int32
    for j, name in enumerate(names):
        assert O.same(got[:, j].numpy(), want[:, j]), (S, name)
    assert np.array_equal(count.numpy(), want_count)
    # strided rows, a taller buffer and a (n_draws, chains, N) array are the same columns
    tall = torch.full((S + 2, len(names) + 3), 7.0, dtype=torch.float64)
    tall[:S, :len(names)] = torch.as_tensor(values)
    assert O.same(predictive.quantiles(tall[:S, :len(names)], PERCENTS).numpy(), want)
    if S % 2 == 0:
        assert O.same(predictive.quantiles(torch.as_tensor(values).reshape(S // 2, 2, -1), PERCENTS).numpy(), want)
    assert O.same(predictive.quantiles(torch.as_tensor(values), 50).numpy(), want[2:3])


def test_quantiles_refuse_other_input():
    from exoplanet_amd import predictive

    with pytest.raises(TypeError):
        predictive.quantiles(torch.zeros(3, 2))
    with pytest.raises(ValueError):
        predictive.quantiles(torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        predictive.quantiles(torch.zeros(3, 4, dtype=torch.float64).T)
    with pytest.raises(ValueError):
        predictive.quantiles(torch.zeros(3, 4, dtype=torch.float64), (50, 101))


def _toy():
    rs = np.random.RandomState(8)
    grid = torch.linspace(-1.0, 1.0, 7, dtype=torch.float64)
    a, b = rs.randn(150, 2, 1), rs.randn(150, 2, 1)
    a[5, 1, 0] = np.nan                                               # a draw outside the model's support
    trace = {"a": torch.as_tensor(a), "b": torch.as_tensor(b), "log_prior": torch.zeros(150, 2, dtype=torch.float64)}
    curves = a.reshape(300, 1) + b.reshape(300, 1) * grid.numpy()[None, :]
    return grid, trace, curves


def test_bands_on_a_toy_model_with_a_dict_trace():
    from exoplanet_amd import predictive

    grid, trace, curves = _toy()
    sizes = []

    def model(a, b):
        sizes.append(tuple(a.shape))
        return a + b * grid

    res = predictive.bands(model, trace, percent=(16, 50, 84, 2.5), chunk=128, mean=True)
    assert sizes == [(128, 1), (128, 1), (44, 1)]                     # S = 300: a short last chunk
    want, want_count = O.quantiles(curves, (16, 50, 84, 2.5))
    assert res["n_draws"] == 300 and res["percent"] == (16, 50, 84, 2.5)
    assert O.same(res["quantiles"].numpy(), want) and np.array_equal(res["n_valid"].numpy(), want_count)
    assert int(res["n_valid"][0]) == 299
    assert O.same(res["mean"].numpy(), torch.nanmean(torch.as_tensor(curves), dim=0).numpy())
    # deterministic thinning: the rows (arange(n) * total) // n
    sizes.clear()
    thin = predictive.bands(model, trace, n_draws=70, chunk=32)
    assert sizes == [(32, 1), (32, 1), (6, 1)] and thin["n_draws"] == 70 and "mean" not in thin
    rows = (np.arange(70) * 300) // 70
    assert O.same(thin["quantiles"].numpy(), O.quantiles(curves[rows], (16, 50, 84))[0])
    one = predictive.bands(model, trace, n_draws=300, chunk=1000)
    assert O.same(one["quantiles"].numpy(), O.quantiles(curves, (16, 50, 84))[0])


def test_bands_argument_errors():
    from exoplanet_amd import predictive

    grid, trace, _ = _toy()
    with pytest.raises(ValueError, match="shape"):
        predictive.bands(lambda a, b: (a + b * grid)[:-1], trace, chunk=128)
    with pytest.raises(ValueError, match="shape"):
        predictive.bands(lambda a, b: (a + b * grid)[:, :, None], trace, chunk=128)
    with pytest.raises(ValueError, match="n_draws"):
        predictive.bands(lambda a, b: a + b * grid, trace, n_draws=301)
    with pytest.raises(TypeError):
        predictive.bands(lambda a, c: a + c * grid, trace)              # a name the trace does not hold
    with pytest.raises(ValueError, match="ParameterSpace"):
        predictive.bands(lambda a, b: a + b * grid, torch.zeros(10, 2, dtype=torch.float64))


def test_bands_with_a_space_on_the_host():
    """unconstrained rows and a Trace go through space.constrain in chunks: the same band as the whole batch at once"""
    from exoplanet_amd import distributions as D
    from exoplanet_amd import predictive
    from exoplanet_amd.sampling import Trace

    space = D.ParameterSpace(a=D.normal(0.0, 1.0), b=D.uniform(0.5, 2.0))
    rs = np.random.RandomState(4)
    z = torch.as_tensor(rs.randn(60, 2, space.n_free))
    grid = torch.linspace(0.0, 1.0, 5, dtype=torch.float64)
    model = lambda a, b: a + b * grid  # noqa: E731
    theta, _ = space.constrain(z.reshape(120, -1))
    want = predictive.quantiles(model(theta["a"], theta["b"]))
    got = predictive.bands(model, Trace(z, {}, None, None, 0, "nuts"), space, chunk=50)
    assert O.same(got["quantiles"].numpy(), want.numpy()) and got["n_draws"] == 120
    rows = predictive.bands(model, z.reshape(120, -1), space, chunk=120)
    assert O.same(rows["quantiles"].numpy(), want.numpy())
