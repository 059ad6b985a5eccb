"""CPU: the per-column arithmetic of exoplanet_amd/csrc/exo_psis_core.hpp compiled for the host (tests/psis_harness.cpp) and
the torch statement that runs for CPU tensors, against the long-double numpy statement of the definition
(tests/psis_oracle.py); the argument checks of the C entry point; `comparison.loo`, `waic` and `compare` on models whose
answer is known.  The kernel itself: tests/test_gpu_psis.py.

The yardstick is measured: per column and output, one unit is the error of the FLOAT64 numpy statement against long double
(relative to max(1, |value|) for elpd, lppd and p_waic, absolute for k, at least one eps), and the allowance is 16 units -- the
margin tests/astrometric_oracle.py set for a different libm and a different order of merged sums.  Worst ratios measured
(DESIGN.md 25.4): host core 2.5, torch statement 8.5."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psis_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64 = ctypes.c_int64

SIZES = (1, 2, 5, 20, 21, 25, 63, 64, 65, 225, 1000, 4000)      # 20 / 21: n <= 4; 225: the two branches of M meet
ALLOWANCE = 16.0
KEYS = {"elpd": "elpd", "k": "k", "lppd": "lppd", "p_waic": "var"}   # the oracle's name -> the library's


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "psis_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "psis_harness.cpp"), os.path.join(csrc, "exo_psis_core.hpp"),
            os.path.join(csrc, "exo_predictive_core.hpp"), os.path.join(csrc, "exo_detrend_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_column_psis.argtypes = [_dp, _i64, _i64, _i64, ctypes.c_int32, _dp, _dp, _dp, _dp, _ip]
    return lib


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def cases():
    """per S: the families' names, the (S, 10) array, M, and the statement in long double and in float64, computed once"""
    out = {}
    for S in SIZES:
        fam = O.column_families(S, np.random.RandomState(100 + S))
        values = np.ascontiguousarray(np.stack(list(fam.values()), axis=1))
        M = O.tail_length(S)
        out[S] = (list(fam), values, M, O.columns(values, M, np.longdouble), O.columns(values, M, np.float64))
    return out


def run_harness(harness, values, M, pad=0):
    """values (S, N) through the host build, its rows N + pad doubles apart"""
    S, N = values.shape
    buf = np.full((S, N + pad), 7.0)           # (what lies between the rows is a number that would show)
    buf[:, :N] = values
    out = {key: np.empty(N) for key in O.OUTPUTS}
    out["n_tail"] = np.empty(N, dtype=np.int32)
    assert harness.harness_column_psis(buf.ctypes.data_as(_dp), S, N, N + pad, M, *[out[k].ctypes.data_as(_dp) for k in O.OUTPUTS],
                                       out["n_tail"].ctypes.data_as(_ip)) == 0
    return out


def check(got, case, label):
    """every output of every family within the allowance; n_tail, the k = inf rule and the NaN columns exactly"""
    names, _, _, ld, f64 = case
    assert np.array_equal(np.asarray(got["n_tail"]), ld["n_tail"]), (label, got["n_tail"], ld["n_tail"])
    worst = {}
    for key in O.OUTPUTS:
        ratio = O.allowance(got[key], f64[key], ld[key], key)
        worst[key] = float(ratio.max())
    print(f"{label}: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})
    for key in O.OUTPUTS:
        ratio = O.allowance(got[key], f64[key], ld[key], key)
        assert ratio.max() <= ALLOWANCE, (label, key, names[int(ratio.argmax())], got[key], ld[key])
    return worst


@pytest.mark.parametrize("S", SIZES)
def test_families_are_regular(cases, S):
    """no family is left out of a comparison: it is one of the three bad ones, NaN everywhere, or nothing of it is NaN, only
    k = +inf is not finite, and the fit's divisions are defined"""
    names, values, M, ld, _ = cases[S]
    for j, name in enumerate(names):
        col = O.column(values[:, j], M, np.longdouble)
        if name in O.BAD:
            assert all(np.isnan(col[key]) for key in O.OUTPUTS) and col["n_tail"] == 0, (S, name)
            continue
        assert all(np.isfinite(col[key]) for key in ("elpd", "lppd", "p_waic")), (S, name)
        assert np.isfinite(col["k"]) or col["k"] == np.inf, (S, name)
        assert (col["k"] == np.inf) == (col["n_tail"] <= 4), (S, name)
        assert col["u_quartile"] is None or col["u_quartile"] != 0, (S, name)
        assert col["n_tail"] <= M
    k = dict(zip(names, ld["k"]))
    tails = dict(zip(names, ld["n_tail"]))
    assert tails["constant"] == 0 and ld["elpd"][names.index("constant")] == -1.25
    if S >= 21:
        assert tails["two values, ties across the cut-off"] < M
    if S >= 1000:
        assert k["normal model"] < 0.5 and k["Student-t outlier"] > 0.7


@pytest.mark.parametrize("S", SIZES)
def test_core_against_the_long_double_statement(harness, cases, S):
    _, values, M, _, _ = cases[S]
    for pad in (0, 3):
        check(run_harness(harness, values, max(M, 1), pad), cases[S], f"host core, S = {S}, pad = {pad}")


@pytest.mark.parametrize("S", SIZES)
def test_torch_statement_against_the_long_double_statement(cases, S):
    from exoplanet_amd import comparison

    names, values, M, _, _ = cases[S]
    assert comparison.tail_length(S) == M
    got = comparison._torch_statement(torch.as_tensor(values), M)
    assert got["n_tail"].dtype == torch.int32
    check({o: got[k].numpy() for o, k in KEYS.items()} | {"n_tail": got["n_tail"].numpy()}, cases[S], f"torch statement, S = {S}")
    # through loo: a strided view of a taller and wider buffer, and a (n_draws, chains, N) array, are the same columns
    tall = torch.full((S + 2, len(names) + 3), 7.0, dtype=torch.float64)
    tall[:S, :len(names)] = torch.as_tensor(values)
    res = comparison.loo(tall[:S, :len(names)])
    assert torch.equal(res["elpd_i"].view(torch.int64), got["elpd"].view(torch.int64))
    assert torch.equal(res["pareto_k"].view(torch.int64), got["k"].view(torch.int64)) and torch.equal(res["n_tail"], got["n_tail"])
    assert res["n_draws"] == S and res["n_data"] == len(names) and np.isnan(res["elpd_loo"])     # (the three bad columns)
    if S % 2 == 0:
        cube = comparison.waic(torch.as_tensor(values).reshape(S // 2, 2, -1))
        assert torch.equal(cube["lppd_i"].view(torch.int64), got["lppd"].view(torch.int64))
        assert torch.equal(cube["elpd_i"].view(torch.int64), (got["lppd"] - got["var"]).view(torch.int64))


def test_tail_length_and_reff():
    from exoplanet_amd import comparison

    assert [comparison.tail_length(S) for S in (1, 2, 5, 20, 21, 224, 225, 226, 4000)] == [1, 1, 1, 4, 5, 45, 45, 46, 190]
    assert comparison.tail_length(4000, reff=0.25) == 380 and comparison.tail_length(116000) == 1022
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            comparison.tail_length(100, bad)
    rs = np.random.RandomState(2)
    ll = -0.5 * (0.3 * rs.randn(400, 3) - 0.5) ** 2
    res = comparison.loo(torch.as_tensor(ll), reff=0.5)
    want = O.columns(ll, O.tail_length(400, 0.5), np.float64)
    assert np.array_equal(res["n_tail"].numpy(), want["n_tail"]) and int(res["n_tail"][0]) == O.tail_length(400, 0.5) == 80
    np.testing.assert_allclose(res["pareto_k"].numpy(), want["k"], rtol=0, atol=1e-11)
    with pytest.raises(ValueError, match="n_draws"):
        comparison.loo(torch.zeros(120000, 1, dtype=torch.float64))                     # a tail of more than 1024 values
    thin = comparison.loo(torch.as_tensor(ll), n_draws=100)
    rows = (np.arange(100) * 400) // 100
    np.testing.assert_allclose(thin["elpd_i"].numpy(), O.columns(ll[rows], O.tail_length(100), np.float64)["elpd"], rtol=1e-13)


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """the pointers are never followed: each of these calls returns before a launch"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib, ops

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    assert "#define EXO_PSIS_MAX_TAIL 1024" in text and ops.PSIS_MAX_TAIL == 1024
    OK, INVALID = 0, 1
    p = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000]

    def call(x=p[0], S=10, N=8, stride=8, M=2, outs=p[1:]):
        return lib.exo_column_psis_f64(x, S, N, stride, M, *outs, None)

    assert call(N=0) == OK and call(N=0, x=None, outs=[None] * 5) == OK                 # nothing to do
    assert call(M=0) == INVALID and call(M=-1) == INVALID and call(M=1025) == INVALID
    assert call(N=0, M=0) == INVALID and call(N=0, M=1025) == INVALID                   # (sizes are checked first)
    assert call(S=-1) == INVALID and call(N=-1) == INVALID and call(S=2 ** 31) == INVALID
    assert call(stride=7) == INVALID and call(x=None) == INVALID
    for j in range(5):
        assert call(outs=[None if i == j else q for i, q in enumerate(p[1:])]) == INVALID


def test_ops_reject_what_the_kernel_cannot_take():
    from exoplanet_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.column_psis(torch.zeros(4, 3, dtype=torch.float64), 1)
    with pytest.raises(ValueError):
        ops.column_psis(torch.zeros(4, dtype=torch.float64), 1)


def test_loo_and_waic_recover_the_exact_leave_one_out_density():
    """y_i ~ N(mu, 1), n = 50, a flat prior: mu | y ~ N(mean(y), 1 / n) exactly, and the leave-one-out predictive density of
    y_i is N(mean of the others, 1 + 1 / (n - 1)).  The lppd errs by about the number of parameters; both estimates must
    take at least three quarters of that error away."""
    from exoplanet_amd import comparison

    rs = np.random.RandomState(11)
    n, S = 50, 4000
    y = 0.4 + rs.randn(n)
    mu = y.mean() + rs.randn(S) / np.sqrt(n)
    ll = -0.5 * np.log(2 * np.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2
    others = (y.sum() - y) / (n - 1)
    v = 1.0 + 1.0 / (n - 1)
    exact = float(np.sum(-0.5 * np.log(2 * np.pi * v) - 0.5 * (y - others) ** 2 / v))
    res, wres = comparison.loo(torch.as_tensor(ll)), comparison.waic(torch.as_tensor(ll))
    lppd = float(res["lppd_i"].sum())
    print("exact", exact, "lppd", lppd, "elpd_loo", res["elpd_loo"], "elpd_waic", wres["elpd_waic"], "max k", float(res["pareto_k"].max()))
    assert abs(res["elpd_loo"] - exact) <= 0.25 * abs(lppd - exact)
    assert abs(wres["elpd_waic"] - exact) <= 0.25 * abs(lppd - exact)
    assert float(res["pareto_k"].max()) < 0.7 and res["n_high_k"] == 0
    assert abs(res["p_loo"] - (lppd - res["elpd_loo"])) < 1e-12 and abs(wres["p_waic"] - float(wres["p_waic_i"].sum())) < 1e-12
    assert res["se"] == pytest.approx(np.sqrt(n * np.var(res["elpd_i"].numpy())), rel=1e-12)
    assert set(res) == {"elpd_i", "pareto_k", "lppd_i", "p_waic_i", "n_tail", "elpd_loo", "se", "p_loo", "n_high_k", "n_draws", "n_data"}


def _line():
    rs = np.random.RandomState(5)
    n, S, sigma = 40, 1000, 0.5
    x = np.linspace(-1.0, 1.0, n)
    y = 0.3 + 2.0 * x + sigma * rs.randn(n)
    X = np.stack([np.ones(n), x], axis=1)
    cov = sigma ** 2 * np.linalg.inv(X.T @ X)
    ab = np.linalg.solve(X.T @ X, X.T @ y) + rs.randn(S, 2) @ np.linalg.cholesky(cov).T
    c = y.mean() + sigma / np.sqrt(n) * rs.randn(S)
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
    return T(x), T(y), sigma, T(ab), T(c)


def test_compare_prefers_the_slope_on_a_line_of_clear_slope():
    from exoplanet_amd import comparison

    x, y, sigma, ab, c = _line()
    slope = comparison.normal_log_likelihood(y, ab[:, :1] + ab[:, 1:] * x, sigma)
    const = comparison.normal_log_likelihood(y, c[:, None].expand(-1, y.numel()), sigma)
    assert slope.shape == (1000, 40)
    want = -0.5 * ((y - (ab[3, 0] + ab[3, 1] * x)) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi)
    assert torch.allclose(slope[3], want, rtol=1e-14, atol=0)
    for fn in (comparison.loo, comparison.waic):
        rows = comparison.compare({"constant": fn(const), "slope": fn(slope)})
        assert [r["name"] for r in rows] == ["slope", "constant"] and [r["rank"] for r in rows] == [0, 1]
        assert rows[0]["elpd_diff"] == 0.0 and rows[0]["dse"] == 0.0
        assert rows[1]["elpd_diff"] > 2.0 * rows[1]["dse"] > 0.0
        d = (fn(slope)["elpd_i"] - fn(const)["elpd_i"]).numpy()
        assert rows[1]["dse"] == pytest.approx(np.sqrt(d.size * np.var(d)), rel=1e-12)
        assert rows[1]["elpd_diff"] == pytest.approx(d.sum(), rel=1e-12)
    with pytest.raises(ValueError, match="different numbers"):
        comparison.compare({"a": comparison.loo(slope), "b": comparison.loo(slope[:, :39])})
    with pytest.raises(ValueError, match="one kind"):
        comparison.compare({"a": comparison.loo(slope), "b": comparison.waic(slope)})
    with pytest.raises(ValueError):
        comparison.compare({})


def test_loo_with_a_callable_over_a_trace():
    """the callable gets what `bands`' model gets, chunk by chunk, and the result is that of the array it forms"""
    from exoplanet_amd import comparison

    x, y, sigma, ab, _ = _line()
    trace = {"a": ab[:, :1].reshape(500, 2, 1), "b": ab[:, 1:].reshape(500, 2, 1), "log_prior": torch.zeros(500, 2, dtype=torch.float64)}
    sizes = []

    def log_likelihood(a, b):
        sizes.append(tuple(a.shape))
        return comparison.normal_log_likelihood(y, a + b * x, sigma)

    res = comparison.loo(log_likelihood, trace, chunk=384)
    assert sizes == [(384, 1), (384, 1), (232, 1)] and res["n_draws"] == 1000 and res["n_data"] == 40
    want = comparison.loo(comparison.normal_log_likelihood(y, ab[:, :1] + ab[:, 1:] * x, sigma))
    assert torch.equal(res["elpd_i"].view(torch.int64), want["elpd_i"].view(torch.int64)) and res["elpd_loo"] == want["elpd_loo"]
    assert res["p_loo"] > 0
    thin = comparison.waic(log_likelihood, trace, n_draws=250, chunk=1000)
    assert thin["n_draws"] == 250 and thin["elpd_waic"] == pytest.approx(want["elpd_loo"], abs=0.5)
    with pytest.raises(ValueError, match="trace"):
        comparison.loo(log_likelihood)
    with pytest.raises(ValueError, match="no trace"):
        comparison.loo(torch.zeros(10, 3, dtype=torch.float64), trace)
    with pytest.raises(TypeError):
        comparison.loo(torch.zeros(10, 3))
    with pytest.raises(ValueError, match="shape"):
        comparison.loo(lambda a, b: comparison.normal_log_likelihood(y, a + b * x, sigma)[:-1], trace)
