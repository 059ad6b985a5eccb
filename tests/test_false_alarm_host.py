"""CPU: what the false-alarm probabilities of exoplanet_amd.estimators hold without a device -- the
resampling tables, the two formulas, chi2_0, the argument errors, the host side of exo_keplerian_max_f64, and the group walk
and three-key arg-max of exoplanet_amd/csrc/exo_keplerian_max.hpp compiled for the host (tests/keplerian_max_harness.cpp)
against the single-series walk of tests/keplerian_harness.cpp, bit for bit.  The kernel itself: tests/test_gpu_false_alarm.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keplerian_oracle as O  # noqa: E402
from test_keplerian_host import columns, run, statements  # noqa: E402
from test_keplerian_host import harness as single_harness  # noqa: E402,F401  (the fixture of the single-series walk)

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i32, _f64 = ctypes.c_int32, ctypes.c_double
WIDTHS = (4, 8, 16)         # the group widths keplerian_max_harness.cpp instantiates


def E():
    from exoplanet_amd import estimators

    return estimators


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "keplerian_max_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "keplerian_max_harness.cpp")] + [
        os.path.join(csrc, h) for h in ("exo_keplerian_max.hpp", "exo_keplerian_core.hpp", "exo_orbit_search.hpp",
                                        "exo_estimators_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_group_table.argtypes = [ctypes.c_int, _dp, _dp, _dp, _i32, ctypes.c_int, _ip, ctypes.c_int, _f64, _dp, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, _dp]
    lib.harness_best3.argtypes = [_dp, _ip, _ip, ctypes.c_int, _dp, _ip]
    return lib


# ---- the resampling tables ------------------------------------------------------------------------------------------------------

INST = np.array([0, 1, 0, 0, 2, 1, 0, 1, 0, 0, 1, 0])        # (instrument 2 owns one epoch)


@pytest.mark.parametrize("replace", [False, True])
def test_resample_indices(replace):
    idx = E().resample_indices(INST.size, 50, instrument=INST, replace=replace, seed=4)
    assert idx.shape == (50, INST.size) and idx.dtype == np.int64
    assert np.array_equal(INST[idx], np.broadcast_to(INST, idx.shape))                # every row stays within the instruments
    for k in range(3):
        own = np.flatnonzero(INST == k)
        drawn = idx[:, own]
        assert np.isin(drawn, own).all()
        if not replace:
            assert np.array_equal(np.sort(drawn, axis=1), np.broadcast_to(own, drawn.shape))      # a permutation of its epochs
    repeats = any(np.unique(row).size < row.size for row in idx)
    assert repeats == replace
    assert not np.array_equal(idx[0], idx[1])
    assert np.array_equal(idx, E().resample_indices(INST.size, 50, instrument=INST, replace=replace, seed=4))
    assert not np.array_equal(idx, E().resample_indices(INST.size, 50, instrument=INST, replace=replace, seed=5))
    one = E().resample_indices(7, 3, replace=replace)                                 # (no instrument: one)
    assert one.shape == (3, 7) and one.min() >= 0 and one.max() < 7
    with pytest.raises(ValueError, match="positive"):
        E().resample_indices(7, 0)


# ---- the two formulas -----------------------------------------------------------------------------------------------------------

def test_false_alarm_probability_on_hand_made_arrays():
    null = np.array([0.2, 0.5, 0.5, np.nan, 0.9])
    fap = E().false_alarm_probability(null, np.array([0.5, 0.95, 0.1, 0.9, np.nan]))
    # ties count (>=); the NaN of the null never counts but stays in R; a NaN peak has no probability
    assert np.array_equal(fap[:4], np.array([4, 1, 5, 2]) / 6) and np.isnan(fap[4])
    assert E().false_alarm_probability(null, 0.5) == 4 / 6
    got = E().false_alarm_probability(torch.as_tensor(null), torch.tensor([[0.5, 0.95], [0.1, 0.9]], dtype=torch.float64))
    assert isinstance(got, torch.Tensor) and torch.equal(got, torch.tensor([[4, 1], [5, 2]], dtype=torch.float64) / 6)


def test_false_alarm_level_on_hand_made_arrays():
    rs = np.random.RandomState(2)
    for R, kth in ((99, 1), (199, 2)):
        null = rs.permutation(np.arange(1.0, R + 1))
        level = E().false_alarm_level(null, 0.01)
        assert level == np.sort(null)[-kth]                                            # the largest; the second largest
        assert E().false_alarm_level(torch.as_tensor(null), 0.01) == level
    null = rs.permutation(np.arange(1.0, 100.0))
    assert E().false_alarm_probability(null, 99.5) == 0.01                            # a peak above the level: exactly 0.01
    assert E().false_alarm_probability(null, 99.0) == 0.02                            # the level itself is not above it
    assert np.isnan(E().false_alarm_level(np.arange(50.0), 0.01))                     # 50 resamplings resolve no 1 % level
    assert E().false_alarm_level(np.arange(50.0), 0.1) == 45.0                         # k = floor(5.1) = 5
    assert E().false_alarm_level(np.arange(99.0), 0.29) == 70.0                        # k = 29, though 0.29 * 100 < 29 in binary
    with_nan = np.array([np.nan, 3.0, 1.0, np.nan, 2.0, 0.5, 0.4, 0.3, 0.2])
    assert E().false_alarm_level(with_nan, 0.2) == 2.0 and np.isnan(E().false_alarm_level(with_nan, 0.85))     # (NaN ranks last)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="level"):
            E().false_alarm_level(null, bad)


# ---- chi2_0 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yerr", [True, False])
@pytest.mark.parametrize("inst", [True, False])
def test_series_chi2_0_against_the_statement(inst, yerr):
    d, _, f64, ld = statements(inst=inst, yerr=yerr)
    got = E().series_chi2_0(torch.as_tensor(d["y"]), torch.as_tensor(d["err"]) if yerr else None, d["inst"] if inst else None)
    assert got.shape == () and got.dtype == torch.float64
    for want in (float(f64["chi2_0"]), float(ld["chi2_0"])):
        assert abs(float(got) - want) <= 1e-13 * want
    rows = E().series_chi2_0(np.stack([d["y"], 2 * d["y"]]), d["err"] if yerr else None, d["inst"] if inst else None)
    assert rows.shape == (2,) and rows[0] == got and abs(float(rows[1]) - 4 * float(got)) <= 1e-13 * 4 * float(got)
    if not yerr:
        assert abs(float(E().series_chi2_0(d["y"], 2.0, d["inst"] if inst else None)) - float(got) / 4) <= 1e-13 * float(got)


# ---- the argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors():
    t = torch.linspace(0, 10, 12, dtype=torch.float64)
    y = torch.sin(t)
    kw = dict(frequencies=[0.1, 0.2])
    ok = E().resample_indices(12, 4, instrument=INST)
    for bad, match in ((ok[:, :-1], "shape"), (ok[0], "shape"), (ok[:0], "shape"), (ok.astype(np.int32), "int64"),
                       (ok.astype(np.float64), "int64"), (ok + 1, "outside"), (ok - 1, "outside")):
        with pytest.raises(ValueError, match=match):
            E().false_alarm(t, y, resamples=bad, instrument=INST, **kw)
    cross = ok.copy()
    cross[2, 0], cross[2, 1] = 1, 0                                                   # (epochs 0 and 1: instruments 0 and 1)
    with pytest.raises(ValueError, match="another instrument"):
        E().false_alarm(t, y, resamples=cross, instrument=INST, **kw)
    with pytest.raises(ValueError, match="another instrument"):
        E().false_alarm(t, y, resamples=torch.as_tensor(E().resample_indices(12, 4)), instrument=INST, **kw)
    with pytest.raises(ValueError, match="method"):
        E().false_alarm(t, y, method="box", **kw)
    with pytest.raises(ValueError, match="instrument must be None"):
        E().false_alarm(t, y, method="lomb_scargle", instrument=INST, **kw)
    with pytest.raises(ValueError, match="one series"):
        E().false_alarm(t, torch.stack([y, y]), **kw)
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError, match="n_resample"):
            E().false_alarm(t, y, n_resample=bad, **kw)
    for bad in ((0.1, 0.0), (1.0,), (-0.01,)):
        with pytest.raises(ValueError, match="level"):
            E().false_alarm(t, y, levels=bad, **kw)
    for bad in (0, 2.5, 70000):
        with pytest.raises(ValueError, match="chunk"):
            E().false_alarm(t, y, chunk=bad, **kw)
    with pytest.raises(ValueError, match="gaps"):
        E().false_alarm(t, y, instrument=2 * INST, **kw)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="frequencies_per_block"):
            E().keplerian_max_power(t, y, frequencies_per_block=bad, **kw)
    with pytest.raises(ValueError, match="ecc"):
        E().keplerian_max_power(t, y, ecc=[1.0], **kw)
    # what is well formed gets as far as the device: there is no CPU fallback
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no CPU fallback"):
            E().false_alarm(t, y, resamples=ok, instrument=INST, **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            E().keplerian_max_power(t, y, **kw)
    assert E().KEPLERIAN_MAX_GROUP in WIDTHS


# ---- the entry point ------------------------------------------------------------------------------------------------------------

def test_abi_of_the_entry_point():
    """argument checks on the host, before any launch; the workspace is sized by pure arithmetic"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    lib = _lib.load()
    assert lib.exo_abi_version() == 21 == _lib.ABI_VERSION
    INVALID, WORKSPACE = 1, 3
    G = E().KEPLERIAN_MAX_GROUP
    columns_of = lambda n, B: 8 * (n + 2 * B * n + 16 * B)            # noqa: E731  (exo_keplerian_workspace_bytes)

    def blocks(B, F, per_block):
        if per_block == 0:                                           # 64 workgroups for each of 256 compute units
            groups = -(-B // G)
            per_block = max(1, F // -(-16384 // groups))
        return -(-F // per_block)

    size = lib.exo_keplerian_max_workspace_bytes
    for n, B, F, per_block in ((100, 1, 5, 0), (100, 1, 50000, 0), (100, 5, 197, 7), (40, 200, 100000, 0), (40, 9000, 300, 0),
                               (40, 3, 11, 11), (40, 3, 11, 12), (40, 3, 0, 0)):
        assert size(n, B, F, per_block) == columns_of(n, B) + 16 * B * blocks(B, F, per_block), (n, B, F, per_block)
    assert size(100, 1, 50000, 0) == columns_of(100, 1) + 16 * 16667                  # (blocks of three frequencies)
    assert size(0, 1, 5, 0) == -1 and size(100, 0, 5, 0) == -1 and size(100, 65536, 5, 0) == -1
    assert size(100, 1, -1, 0) == -1 and size(100, 1, 5, -1) == -1
    off = (ctypes.c_int32 * 3)(0, 40, 100)
    ecc = (ctypes.c_double * 3)(0.0, 0.5, 0.9)
    names = ["t", "y", "yerr", "n_yerr", "n", "n_series", "off", "n_inst", "freq", "n_freq", "ecc", "n_ecc", "n_phase", "per_block",
             "power", "index", "cand", "ws", "ws_bytes", "stream"]
    ok = [8, 8, None, 0, 100, 1, ctypes.addressof(off), 2, 8, 5, ctypes.addressof(ecc), 3, 16, 0, 8, 8, 8, 8, 1 << 20, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.exo_keplerian_max_f64(*args)

    one = (ctypes.c_double * 3)(0.0, 1.0, 0.5)
    nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.5)
    gap = (ctypes.c_int32 * 3)(0, 0, 100)
    short = (ctypes.c_int32 * 3)(0, 40, 99)
    late = (ctypes.c_int32 * 3)(1, 40, 100)
    for bad in (dict(t=None), dict(y=None), dict(n=0), dict(n_series=0), dict(n_series=65536), dict(n_yerr=1), dict(n_yerr=3, yerr=8),
                dict(off=None), dict(n_inst=0), dict(n_inst=9), dict(freq=None), dict(n_freq=-1), dict(ecc=None), dict(n_ecc=0),
                dict(n_ecc=65), dict(n_phase=0), dict(n_phase=4097), dict(per_block=-1), dict(power=None), dict(index=None),
                dict(cand=None), dict(ws=None), dict(ecc=ctypes.addressof(one)), dict(ecc=ctypes.addressof(nan)),
                dict(off=ctypes.addressof(gap)), dict(off=ctypes.addressof(short)), dict(off=ctypes.addressof(late))):
        assert call(**bad) == INVALID, bad
    assert call(ws_bytes=size(100, 1, 5, 0) - 1) == WORKSPACE
    assert call(per_block=1, ws_bytes=size(100, 1, 5, 1) - 1) == WORKSPACE


# ---- the group walk and the arg-max, on the host --------------------------------------------------------------------------------

def batch(n_series):
    """the main input and its rows perturbed as tests/test_gpu_keplerian.py perturbs them, then further ones alike"""
    d = O.main_input()
    rs = np.random.RandomState(3)
    n = d["t"].size
    ys = np.concatenate([d["y"][None], d["y"][None, :] + rs.randn(n_series, n)])[:n_series]
    errs = np.concatenate([d["err"][None], d["err"][None, :] * rs.uniform(0.8, 1.25, (n_series, n))])[:n_series]
    return d, ys, errs


@pytest.mark.parametrize("G", WIDTHS)
def test_the_group_walk_is_the_single_walk_bit_for_bit(harness, single_harness, G):  # noqa: F811
    d, ys, errs = batch(G + 1)
    f = d["f"][::40]
    C = d["ecc"].size * d["n_phase"]
    single = np.stack([run(single_harness, d["t"], ys[b], errs[b], d["inst"], f, d["ecc"], d["n_phase"])["table"] for b in range(G + 1)])
    assert np.isfinite(single).sum() == (G + 1) * f.size * 289
    for n_series in (1, 2, G + 1):
        cols = [columns(d["t"], ys[b], errs[b], d["inst"]) for b in range(n_series)]
        tt, off = cols[0][0], cols[0][3]
        w, wy = np.ascontiguousarray([c[1] for c in cols]), np.ascontiguousarray([c[2] for c in cols])
        for tile in (harness.harness_tile(), 7):              # (7: segments that end at a tile's last epoch and inside one)
            table = np.full((f.size, n_series, C), np.nan)
            for i, fi in enumerate(f):
                assert harness.harness_group_table(G, _p(tt), _p(w), _p(wy), tt.size, n_series, _p(off, _ip), off.size - 1, fi,
                                                   _p(d["ecc"]), d["ecc"].size, d["n_phase"], tile, _p(table[i])) == 0
            assert np.array_equal(table.transpose(1, 0, 2), single[:n_series]), (n_series, tile)
    assert harness.harness_group_table(5, *[None] * 3, 0, 0, None, 0, 0.0, None, 0, 0, 1, None) == -1


def test_the_three_key_argmax(harness):
    def best(power, frequency, candidate):
        power = np.ascontiguousarray(power, dtype=np.float64)
        frequency, candidate = (np.ascontiguousarray(a, dtype=np.int32) for a in (frequency, candidate))
        top, where = np.empty(1), np.empty(2, dtype=np.int32)
        harness.harness_best3(_p(power), _p(frequency, _ip), _p(candidate, _ip), power.size, _p(top), _p(where, _ip))
        return float(top[0]), int(where[0]), int(where[1])

    assert best([1.0, 3.0, 2.0], [0, 1, 2], [5, 6, 7]) == (3.0, 1, 6)                  # the larger power
    assert best([3.0, 3.0, 3.0], [4, 2, 9], [0, 8, 1]) == (3.0, 2, 8)                  # of equals the lower frequency ...
    assert best([3.0, 3.0, 3.0], [9, 4, 2], [0, 8, 1]) == (3.0, 2, 1)                  # ... in whatever order they come
    assert best([3.0, 3.0, 3.0], [2, 2, 2], [7, 3, 5]) == (3.0, 2, 3)                  # then the lower candidate
    assert best([np.nan, 1.0, np.nan], [0, 5, 1], [0, 8, 1]) == (1.0, 5, 8)            # NaN never wins
    assert best([np.nan, np.nan], [0, 1], [0, 1]) == (-np.inf, -1, -1)
    assert best([-np.inf, -np.inf], [3, 2], [3, 2]) == (-np.inf, -1, -1)               # nothing finite: none
    assert best([-np.inf, -1e300], [0, 1], [0, 1]) == (-1e300, 1, 1)
    assert best([], [], []) == (-np.inf, -1, -1)
