"""CPU: what the Keplerian periodogram and the astrometric orbit search share, exoplanet_amd/csrc/exo_orbit_search.hpp compiled
for the host (tests/orbit_search_harness.cpp): the lanes per workgroup, the candidate grid, the check of the eccentricity grid
and of the sizes, and the arg-max over lanes.  Every expected value is derived here from the rule, not from the header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i32, _i64 = ctypes.c_int32, ctypes.c_int64


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "orbit_search_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "orbit_search_harness.cpp"), os.path.join(ROOT, "tests", "orbit_lanes.hpp")] + [
        os.path.join(csrc, h) for h in ("exo_orbit_search.hpp", "exo_estimators_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_threads_for.argtypes = [_i64]
    lib.harness_candidate_of.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp]
    lib.harness_ecc_grid.argtypes = [_dp, ctypes.c_int, _dp]
    lib.harness_sizes_ok.argtypes = [_i64, _i64, _i64, _i32, _i32]
    lib.harness_lanes_best.restype = _i32
    lib.harness_lanes_best.argtypes = [_dp, _ip, ctypes.c_int, ctypes.c_int]
    return lib


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def fewest_idle_lanes(n_cand):
    """of 64, 128 and 256 lanes the count whose passes over the candidates leave the fewest lanes idle, the larger of equals"""
    idle = {nt: -(-n_cand // nt) * nt - n_cand for nt in (64, 128, 256)}
    return max(nt for nt in idle if idle[nt] == min(idle.values()))


@pytest.mark.parametrize("n_cand, want", [(1, 64), (64, 64), (65, 128), (192, 64), (256, 256), (640, 128), (64 * 4096, 256)])
def test_lanes_per_workgroup(harness, n_cand, want):
    assert fewest_idle_lanes(n_cand) == want                                   # (the table is the rule's)
    assert harness.harness_threads_for(n_cand) == want


def test_lanes_per_workgroup_is_the_rule_everywhere(harness):
    for n_cand in list(range(1, 1300)) + [4095, 4096, 4097, 64 * 4096 - 1]:
        assert harness.harness_threads_for(n_cand) == fewest_idle_lanes(n_cand), n_cand


def test_the_candidate_grid(harness):
    ecc = np.array([0.0, 0.3, 0.0, 0.999, 0.45])
    n_phase = 13
    n_cand = ecc.size * n_phase
    out = np.empty(4)
    live = []
    for c in range(n_cand + 70):                                               # (past the grid: the idle lanes of a last pass)
        is_live = bool(harness.harness_candidate_of(c, n_cand, n_phase, _p(ecc), _p(out)))
        live.append(is_live)
        if c >= n_cand:
            assert not is_live, c
            continue
        j, k = divmod(c, n_phase)                                              # phase fastest
        assert is_live == (ecc[j] != 0.0 or k == 0), c                         # e == 0: every phase is the same model
        if is_live:
            assert out[0] == ecc[j] and out[1] == np.sqrt(1.0 - ecc[j]) and out[2] == np.sqrt(1.0 + ecc[j]), c
            assert out[3] == k / n_phase, c
    assert sum(live) == 2 + 3 * n_phase


def test_the_check_of_the_eccentricity_grid(harness):
    copy = np.empty(4)

    def accepted(*e):
        return bool(harness.harness_ecc_grid(_p(np.array(e, dtype=np.float64)), len(e), _p(copy)))

    for bad in (-0.1, 1.0, np.nan, np.inf, 1.5):
        assert not accepted(bad) and not accepted(0.0, 0.5, bad) and not accepted(bad, 0.5), bad
    assert accepted(0.0) and accepted(0.999) and accepted(0.0, 0.999, np.nextafter(1.0, 0.0), 0.5)
    assert np.array_equal(copy, [0.0, 0.999, np.nextafter(1.0, 0.0), 0.5])     # the copy that travels to the kernel


def test_the_check_of_the_sizes(harness):
    ok = dict(n=100, n_series=1, n_frequency=5, n_ecc=3, n_phase=16)
    call = lambda **kw: bool(harness.harness_sizes_ok(*{**ok, **kw}.values()))  # noqa: E731
    assert call() and call(n_frequency=0) and call(n=2 ** 31 - 1, n_series=65535, n_frequency=2 ** 31 - 1, n_ecc=64, n_phase=4096)
    for bad in (dict(n=0), dict(n=2 ** 31), dict(n_series=0), dict(n_series=65536), dict(n_frequency=-1), dict(n_frequency=2 ** 31),
                dict(n_ecc=0), dict(n_ecc=65), dict(n_phase=0), dict(n_phase=4097)):
        assert not call(**bad), bad


@pytest.mark.parametrize("n_lane", [1, 7, 64, 128, 256])
def test_the_argmax_does_not_depend_on_the_lanes(harness, n_lane):
    """a table with planted equal maxima, NaN and entries that are no candidates: the winner is the lowest number among the
    largest powers of those that count, whatever the number of lanes -- the widths the kernels run (64, 128, 256) included"""
    rs = np.random.RandomState(29)
    n_cand = 577
    power = rs.uniform(0.0, 1.0, n_cand)
    counts = (rs.uniform(size=n_cand) < 0.8).astype(np.int32)
    power[rs.choice(n_cand, 20, replace=False)] = np.nan
    planted = np.array([5, 130, 131, 320, 449, 576])                           # (different lanes at every width, two neighbours)
    power[planted] = 2.0
    counts[planted] = 1
    counts[5] = 0                                                              # the first of them is no candidate
    power[7] = 3.0                                                             # nor is the largest power of all
    counts[7] = 0
    ok = (counts != 0) & ~np.isnan(power)
    want = int(np.flatnonzero(ok & (power == power[ok].max()))[0])
    assert want == 130
    assert harness.harness_lanes_best(_p(power), _p(counts, _ip), n_cand, n_lane) == want
    # nothing counts, or nothing but NaN: no winner
    none = np.iinfo(np.int32).max
    assert harness.harness_lanes_best(_p(power), _p(np.zeros(n_cand, np.int32), _ip), n_cand, n_lane) == none
    assert harness.harness_lanes_best(_p(np.full(n_cand, np.nan)), _p(counts, _ip), n_cand, n_lane) == none
