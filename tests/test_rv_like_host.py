"""CPU: the radial-velocity likelihood's arithmetic -- exoplanet_amd/csrc/exo_rv_like_core.hpp compiled for the host
(tests/rv_like_harness.cpp: a draw walked in the kernel's order of summation) -- against the multiprecision fixture
tests/golden/rv_like_mp.npz, and the host-side argument checks of exo_rv_loglike_vjp_f64.  Tolerances and the condition on
the inputs: tests/rv_like_cases.py (derived there).  The kernel itself: tests/test_gpu_rv_like.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rv_like_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64 = ctypes.c_int64
_int = ctypes.c_int


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "rv_like_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "rv_like_harness.cpp")] + [
        os.path.join(csrc, h) for h in ("exo_rv_like_core.hpp", "exo_draw_block.hpp", "exo_rv_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_block_threads.argtypes = [_i64]
    lib.harness_draw.restype = None
    lib.harness_draw.argtypes = [_dp, _dp, _ip, _dp, _dp, _i64, _i64, _dp, _int, _dp, _int, _dp, _dp, _int, _dp, _dp, _dp, _dp, _dp]
    return lib


@pytest.fixture(scope="module")
def g():
    return K.load()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_dp)


def harness_outputs(lib, c):
    D, Pn, T, I = c.params.shape[0], c.params.shape[1], c.trend.shape[1], c.n_inst
    got = dict(loglike=np.empty(D), gparams=np.empty((D, Pn, 6)), gtrend=np.empty((D, T)), goffset=np.empty((D, I)),
               gjit2=np.empty((D, I)))
    inst = np.ascontiguousarray(c.inst, dtype=np.int32)
    for d in range(D):
        lib.harness_draw(_p(c.t), _p(c.tau), inst.ctypes.data_as(_ip), _p(c.rv), _p(c.var), c.t.size, c.var.size,
                         _p(c.params[d]), Pn, _p(c.trend[d]) if T else None, T, None if c.offset is None else _p(c.offset[d]),
                         None if c.jit2 is None else _p(c.jit2[d]), I, _p(got["loglike"][d:d + 1]), _p(got["gparams"][d]),
                         _p(got["gtrend"][d]) if T else None, _p(got["goffset"][d]), _p(got["gjit2"][d]))
    return got


def test_fixture_covers_the_kernel_paths(harness, g):
    """the shapes of the fixture against the constants of the code: one epoch past the tile, both widths of the workgroup,
    both maxima"""
    assert harness.harness_tile() == K.TILE and g["e_t"].size == K.TILE + 1
    assert harness.harness_max_trend() == K.MAX_TREND == g["d_trend"].shape[1]
    assert harness.harness_max_inst() == K.MAX_INST == g["f_offset"].shape[1]
    widths = {name: harness.harness_block_threads(g[f"{name}_t"].size) for name in K.SYSTEMS}
    assert set(widths.values()) == {64, 256}, widths
    assert g["f_params"].shape[1] == 16
    assert not np.any(g["c_inst"] == 2) and g["c_offset"].shape[1] == 3
    assert os.path.getsize(os.path.join(K.GOLD, "rv_like_mp.npz")) < 200_000


@pytest.mark.parametrize("name", K.SYSTEMS)
def test_restatement_meets_the_condition_on_the_inputs(name, g):
    unit = K.oracle_unit(g, name)
    print(f"system {name}: unit = {unit:.3g}")
    assert unit <= K.UNIT_CEILING


@pytest.mark.parametrize("name", K.SYSTEMS)
def test_device_arithmetic_on_host_matches_the_fixture(name, harness, g):
    c = K.case(g, name)
    got = harness_outputs(harness, c)
    K.check("device_math_on_host", c, got)
    if name == "c":      # the instrument without epochs
        assert np.all(got["goffset"][:, 2] == 0.0) and np.all(got["gjit2"][:, 2] == 0.0)


def test_bad_eccentricity_and_bad_instrument_are_nan(harness, g):
    c = K.case(g, "b")
    c.params = c.params.copy()
    c.params[1, 0, 2] = 1.2
    got = harness_outputs(harness, c)
    assert np.isnan(got["loglike"][1]) and np.isfinite(got["loglike"][[0, 2]]).all()
    c = K.case(g, "c")
    c.inst = c.inst.copy()
    c.inst[5] = 3                                        # outside [0, n_inst): never read, NaN
    assert np.isnan(harness_outputs(harness, c)["loglike"]).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from exoplanet_amd import _lib

    return _lib.load()


def test_entry_point_checks_its_arguments_on_the_host(lib):
    INVALID = 1
    names = ("t tau inst rv var n_cad n_var params n_draw n_planet trend n_trend offset jit2 n_inst loglike gparams gtrend "
             "goffset gjit2 stream").split()
    ok = [8, 8, 8, 8, 8, 100, 100, 8, 4, 2, 8, 2, 8, 8, 3, 8, 8, 8, 8, 8, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.exo_rv_loglike_vjp_f64(*a)

    for bad in (dict(params=None), dict(loglike=None), dict(t=None), dict(rv=None), dict(var=None), dict(trend=None),
                dict(tau=None), dict(n_trend=5), dict(n_trend=-1), dict(n_inst=0), dict(n_inst=9), dict(inst=None),
                dict(n_var=7), dict(n_var=0), dict(n_cad=-1, n_var=1), dict(n_draw=-1), dict(n_planet=0), dict(n_planet=17)):
        assert call(**bad) == INVALID, bad
    assert call(n_draw=0) == 0
    assert call(n_draw=0, t=None, tau=None, inst=None, rv=None, var=None, params=None, trend=None, loglike=None) == 0
    assert call(n_draw=0, n_inst=9) == INVALID and call(n_draw=0, n_var=7) == INVALID      # sizes are checked first


def test_new_constants_match_the_python_side():
    from exoplanet_amd import ops

    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert int(consts["EXO_RV_MAX_TREND"]) == ops.RV_MAX_TREND == K.MAX_TREND
    assert int(consts["EXO_RV_MAX_INST"]) == ops.RV_MAX_INST == K.MAX_INST
