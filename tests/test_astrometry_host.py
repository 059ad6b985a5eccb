"""CPU: the astrometric likelihood's arithmetic -- exoplanet_amd/csrc/exo_astrometry_core.hpp compiled for the host
(tests/astrometry_harness.cpp: a draw walked in the kernel's order of summation) -- against the multiprecision fixture
tests/golden/astrometry_mp.npz, and the host-side argument checks of exo_astrometry_loglike_vjp_f64.  Tolerances and the
condition on the inputs: tests/astrometry_cases.py.  The kernel itself: tests/test_gpu_astrometry.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import astrometry_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_i64 = ctypes.c_int64
_int = ctypes.c_int
_dbl = ctypes.c_double


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "astrometry_harness.so")
    csrc = os.path.join(ROOT, "exoplanet_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "astrometry_harness.cpp")] + [
        os.path.join(csrc, h) for h in ("exo_astrometry_core.hpp", "exo_draw_block.hpp", "exo_rv_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_block_threads.argtypes = [_i64]
    lib.harness_draw.restype = None
    lib.harness_draw.argtypes = [_dp, _dp, _dp, _dp, _dp, _i64, _dp, _i64, _i64, _dp, _dbl, _dbl, _int, _dp, _dp, _dp, _dp]
    return lib


@pytest.fixture(scope="module")
def g():
    return K.load()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(_dp)


def harness_outputs(lib, c, with_rec=True):
    D = c.params.shape[0]
    got = dict(loglike=np.empty(D), gparams=np.full((D, 10), np.nan), gjit2_rho=np.empty(D), gjit2_theta=np.empty(D))
    cn, sn = np.cos(c.theta), np.sin(c.theta)
    for d in range(D):
        lib.harness_draw(_p(c.t), _p(c.rho), _p(cn), _p(sn), _p(c.var_rho), c.var_rho.size, _p(c.var_theta), c.var_theta.size,
                         c.t.size, _p(c.params[d]), 0.0 if c.jit2_rho is None else c.jit2_rho[d],
                         0.0 if c.jit2_theta is None else c.jit2_theta[d], int(with_rec), _p(got["loglike"][d:d + 1]),
                         _p(got["gparams"][d]), _p(got["gjit2_rho"][d:d + 1]), _p(got["gjit2_theta"][d:d + 1]))
    if not with_rec:
        del got["gparams"]
    return got


def test_fixture_covers_the_kernel_paths(harness, g):
    """the shapes of the fixture against the constants of the code: one epoch, one epoch past the narrow limit, and on the
    wide workgroup lanes with one epoch and lanes with two; every combination of null jitters; both variance layouts"""
    assert harness.harness_narrow_cad() == K.NARROW_CAD and harness.harness_wide() == K.WIDE and harness.harness_slots() == 16
    n = {name: g[f"{name}_t"].size for name in K.SYSTEMS}
    assert n == K.N_EPOCH and n["a"] == 1 and n["b"] == 45 and n["c"] == K.NARROW_CAD + 1 and K.WIDE < n["d"] < 2 * K.WIDE
    widths = {name: harness.harness_block_threads(n[name]) for name in K.SYSTEMS}
    assert widths == dict(a=harness.harness_narrow(), b=harness.harness_narrow(), c=K.WIDE, d=K.WIDE), widths
    assert harness.harness_block_threads(K.NARROW_CAD) == harness.harness_narrow() == 64
    have = {name: ("%s_jit2_rho" % name in g.files, "%s_jit2_theta" % name in g.files) for name in K.SYSTEMS}
    assert have == dict(a=(False, True), b=(False, False), c=(True, True), d=(True, False)), have
    assert g["b_var_rho"].size == 45 and g["d_var_rho"].size == 1 and g["d_var_theta"].size == 1
    # c: angles stored in [0, 2 pi) and an orbit that crosses the branch cut -- the unwrapped difference is off by 2 pi
    c = K.case(g, "c")
    assert c.theta.min() >= 0.0 and c.theta.max() < 2 * np.pi and c.t.min() > 2.4e6
    out = K.P.orbit_vector(c.t, c.params[:, None, :])
    theta_m = np.arctan2(out[:, :, 0, 1], out[:, :, 0, 0])
    assert np.any(np.abs(theta_m - c.theta[None, :]) > np.pi)
    assert np.all(g["d_params"][:, 2:5] == [0.0, 1.0, 0.0]) and np.all(g["d_params"][:, 8:10] == [1.0, 0.0])
    assert os.path.getsize(os.path.join(K.GOLD, "astrometry_mp.npz")) < 200_000


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
    # without the record's cotangent the reverse arithmetic is skipped and the rest is the same, bit for bit
    short = harness_outputs(harness, c, with_rec=False)
    for k in short:
        assert np.array_equal(short[k], got[k]), k


def test_forgetting_the_wrap_fails_system_c(g):
    """the check has teeth: the restatement with the plain difference theta_m - theta_n misses system c's value"""
    c = K.case(g, "c")
    out = K.P.orbit_vector(c.t, c.params[:, None, :])
    X, Y = out[:, :, 0, 0], out[:, :, 0, 1]
    s2r, s2t = c.var_rho[None, :] + c.jit2_rho[:, None], c.var_theta[None, :] + c.jit2_theta[:, None]
    r, delta = c.rho[None, :] - np.sqrt(X * X + Y * Y), np.arctan2(Y, X) - c.theta[None, :]
    ll = -0.5 * (r * r / s2r + np.log(s2r) + delta * delta / s2t + np.log(s2t)).sum(1) - c.t.size * np.log(2 * np.pi)
    assert np.all(K.ratio(ll, c.want["loglike"], c.norm["loglike"]) > 1e3 * K.tol(0.0))


def test_bad_eccentricity_and_zero_separation_are_nan_in_their_draw_only(harness, g):
    c = K.case(g, "b")
    c.params = c.params.copy()
    c.params[1, 2] = 1.2
    got = harness_outputs(harness, c)
    for k, v in got.items():
        assert np.isnan(v[1]).all() and np.isfinite(v[[0, 2]]).all(), k
    c = K.case(g, "b")
    c.params = c.params.copy()
    c.params[2, 7] = 0.0                                  # amplitude 0: a separation of exactly 0 has no direction
    got = harness_outputs(harness, c)
    used = [k for k in range(10) if k != 6]               # (SINI moves Z alone: its slot is 0 times the cotangent of Z)
    assert np.isnan(got["loglike"][2]) and np.isnan(got["gparams"][2, used]).all()
    assert np.isfinite(got["loglike"][:2]).all() and np.isfinite(got["gparams"][:2]).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from exoplanet_amd import _lib

    return _lib.load()


def test_entry_point_checks_its_arguments_on_the_host(lib):
    INVALID = 1
    names = ("t rho cos_theta sin_theta var_rho n_var_rho var_theta n_var_theta n_cad params n_draw jit2_rho jit2_theta loglike "
             "gparams gjit2_rho gjit2_theta stream").split()
    # (8 is no address of anything: a pointer that were followed would fault)
    ok = [8, 8, 8, 8, 8, 100, 8, 1, 100, 8, 4, 8, 8, 8, 8, 8, 8, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.exo_astrometry_loglike_vjp_f64(*a)

    for bad in (dict(params=None), dict(loglike=None), dict(t=None), dict(rho=None), dict(cos_theta=None), dict(sin_theta=None),
                dict(var_rho=None), dict(var_theta=None), dict(n_var_rho=7), dict(n_var_rho=0), dict(n_var_theta=99),
                dict(n_var_theta=0), dict(n_var_theta=-1), dict(n_cad=-1, n_var_rho=1), dict(n_draw=-1), dict(n_draw=2 ** 31)):
        assert call(**bad) == INVALID, bad
    assert call(n_draw=0) == 0
    assert call(n_draw=0, t=None, rho=None, cos_theta=None, sin_theta=None, var_rho=None, var_theta=None, params=None,
                loglike=None) == 0
    assert call(n_draw=0, n_var_rho=7) == INVALID and call(n_draw=0, n_cad=-1, n_var_rho=1) == INVALID      # sizes are checked first


def test_abi_line_and_bindings_agree():
    from exoplanet_amd import _lib

    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    version = int(re.search(r"#define\s+EXO_ABI_VERSION\s+(\d+)", text).group(1))
    assert version == _lib.ABI_VERSION == 21
    assert re.search(r"^ \* 21: .*exo_astrometry_loglike_vjp_f64", text, re.M)
    assert len(_lib._SIGNATURES["exo_astrometry_loglike_vjp_f64"][1]) == 18
