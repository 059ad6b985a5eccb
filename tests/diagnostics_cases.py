"""What the tests of exoplanet_amd.diagnostics share: the cases behind tests/golden/diagnostics_mp.npz (written by
tests/make_diagnostics_golden.py with mpmath at 40 digits), the host build of exoplanet_amd/csrc/exo_diagnostics_core.hpp
(tests/diagnostics_harness.cpp) and the error measure (tests/test_diagnostics_host.py, tests/test_diagnostics.py on the CPU,
tests/test_gpu_diagnostics.py on the device)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "diagnostics_mp.npz")
ULP = 2.220446049250313e-16
MARGIN = 1e-9                   # no comparison of a case hinges on less than this, relative (asserted by the generator)

# the columns of the harness / the library (include/exoplanet_amd.h: out of exo_diag_finish_f64)
COLUMNS = ("mean", "sd", "q05", "q50", "q95", "mcse_mean", "ess_bulk", "ess_tail", "ess_mean", "r_hat", "max_t_bulk", "max_t_low",
           "max_t_high", "max_t_mean", "r_hat_z", "r_hat_folded")
FLOATS = ("mean", "sd", "q05", "q50", "q95", "mcse_mean", "ess_bulk", "ess_tail", "ess_mean", "r_hat")
LOCATIONS = ("mean", "q05", "q50", "q95")
INTS = ("max_t_bulk", "max_t_low", "max_t_high", "max_t_mean")

ALL = ("iid", "ar9", "arm5", "cauchy", "ties", "stuck", "shifted", "offset", "const", "nan")
# name: (chains, draws, seed, kinds) -- several parameters per call, so that indexing is exercised
SHAPES = {
    "c1_n8": (1, 8, 11, ("iid", "ar9", "ties", "offset", "const", "nan")),
    "c3_n37": (3, 37, 12, ALL),                      # odd: the middle draw is dropped, L = 18
    "c4_n101": (4, 101, 13, ALL),
    "c33_n64": (33, 64, 14, ALL),                    # 66 half-chains: a full wave and a tail
    "c130_n64": (130, 64, 15, ("iid", "ar9", "stuck", "offset")),   # more than one block of half-chains
    "c64_n200": (64, 200, 16, ("iid", "ar9", "arm5")),              # ar9: truncation runs over several lag blocks
    "c2_n3": (2, 3, 17, ("iid", "const")),           # fewer than four draws: NaN
}


def _ar1(rng, N, C, phi, burn=200):
    e = rng.standard_normal((N + burn, C))
    y = np.zeros_like(e)
    for n in range(1, N + burn):
        y[n] = phi * y[n - 1] + e[n]
    return y[burn:] * np.sqrt(1.0 - phi * phi)


def series(kind, rng, N, C):
    """(N, C) draws of a kind; values are rounded to float32 (the fixture compresses; nothing else depends on it)"""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    if kind == "iid":
        return r32(rng.standard_normal((N, C)))
    if kind == "ar9":
        return r32(_ar1(rng, N, C, 0.9))
    if kind == "arm5":
        return r32(_ar1(rng, N, C, -0.5))
    if kind == "cauchy":
        return r32(rng.standard_cauchy((N, C)))
    if kind == "ties":                    # every third draw repeats the one before, as a rejected proposal does
        y = _ar1(rng, N, C, 0.5)
        y[2::3] = y[1::3][:y[2::3].shape[0]]
        return r32(y)
    if kind == "stuck":                   # one chain at a constant among moving ones
        y = rng.standard_normal((N, C))
        y[:, 0] = y[0, 0]
        return r32(y)
    if kind == "shifted":                 # one chain three standard deviations off
        y = rng.standard_normal((N, C))
        y[:, 0] += 3.0
        return r32(y)
    if kind == "offset":                  # mean 1e8 beside a unit spread
        return 1e8 + r32(rng.standard_normal((N, C)))
    if kind == "const":
        return np.full((N, C), 2.5)
    if kind == "nan":
        y = r32(rng.standard_normal((N, C)))
        y[N // 3, C // 2] = np.nan
        return y
    raise ValueError(kind)


def cases():
    """{name: x (N, C, P)}"""
    out = {}
    for name, (C, N, seed, kinds) in SHAPES.items():
        rng = np.random.default_rng(seed)
        out[name] = np.stack([series(k, rng, N, C) for k in kinds], axis=2)
    return out


# ---- the host build of the core ------------------------------------------------------------------------------------------------
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "diagnostics_harness.so")
    srcs = [os.path.join(ROOT, "tests", "diagnostics_harness.cpp"),
            os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_diagnostics_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_summary.restype = None
    lib.harness_summary.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    lib.harness_ndtri.restype = ctypes.c_double
    lib.harness_ndtri.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    return lib


def run_harness(lib, x, long_double):
    """x (N, C, P) -> {column: (P,)}"""
    N, C, P = x.shape
    xp = np.ascontiguousarray(x.transpose(2, 0, 1), dtype=np.float64)
    out = np.zeros((P, lib.harness_n_out()))
    lib.harness_summary(int(long_double), xp.ctypes.data, P, N, C, out.ctypes.data)
    return table(out)


def table(out):
    """(P, 16) array of the library's columns -> {column: (P,)}, the max_t as integers"""
    out = np.asarray(out)
    return {k: (out[:, i].astype(np.int64) if k in INTS else out[:, i].copy()) for i, k in enumerate(COLUMNS)}


def load():
    """the fixture as {case: (x, expected {column: (P,)})} and E_host"""
    z = np.load(GOLD)
    got = {}
    for name in SHAPES:
        got[name] = (z[name + "/x"], {k: z[f"{name}/{k}"] for k in FLOATS + INTS})
    return got, float(z["E_host"])


def errors(got, want):
    """{column: largest error}: locations (mean, quantiles) relative to max(|value|, sd) of their series, everything else
    relative to the value.  The pattern of values that are not finite and every max_t must match exactly (asserted)."""
    res = {}
    sd = np.asarray(want["sd"], dtype=np.float64)
    for k in FLOATS:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b)), (k, a, b)
        scale = np.abs(b)
        if k in LOCATIONS:
            scale = np.maximum(scale, np.where(np.isfinite(sd), sd, 0.0))
        err = np.abs(a - b)[fin] / np.where(scale[fin] > 0, scale[fin], 1.0)
        res[k] = float(err.max()) if err.size else 0.0
    for k in INTS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (k, got[k], want[k])
    return res
