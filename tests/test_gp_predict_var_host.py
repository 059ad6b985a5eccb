"""CPU: the predictive variance of exo_celerite_predict.hpp -- the factorisation as a Kalman filter followed by its smoother --
compiled for the host (tests/gp_predict_var_harness.cpp) and run draw by draw, against the dense definition
k2(0) - diag(K2(t*, t) (K + diag)^-1 K2(t, t*)).  On the GPU the same lane function runs one lane per draw
(tests/test_gpu_gp_predict_var.py checks that build through GaussianProcess.predict)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import numpy_port as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "gp_predict_var_harness.so")
    srcs = [os.path.join(ROOT, "tests", "gp_predict_var_harness.cpp")] + [
        os.path.join(ROOT, "exoplanet_amd", "csrc", f) for f in ("exo_celerite_predict.hpp", "exo_celerite_core.hpp", "exo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_predict_var_work_doubles.restype = ctypes.c_int64
    lib.harness_predict_var_work_doubles.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    return lib


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def run(lib, t, diag, real, cplx, kind, tq, mask=None):
    """-> var (D, M) from the lane functions"""
    t, tq, diag = (np.ascontiguousarray(x, dtype=np.float64) for x in (t, tq, diag))
    real, cplx = np.ascontiguousarray(real, dtype=np.float64), np.ascontiguousarray(cplx, dtype=np.float64)
    kind = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
    D, n_real, n_complex = real.shape[0], real.shape[1], cplx.shape[1]
    n, m = t.size, tq.size
    J = n_real + 2 * n_complex
    nw = lib.harness_predict_var_work_doubles(n, m, J, D)
    assert nw == (n + m) * (J + 1) * D
    work = np.full(nw, np.nan)     # (nothing may depend on what the workspace held)
    var = np.full((D, m), np.nan)
    rc = lib.harness_predict_var(_p(t), _p(diag), ctypes.c_int64(diag.shape[0]), ctypes.c_int64(n), _p(real), n_real, _p(cplx),
                                 n_complex, _p(kind, _ip), _p(mask, _ip), ctypes.c_int64(D), _p(tq), ctypes.c_int64(m), _p(var),
                                 _p(work))
    assert rc == 0
    return var


def kernel_dense(tau, real, cplx, kind, keep_real, keep_pair):
    """k2(tau) of one draw: the real slots and pair slots whose keep flag is set (a pair slot of kind 1: two real terms)"""
    tau = np.abs(tau)
    k = np.zeros_like(tau)
    for (a, c), keep in zip(real, keep_real):
        if keep:
            k += a * np.exp(-c * tau)
    for s, (p, keep) in enumerate(zip(cplx, keep_pair)):
        if not keep:
            continue
        if kind is not None and kind[s]:
            k += p[0] * np.exp(-p[1] * tau) + p[2] * np.exp(-p[3] * tau)
        else:
            k += np.exp(-p[2] * tau) * (p[0] * np.cos(p[3] * tau) + p[1] * np.sin(p[3] * tau))
    return k


def var_dense(t, diag, real, cplx, kind, tq, mask=None):
    nr = real.shape[0]
    mask = np.ones(nr + cplx.shape[0], dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    full = np.ones_like(mask)
    A = kernel_dense(t[:, None] - t[None, :], real, cplx, kind, full[:nr], full[nr:]) + np.diag(diag)
    K2 = kernel_dense(tq[:, None] - t[None, :], real, cplx, kind, mask[:nr], mask[nr:])
    k0 = kernel_dense(np.zeros(1), real, cplx, kind, mask[:nr], mask[nr:])[0]
    return k0 - np.einsum("mn,nm->m", K2, np.linalg.solve(A, K2.T)), k0


def draw_terms(rng, n_real, kinds):
    """one draw: real slots (a, c) and pair slots -- a complex term (kind 0) or an SHO with Q < 1/2 (kind 1: two real terms,
    the second amplitude negative)"""
    real =np.stack([rng.uniform(0.3, 1.5, n_real), rng.uniform(0.05, 2.0, n_real)], -1).reshape(n_real, 2)
    pairs = []
    for k in kinds:
        if k:
            S0, w0 = P.sho_from_sigma_rho(rng.uniform(0.6, 1.2), rng.uniform(2.0, 8.0), 0.3)
            ar, cr, *_ = P.sho_coefficients(S0, w0, 0.3)
            pairs.append([ar[0], cr[0], ar[1], cr[1]])
        else:
            a, c, d = rng.uniform(0.3, 1.5), rng.uniform(0.05, 1.0), rng.uniform(0.3, 4.0)
            pairs.append([a, rng.uniform(-0.9, 0.9) * a * c / d, c, d])
    return real, np.array(pairs).reshape(len(kinds), 4)


def series(rng, n):
    t = np.sort(rng.uniform(0.0, 30.0, n))
    t[n // 3:] += 4.0              # a gap
    t[n // 2 + 1] = t[n // 2]      # a repeated time stamp
    return t


def queries(rng, t):
    tq = np.concatenate([[t[0] - 6.0, t[0] - 0.1, t[0], t[17], t[17], t[-1], t[-1] + 0.3, t[-1] + 4.0],
                         rng.uniform(t[0], t[-1], 25), t[40:43] + 1e-3, [0.5 * (t[60] + t[61])] * 2])
    return np.sort(tq)


# (n_real, pair kinds of each of the D = 3 draws, slot masks to try)
CASES = [
    (1, [[], [], []], [None]),                                                  # J = 1
    (0, [[0], [1], [0]], [None]),                                               # J = 2: the batch straddles Q = 1/2
    (2, [[], [], []], [None, [1, 0], [0, 1]]),                                  # J = 2: two real terms
    (1, [[1], [0], [1]], [None, [1, 0], [0, 1]]),                               # J = 3
    (1, [[0, 1], [0, 0], [1, 0]], [None, [0, 1, 0], [1, 0, 1], [0, 0, 1]]),     # J = 5
    (0, [[0, 0, 1], [1, 0, 0], [0, 0, 0]], [None, [0, 0, 1], [1, 1, 0]]),       # J = 6
    (2, [[0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 1]], [None, [0, 1, 0, 1, 0, 0]]),   # J = 10
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_predict_var_lane_vs_dense(harness, case):
    n_real, kinds, masks = CASES[case]
    rng = np.random.default_rng(100 + case)
    D, n = 3, 150
    t = series(rng, n)
    tq = queries(rng, t)
    terms = [draw_terms(rng, n_real, kinds[d]) for d in range(D)]
    real = np.stack([r for r, _ in terms])
    cplx = np.stack([c for _, c in terms])
    kind = np.array(kinds, dtype=np.int32).reshape(D, -1) if cplx.shape[1] else None
    diag = rng.uniform(0.05, 0.3, (D, n))
    for mask in masks:
        got = run(harness, t, diag, real, cplx, kind, tq, mask)
        for d in range(D):
            want, k0 = var_dense(t, diag[d], real[d], cplx[d], None if kind is None else kind[d], tq, mask)
            assert np.all(want > -1e-12 * k0)
            np.testing.assert_allclose(got[d], want, rtol=0, atol=1e-9 * k0, err_msg=f"draw {d}, mask {mask}")
    # one diagonal for every draw
    got = run(harness, t, diag[:1], real, cplx, kind, tq)
    for d in range(D):
        want, k0 = var_dense(t, diag[0], real[d], cplx[d], None if kind is None else kind[d], tq)
        np.testing.assert_allclose(got[d], want, rtol=0, atol=1e-9 * k0)


def test_predict_var_at_data_times(harness):
    """at the data times the variance is sigma^2 - sigma^4 (A^-1)_nn"""
    rng = np.random.default_rng(7)
    n = 120
    t = series(rng, n)
    real, cplx = draw_terms(rng, 1, [0, 1])
    kind = np.array([[0, 1]], dtype=np.int32)
    diag = rng.uniform(0.1, 0.5, n)
    got = run(harness, t, diag[None], real[None], cplx[None], kind, t)[0]
    A = kernel_dense(t[:, None] - t[None, :], real, cplx, kind[0], [1], [1, 1]) + np.diag(diag)
    want = diag - diag ** 2 * np.diag(np.linalg.inv(A))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10 * kernel_dense(np.zeros(1), real, cplx, kind[0], [1], [1, 1])[0])


def test_predict_var_not_positive_definite_is_nan(harness):
    """a draw whose factorisation meets d <= 0 gets NaN at every query time; the other draws are unaffected"""
    rng = np.random.default_rng(8)
    n = 80
    t = series(rng, n)
    tq = queries(rng, t)
    terms = [draw_terms(rng, 1, [0]) for _ in range(2)]
    real, cplx = np.stack([r for r, _ in terms]), np.stack([c for _, c in terms])
    diag = rng.uniform(0.05, 0.3, (2, n))
    diag[1, 30] = -50.0
    got = run(harness, t, diag, real, cplx, None, tq)
    assert np.all(np.isnan(got[1]))
    want, k0 = var_dense(t, diag[0], real[0], cplx[0], None, tq)
    np.testing.assert_allclose(got[0], want, rtol=0, atol=1e-9 * k0)
