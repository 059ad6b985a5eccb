"""CPU: the orbit-side oracle (numpy port, C port) and the device arithmetic compiled for the host (exo_math.hpp,
exo_rv_core.hpp through tests/host_harness.cpp) against the multiprecision fixture tests/golden/orbit_mp.npz: the Kepler
solve at |M| up to 7e8 and e up to 1 - 1e-12 with its closed-form partials, the radial velocity and the position /
velocity / acceleration vectors with their vector-Jacobian products at e up to 0.999 (values up to 1 - 1e-8), BJD-sized
times, omega on the quadrants, edge-on and face-on.  Tolerances: tests/orbit_mp_cases.py (derived there).

Not held here: oracle.numpy_port.KeplerianOrbit's nine vector methods.  Its constructor takes omega, incl and Omega as
angles and re-derives t0 / tref from t_periastron, so no record of the fixture is reproduced exactly by it (cos(pi/2) is
not 0; t0 rounds at the size of a BJD); the record-level oracle.numpy_port.orbit_vector, which restates the same formulas
on the kernel's own record, is what is held.  The torch KeplerianOrbit takes cos / sin omega and t_periastron as given and
is held on the GPU for the systems that map (tests/test_gpu_orbit_mp.py)."""
import ctypes

import numpy as np
import pytest

import orbit_mp_cases as K
from oracle import c_port as C
from oracle import numpy_port as P
from test_oracle import harness  # noqa: F401  (the fixture that compiles tests/host_harness.cpp)

OPS = ("rv",) + K.MODES


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope="module")
def g():
    return K.load()


@pytest.mark.parametrize("impl", ["numpy", "c", "device_math_on_host"])
def test_kepler_wide(impl, harness, g):  # noqa: F811
    """sin f, cos f at |M| = 1e3 ... 7e8 (on and beside multiples of pi), e = 0 ... 1 - 1e-12, and small |M| near-parabolic"""
    pts = K.kepler_points(g, "wide")
    M, e = np.ascontiguousarray(pts[0]), np.ascontiguousarray(pts[1])
    if impl == "numpy":
        s, c = P.kepler(M, e)
    elif impl == "c":
        s, c = C.kepler(M, e)
    else:
        s, c = np.empty_like(M), np.empty_like(M)
        harness.harness_kepler(_p(M), _p(e), _p(s), _p(c), ctypes.c_int64(M.size))
    tol = K.kepler_value_tol(pts)
    err = np.maximum(np.abs(s - pts[3]), np.abs(c - pts[4]))
    K.report(f"kepler_wide[{impl}]", n=M.size, worst_error_over_tol=err / tol, worst_tol=tol)
    assert np.all(err <= tol)


@pytest.mark.parametrize("which", ["r1", "wide"])
def test_kepler_grad_closed_form(which, g):
    """numpy_port.kepler_grad fed with the fixture's rounded sin f, cos f: all four partials, every eccentricity (the
    1 - e * e it used to form lost 1.3e-8 at e = 1 - 1e-8)"""
    pts = K.kepler_points(g, which)
    e, s, c = pts[1], pts[3], pts[4]
    dfdM, dfde = P.kepler_grad(s, c, e)
    got = (c * dfdM, -s * dfdM, c * dfde, -s * dfde)
    for name, a, w, tol in zip(("dsinf_dM", "dcosf_dM", "dsinf_de", "dcosf_de"), got, pts[5:], K.kepler_closed_form_bound(pts)):
        err = np.abs(a - w)
        K.report(f"kepler_grad[{which}] {name}", worst_error_over_tol=err / tol,
                 worst_relative_error=err / np.where(w != 0, np.abs(w), 1.0))
        assert np.all(err <= tol), name


def _harness_eval(harness, t, rec, op, go):  # noqa: F811
    t, rec, go = (np.ascontiguousarray(x, dtype=np.float64) for x in (t, rec, go))
    out, grec = np.empty(go.shape), np.empty(rec.size)
    if op == "rv":
        harness.harness_rv(_p(t), ctypes.c_int64(t.size), _p(rec), _p(go), _p(out), _p(grec))
    else:
        harness.harness_ov(ctypes.c_int(K.MODES.index(op)), _p(t), ctypes.c_int64(t.size), _p(rec), _p(go), _p(out), _p(grec))
    return out, grec


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("impl", ["numpy", "device_math_on_host"])
def test_values_and_vjps(impl, op, harness, g):  # noqa: F811
    """every system alone: values of all 24, vector-Jacobian products of the 18 with e <= 0.999"""
    worst_v = worst_g = worst_u = 0.0
    for i in range(K.n_systems(g)):
        rec, want, J = K.case(g, i, op)
        go = K.cotangent(i, op, want.shape)
        out, gp = K.oracle(g["t"][i], rec, op, go) if impl == "numpy" else _harness_eval(harness, g["t"][i], rec, op, go)
        rv = np.max(np.abs(out - want) / K.value_tol(g, i, op))
        worst_v = max(worst_v, rv)
        line = dict(value_error_over_tol=rv)
        if g["sys_grad"][i]:
            unit = K.oracle_unit(g, i, op)
            gw, den = K.vjp_want(J, go)
            rg = np.abs(gp - gw) / den
            worst_g, worst_u = max(worst_g, rg.max()), max(worst_u, unit.max())
            line.update(unit=unit, vjp_error=rg, vjp_tol=K.vjp_tol(unit).min())
            # the condition on the inputs: a float64 evaluation of these systems is this well determined
            assert unit.max() <= K.UNIT_CEILING, (i, op, unit)
            assert np.all(rg <= K.vjp_tol(unit)), (i, op, rg)
        K.report(f"{op}[{impl}] system {i} e={rec[2]:.10g} layout {int(g['sys_layout'][i])}", **line)
        assert rv <= 1.0, (i, op, rv)
    K.report(f"{op}[{impl}] worst", value_error_over_tol=worst_v, vjp_error=worst_g, unit=worst_u)


def test_mean_anomaly_reduction(g):
    """numpy_port.mean_anomaly_reduced and the reduction inside numpy_port.kepler_E against mpmath's M_red: the first keeps
    (t - tp) n as a sum of two doubles (|M| ~ 3e7 with tp = 0.3 and BJD times), the second takes an exact k * fl(2 pi) off"""
    pts = K.kepler_points(g, "wide")
    M, Mred = pts[0], pts[2]
    got = P.mean_anomaly_reduced(M, 0.0, 1.0)
    err = np.abs(np.angle(np.exp(1j * (got - Mred))))       # (+-pi are the same point)
    K.report("mean_anomaly_reduced(M, 0, 1)", worst_error=err, bound=4 * K.EPS)
    assert np.all(err <= 4 * K.EPS)
