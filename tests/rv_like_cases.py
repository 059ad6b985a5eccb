"""What tests/test_rv_like_host.py and tests/test_gpu_rv_like.py share: the multiprecision fixture tests/golden/rv_like_mp.npz
(tools/make_rv_like_golden.py), the tolerance -- derived here, not taken from the code under test -- and the float64
restatement's own error ("unit") on the same inputs.

Tolerance (the convention of tests/orbit_mp_cases.py for summed quantities)
--------------------------------------------------------------------------
Every output of exo_rv_loglike_vjp_f64 is a sum over the epochs.  For each scalar output

    |error| / (sum of the absolute values of its terms)  <=  max(16 unit, 1e-13),

where the terms are the products that are added, before any cancellation between them -- w r^2 / 2, |log s2| / 2 and the
constant n / 2 log 2 pi for the value; |rho dm/drec|, |rho tau^k|, |rho|, (rho^2 + w) / 2 for the gradients -- summed in
mpmath by the fixture's generator, and `unit` is that same ratio for the float64 numpy restatement below
(oracle.numpy_port.radial_velocity with its Jacobian, plain numpy for the rest) on the same inputs.  A term carries the
rounding of rho = w (rv - m), in which m is a sum of a few numbers of the size of the signal: relative to the sum of absolute
terms that is a few EPS times signal / residual, the same for any float64 evaluation, and it is what the unit measures; the
factor 16 covers the order of summation (up to 256 lanes, a shuffle tree, the waves and the tiles in turn) against numpy's
pairwise sums, and the floor 1e-13 a unit that happens to be tiny.  An output without terms (an instrument without epochs)
must be exactly 0.

Condition on the inputs: every system's unit <= 1e-12 (UNIT_CEILING).  The generator checks it when it writes the fixture,
the host test asserts it.
"""
import os
from types import SimpleNamespace

import numpy as np

from oracle import numpy_port as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYSTEMS = ("a", "b", "c", "d", "e", "f")
OUTPUTS = ("loglike", "gparams", "gtrend", "goffset", "gjit2")
UNIT_CEILING = 1e-12
FLOOR = 1e-13
MAX_TREND, MAX_INST = 4, 8       # include/exoplanet_amd.h EXO_RV_MAX_TREND, EXO_RV_MAX_INST
TILE = 1024                      # exo_rv_like_core.hpp kTile (system e has TILE + 1 epochs)


def load():
    return np.load(os.path.join(GOLD, "rv_like_mp.npz"))


def case(g, name):
    """inputs of system ``name`` (offset / jit2: None where the fixture passes a null pointer) and the wanted outputs with
    their normalisers (``want``, ``norm``: dicts over OUTPUTS)"""
    get = lambda k: g[f"{name}_{k}"] if f"{name}_{k}" in g.files else None  # noqa: E731
    c = SimpleNamespace(name=name, **{k: get(k) for k in ("t", "inst", "rv", "var", "params", "trend", "offset", "jit2")})
    c.tref = float(get("tref"))
    c.tau = c.t - c.tref
    c.n_inst = get("goffset").shape[1]
    c.want = {k: get(k) for k in OUTPUTS}
    c.norm = {k: get("n_" + k) for k in OUTPUTS}
    return c


def restatement(c):
    """the definitions of include/exoplanet_amd.h (exo_rv_loglike_vjp_f64) in float64 numpy"""
    D, N, T, I = c.params.shape[0], c.t.size, c.trend.shape[1], c.n_inst
    rv_p, J = P.radial_velocity(c.t, c.params, jac=True)                  # (D, N, P), (D, N, P, 6)
    pw = c.tau[:, None] ** np.arange(T)[None, :]                          # (N, T)
    onehot = (c.inst[:, None] == np.arange(I)[None, :]).astype(np.float64)
    offset = np.zeros((D, I)) if c.offset is None else c.offset
    jit2 = np.zeros((D, I)) if c.jit2 is None else c.jit2
    m = rv_p.sum(-1) + c.trend @ pw.T + offset[:, c.inst]
    s2 = np.broadcast_to(c.var, (N,))[None, :] + jit2[:, c.inst]
    w = 1.0 / s2
    r = c.rv[None, :] - m
    rho = w * r
    return dict(loglike=-0.5 * (w * r * r + np.log(s2)).sum(1) - 0.5 * N * np.log(2 * np.pi),
                gparams=np.einsum("dn,dnpk->dpk", rho, J), gtrend=rho @ pw, goffset=rho @ onehot,
                gjit2=0.5 * ((rho * rho - w) @ onehot))


def ratio(got, want, norm):
    """|got - want| over the normaliser; where there are no terms: 0 for an exact 0, inf otherwise"""
    err = np.abs(np.asarray(got) - want)
    return np.where(norm > 0, err / np.where(norm > 0, norm, 1.0), np.where(err == 0, 0.0, np.inf))


def units(c):
    """per output, the restatement's error over the normaliser (same shape as the output)"""
    got = restatement(c)
    return {k: ratio(got[k], c.want[k], c.norm[k]) for k in OUTPUTS}


def oracle_unit(g, name):
    """the largest unit of system ``name``"""
    return max([float(u.max()) for u in units(case(g, name)).values() if u.size] + [0.0])


def tol(unit):
    return np.maximum(16 * unit, FLOOR)


def check(label, c, got, unit=None):
    """print the figures of every output in ``got`` (dict over OUTPUTS; the value is required), then assert them against the
    fixture"""
    unit = units(c) if unit is None else unit
    bad = []
    assert "loglike" in got
    for k in OUTPUTS:
        if k not in got or not c.want[k].size:
            continue
        err = ratio(got[k], c.want[k], c.norm[k])
        print(f"{label} system {c.name} {k}: worst error / normaliser = {err.max():.3g}, unit = {unit[k].max():.3g}, "
              f"worst error / tolerance = {(err / tol(unit[k])).max():.3g}")
        if not np.all(err <= tol(unit[k])):
            bad.append((k, float(err.max()), float((err / tol(unit[k])).max())))
    assert not bad, (label, c.name, bad)
