"""Helpers of the distributions tests: one implementation of ParameterSpace.constrain -- the composed torch statement, the
host build of csrc/exo_priors_core.hpp, the kernels -- evaluated on a case of tests/golden/priors.npz, and the error measure.

The measure: max |got - want| / (1 + |want|) over an array -- relative for large results (a log prior of -1e5, exp(36)),
absolute on the scale 1 for the constrained values and derivatives, which live on unit intervals (a derivative of 1e-16
at |z| = 36 is not asked for sixteen digits of its own)."""
import ctypes
import os
import subprocess

import numpy as np
import torch


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
_dp = ctypes.POINTER(ctypes.c_double)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "priors.npz"))


def err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.all(np.isfinite(got) == np.isfinite(want)):
        return np.inf
    ok = np.isfinite(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / (1.0 + np.abs(want[ok])), initial=0.0))


def rel_err(got, want):
    """max |got - want| / |want| over the entries the fixture has non-zero: purely relative, however small the entry (a
    derivative of 1e-16 at |z| = 36 is asked for its own digits)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.all(np.isfinite(got) == np.isfinite(want)) or np.any(got[want == 0] != 0):
        return np.inf
    ok = np.isfinite(want) & (want != 0)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]), initial=0.0))


def torch_path(space, z, device="cpu", composed=True):
    """(values (N, n_values), log prior, its gradient, Jacobian (N, n_values, n_free)) by autograd"""
    z = torch.as_tensor(z, dtype=torch.float64, device=device).requires_grad_(True)
    theta, lp = space.constrain_composed(z) if composed else space.constrain(z)
    cols = [theta[k][:, c] for k, n in space.outputs for c in range(n)]
    (dlp,) = torch.autograd.grad(lp.sum(), z, retain_graph=True)
    jac = [torch.autograd.grad(col.sum(), z, retain_graph=True, allow_unused=True)[0] for col in cols]
    jac = [torch.zeros_like(z) if j is None else j for j in jac]
    out = torch.stack(cols, 1), lp, dlp, torch.stack(jac, 1)
    return tuple(x.detach().cpu().numpy() for x in out)


def load_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "priors_harness.so")
    srcs = [os.path.join(ROOT, "tests", "priors_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_priors_core.hpp"),
            os.path.join(ROOT, "include", "exoplanet_amd.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_digamma.restype = ctypes.c_double
    lib.harness_digamma.argtypes = [ctypes.c_double]
    return lib


def harness_path(lib, space, z):
    """the same four arrays from the host build of the core header: one reverse call per value column"""
    table = space.table()
    z = np.ascontiguousarray(z, dtype=np.float64)
    N, n = z.shape
    outs = [np.empty((N, c)) for c in table.out_cols]
    lp = np.empty(N)
    ptrs = (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    zp = z.ctypes.data_as(ctypes.c_void_p)
    assert lib.harness_prior_transform(zp, ctypes.c_int64(N), n, table.blocks, table.n_block, ptrs, lp.ctypes.data_as(ctypes.c_void_p)) == 0

    def vjp(gouts, glp):
        gz = np.full((N, n), np.nan)
        gp = (ctypes.c_void_p * len(outs))(*[None if g is None else g.ctypes.data for g in gouts])
        assert lib.harness_prior_transform_vjp(zp, ctypes.c_int64(N), n, table.blocks, table.n_block, gp,
                                               None if glp is None else glp.ctypes.data_as(ctypes.c_void_p),
                                               gz.ctypes.data_as(ctypes.c_void_p)) == 0
        return gz

    dlp = vjp([None] * len(outs), np.ones(N))
    jac = []
    for k, c in enumerate(table.out_cols):
        for col in range(c):
            g = np.zeros((N, c))
            g[:, col] = 1.0
            jac.append(vjp([g if i == k else None for i in range(len(outs))], None))
    return np.concatenate(outs, 1), lp, dlp, np.stack(jac, 1)


def kernel_path(space, z, device):
    """the same four arrays from the kernels (ParameterSpace.constrain on a device tensor)"""
    return torch_path(space, z, device=device, composed=False)


def errors(case, got, data=None):
    """the error of (values, log prior, gradient, Jacobian) against the fixture, by array"""
    data = golden() if data is None else data
    return {k: err(g, data[f"{case}/{k}"]) for k, g in zip(("values", "log_prior", "dlog_prior", "jacobian"), got)}


# ---- what is sampled: prior-only NUTS runs (the reference's statistical tests, restated) -----------------------------------------

def sample(xd, space, logp_fn, D, seed, device="cpu", warm=200, keep=150, start=None):
    """NUTS on space.wrap(logp_fn): ``warm`` adaptive steps (step sizes and masses), ``keep`` kept; -> ({name: draws}, sampler,
    whether every chain had a valid leaf at the end of the warm-up).  The chains start at z = 0.5 N(0, 1), or scattered a
    little around the constrained values ``start`` (a potential with a bounded support wants a start inside it)"""
    from exoplanet_amd import NUTS

    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    z0 = torch.randn(D, space.n_free, dtype=torch.float64, device=device, generator=gen)
    z0 = 0.5 * z0 if start is None else space.unconstrain(D, **start).to(device) + 0.02 * z0
    nuts = NUTS(space.wrap(logp_fn), [z0], step_size=0.1, generator=gen)
    nuts.warmup(warm, adapt_mass=True)
    ok_after_warmup = bool(nuts.last_adapt_ok.all())
    draws = []
    for _ in range(keep):
        nuts.step()
        draws.append(nuts.params[0].clone())
    with torch.no_grad():
        theta, _ = space.constrain(torch.cat(draws))
    return {k: v.cpu().numpy() for k, v in theta.items()}, nuts, ok_after_warmup


def _mixture_cdf(f):
    from scipy.stats import halfnorm, rayleigh

    return lambda x: (1 - f) * halfnorm.cdf(x, scale=0.049) + f * rayleigh.cdf(x, scale=0.26)


def _uniform_cdf(lo, hi):
    return lambda x: np.clip((x - lo) / (hi - lo), 0.0, 1.0)


def _truncated_beta_cdf(a, b, lo, hi):
    from scipy.stats import beta

    return lambda x: (beta.cdf(x, a, b) - beta.cdf(lo, a, b)) / (beta.cdf(hi, a, b) - beta.cdf(lo, a, b))


def ks_cases(xd):
    """id -> (space, logp_fn of the constrained parameters, [(statistic of the draws, its distribution function)], bounds
    {name: (lo, hi)} every draw must respect[, constrained values the chains start around])"""
    from scipy.stats import beta

    nothing = lambda **_: 0.0  # noqa: E731
    e2 = lambda secosw, sesinw: secosw ** 2 + sesinw ** 2  # noqa: E731
    disk = lambda: xd.ParameterSpace(h=xd.unit_disk(names=("secosw", "sesinw")))  # noqa: E731
    ecc = lambda th: th["ecc"].ravel()  # noqa: E731
    obs = lambda th: e2(th["secosw"], th["sesinw"]).ravel()  # noqa: E731
    unit = _uniform_cdf(0.0, 1.0)
    cases = {
        "kipping13_all": (xd.ParameterSpace(ecc=xd.kipping13(shape=2)), nothing, [(ecc, lambda x: beta.cdf(x, 1.12, 3.09))], {"ecc": (0, 1)}),
        "kipping13_long": (xd.ParameterSpace(ecc=xd.kipping13(long=True, shape=3)), nothing, [(ecc, lambda x: beta.cdf(x, 1.12, 3.09))],
                           {"ecc": (0, 1)}),
        "kipping13_short": (xd.ParameterSpace(ecc=xd.kipping13(long=False, shape=4)), nothing, [(ecc, lambda x: beta.cdf(x, 0.697, 3.27))],
                            {"ecc": (0, 1)}),
        "vaneylen19_single": (xd.ParameterSpace(ecc=xd.vaneylen19(shape=2)), nothing, [(ecc, _mixture_cdf(0.76))], {"ecc": (0, 1)}),
        "vaneylen19_multi": (xd.ParameterSpace(ecc=xd.vaneylen19(multi=True, shape=3)), nothing, [(ecc, _mixture_cdf(0.08))], {"ecc": (0, 1)}),
        "kipping13_observed": (disk(), lambda secosw, sesinw: xd.kipping13().logp(e2(secosw, sesinw)).sum(1),
                               [(obs, lambda x: beta.cdf(x, 1.12, 3.09))], {}),
        "vaneylen19_observed": (disk(), lambda secosw, sesinw: xd.vaneylen19().logp(e2(secosw, sesinw)).sum(1),
                                [(obs, _mixture_cdf(0.76))], {}),
        "unit_disk": (xd.ParameterSpace(h=xd.unit_disk(shape=2)), nothing,
                      [(lambda th: (th["x"] ** 2 + th["y"] ** 2).ravel(), unit),
                       (lambda th: np.arctan2(th["y"], th["x"]).ravel(), _uniform_cdf(-np.pi, np.pi))], {}),
        "angle": (xd.ParameterSpace(omega=xd.angle(shape=2)), nothing, [(lambda th: th["omega"].ravel(), _uniform_cdf(-np.pi, np.pi))],
                  {"omega": (-np.pi, np.pi)}),
        "impact_parameter": (xd.ParameterSpace(r=xd.uniform(0.01, 0.3), b=xd.impact_parameter("r")), nothing,
                             [(lambda th: (th["b"] / (1 + th["r"])).ravel(), unit), (lambda th: th["r"].ravel(), _uniform_cdf(0.01, 0.3))],
                             {"r": (0.01, 0.3)}),
        "quad_limb_dark": (xd.ParameterSpace(u=xd.quad_limb_dark()), nothing,
                           [(lambda th: ((th["u1"] + th["u2"]) ** 2).ravel(), unit),
                            (lambda th: (th["u1"] / (2 * (th["u1"] + th["u2"]))).ravel(), unit)], {}),
        "kipping13_lower": (xd.ParameterSpace(ecc=xd.kipping13(lower=0.1)), nothing, [(ecc, _truncated_beta_cdf(1.12, 3.09, 0.1, 1.0))],
                            {"ecc": (0.1, 1.0)}),
        "kipping13_upper": (xd.ParameterSpace(ecc=xd.kipping13(upper=0.5)), nothing, [(ecc, _truncated_beta_cdf(1.12, 3.09, 0.0, 0.5))],
                            {"ecc": (0.0, 0.5)}),
        "kipping13_both": (xd.ParameterSpace(ecc=xd.kipping13(lower=0.3, upper=0.4)), nothing,
                           [(ecc, _truncated_beta_cdf(1.12, 3.09, 0.3, 0.4))], {"ecc": (0.3, 0.4)}),
        "kipping13_observed_bounded": (disk(), lambda secosw, sesinw: xd.kipping13(lower=0.2, upper=0.4).logp(e2(secosw, sesinw)).sum(1),
                                       [(obs, _truncated_beta_cdf(1.12, 3.09, 0.2, 0.4))], {},
                                       # as in the reference's test: eccentricity at the middle of the bounds, any direction
                                       dict(secosw=np.sqrt(0.3) * np.cos(np.pi / 4), sesinw=np.sqrt(0.3) * np.sin(np.pi / 4))),
        "vaneylen19_bounded": (xd.ParameterSpace(ecc=xd.vaneylen19(lower=0.2, upper=0.4, shape=2)), nothing, [], {"ecc": (0.2, 0.4)}),
        "kipping13_free": (xd.ParameterSpace(ecc=xd.kipping13(fixed=False, shape=10)), nothing, [], {"ecc": (0, 1)}),
        "vaneylen19_free": (xd.ParameterSpace(ecc=xd.vaneylen19(fixed=False, shape=10)), nothing, [], {"ecc": (0, 1), "ecc::frac": (0, 1)}),
    }
    return cases


KS_BOUND = 0.05        # the reference's threshold (its tests/distributions_test.py)
