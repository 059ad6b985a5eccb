"""CPU: exoplanet_amd.distributions on its composed-torch path and the arithmetic of exoplanet_amd/csrc/exo_priors_core.hpp
compiled for the host (tests/priors_harness.cpp), against the multiprecision fixture tests/golden/priors.npz
(tools/make_priors_golden.py: mpmath, from the density definitions), scipy.stats, torch.autograd.gradcheck and the
reference's own statistical tests restated on CPU NUTS.  The kernels themselves: tests/test_gpu_distributions.py."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import priors_cases as C  # noqa: E402
import priors_check as K  # noqa: E402

from exoplanet_amd import distributions as xd  # noqa: E402

# The error of the torch path and of the host-compiled core against the fixture, measured (the
# measure: priors_check.err): at most 8.9e-15 (torch) and 8.1e-15 (host core), both in the gradient of the kipping13(fixed=False)
# log prior with respect to log alpha -- a sum of log s(z_j) against n (digamma(alpha) - digamma(alpha + beta)), scaled by
# alpha; every other array of every case is below 2.2e-15.  Asserted at 4x the larger of the two (floor: 8 ulp).
TOL = max(4 * 8.9e-15, 8 * K.ULP)


# The same arrays held RELATIVELY, entry by entry, however small (priors_check.rel_err): the values and their Jacobian are products
# of factors that each keep their relative precision, down to 1e-16 at |z| = 36.  Measured for the host-compiled core: values
# 2.0e-15 (unit_disk: the 2^-49 shrink of x), Jacobian 1.5e-15; the kernels on an MI355X: see tests/test_gpu_distributions.py.
# Asserted at 4x.  The torch path is NOT held to this: autograd differentiates sigmoid as s (1 - s) from the rounded s, which is 4 %
# off where 1 - s is 2e-16 -- an absolute error of 1e-17 in a derivative that multiplies cotangents of order one; its values are.
# The gradient of the log prior changes sign inside the grid, so only the mixed measure above applies to it.
REL_TOL = max(4 * 2.0e-15, 8 * K.ULP)


@pytest.fixture(scope="module")
def harness():
    return K.load_harness()


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_definitions_against_the_multiprecision_fixture(harness, case):
    data = K.golden()
    space = C.build(xd, case)
    z = data[case + "/z"]
    assert z.shape == (C.N_ROWS, space.n_free) and np.abs(z).max() >= (36.0 if case != "normal" else 3.0)
    for name, got in (("torch", K.torch_path(space, z)), ("host core", K.harness_path(harness, space, z))):
        e = K.errors(case, got, data)
        print(case, name, {k: "%.2e" % v for k, v in e.items()})
        assert max(e.values()) <= TOL, (name, e)
        r = {"values": K.rel_err(got[0], data[case + "/values"]), "jacobian": K.rel_err(got[3], data[case + "/jacobian"])}
        print(case, name, "relative", {k: "%.2e" % v for k, v in r.items()})
        assert r["values"] <= REL_TOL and (name == "torch" or r["jacobian"] <= REL_TOL), (name, r)


def test_digamma_and_incomplete_beta(harness):
    from scipy.special import betainc, digamma

    x = np.concatenate([np.exp(np.linspace(np.log(1e-3), np.log(1e4), 400)), [1.0, 2.0, 10.0, 0.697, 3.27]])
    got = np.array([harness.harness_digamma(v) for v in x])
    print("digamma:", K.err(got, digamma(x)))
    assert K.err(got, digamma(x)) <= TOL
    for a, b in ((1.12, 3.09), (0.697, 3.27), (5.0, 0.5)):
        for v in (1e-6, 0.1, 0.3, 0.5, 0.8, 0.999):
            assert xd._betainc(a, b, v) == pytest.approx(betainc(a, b, v), rel=1e-13)


def test_logp_of_constrained_values_against_scipy():
    from scipy import stats

    x = torch.tensor(np.concatenate([np.linspace(1e-4, 0.9999, 301), [1e-12, 0.25]]))
    xn = x.numpy()
    checks = [
        (xd.kipping13().logp(x), stats.beta.logpdf(xn, 1.12, 3.09)),
        (xd.kipping13(long=False).logp(x), stats.beta.logpdf(xn, 0.697, 3.27)),
        (xd.normal(0.3, 0.2).logp(x), stats.norm.logpdf(xn, 0.3, 0.2)),
        (xd.lognormal(0.3, 0.2).logp(x), stats.lognorm.logpdf(xn, 0.2, scale=math.exp(0.3))),
        (xd.uniform(-1.0, 3.0).logp(x), stats.uniform.logpdf(xn, -1.0, 4.0)),
    ]
    for f in (0.76, 0.08):
        mix = np.logaddexp(math.log(1 - f) + stats.halfnorm.logpdf(xn, scale=0.049), math.log(f) + stats.rayleigh.logpdf(xn, scale=0.26))
        checks.append((xd.vaneylen19(multi=f < 0.5).logp(x), mix))
        lo, hi = 0.1, 0.6
        checks.append((xd.vaneylen19(multi=f < 0.5, lower=lo, upper=hi).logp(x),
                       np.where((xn >= lo) & (xn <= hi), mix - math.log(hi - lo), -np.inf)))
    for (a, b), (lo, hi) in (((1.12, 3.09), (0.1, 0.8)), ((0.697, 3.27), (0.0, 0.5)), ((1.12, 3.09), (0.3, 1.0))):
        mass = stats.beta.cdf(hi, a, b) - stats.beta.cdf(lo, a, b)
        want = np.where((xn >= lo) & (xn <= hi), stats.beta.logpdf(xn, a, b) - math.log(mass), -np.inf)
        checks.append((xd.kipping13(long=a > 1, lower=lo or None, upper=hi if hi < 1 else None).logp(x), want))
    for got, want in checks:
        assert K.err(got.numpy(), want) <= TOL
    # outside the support and on its edges: -inf, and a gradient without NaN
    for dist in (xd.kipping13(), xd.kipping13(long=False, lower=0.1, upper=0.8), xd.vaneylen19(), xd.vaneylen19(upper=0.5), xd.lognormal(0, 1)):
        v = torch.tensor([-0.5, 0.0, 0.05, 0.3, 0.9, 1.0, 1.5], dtype=torch.float64, requires_grad=True)
        lp = dist.logp(v)
        (g,) = torch.autograd.grad(lp[torch.isfinite(lp)].sum(), v)
        assert not torch.isnan(lp).any() and not torch.isnan(g).any() and bool((lp[:2] == -np.inf).all())
    # the hyperpriors: normals truncated at zero (and to [0, 1]) with their log-Jacobians, through the composed statement
    space = xd.ParameterSpace(ecc=xd.vaneylen19(fixed=False))
    z = torch.tensor(np.random.RandomState(3).randn(50, 4) * 0.3 + [math.log(0.049), math.log(0.26), 1.0, 0.0])
    theta, lp = space.constrain(z)
    sg, sr, f, e = (theta[k].numpy()[:, 0] for k in ("ecc::sigma_gauss", "ecc::sigma_rayleigh", "ecc::frac", "ecc"))
    zz = z.numpy()
    tn = lambda v, mu, sd, hi=np.inf: stats.truncnorm.logpdf(v, (0 - mu) / sd, (hi - mu) / sd, loc=mu, scale=sd)  # noqa: E731
    L = lambda v: np.log(v) + np.log1p(-v)  # noqa: E731
    want = (tn(sg, 0.049, 0.02) + zz[:, 0] + tn(sr, 0.26, 0.05) + zz[:, 1] + tn(f, 0.76, 0.2, 1.0) + L(f) + L(e)
            + np.logaddexp(np.log1p(-f) + stats.halfnorm.logpdf(e, scale=sg), np.log(f) + stats.rayleigh.logpdf(e, scale=sr)))
    assert K.err(lp.numpy(), want) <= TOL


def every_kind():
    return xd.ParameterSpace(
        p=xd.normal(3.5, 0.5), m=xd.lognormal(0.1, 0.5, shape=2), r=xd.uniform(0.01, 0.3, shape=2),
        b=xd.impact_parameter("r", shape=2), bc=xd.impact_parameter(0.1), u=xd.quad_limb_dark(), h=xd.unit_disk(),
        e1=xd.kipping13(shape=2), e2=xd.kipping13(long=False, lower=0.1, upper=0.8), e3=xd.vaneylen19(),
        e4=xd.vaneylen19(multi=True, upper=0.5), e5=xd.kipping13(fixed=False, shape=2), e6=xd.vaneylen19(fixed=False, shape=2),
        omega=xd.angle(), w=xd.angle(regularization=None))


def test_gradcheck_of_constrain():
    space = every_kind()
    assert space.n_free == 30 and space.names == ["p", "m", "r", "b", "bc", "u1", "u2", "x", "y", "e1", "e2", "e3", "e4", "e5", "e6", "omega", "w"]
    assert [k for k, _ in space.outputs if "::" in k] == ["e5::alpha", "e5::beta", "e6::sigma_gauss", "e6::sigma_rayleigh", "e6::frac"]
    z = torch.tensor(np.random.RandomState(11).randn(3, space.n_free))
    z[:, 0] += 3.5
    z.requires_grad_(True)

    def f(z):
        theta, lp = space.constrain(z)
        return torch.cat(list(theta.values()) + [lp[:, None]], 1)

    assert torch.autograd.gradcheck(f, (z,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_round_trips_and_argument_errors():
    space = every_kind()
    rs = np.random.RandomState(5)
    z = rs.uniform(-20, 20, size=(400, space.n_free))
    hyper = [i for _, d, off, _, _ in space.blocks for i in range(off, off + len(d.hyper))]
    ang = [i for _, d, off, _, _ in space.blocks if d.kind == xd.ANGLE for i in range(off, off + 2)]
    z[:, hyper] = rs.uniform(-2, 2, size=(400, len(hyper)))
    z[:, 0] = 3.5 + rs.randn(400)
    z[:, 1:3] = rs.randn(400, 2)
    z = torch.tensor(z)
    theta, _ = space.constrain(z)
    back = space.unconstrain(400, **theta)
    # the logistic function resolves z to one rounding of s(z) or s(-z), whichever is smaller: an error of
    # ulp / min(s, 1 - s) = ulp (1 + e^|z|) in z (twice over for the second coordinate of a pair, which divides by a rounded root)
    tol = 8 * K.ULP * (1.0 + np.exp(np.abs(z.numpy()))) + 8 * K.ULP * np.abs(z.numpy())
    tol[:, ang] = np.inf                                  # an angle keeps its direction, not its radius: checked below
    # y of a unit_disk is divided by sqrt(1 - x^2) on the way back, which the rounded x resolves to ulp / (1 - |x|) only
    h = [off for name, _, off, _, _ in space.blocks if name == "h"][0]
    tol[:, h + 1] *= 1.0 + np.exp(np.abs(z.numpy()[:, h]))
    assert np.all(np.abs(back.numpy() - z.numpy()) <= tol)
    again, _ = space.constrain(back)
    for k in ("omega", "w"):
        assert K.err(again[k].numpy(), theta[k].numpy()) <= TOL
    # the reverse: constrained values -> z -> the same values
    vals = dict(p=3.4, m=[1.0, 2.0], r=[0.05, 0.2], b=[0.3, 1.1], bc=0.9, u1=0.3, u2=0.2, x=-0.3, y=0.6, e1=[0.1, 0.7], e2=0.5, e3=0.02,
                e4=0.4, e5=[0.2, 0.3], e6=[0.1, 0.01], omega=0.5, w=-3.0)
    z0 = space.unconstrain(7, **vals, **{"e5::alpha": 1.3})
    assert z0.shape == (7, space.n_free) and z0.dtype == torch.float64
    th, lp = space.constrain(z0)
    assert bool(torch.isfinite(lp).all())
    for k, v in vals.items():
        assert K.err(th[k].numpy(), np.broadcast_to(np.atleast_1d(v), th[k].shape)) <= TOL, k
    assert K.err(th["e5::alpha"].numpy(), np.full((7, 1), 1.3)) <= TOL and K.err(th["e6::frac"].numpy(), np.full((7, 1), 0.76)) <= TOL
    per_chain = space.unconstrain(7, **dict(vals, p=torch.linspace(3.0, 4.0, 7, dtype=torch.float64)))
    assert K.err(space.constrain(per_chain)[0]["p"].numpy()[:, 0], np.linspace(3.0, 4.0, 7)) <= TOL
    for bad in (dict(r=[0.05, 0.31]), dict(b=[0.3, 1.21]), dict(u1=0.9, u2=0.2), dict(x=0.8, y=0.7), dict(e2=0.05), dict(e4=0.6),
                dict(e1=[0.1, 1.0]), dict(m=[1.0, -1.0])):
        with pytest.raises(ValueError):
            space.unconstrain(7, **dict(vals, **bad))
    with pytest.raises(ValueError):
        space.unconstrain(7, **{k: v for k, v in vals.items() if k != "w"})
    with pytest.raises(ValueError, match="D == count"):
        space.unconstrain(2, **vals)                      # m = [1, 2] with two chains: per chain or per element?
    assert space.unconstrain(2, **dict(vals, m=torch.tensor([[1.0, 2.0]]), r=torch.tensor([[0.05, 0.2]]), b=torch.tensor([[0.3, 1.1]]),
                                       e1=torch.tensor([[0.1, 0.7]]), e5=torch.tensor([[0.2, 0.3]]), e6=torch.tensor([[0.1, 0.01]]))).shape == (2, 30)
    with pytest.raises(NotImplementedError, match="incomplete beta"):
        xd.kipping13(fixed=False, upper=0.5)
    with pytest.raises(ValueError, match="earlier"):
        xd.ParameterSpace(b=xd.impact_parameter("r"), r=xd.uniform(0, 1))
    with pytest.raises(ValueError, match="one name"):
        xd.ParameterSpace(h=xd.unit_disk(), k=xd.unit_disk())
    with pytest.raises(ValueError):
        space.constrain(torch.zeros(3, space.n_free + 1, dtype=torch.float64))


def test_closed_supports_and_finiteness_up_to_36(harness):
    """every value inside its closed support, log prior and gradient finite, for every |z| <= 36 -- and no NaN far beyond"""
    g = np.concatenate([np.linspace(-36, 36, 145), [-35.99, 1e-3, -1e-9, 0.0, 17.3]])
    pair = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    one = g[:, None]
    spaces = [
        (xd.ParameterSpace(u=xd.quad_limb_dark()), pair), (xd.ParameterSpace(h=xd.unit_disk()), pair),
        (xd.ParameterSpace(r=xd.uniform(0.01, 0.3), b=xd.impact_parameter("r")), pair),
        (xd.ParameterSpace(w=xd.angle(regularization=None)), pair),
        (xd.ParameterSpace(w=xd.angle()), pair[(pair != 0).any(1)]),
        (xd.ParameterSpace(a=xd.kipping13(), b=xd.kipping13(long=False), c=xd.kipping13(lower=0.3, upper=0.4), d=xd.kipping13(lower=0.1),
                           e=xd.kipping13(upper=0.5), f=xd.vaneylen19(), g=xd.vaneylen19(multi=True), h=xd.vaneylen19(lower=0.2, upper=0.4),
                           i=xd.vaneylen19(upper=0.3), j=xd.uniform(-2.0, 5.0), k=xd.impact_parameter(0.1), m=xd.lognormal(0, 1),
                           n=xd.normal(0, 1)), np.repeat(one, 13, 1)),
        (xd.ParameterSpace(e=xd.kipping13(fixed=False), f=xd.vaneylen19(fixed=False, lower=0.1, upper=0.7)), np.repeat(one, 7, 1)),
    ]
    bounds = dict(a=(0, 1), b=(0, 1), c=(0.3, 0.4), d=(0.1, 1), e=(0, 0.5), f=(0, 1), g=(0, 1), h=(0.2, 0.4), i=(0, 0.3), j=(-2, 5), k=(0, 1.1))
    for n_space, (space, z) in enumerate(spaces):
        for values, lp, dlp, _ in (K.torch_path(space, z), K.harness_path(harness, space, z)):
            assert np.isfinite(lp).all() and np.isfinite(dlp).all() and np.isfinite(values).all()
            th = dict(zip([k for k, _ in space.outputs], values.T))
            if "u1" in th:
                assert (th["u1"] >= 0).all() and (th["u1"] + th["u2"] <= 1).all() and (th["u1"] + 2 * th["u2"] >= 0).all()
            elif "x" in th:
                assert (th["x"] ** 2 + th["y"] ** 2 <= 1).all()
            elif "r" in th:
                assert (th["b"] >= 0).all() and (th["b"] <= 1 + th["r"]).all() and (th["r"] >= 0.01).all() and (th["r"] <= 0.3).all()
            elif "w" in th:
                assert (np.abs(th["w"]) <= np.pi).all()
            elif n_space == 5:
                for k, (lo, hi) in bounds.items():
                    assert (th[k] >= lo).all() and (th[k] <= hi).all(), k
            else:
                assert (th["e"] >= 0).all() and (th["e"] <= 1).all() and (th["f"] >= 0.1).all() and (th["f"] <= 0.7).all()
                assert (th["f::frac"] >= 0).all() and (th["f::frac"] <= 1).all() and (th["e::alpha"] > 0).all()
    # a regularised angle at the origin: log prior -inf (the reference's own), nothing NaN
    for got in (K.torch_path(xd.ParameterSpace(w=xd.angle()), np.zeros((1, 2))), K.harness_path(harness, xd.ParameterSpace(w=xd.angle()), np.zeros((1, 2)))):
        assert got[1][0] == -np.inf and not np.isnan(got[0]).any()
    # no NaN for any finite z: far beyond the range anything is asked of
    far = np.array([[-800.0], [-700.0], [50.0], [700.0], [800.0]])
    space, z = spaces[5][0], np.repeat(far, 13, 1)
    z[:, 11:] = np.clip(z[:, 11:], -300, 300)          # (exp(800) is inf as a lognormal value: not a NaN, and not this test's business)
    for values, lp, dlp, jac in (K.torch_path(space, z), K.harness_path(harness, space, z)):
        assert not np.isnan(values).any() and not np.isnan(lp).any()
    values, lp, dlp, jac = K.harness_path(harness, space, z)
    assert not np.isnan(dlp).any() and not np.isnan(jac).any()


@pytest.mark.parametrize("case", sorted(K.ks_cases(xd)))
def test_what_is_sampled(case):
    """the reference's statistical tests on CPU NUTS through space.wrap: 64 chains, 200 warm-up steps with mass adaptation, 150
    kept steps; Kolmogorov-Smirnov distance below the reference's 0.05, every draw inside its bounds, no chain stuck"""
    from scipy.stats import kstest

    space, logp_fn, statistics, bounds, *start = K.ks_cases(xd)[case]
    theta, nuts, ok_after_warmup = K.sample(xd, space, logp_fn, D=64, seed=19910626, start=start[0] if start else None)
    assert ok_after_warmup and bool(nuts.last_adapt_ok.all())
    for k, v in theta.items():
        assert np.isfinite(v).all(), k
    for k, (lo, hi) in bounds.items():
        assert (theta[k] >= lo).all() and (theta[k] <= hi).all(), k
    for stat, cdf in statistics:
        s = kstest(stat(theta), cdf).statistic
        print(case, "KS distance %.4f" % s, "divergences", float(nuts.n_divergent.sum()))
        assert s < K.KS_BOUND


def test_abi_of_the_prior_entry_points():
    """argument checks on the host, before any launch (no GPU needed)"""
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib, ops

    lib = _lib.load()
    INVALID = 1
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    import re

    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    for name in ("NORMAL", "LOGNORMAL", "UNIFORM", "ANGLE", "UNIT_DISK", "QUAD_LIMB_DARK", "IMPACT_PARAMETER", "KIPPING13", "VANEYLEN19",
                 "KIPPING13_HYPER", "VANEYLEN19_HYPER"):
        assert int(consts["EXO_PRIOR_" + name]) == getattr(xd, name)
    assert int(consts["EXO_PRIOR_MAX_BLOCKS"]) == xd.MAX_BLOCKS and int(consts["EXO_PRIOR_MAX_OUTPUTS"]) == xd.MAX_OUTPUTS
    assert ctypes.sizeof(_lib.PriorBlock) == 6 * 4 + 8 * 8

    def table(*rows, n_free=4):
        return ops.PriorTable([dict(dict(kind=xd.UNIFORM, offset=0, count=1, link=-1, out=0, flags=0, p=(0.0, 1.0)), **r) for r in rows],
                              n_free, [1] * 8)

    outs = (ctypes.c_void_p * 48)(*([8] * 48))
    fwd = lambda t, z=8, D=10, n_free=4, n_block=None, theta=outs, lp=8: lib.exo_prior_transform_f64(  # noqa: E731
        z, D, n_free, t.blocks, t.n_block if n_block is None else n_block, theta, lp, None)
    vjp = lambda t, z=8, D=10, n_free=4, gtheta=outs, gz=8: lib.exo_prior_transform_vjp_f64(  # noqa: E731
        z, D, n_free, t.blocks, t.n_block, gtheta, None, gz, None)
    ok = table(dict(), dict(kind=xd.IMPACT_PARAMETER, offset=1, link=0, out=1), dict(kind=xd.ANGLE, offset=2, out=2))
    assert fwd(ok, D=0) == 0 and vjp(ok, D=0) == 0                                     # no chains: nothing to do
    assert fwd(ok, D=0, z=None, theta=None, lp=None) == 0
    for call in (fwd, vjp):
        assert call(ok, D=-1) == INVALID and call(ok, z=None) == INVALID and call(ok, n_free=3) == INVALID and call(ok, n_free=0) == INVALID
        assert call(table(dict(kind=11))) == INVALID and call(table(dict(kind=-1))) == INVALID            # unknown kind
        assert call(table(dict(count=0))) == INVALID and call(table(dict(offset=-1))) == INVALID
        assert call(table(dict(), dict(offset=0, out=1))) == INVALID                                         # overlapping coordinates
        assert call(table(dict(kind=xd.VANEYLEN19_HYPER, count=2))) == INVALID                              # 3 + 2 coordinates in 4 columns
        assert call(table(dict(), dict(kind=xd.IMPACT_PARAMETER, offset=1, link=1, out=1))) == INVALID      # linked to itself
        assert call(table(dict(kind=xd.IMPACT_PARAMETER, link=1, out=1), dict(offset=1))) == INVALID        # linked forward
        assert call(table(dict(kind=xd.ANGLE), dict(kind=xd.IMPACT_PARAMETER, offset=2, link=0, out=1))) == INVALID   # not a scalar block
        assert call(table(dict(count=2), dict(kind=xd.IMPACT_PARAMETER, offset=2, count=1, link=0, out=1))) == INVALID
        assert call(table(dict(offset=2 ** 31 - 1))) == INVALID and call(table(dict(kind=xd.ANGLE, count=2 ** 30), n_free=2 ** 31 - 1)) == INVALID
        assert call(table(dict(out=2 ** 31 - 1))) == INVALID
        assert call(table(dict(out=48))) == INVALID and call(table(dict(kind=xd.UNIT_DISK, out=47))) == INVALID
    assert lib.exo_prior_transform_f64(8, 10, 4, None, 1, outs, 8, None) == INVALID
    assert fwd(ok, n_block=0) == INVALID and fwd(ok, n_block=33) == INVALID
    assert fwd(ok, theta=None) == INVALID and fwd(ok, lp=None) == INVALID and vjp(ok, gtheta=None) == INVALID and vjp(ok, gz=None) == INVALID
    hole = (ctypes.c_void_p * 48)(*([8, None] + [8] * 46))
    assert fwd(ok, theta=hole) == INVALID                                               # every output is required ...
    # (... while a missing cotangent is a null pointer by design: nothing to reject there without a launch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.prior_transform(torch.zeros(3, 4, dtype=torch.float64), ok)
