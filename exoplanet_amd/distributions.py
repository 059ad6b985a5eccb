"""Priors and constrained parameters for the batched samplers (the reference's ``exoplanet.distributions`` on top of PyMC's
default interval / log transforms, restated for a batch of chains).

A :class:`ParameterSpace` is an ordered set of named blocks.  It maps ONE unconstrained array ``z (D, n_free)`` -- the flat
array `HMC` / `NUTS` integrate -- to the constrained, named parameters a model's ``logp_fn`` takes, and returns with them
the log prior density of every chain INCLUDING the log-Jacobians of the transforms, so that what is sampled in ``z`` is the
prior times the likelihood in the constrained parameters::

    space = xd.ParameterSpace(period=xd.normal(3.5, 1e-3), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              u=xd.quad_limb_dark(), ecc=xd.kipping13(), omega=xd.angle())
    z0 = space.unconstrain(D, period=3.5, r=0.1, b=0.3, u1=0.3, u2=0.2, ecc=0.1, omega=0.5)
    nuts = NUTS(space.wrap(logp), [z0], step_size=0.01)       # logp(period, r, b, u1, u2, ecc, omega) -> (D,)
    theta, log_prior = space.constrain(nuts.params[0])

Where ``z`` lives decides which code runs: on a ROCm tensor ``constrain`` is one HIP kernel forward and one in the reverse
pass (``ops.prior_transform``, csrc/exo_priors.hip); on a CPU tensor it is the same definitions as composed torch
operations, which are also reachable on any device as ``constrain_composed`` (the statement the kernels are tested and timed
against).

Definitions.  s(z) = 1 / (1 + exp(-z)); L(z) = log s(z) + log s(-z), the log-Jacobian of the unit-interval transform.

===========================  ==========  ==========================================  =============================================
block                        free        constrained value(s)                        contribution to the log prior
===========================  ==========  ==========================================  =============================================
``normal(mu, sd)``           z           x = z                                       -((x-mu)/sd)^2/2 - log sd - log(2 pi)/2
``lognormal(mu, sd)``        z           x = exp z                                   the normal log-density of z
``uniform(lo, hi)``          z           x = lo + (hi-lo) s(z)                       L(z)
``angle(regularization)``    z1, z2      theta = atan2(z1, z2)                       -(z1^2+z2^2)/2 - log 2pi + reg log(z1^2+z2^2)
``unit_disk()``              z1, z2      x = 2 s(z1) - 1, y = (2 s(z2) - 1) w        L(z1) + L(z2) + log w,  w = sqrt(1 - x^2)
                                                                                     = 2 sqrt(s(z1) s(-z1))
``quad_limb_dark()``         z1, z2      q = s(z): u1 = 2 sqrt(q1) q2,               L(z1) + L(z2)
                                         u2 = sqrt(q1) (1 - 2 q2)
``impact_parameter(ror)``    z           b = s(z) (1 + ror); ror: a block's name     L(z)
                                         or one number
``kipping13(...)``           z           e = lo + (hi-lo) s(z)                       log Beta(e; alpha, beta) - log(I_hi - I_lo)
                                                                                     + log(hi-lo) + L(z)
``vaneylen19(...)``          z           e = lo + (hi-lo) s(z)                       L(z) + logaddexp(log(1-f) + halfnormal(e; sg),
                                                                                     log f + Rayleigh(e; sr))
===========================  ==========  ==========================================  =============================================

Unbounded, the ``kipping13`` row is alpha log s(z) + beta log s(-z) - log B(alpha, beta), finite for large ``|z|``.  As in the
reference, the ``vaneylen19`` mixture is not renormalised on [lo, hi].  ``fixed=False`` adds the reference's hyperpriors as
free coordinates shared by the block's elements: normals truncated below at zero through x = exp z (log-Jacobian z) and, for
``frac``, a normal truncated to [0, 1] through the interval transform, each with its truncation constant; they come back from
``constrain`` as ``"<name>::alpha"`` etc. and are not handed to ``logp_fn``.  Every value on a closed interval is clamped to
it after rounding; no ``log`` is taken of a rounded s(z) where the ``log s`` form exists, and on a bounded interval e and
1 - e are each summed from non-negative parts.  A regularised ``angle`` at z1 = z2 = 0 has log prior -inf (the reference's
own; the samplers treat a non-finite energy as "no valid leaf").

Every distribution also has ``.logp(x)``: the plain log-density of a CONSTRAINED value as a differentiable torch expression,
for the reference's ``observed=`` use (``kipping13().logp(secosw**2 + sesinw**2)`` added inside ``logp_fn``).
"""
import math

import torch
import torch.nn.functional as F

__all__ = ["ParameterSpace", "normal", "lognormal", "uniform", "angle", "unit_disk", "quad_limb_dark", "impact_parameter",
           "kipping13", "vaneylen19"]

# include/exoplanet_amd.h EXO_PRIOR_*
NORMAL, LOGNORMAL, UNIFORM, ANGLE, UNIT_DISK, QUAD_LIMB_DARK, IMPACT_PARAMETER, KIPPING13, VANEYLEN19, KIPPING13_HYPER, \
    VANEYLEN19_HYPER = range(11)
MAX_BLOCKS, MAX_OUTPUTS = 32, 48

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_HYPER_NAMES = {KIPPING13_HYPER: ("alpha", "beta"), VANEYLEN19_HYPER: ("sigma_gauss", "sigma_rayleigh", "frac")}


# ---- host arithmetic --------------------------------------------------------------------------------------------------------

def _log_ncdf(x):
    return math.log(0.5 * math.erfc(-x / math.sqrt(2.0)))


def _log_beta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


def _betainc(a, b, x):
    """the regularised incomplete beta function I_x(a, b) by its continued fraction (modified Lentz), in the half where it
    converges fast"""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    if x > (a + 1.0) / (a + b + 2.0):
        return 1.0 - _betainc(b, a, 1.0 - x)
    tiny = 1e-300
    c, d = 1.0, 1.0 - (a + b) * x / (a + 1.0)
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 1000):
        for aa in (m * (b - m) * x / ((a + 2 * m - 1.0) * (a + 2 * m)), -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1.0))):
            d = 1.0 + aa * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + aa / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return math.exp(a * math.log(x) + b * math.log1p(-x) - _log_beta(a, b)) * h / a


def _sig(z):
    return torch.sigmoid(z), torch.sigmoid(-z), F.logsigmoid(z), F.logsigmoid(-z)


def _logit(u):
    return torch.log(u) - torch.log1p(-u)


# ---- the distributions ------------------------------------------------------------------------------------------------------

class Distribution:
    """one block of a ParameterSpace: ``count`` elements (``shape=(P,)``: one per planet) of one kind"""
    kind = None
    n_coord = 1            # free coordinates per element
    hyper = ()             # names of the shared hyperparameters (fixed=False)

    def __init__(self, shape=()):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        if len(shape) > 1 or any(int(n) < 1 for n in shape):
            raise ValueError("shape must be () or (P,)")
        self.count = int(shape[0]) if shape else 1

    def value_names(self, name):
        return (name,)

    def table_entry(self):
        """(flags, p[...]) of the block's exo_prior_block"""
        raise NotImplementedError

    def composed(self, z, ror):
        """z: list of (D, count) coordinate arrays (hyperparameters first, (D, 1) each) -> (values, log prior (D,))"""
        raise NotImplementedError

    def inverse(self, values, ror):
        raise NotImplementedError

    def logp(self, x):
        raise NotImplementedError


def _normal_logp(x, mu, sd):
    return -0.5 * ((x - mu) / sd) ** 2 - math.log(sd) - _HALF_LOG_2PI


def _inside(x, lo, hi, value):
    return torch.where((x >= lo) & (x <= hi), value, torch.full_like(value, float("-inf")))


def _density_on(x, lo, hi, fn):
    """``fn(x)`` where lo <= x <= hi and 0 < x < 1, -inf elsewhere -- with ``fn`` evaluated on the middle of the interval there, so
    that neither a NaN nor an infinite derivative of the branch that is not taken reaches the gradient (0 * inf under autograd).
    x = 0 or 1 exactly counts as outside: the densities here are 0 or infinite there, and a set of measure zero"""
    ok = (x >= lo) & (x <= hi) & (x > 0.0) & (x < 1.0)
    value = fn(torch.where(ok, x, torch.full_like(x, 0.5 * (lo + hi))))
    return torch.where(ok, value, torch.full_like(value, float("-inf")))


class _Normal(Distribution):
    kind = NORMAL

    def __init__(self, mu, sd, shape=()):
        super().__init__(shape)
        self.mu, self.sd = float(mu), float(sd)
        if not self.sd > 0:
            raise ValueError("need sd > 0")

    def table_entry(self):
        return 0, (self.mu, self.sd)

    def composed(self, z, ror):
        return [z[0]], _normal_logp(z[0], self.mu, self.sd).sum(1)

    def inverse(self, values, ror):
        return [values[0]]

    def logp(self, x):
        return _normal_logp(x, self.mu, self.sd)


class _LogNormal(_Normal):
    kind = LOGNORMAL

    def composed(self, z, ror):
        return [torch.exp(z[0])], _normal_logp(z[0], self.mu, self.sd).sum(1)

    def inverse(self, values, ror):
        if not bool((values[0] > 0).all()):
            raise ValueError("a lognormal value must be positive")
        return [torch.log(values[0])]

    def logp(self, x):
        ok = x > 0
        v = torch.where(ok, x, torch.ones_like(x))
        return torch.where(ok, _normal_logp(torch.log(v), self.mu, self.sd) - torch.log(v), torch.full_like(x, float("-inf")))


def _interval(z, lo, hi):
    """x = lo + (hi - lo) s(z) on the closed interval, and L(z)"""
    s, _, ls, lsm = _sig(z)
    return torch.clamp(lo + (hi - lo) * s, lo, hi), ls + lsm


def _interval_inverse(x, lo, hi, what):
    if not bool(((x > lo) & (x < hi)).all()):
        raise ValueError(f"{what} must lie inside ({lo}, {hi})")
    return _logit((x - lo) / (hi - lo))


class _Uniform(Distribution):
    kind = UNIFORM

    def __init__(self, lo, hi, shape=()):
        super().__init__(shape)
        self.lo, self.hi = float(lo), float(hi)
        if not self.hi > self.lo:
            raise ValueError("need hi > lo")

    def table_entry(self):
        return 0, (self.lo, self.hi)

    def composed(self, z, ror):
        x, L = _interval(z[0], self.lo, self.hi)
        return [x], L.sum(1)

    def inverse(self, values, ror):
        return [_interval_inverse(values[0], self.lo, self.hi, "a uniform value")]

    def logp(self, x):
        return _inside(x, self.lo, self.hi, torch.full_like(x, -math.log(self.hi - self.lo)))


class _Angle(Distribution):
    kind = ANGLE
    n_coord = 2

    def __init__(self, regularization=10.0, shape=()):
        super().__init__(shape)
        self.reg = None if regularization is None else float(regularization)

    def table_entry(self):
        return (0, (0.0,)) if self.reg is None else (1, (self.reg,))

    def composed(self, z, ror):
        z1, z2 = z
        r2 = z1 * z1 + z2 * z2
        lp = -0.5 * r2 - math.log(2.0 * math.pi)
        if self.reg is not None:
            lp = lp + self.reg * torch.log(r2)
        return [torch.atan2(z1, z2)], lp.sum(1)

    def inverse(self, values, ror):
        return [torch.sin(values[0]), torch.cos(values[0])]

    def logp(self, x):
        return torch.full_like(x, -math.log(2.0 * math.pi))


class _UnitDisk(Distribution):
    kind = UNIT_DISK
    n_coord = 2

    def __init__(self, names=("x", "y"), shape=()):
        super().__init__(shape)
        self.names = tuple(names)

    def value_names(self, name):
        return self.names

    def table_entry(self):
        return 0, ()

    def composed(self, z, ror):
        s1, s1m, ls1, ls1m = _sig(z[0])
        s2, s2m, ls2, ls2m = _sig(z[1])
        w = 2.0 * torch.sqrt(s1 * s1m)
        L1 = ls1 + ls1m
        # after rounding (csrc/exo_priors_core.hpp, disk_ymax): x 2^-49 towards zero, |y| capped at what passes x * x + y * y <= 1 in fp64
        x = (s1 - s1m) * (1.0 - 2.0 ** -49)
        ymax = torch.sqrt(torch.clamp(1.0 - x * x, min=0.0) + 2.0 ** -54) * (1.0 - 2.0 ** -51)
        return [x, torch.maximum(torch.minimum((s2 - s2m) * w, ymax), -ymax)], (L1 + (ls2 + ls2m) + (math.log(2.0) + 0.5 * L1)).sum(1)

    def inverse(self, values, ror):
        x, y = values
        if not bool((x * x + y * y < 1).all()):
            raise ValueError("a unit_disk point must lie inside the unit circle")
        return [_logit(0.5 * (x + 1.0)), _logit(0.5 * (y / torch.sqrt((1.0 - x) * (1.0 + x)) + 1.0))]

    def logp(self, x, y):
        return _inside(x * x + y * y, 0.0, 1.0, torch.full_like(x, -math.log(math.pi)))


class _QuadLimbDark(Distribution):
    kind = QUAD_LIMB_DARK
    n_coord = 2

    def value_names(self, name):
        return (name + "1", name + "2")

    def table_entry(self):
        return 0, ()

    def composed(self, z, ror):
        s1, _, ls1, ls1m = _sig(z[0])
        s2, s2m, ls2, ls2m = _sig(z[1])
        sq = torch.sqrt(s1)
        u1 = 2.0 * sq * s2
        # (the triangle's edges u1 + 2 u2 >= 0 and u1 + u2 <= 1, after rounding)
        return [u1, torch.maximum(torch.minimum(sq * (s2m - s2), 1.0 - u1), -0.5 * u1)], ((ls1 + ls1m) + (ls2 + ls2m)).sum(1)

    def inverse(self, values, ror):
        u1, u2 = values
        q1, q2 = (u1 + u2) ** 2, 0.5 * u1 / (u1 + u2)
        return [_interval_inverse(q1, 0.0, 1.0, "(u1 + u2)^2"), _interval_inverse(q2, 0.0, 1.0, "u1 / (2 (u1 + u2))")]

    def logp(self, u1, u2):
        """uniform over Kipping's triangle u1 >= 0, u1 + u2 <= 1, u1 + 2 u2 >= 0 (its area is 1)"""
        ok = (u1 >= 0) & (u1 + u2 <= 1) & (u1 + 2 * u2 >= 0)
        return torch.where(ok, torch.zeros_like(u1), torch.full_like(u1, float("-inf")))


class _ImpactParameter(Distribution):
    kind = IMPACT_PARAMETER

    def __init__(self, ror, shape=()):
        super().__init__(shape)
        if torch.is_tensor(ror):
            if ror.numel() != 1:
                raise NotImplementedError("impact_parameter: ror is a block's name or ONE number; a radius ratio per planet or "
                                          "per chain is a block of its own (uniform, lognormal, ...) named here")
            ror = float(ror)
        self.ror = ror if isinstance(ror, str) else float(ror)

    def table_entry(self):
        return 0, (0.0 if isinstance(self.ror, str) else self.ror,)

    def composed(self, z, ror):
        s, _, ls, lsm = _sig(z[0])
        return [s * (1.0 + ror)], (ls + lsm).sum(1)

    def inverse(self, values, ror):
        b = values[0]
        if not bool(((b > 0) & (b < 1.0 + ror)).all()):
            raise ValueError("an impact parameter must lie inside (0, 1 + ror)")
        return [_logit(b / (1.0 + ror))]

    def logp(self, b, ror=None):
        ror = self.ror if ror is None else ror
        if isinstance(ror, str):
            raise ValueError("pass ror= (this block takes it from the block named %r)" % ror)
        top = 1.0 + ror
        return _inside(b, 0.0, top, torch.zeros_like(b) - (torch.log(top) if torch.is_tensor(top) else math.log(top)))


def _bounds(lower, upper):
    bounded = lower is not None or upper is not None
    lo, hi = 0.0 if lower is None else float(lower), 1.0 if upper is None else float(upper)
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError("need 0 <= lower < upper <= 1")
    return bounded, lo, hi


def _positive_hyper(z, mu, sd):
    """x = exp z under a normal(mu, sd) truncated below at zero: (x, log prior with the log-Jacobian z)"""
    x = torch.exp(z)
    return x, (_normal_logp(x, mu, sd) - _log_ncdf(mu / sd) + z).sum(1)


class _Kipping13(Distribution):
    def __init__(self, fixed=True, long=None, lower=None, upper=None, shape=()):
        super().__init__(shape)
        # Kipping (2013b): the fit to the full sample / the long-period half, and the short-period half
        self.alpha_mu, self.alpha_sd, self.beta_mu, self.beta_sd = (0.697, 0.4, 3.27, 0.3) if long is False else (1.12, 0.1, 3.09, 0.3)
        self.fixed = bool(fixed)
        self.bounded, self.lo, self.hi = _bounds(lower, upper)
        if not self.fixed and self.bounded:
            raise NotImplementedError("kipping13(fixed=False) with bounds needs the derivatives of the incomplete beta function in "
                                      "its parameters, which are not implemented: bound the prior or marginalise over it, not both")
        self.kind = KIPPING13 if self.fixed else KIPPING13_HYPER
        self.hyper = () if self.fixed else _HYPER_NAMES[KIPPING13_HYPER]
        a, b = self.alpha_mu, self.beta_mu
        self.const = -_log_beta(a, b)
        if self.bounded:
            self.const += math.log(self.hi - self.lo) - math.log(_betainc(a, b, self.hi) - _betainc(a, b, self.lo))

    def table_entry(self):
        if self.fixed:
            return int(self.bounded), (self.alpha_mu, self.beta_mu, self.lo, self.hi, self.const)
        return 0, (self.alpha_mu, self.alpha_sd, self.beta_mu, self.beta_sd)

    def _ecc(self, z, a, b):
        s, sm, ls, lsm = _sig(z)
        if not self.bounded:
            return s, a * ls + b * lsm
        w = self.hi - self.lo
        e, em = self.lo + w * s, (1.0 - self.hi) + w * sm
        return torch.clamp(e, self.lo, self.hi), (a - 1.0) * torch.log(e) + (b - 1.0) * torch.log(em) + (ls + lsm)

    def composed(self, z, ror):
        if self.fixed:
            e, lp = self._ecc(z[0], self.alpha_mu, self.beta_mu)
            return [e], (lp + self.const).sum(1)
        a, lpa = _positive_hyper(z[0], self.alpha_mu, self.alpha_sd)
        b, lpb = _positive_hyper(z[1], self.beta_mu, self.beta_sd)
        e, lp = self._ecc(z[2], a, b)
        return [e, a, b], (lp - (torch.lgamma(a) + torch.lgamma(b) - torch.lgamma(a + b))).sum(1) + lpa + lpb

    def hyper_start(self):
        return [math.log(self.alpha_mu), math.log(self.beta_mu)]

    def inverse(self, values, ror):
        return [_interval_inverse(values[0], self.lo, self.hi, "an eccentricity")]

    def logp(self, x):
        if not self.fixed:
            raise NotImplementedError("logp of an observed value needs fixed hyperparameters")
        a, b = self.alpha_mu, self.beta_mu
        const = self.const - (math.log(self.hi - self.lo) if self.bounded else 0.0)
        return _density_on(x, self.lo, self.hi, lambda v: (a - 1.0) * torch.log(v) + (b - 1.0) * torch.log1p(-v) + const)


class _VanEylen19(Distribution):
    def __init__(self, fixed=True, multi=False, lower=None, upper=None, shape=()):
        super().__init__(shape)
        # Van Eylen et al. (2019): widths of the half-normal and the Rayleigh component, weight of the latter
        self.mu = (0.049, 0.26, 0.08 if multi else 0.76)
        self.sd = (0.02, 0.05, 0.08 if multi else 0.2)
        self.fixed = bool(fixed)
        self.bounded, self.lo, self.hi = _bounds(lower, upper)
        self.kind = VANEYLEN19 if self.fixed else VANEYLEN19_HYPER
        self.hyper = () if self.fixed else _HYPER_NAMES[VANEYLEN19_HYPER]

    def table_entry(self):
        if self.fixed:
            return 0, (*self.mu, self.lo, self.hi)
        return 0, (self.mu[0], self.sd[0], self.mu[1], self.sd[1], self.mu[2], self.sd[2], self.lo, self.hi)

    @staticmethod
    def _mixture(e, loge, sg, sr, log1mf, logf):
        # (fixed hyperparameters are Python numbers: no tensor is made of them -- that would be a host-to-device copy per call)
        log = lambda v: torch.log(v) if torch.is_tensor(v) else math.log(v)  # noqa: E731
        ga = log1mf + 0.5 * math.log(2.0 / math.pi) - log(sg) - 0.5 * e * e / (sg * sg)
        ra = logf + loge - 2.0 * log(sr) - 0.5 * e * e / (sr * sr)
        return torch.logaddexp(ga, ra)

    def _ecc(self, z, sg, sr, log1mf, logf):
        s, _, ls, lsm = _sig(z)
        w = self.hi - self.lo
        e = self.lo + w * s
        loge = math.log(w) + ls if self.lo == 0.0 else torch.log(e)
        return torch.clamp(e, self.lo, self.hi), (ls + lsm) + self._mixture(e, loge, sg, sr, log1mf, logf)

    def composed(self, z, ror):
        if self.fixed:
            sg, sr, f = self.mu
            e, lp = self._ecc(z[0], sg, sr, math.log1p(-f), math.log(f))
            return [e], lp.sum(1)
        sg, lpg = _positive_hyper(z[0], self.mu[0], self.sd[0])
        sr, lpr = _positive_hyper(z[1], self.mu[1], self.sd[1])
        f, _, lf, l1mf = _sig(z[2])
        mu, sd = self.mu[2], self.sd[2]
        mass = 0.5 * (math.erfc(-(1.0 - mu) / sd / math.sqrt(2.0)) - math.erfc(mu / sd / math.sqrt(2.0)))
        lpf = (_normal_logp(f, mu, sd) - math.log(mass) + (lf + l1mf)).sum(1)
        e, lp = self._ecc(z[3], sg, sr, l1mf, lf)
        return [e, sg, sr, f], lp.sum(1) + lpg + lpr + lpf

    def hyper_start(self):
        return [math.log(self.mu[0]), math.log(self.mu[1]), math.log(self.mu[2]) - math.log1p(-self.mu[2])]

    def inverse(self, values, ror):
        return [_interval_inverse(values[0], self.lo, self.hi, "an eccentricity")]

    def logp(self, x):
        if not self.fixed:
            raise NotImplementedError("logp of an observed value needs fixed hyperparameters")
        sg, sr, f = self.mu
        const = math.log(self.hi - self.lo)
        return _density_on(x, self.lo, self.hi, lambda v: self._mixture(v, torch.log(v), sg, sr, math.log1p(-f), math.log(f)) - const)


def normal(mu, sd, shape=()):
    return _Normal(mu, sd, shape)


def lognormal(mu, sd, shape=()):
    """x = exp z with z ~ normal(mu, sd)"""
    return _LogNormal(mu, sd, shape)


def uniform(lo, hi, shape=()):
    return _Uniform(lo, hi, shape)


def angle(regularization=10.0, shape=()):
    """an angle in (-pi, pi] without a boundary: two normal coordinates, theta = atan2(z1, z2); ``regularization`` keeps the
    sampler away from the origin, where the angle is not defined, without changing the distribution of theta"""
    return _Angle(regularization, shape)


def unit_disk(names=("x", "y"), shape=()):
    """two parameters, named ``names``, uniform over the unit disk x^2 + y^2 <= 1"""
    return _UnitDisk(names, shape)


def quad_limb_dark(shape=()):
    """quadratic limb-darkening coefficients ``<name>1``, ``<name>2``, uniform over the physical triangle (Kipping 2013a)"""
    return _QuadLimbDark(shape)


def impact_parameter(ror, shape=()):
    """b uniform on [0, 1 + ror]; ``ror``: the name of an earlier normal / lognormal / uniform block (of ``shape`` or of one
    element), or ONE number (a one-element tensor counts as a number; a radius ratio per planet or per chain is a block)"""
    return _ImpactParameter(ror, shape)


def kipping13(fixed=True, long=None, lower=None, upper=None, shape=()):
    """the Beta distribution Kipping (2013b) fitted to the eccentricities of radial-velocity planets"""
    return _Kipping13(fixed, long, lower, upper, shape)


def vaneylen19(fixed=True, multi=False, lower=None, upper=None, shape=()):
    """the half-normal + Rayleigh mixture Van Eylen et al. (2019) fitted to small transiting planets"""
    return _VanEylen19(fixed, multi, lower, upper, shape)


# ---- the space --------------------------------------------------------------------------------------------------------------

class ParameterSpace:
    """``ParameterSpace(name=distribution, ..., device=None)``: the blocks in the order given.

    ``names``: the constrained parameters handed to ``logp_fn`` by keyword, in order; ``n_free``: columns of ``z``.
    """

    def __init__(self, device=None, **blocks):
        if not blocks:
            raise ValueError("a ParameterSpace needs at least one block")
        if len(blocks) > MAX_BLOCKS:
            raise ValueError(f"at most {MAX_BLOCKS} blocks")
        self.device = None if device is None else torch.device(device)
        self.blocks = []          # (name, distribution, offset, first output, index of the linked block or -1)
        self.names, self.outputs = [], []     # outputs: (name, columns) of every array constrain returns
        index, offset = {}, 0
        for name, dist in blocks.items():
            if not isinstance(dist, Distribution):
                raise TypeError(f"{name}: not a distribution")
            link = -1
            if dist.kind == IMPACT_PARAMETER and isinstance(dist.ror, str):
                if dist.ror not in index:
                    raise ValueError(f"{name}: ror names the block {dist.ror!r}, which must come earlier in the space")
                link = index[dist.ror]
                target = self.blocks[link][1]
                if target.kind not in (NORMAL, LOGNORMAL, UNIFORM) or target.count not in (1, dist.count):
                    raise ValueError(f"{name}: ror must name a normal, lognormal or uniform block of {dist.count} element(s) or one")
            index[name] = len(self.blocks)
            self.blocks.append((name, dist, offset, len(self.outputs), link))
            values = dist.value_names(name)
            self.names += values
            self.outputs += [(v, dist.count) for v in values] + [(f"{name}::{h}", 1) for h in dist.hyper]
            offset += len(dist.hyper) + dist.n_coord * dist.count
        self.n_free = offset
        keys = [k for k, _ in self.outputs]
        if len(set(keys)) != len(keys):
            raise ValueError("two parameters of one name: %s" % sorted(k for k in set(keys) if keys.count(k) > 1))
        if len(self.outputs) > MAX_OUTPUTS:
            raise ValueError(f"at most {MAX_OUTPUTS} parameter arrays")
        self._table = None

    # -- the table of the kernels
    def table(self):
        """the space as ``ops.PriorTable`` (the exo_prior_block array of include/exoplanet_amd.h)"""
        if self._table is None:
            from . import ops

            rows = []
            for _, dist, offset, out, link in self.blocks:
                flags, p = dist.table_entry()
                rows.append(dict(kind=dist.kind, offset=offset, count=dist.count, link=link, out=out, flags=flags, p=p))
            self._table = ops.PriorTable(rows, self.n_free, [c for _, c in self.outputs])
        return self._table

    def _check(self, z):
        if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != self.n_free or z.dtype != torch.float64:
            raise ValueError(f"z must be a float64 tensor of shape (D, {self.n_free})")

    def _split(self, z, dist, offset):
        cols, at = [], offset
        for _ in dist.hyper:
            cols.append(z[:, at:at + 1])
            at += 1
        for _ in range(dist.n_coord):
            cols.append(z[:, at:at + dist.count])
            at += dist.count
        return cols

    def constrain_composed(self, z):
        """``constrain`` as composed torch operations, on any device: the statement of the definitions"""
        self._check(z)
        theta, values, log_prior = {}, [], 0.0
        for name, dist, offset, out, link in self.blocks:
            ror = values[self.blocks[link][3]] if link >= 0 else getattr(dist, "ror", None)
            vals, lp = dist.composed(self._split(z, dist, offset), ror)
            values += vals
            log_prior = log_prior + lp
        for (key, _), v in zip(self.outputs, values):
            theta[key] = v
        return theta, log_prior

    def constrain(self, z):
        """z (D, n_free) -> ({name: (D, count) tensor}, log prior (D,)), differentiable.  On a ROCm tensor: one kernel each way."""
        self._check(z)
        if not z.is_cuda:
            return self.constrain_composed(z)
        from . import ops

        log_prior, *values = ops.prior_transform(z, self.table())
        return {key: v for (key, _), v in zip(self.outputs, values)}, log_prior

    def wrap(self, logp_fn):
        """``z -> logp_fn(**theta) + log prior``: what `HMC` / `NUTS` take, with ``[z0]`` as their parameters"""
        names = list(self.names)

        def logp(z):
            theta, log_prior = self.constrain(z)
            return logp_fn(**{k: theta[k] for k in names}) + log_prior

        return logp

    def free_mask(self, names):
        """(n_free,) mask, 1 in the columns of the named BLOCKS (their hyperparameters' columns included) and 0 elsewhere: the
        ``free=[...]`` of `optimize` / `LBFGS`, what ``vars=`` is to the reference's ``pmx.optimize``"""
        names = [names] if isinstance(names, str) else list(names)
        mask = torch.zeros(self.n_free, dtype=torch.float64, device=self.device)
        ends = [b[2] for b in self.blocks[1:]] + [self.n_free]
        spans = {b[0]: (b[2], end) for b, end in zip(self.blocks, ends)}
        for name in names:
            if name not in spans:
                owner = [b[0] for b in self.blocks if name in b[1].value_names(b[0]) or str(name).startswith(b[0] + "::")]
                raise ValueError(f"{name!r} is a value of the block {owner[0]!r}: a mask names whole blocks" if owner else
                                 f"no block named {name!r} (blocks: {[b[0] for b in self.blocks]})")
            mask[spans[name][0]:spans[name][1]] = 1.0
        return mask

    def unconstrain(self, D, **values):
        """starting points: the constrained ``values`` (numbers, or tensors of shape (count,), (D,), (D, 1), (1, count) or (D, count);
        a 1-D value is one per element when its length is ``count``, one per chain when it is D, and refused when D == count) of every
        name in ``names`` -> z (D, n_free).  Hyperparameters (``**{"ecc::alpha": ...}``) default to their priors' centres.
        A value outside its support raises ``ValueError``."""
        D = int(D)
        device = self.device if self.device is not None else next(
            (v.device for v in values.values() if torch.is_tensor(v)), torch.device("cpu"))
        known = set(self.names) | {k for k, _ in self.outputs}
        if set(values) - known or set(self.names) - set(values):
            raise ValueError("unconstrain needs a value for each of %s (got %s)" % (self.names, sorted(values)))

        def expand(v, count):
            v = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
            if v.dim() == 1 and count == D and D > 1 and v.numel() == D:
                raise ValueError(f"a 1-D value of length {D} could be one per chain or one per element here (D == count): "
                                 f"pass it as (D, 1) or (1, {count})")
            if v.dim() == 1:
                v = v.reshape(1, count) if (v.numel() == count and count != D) or D == 1 else v.reshape(D, 1)
            return v.expand(D, count).clone() if v.dim() else v.reshape(1, 1).expand(D, count).clone()

        cols, given = [], {}
        for name, dist, offset, out, link in self.blocks:
            vals = [expand(values[k], dist.count) for k in dist.value_names(name)]
            ror = given[self.blocks[link][0]] if link >= 0 else getattr(dist, "ror", None)
            given[name] = vals[0]
            if dist.hyper:
                start = dist.hyper_start()
                for h, z_h in zip(dist.hyper, start):
                    key = f"{name}::{h}"
                    if key in values:
                        x = expand(values[key], 1)
                        if h == "frac":
                            z_col = _interval_inverse(x, 0.0, 1.0, key)
                        else:
                            if not bool((x > 0).all()):
                                raise ValueError(f"{key} must be positive")
                            z_col = torch.log(x)
                    else:
                        z_col = torch.full((D, 1), z_h, dtype=torch.float64)
                    cols.append(z_col)
            cols += dist.inverse(vals, ror)
        z = torch.cat(cols, dim=1)
        if not bool(torch.isfinite(z).all()):
            raise ValueError("a starting value lies on the edge of its support")
        return z.to(device).contiguous()
