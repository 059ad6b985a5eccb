"""The Laplace approximation at the chains' modes: the step between `optimize` and `sample`.

`optimize` brings every chain to a posterior mode and says nothing about the shape of the posterior there.  `laplace`
computes, per chain, the Hessian of ``f = -logp`` at the chain's position by central differences of the batched gradient --
the ``2 m`` (order 2) or ``4 m`` (order 4) perturbed points of all D chains are ``order m D`` more rows of the draw dimension
of the value + gradient kernels; no likelihood here is twice differentiable through autograd --, and from it the covariance
``H^-1``, the marginal standard deviations, ``log det H`` and the Laplace log-evidence ``logp + (m / 2) log(2 pi) - (1 / 2) log
det H``, with two quality numbers: the asymmetry of the raw difference matrix and, at order 4, the difference between the
``h`` and the ``2 h`` stencil.  The covariance is what ``NUTS(cov=, center=)`` / ``set_metric`` take (`Laplace.metric`);
Gaussian draws (`Laplace.draws`) are rows for ``space.constrain``, `predictive.bands` and `comparison.loo`: error bars
without a sampler; `Laplace.importance` says whether the Gaussian can be trusted (Pareto k of the ratios posterior /
Gaussian, from the PSIS kernel of `comparison`).

Definition: DESIGN.md section 28; the numpy statement is tests/laplace_oracle.py.  This module carries the TORCH STATEMENT
(`_points_torch`, `_factor_torch`): it is what runs for CPU tensors and with ``native=False``.  For ROCm tensors the two
steps are the kernels of csrc/exo_laplace.hip.

Out of scope: a metric per chain in the samplers, more than 64 free coordinates, second derivatives
in the kernels themselves."""
import math

import torch

from .sampling import METRIC_FORWARD, _ChainSampler, _metric_apply_torch

__all__ = ["laplace", "Laplace", "MAX_N", "DEFAULT_DELTA"]

MAX_N = 64                                                  # EXO_LAPLACE_MAX_N of include/exoplanet_amd.h
STATUS_OK, STATUS_NOT_FINITE, STATUS_NOT_POSITIVE = 0, 1, 2    # EXO_LAPLACE_STATUS_*
EPS = 2.220446049250313e-16
CBRT_EPS = 6.0554544523933395e-06                           # EPS ** (1 / 3)
# the final pass's step in units of the posterior's own scale 1 / sqrt(H_kk), per order (the sweeps)
DEFAULT_DELTA = {2: 1e-4, 4: 1e-3}
HIGH_K = 0.7


# ---- the torch statement ---------------------------------------------------------------------------------------------------------
def _steps_torch(x, free_index, scale, hess, delta):
    xf = x[:, free_index]
    sc = torch.clamp(xf.abs(), min=1.0) if scale is None else scale.expand_as(x)[:, free_index]
    h = CBRT_EPS * sc
    if hess is not None:
        hkk = torch.diagonal(hess, dim1=1, dim2=2)
        good = torch.isfinite(hkk) & (hkk > 0)
        # (a tensor over a tensor: a Python number over a tensor is a reciprocal and a product, two roundings)
        hf = torch.full_like(hkk, delta) / torch.sqrt(torch.where(good, hkk, torch.ones_like(hkk)))
        good = good & torch.isfinite(hf) & (hf > 0)
        h = torch.where(good, hf, h)
    return h


def _points_torch(x, free_index, scale, hess, delta, order):
    """(points (D, order m, n), dx (D, order m)): row s m + k moves coordinate free_index[k] by +h, -h, +2h, -2h"""
    D, n = x.shape
    m = int(free_index.shape[0])
    h = _steps_torch(x, free_index, scale, hess, delta)
    off = torch.cat([h, -h, 2.0 * h, -(2.0 * h)][:order], dim=1)               # (D, order m)
    col = free_index.repeat(order)                                             # the moved coordinate of every row
    pts = x[:, None, :].repeat(1, order * m, 1)
    r = torch.arange(order * m, device=x.device)
    xf = x[:, col]
    p = xf + off
    pts[:, r, col] = p
    return pts, p - xf


def _factor_torch(grad, dx, logp, free_index, order):
    """the outputs of the factor kernel, all chains at once (a dict; "status" int32)"""
    D = grad.shape[0]
    m = int(free_index.shape[0])
    g = grad[:, :, free_index]                                                  # (D, order m, m): row r, free coordinate i
    nan = torch.full((), float("nan"), dtype=grad.dtype, device=grad.device)

    def raw(s):
        den = dx[:, s * m:(s + 1) * m] - dx[:, (s + 1) * m:(s + 2) * m]
        A = -(g[:, s * m:(s + 1) * m] - g[:, (s + 1) * m:(s + 2) * m]) / den[:, :, None]    # [d][k][i]
        return A.transpose(1, 2), den

    A1, den = raw(0)
    bad = ~torch.isfinite(g).reshape(D, -1).all(1) | ~torch.isfinite(dx).all(1) | (den == 0).any(1)
    A = A1
    if order == 4:
        A2, den2 = raw(2)
        bad = bad | (den2 == 0).any(1)
        A = (4.0 * A1 - A2) / 3.0
    H = 0.5 * (A + A.transpose(1, 2))
    hd = torch.diagonal(H, dim1=1, dim2=2)
    scale = torch.sqrt((hd[:, :, None] * hd[:, None, :]).abs())
    low = torch.tril(torch.ones(m, m, dtype=torch.bool, device=grad.device), -1)
    zero = torch.zeros((), dtype=grad.dtype, device=grad.device)

    def worst(values, where):
        v = torch.where(where & ~torch.isnan(values), values, zero)
        return v.reshape(D, -1).amax(1)

    out = {"hess": H, "asymmetry": worst((A - A.transpose(1, 2)).abs() / scale, low)}
    if order == 4:
        H1, H2 = 0.5 * (A1 + A1.transpose(1, 2)), 0.5 * (A2 + A2.transpose(1, 2))
        out["fd_error"] = worst((H1 - H2).abs() / scale, low | torch.eye(m, dtype=torch.bool, device=grad.device))
    else:
        out["fd_error"] = nan.expand(D).clone()
    bad = bad | ~torch.isfinite(hd).all(1)
    neg = ~bad & (hd <= 0).any(1)
    go = ~bad & ~neg
    eye = torch.eye(m, dtype=grad.dtype, device=grad.device)
    s = 1.0 / torch.sqrt(torch.where(go[:, None], hd, torch.ones_like(hd)))
    C = torch.where(go[:, None, None], s[:, :, None] * H * s[:, None, :], eye)
    C = C - torch.diag_embed(torch.diagonal(C, dim1=1, dim2=2)) + eye          # the unit diagonal, exactly
    R, info = torch.linalg.cholesky_ex(C)
    pivots = torch.diagonal(R, dim1=1, dim2=2) ** 2
    fell = go & ((info != 0) | ~(pivots > m * EPS).all(1))
    ok = go & ~fell
    R = torch.where(ok[:, None, None], R, eye)
    T = torch.linalg.solve_triangular(R, eye.expand(D, m, m), upper=False)
    cov = s[:, :, None] * s[:, None, :] * (T.transpose(1, 2) @ T)
    cov = 0.5 * (cov + cov.transpose(1, 2))
    logdet = torch.log(torch.where(ok[:, None], hd, torch.ones_like(hd))).sum(1) \
        + 2.0 * torch.log(torch.diagonal(R, dim1=1, dim2=2)).sum(1)
    out["cov"] = torch.where(ok[:, None, None], cov, nan)
    out["sd"] = torch.where(ok[:, None], torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)), nan)
    out["logdet"] = torch.where(ok, logdet, nan)
    out["log_evidence"] = torch.where(ok, (logp + 0.5 * m * math.log(2.0 * math.pi)) - 0.5 * logdet, nan)
    out["status"] = torch.where(bad, STATUS_NOT_FINITE, torch.where(ok, STATUS_OK, STATUS_NOT_POSITIVE)).to(torch.int32)
    return out


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def _points_native(x, free_index, scale, hess, delta, order, points, dx):
    from . import _lib

    D, n = x.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().exo_laplace_points_f64(
            x.data_ptr(), D, n, free_index.data_ptr(), int(free_index.shape[0]), None if scale is None else scale.data_ptr(),
            int(scale is not None and scale.dim() == 2), None if hess is None else hess.data_ptr(), float(delta), order,
            points.data_ptr(), dx.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream), "exo_laplace_points_f64")


def _factor_native(grad, dx, logp, free_index, order, out):
    from . import _lib

    D, _, n = grad.shape
    with torch.cuda.device(grad.device):
        _lib.check(_lib.load().exo_laplace_factor_f64(
            grad.data_ptr(), dx.data_ptr(), logp.data_ptr(), D, n, free_index.data_ptr(), int(free_index.shape[0]), order,
            *(out[k].data_ptr() for k in ("hess", "cov", "sd", "logdet", "log_evidence", "asymmetry", "fd_error", "status")),
            torch.cuda.current_stream(grad.device).cuda_stream), "exo_laplace_factor_f64")


class _Rows:
    """value + gradient of ``logp_fn`` over any number of flat rows: `_ChainSampler._value_and_grad_flat` with the rows of a
    chunk in the chains' place"""

    _flat, _parts, _value_and_grad_flat = _ChainSampler._flat, _ChainSampler._parts, _ChainSampler._value_and_grad_flat

    def __init__(self, logp_fn, params):
        self.logp_fn = logp_fn
        self._tails = [tuple(p.shape[1:]) for p in params]
        self._sizes = [int(p[0].numel()) for p in params]

    def _over(self, rows):
        self.D = int(rows.shape[0])
        self._shapes = [(self.D,) + tail for tail in self._tails]

    def value_and_grad(self, rows, logp_out, grad_out, chunk):
        """logp (S,) and its gradient (S, n) of the flat rows (S, n), ``chunk`` rows per call of logp_fn"""
        for lo in range(0, int(rows.shape[0]), chunk):
            part = rows[lo:lo + chunk]
            self._over(part)
            lp, _ = self._value_and_grad_flat(part, grad_out=grad_out[lo:lo + chunk])
            if logp_out is not None:
                logp_out[lo:lo + chunk].copy_(lp)

    def value(self, rows, chunk):
        out = torch.empty(int(rows.shape[0]), dtype=rows.dtype, device=rows.device)
        with torch.no_grad():
            for lo in range(0, int(rows.shape[0]), chunk):
                part = rows[lo:lo + chunk]
                self._over(part)
                out[lo:lo + chunk].copy_(self.logp_fn(*self._parts(part)))
        return out


class Laplace:
    """The result of `laplace`.  Device tensors: ``center`` (D, n) -- the positions, all blocks of a chain side by side --,
    ``logp`` (D), ``hess`` and ``cov`` (D, m, m) over the free coordinates ``free_index`` (m, int32), ``sd`` (D, m), ``logdet``,
    ``log_evidence``, ``asymmetry``, ``fd_error`` (D; NaN at order 2), ``status`` (D, int32: 0 ok, 1 a non-finite gradient or a
    step lost to rounding, 2 the Hessian is not positive definite: ``cov``, ``sd``, ``logdet`` and ``log_evidence`` of that chain
    are NaN) and ``n_eval`` (D, int32: the rows evaluated per chain)."""

    def __init__(self, rows, fields, free_index, order, delta):
        self._rows = rows
        self.free_index, self.order, self.delta = free_index, order, delta
        for key, value in fields.items():
            setattr(self, key, value)

    def best(self):
        """the index of the ok chain with the largest logp"""
        ok = (self.status == STATUS_OK) & torch.isfinite(self.logp)
        if not bool(ok.any()):
            raise ValueError("no chain has a Laplace approximation (status)")
        return int(torch.argmax(torch.where(ok, self.logp, torch.full_like(self.logp, float("-inf")))))

    def _chain(self, chain, need_all):
        chain = self.best() if chain is None else int(chain)
        n, m = int(self.center.shape[1]), int(self.free_index.shape[0])
        if need_all and m < n:
            raise ValueError(f"{n - m} of {n} coordinates were held: a held coordinate has no variance to give to a metric")
        if int(self.status[chain]) != STATUS_OK:
            raise ValueError(f"chain {chain} has no Laplace approximation (status {int(self.status[chain])}): no variance to give")
        return chain

    def metric(self, chain=None):
        """(cov (n, n), center (n,)) of one chain (default: `best`) for ``NUTS(cov=, center=)`` / ``set_metric``; every coordinate
        must be free and the chain's status ok"""
        chain = self._chain(chain, True)
        return self.cov[chain].clone(), self.center[chain].clone()

    def _gaussian(self, n_draws, chain, generator):
        chain = self._chain(chain, False)
        m = int(self.free_index.shape[0])
        cov, center = self.cov[chain], self.center[chain]
        L = torch.linalg.cholesky(cov)
        xi = torch.randn((int(n_draws), m), dtype=cov.dtype, device=cov.device, generator=generator)
        mean = center[self.free_index.long()].contiguous()
        if cov.is_cuda:
            from . import _lib

            moved = torch.empty_like(xi)
            with torch.cuda.device(cov.device):
                _lib.check(_lib.load().exo_metric_apply_f64(L.data_ptr(), mean.data_ptr(), xi.data_ptr(), moved.data_ptr(),
                                                            int(n_draws), m, METRIC_FORWARD,
                                                            torch.cuda.current_stream(cov.device).cuda_stream), "exo_metric_apply_f64")
        else:
            moved = _metric_apply_torch(L, mean, xi, METRIC_FORWARD)
        rows = center.expand(int(n_draws), -1).clone()
        rows[:, self.free_index.long()] = moved
        return rows, xi, L

    def draws(self, n_draws, chain=None, generator=None):
        """(n_draws, n) unconstrained rows of the Gaussian N(center, cov) of one chain (default: `best`): ``center + L xi`` in
        the free coordinates, L the Cholesky factor of ``cov``; held coordinates stay at the centre.  What ``space.constrain``,
        ``predictive.bands(model, rows, space)`` and ``comparison.loo`` take."""
        if int(n_draws) < 1:
            raise ValueError("need n_draws >= 1")
        return self._gaussian(n_draws, chain, generator)[0]

    def importance(self, n_draws, chain=None, generator=None, chunk=4096):
        """The check of whether the Gaussian can be trusted: over ``n_draws`` of its draws z_s, rho_s = logp(z_s) - log q(z_s).
        Returns {"pareto_k": the Pareto shape of the ratios' tail (`comparison`'s PSIS kernel on the column -rho; above 0.7 the
        Gaussian is NOT a usable stand-in for the posterior), "log_evidence_is": logsumexp(rho) - log S, the plain
        importance-sampling estimate of the evidence, "log_ratio": rho (S,)}."""
        from . import comparison

        if int(n_draws) < 1:
            raise ValueError("need n_draws >= 1")
        rows, xi, L = self._gaussian(n_draws, chain, generator)
        m = int(self.free_index.shape[0])
        logq = -0.5 * (xi * xi).sum(1) - 0.5 * m * math.log(2.0 * math.pi) - torch.log(torch.diagonal(L)).sum()
        rho = self._rows.value(rows, int(chunk)) - logq
        k = comparison._pointwise((-rho)[:, None].contiguous(), 1.0)["k"][0]
        return {"pareto_k": k, "log_evidence_is": torch.logsumexp(rho, 0) - math.log(int(n_draws)), "log_ratio": rho}


def laplace(logp_fn, params, *, free=None, order=2, delta=None, passes=2, scale=None, chunk=4096, native=True):
    """The Laplace approximation of ``logp_fn`` at ``params`` (tensors with a common leading chain dimension D, as `LBFGS` takes
    them -- the positions `optimize` returns): a `Laplace`.

    ``free``: one 0 / 1 mask per parameter, as `LBFGS`; the same for every chain.  The Hessian is taken over the m free
    elements, m <= n <= 64.  ``order``: 2 (2 m rows per chain and pass) or 4 (4 m rows, Richardson's combination of the h and
    the 2 h difference).  Two ``passes``: a pilot pass with the steps ``h_k = eps^(1/3) scale_k`` (``scale``: (n,) or (D, n),
    default ``max(|x|, 1)``), then the final pass with ``h_k = delta / sqrt(H_kk)`` of the pilot Hessian -- ``delta`` posterior
    standard deviations, conditional on the other coordinates; ``DEFAULT_DELTA[order]`` --; ``passes=1`` stops after the pilot
    pass.  The result comes from the last pass alone.  ``chunk`` rows go to one call of ``logp_fn``.  Nothing synchronises with
    the host between the passes.  On a ROCm device the stencil and the factorisation are native kernels; on the CPU, or with
    ``native=False``, the torch statement runs."""
    params = [p.detach() for p in params]
    if not params or any(p.dim() < 1 or p.shape[0] != params[0].shape[0] for p in params):
        raise ValueError("params must be tensors with a common leading chain dimension")
    if any(p.dtype != torch.float64 or p.device != params[0].device for p in params):
        raise ValueError("params must be float64 tensors on one device")
    order, passes, chunk = int(order), int(passes), int(chunk)
    if order not in (2, 4) or passes not in (1, 2) or chunk < 1:
        raise ValueError("need order 2 or 4, passes 1 or 2 and chunk >= 1")
    delta = DEFAULT_DELTA[order] if delta is None else float(delta)
    if not delta > 0:
        raise ValueError("need delta > 0")
    if free is not None and len(free) != len(params):
        raise ValueError("free must hold one mask per parameter")
    D = int(params[0].shape[0])
    dev = params[0].device
    x = torch.cat([p.reshape(D, -1) for p in params], dim=1).contiguous()
    n = int(x.shape[1])
    masks = [torch.ones_like(p) if f is None else torch.as_tensor(f, dtype=p.dtype, device=p.device).expand_as(p)
             for p, f in zip(params, free or [None] * len(params))]
    mask = torch.cat([f.reshape(D, -1) for f in masks], dim=1)
    if bool(((mask != 0) & (mask != 1)).any()):
        raise ValueError("free must be masks of 0 and 1")
    if D > 0 and bool((mask != mask[:1]).any()):
        raise ValueError("free must be the same for every chain: the chains share one set of free coordinates")
    free_index = torch.nonzero(mask[0] != 0).reshape(-1).to(torch.int32) if D > 0 else torch.arange(n, dtype=torch.int32, device=dev)
    m = int(free_index.shape[0])
    if not 1 <= m <= n <= MAX_N:
        raise ValueError(f"need 1 <= free coordinates <= parameters <= {MAX_N} per chain (MAX_N), got {m} of {n}")
    if scale is not None:
        scale = torch.as_tensor(scale, dtype=x.dtype, device=dev).contiguous()
        if tuple(scale.shape) not in ((n,), (D, n)):
            raise ValueError(f"scale must be ({n},) or ({D}, {n})")
    use_native = bool(native) and x.is_cuda
    rows = _Rows(logp_fn, params)
    new = lambda *shape, dtype=x.dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    logp, g0 = new(D), new(D, n)
    points, dx, grad = new(D, order * m, n), new(D, order * m), new(D, order * m, n)
    out = dict(hess=new(D, m, m), cov=new(D, m, m), sd=new(D, m), logdet=new(D), log_evidence=new(D), asymmetry=new(D),
               fd_error=new(D), status=new(D, dtype=torch.int32))
    if D > 0:
        rows.value_and_grad(x, logp, g0, chunk)
    index = free_index.long()
    for k in range(passes if D > 0 else 0):
        hess = out["hess"] if k else None
        with torch.no_grad():
            if use_native:
                _points_native(x, free_index, scale, hess, delta, order, points, dx)
            else:
                pts, off = _points_torch(x, index, scale, hess, delta, order)
                points.copy_(pts)
                dx.copy_(off)
        rows.value_and_grad(points.reshape(D * order * m, n), None, grad.reshape(D * order * m, n), chunk)
        with torch.no_grad():
            if use_native:
                _factor_native(grad, dx, logp, free_index, order, out)
            else:
                for key, value in _factor_torch(grad, dx, logp, index, order).items():
                    out[key].copy_(value)
    # (the last pass's stencil and gradient rows, for the tests that hold the kernels to the host build on the same rows)
    out.update(_points=points, _dx=dx, _grad=grad)
    out.update(center=x, logp=logp, n_eval=torch.full((D,), 1 + passes * order * m, dtype=torch.int32, device=dev))
    return Laplace(rows, out, free_index, order, delta)
