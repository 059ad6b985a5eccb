"""Posterior bands: a model evaluated at every kept draw of a trace and, per cadence or phase, the percentiles of those curves --
the figure every tutorial of the reference ends with (``np.percentile(trace.posterior["light_curves"], [16, 50, 84],
axis=(0, 1))``), computed where the draws are.

`quantiles` is the order statistic along the strided axis of an (S, N) array of curves; `bands` evaluates a model over a
trace's draws in chunks, into one (S, N) array, and calls it.  This module carries the TORCH STATEMENT of the definition
(`_torch_statement`): it is what runs for CPU tensors.  For a ROCm tensor the work goes to the kernel of
csrc/exo_predictive.hip (`ops.column_quantiles`): selection by counting passes, no sort and no copy of the array.

Definition, per column.  The m values that are not NaN take part (numpy's ``nanquantile`` rule; m = 0:
NaN).  A percent p is the exact rational p / 100 = a / b (``Fraction(str(p)) / 100``: 2.5 is 1 / 40).  The position is formed
from whole numbers, (m - 1) a = lo b + rem.  rem = 0: the result is x_(lo), untouched -- percent 0 and 100 are the minimum
and the maximum, infinities included.  Otherwise x_(lo) + (rem / b) (x_(lo+1) - x_(lo)): one division, one subtraction, one
multiplication, one addition, in that order.  x_(k) is the k-th smallest as a NUMBER: a zero comes back as +0.  For
whole-number percents this is `diagnostics._quantile_sorted` on the sorted values, bit for bit.

Out of scope: highest-density intervals, weighted draws, float32 input, a fused model + selection that
never forms the (S, N) array, plotting."""
from fractions import Fraction

import torch

__all__ = ["quantiles", "bands"]

MAX_DENOMINATOR = 10 ** 9


def _fraction(p):
    """percent -> (a, b) with p / 100 = a / b in lowest terms"""
    try:
        f = Fraction(str(p)) / 100
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"percent {p!r} is not a number") from None
    if f < 0 or f > 1:
        raise ValueError(f"percent {p!r} is outside [0, 100]")
    if f.denominator > MAX_DENOMINATOR:
        raise ValueError(f"percent {p!r}: more digits than a denominator of 1e9 holds")
    return f.numerator, f.denominator


def _fractions(percent):
    if isinstance(percent, torch.Tensor):
        percent = percent.tolist()
    if not isinstance(percent, (list, tuple)):
        percent = [percent]
    if not percent:
        raise ValueError("at least one percent")
    return [_fraction(p) for p in percent]


def _torch_statement(values, fractions):
    """values (S, N), fractions [(a, b)] -> ((Q, N), int32 (N,)): the definition, on any device"""
    S, N = values.shape
    valid = ~torch.isnan(values)
    m = valid.sum(0)                                                   # (N,) int64
    sv = torch.sort(values, dim=0).values + 0.0                        # (NaN last; -0 -> +0: an order statistic is a number)
    nan = torch.full((N,), float("nan"), dtype=values.dtype, device=values.device)
    rows = []
    for a, b in fractions:
        if S == 0:
            rows.append(nan)
            continue
        num = torch.clamp(m - 1, min=0) * a
        lo, rem = num // b, num % b
        x0 = sv.gather(0, lo[None, :])[0]
        x1 = sv.gather(0, torch.clamp(lo + 1, max=S - 1)[None, :])[0]
        frac = rem.to(values.dtype) / float(b)
        d = x1 - x0
        s = frac * d
        rows.append(torch.where(m == 0, nan, torch.where(rem == 0, x0, x0 + s)))
    return torch.stack(rows), m.to(torch.int32)


def _as_rows(values):
    """(S, N) or (n_draws, chains, N) -> (S, N), a view where the leading axes allow one"""
    if not isinstance(values, torch.Tensor) or values.dim() not in (2, 3):
        raise ValueError("values must be a tensor of shape (S, N) or (n_draws, chains, N)")
    if values.dtype != torch.float64:
        raise TypeError("quantiles take float64 values")
    if values.shape[-1] > 1 and values.stride(-1) != 1:
        raise ValueError("the last axis of values must be contiguous")
    return values.detach() if values.dim() == 2 else values.detach().reshape(-1, values.shape[-1])


def quantiles(values, percent=(16, 50, 84), *, return_count=False):
    """The ``percent`` percentiles over the draws: ``values`` (S, N) or (n_draws, chains, N), float64, last axis contiguous, any
    row stride >= N taken as it is (``buf[:S]``, ``curves[::k]``: no copy) -> (Q, N); with ``return_count`` also the int32
    (N,) number of values that took part (those that are not NaN).  Definition: the module's docstring."""
    res = _quantiles(_as_rows(values), _fractions(percent))
    return res if return_count else res[0]


def _quantiles(rows, fractions):
    if rows.is_cuda:
        from . import ops

        return ops.column_quantiles(rows, [a for a, _ in fractions], [b for _, b in fractions], return_count=True)
    return _torch_statement(rows, fractions)


def _draw_rows(trace, space):
    """the (total, ...) rows of a trace, as {name: (total, count)} arrays (space None) or as unconstrained rows"""
    if isinstance(trace, dict):
        if space is not None:
            raise ValueError("a dict of constrained draws takes no space")
        theta = {}
        for key, v in trace.items():
            if key == "log_prior":
                continue
            if not isinstance(v, torch.Tensor) or v.dim() < 2:
                raise ValueError(f"{key}: need (n_draws, chains, count)")
            theta[key] = v.reshape(v.shape[0] * v.shape[1], -1)
        totals = {int(v.shape[0]) for v in theta.values()}
        if len(totals) != 1:
            raise ValueError("the arrays of the trace must share (n_draws, chains)")
        return theta, None, totals.pop()
    if space is None:
        raise ValueError("a Trace or an array of unconstrained rows needs its ParameterSpace")
    z = trace.draws if hasattr(trace, "draws") else trace
    if not isinstance(z, torch.Tensor) or z.dim() not in (2, 3) or z.shape[-1] != space.n_free:
        raise ValueError(f"trace must be a Trace, a dict or a tensor (S, {space.n_free})")
    z = z.detach().reshape(-1, space.n_free)
    return None, z, int(z.shape[0])


def _model_over_draws(model, trace, space, n_draws, chunk):
    """``model`` at the kept draws of ``trace``, in chunks, as one (S, N) float64 array (`bands`: its curves; `comparison.loo`:
    its pointwise log-likelihoods).  The arguments are those of `bands`."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    theta_all, z, total = _draw_rows(trace, space)
    if total < 1:
        raise ValueError("the trace holds no draw")
    if n_draws is None:
        S, index = total, None
    else:
        S = int(n_draws)
        if S < 1 or S > total:
            raise ValueError(f"n_draws must be in 1 .. {total}, the draws of the trace")
        device = z.device if z is not None else next(iter(theta_all.values())).device
        index = (torch.arange(S, dtype=torch.int64, device=device) * total) // S
    if theta_all is not None:
        names = list(theta_all)
    else:
        names = list(space.names)

    def take(x, lo, hi):
        return x[lo:hi] if index is None else x.index_select(0, index[lo:hi])

    def curves(lo, hi):
        if theta_all is not None:
            theta = {k: take(v, lo, hi) for k, v in theta_all.items()}
        else:
            theta, _ = space.constrain(take(z, lo, hi).contiguous())
            missing = [k for k in names if k not in theta]
            if missing:
                raise ValueError(f"the space gives no parameter named {missing}")
        y = model(**{k: theta[k] for k in names})
        if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.shape[0] != hi - lo or y.dtype != torch.float64:
            raise ValueError(f"model must return a float64 tensor of shape ({hi - lo}, N), not "
                             f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__}")
        return y

    with torch.no_grad():
        first = curves(0, min(chunk, S))
        N = int(first.shape[1])
        buf = torch.empty((S, N), dtype=torch.float64, device=first.device)     # the one (S, N) array
        buf[:first.shape[0]] = first
        del first
        for lo in range(chunk, S, chunk):
            hi = min(lo + chunk, S)
            y = curves(lo, hi)
            if y.shape[1] != N:
                raise ValueError(f"model returned {y.shape[1]} columns after {N}")
            buf[lo:hi] = y
    return buf


def bands(model, trace, space=None, *, percent=(16, 50, 84), n_draws=None, chunk=1024, mean=False):
    """The band of ``model`` over the draws of ``trace``.

    ``trace``: a `sampling.Trace` or an (S, n_free) tensor of unconstrained rows, with ``space`` (a `ParameterSpace`); or a
    dict {name: (n_draws, chains, count)} as ``Trace.constrain`` returns, with ``space=None`` (a "log_prior" key is ignored).
    The n_draws * chains rows are taken in order; ``n_draws=`` takes the rows ``(arange(n_draws) * total) // n_draws`` instead
    (deterministic thinning).  Under ``torch.no_grad()`` the rows go through ``space.constrain`` in chunks of ``chunk``, and
    ``model(**theta)`` -- the names ``space.wrap`` would pass (a dict: its keys), each (chunk, count) -- must return (chunk, N).
    Every chunk is written into its rows of one (S, N) array; then `quantiles`.

    Returns {"percent", "quantiles" (Q, N), "n_valid" (N,), "n_draws": S} and, with ``mean=True``, "mean" (N,): the
    ``torch.nanmean`` over the draws.  The host reads nothing from the device."""
    fractions = _fractions(percent)
    buf = _model_over_draws(model, trace, space, n_draws, chunk)
    S = int(buf.shape[0])
    with torch.no_grad():
        q, n_valid = _quantiles(buf, fractions)
        out = {"percent": tuple(percent) if isinstance(percent, (list, tuple)) else percent, "quantiles": q, "n_valid": n_valid,
               "n_draws": S}
        if mean:
            out["mean"] = torch.nanmean(buf, dim=0)
    return out
