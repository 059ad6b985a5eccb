"""Model comparison: PSIS-LOO and WAIC over the draws of a trace, and `compare` -- what ``az.loo``, ``az.waic`` and
``az.compare`` answer (is the eccentric orbit warranted over the circular one? one planet or two? a jitter term or not?),
computed where the draws are.  Pareto-smoothed importance-sampling leave-one-out cross-validation: Vehtari, Gelman & Gabry
(2017), Vehtari et al. (2024); the generalised-Pareto fit: Zhang & Stephens (2009) as ArviZ's ``_gpdfit`` applies it.

Both come from the pointwise log-likelihood, an (S, N) array with one row per draw and one column per observation -- the
array `predictive.bands` forms for a model's curves.  This module carries the TORCH STATEMENT of the definition
(`_torch_statement`): it is what runs for CPU tensors.  For a ROCm tensor the work goes to the kernel of csrc/exo_psis.hip
(`ops.column_psis`): selection by counting passes for the cut-off and the tail sorted and fitted in LDS, no sort and no copy
of the array.

Definition (the numpy statement is tests/psis_oracle.py).  M = ceil(min(S / 5, 3 sqrt(S / reff))).  Per
column l_s: a NaN or an infinity gives NaN in every floating output and n_tail = 0.  Otherwise x_s = l_min - l_s (the log
ratios -l, shifted to a maximum of 0); the cut-off c = max(x_(S-M-1), log(DBL_MIN)) (the index clamped to 0); the tail
{x_s > c} of n <= M values.  n <= 4: k = +inf, nothing is smoothed.  Otherwise, with the tail ascending, u_j = exp(x_(j)) -
exp(c): m = 30 + floor(sqrt(n)) trial values b_i = (1 - sqrt(m / (i - 0.5))) / (3 u_[floor(n/4 + 0.5) - 1]) + 1 / u_[n-1], k_i
= mean_j log1p(-b_i u_j), L_i = n (log(-b_i / k_i) - k_i - 1), w_i = 1 / sum_i' exp(L_i' - L_i), the w_i < 10 eps dropped and
the rest renormalised, b = sum_i b_i w_i, k' = mean_j log1p(-b u_j), sigma = -k' / b, k = (n k' + 5) / (n + 10).  A finite k
replaces the j-th tail value by min(log(sigma expm1(-k log1p(-p_j)) / k + exp(c)), 0), p_j = (j + 0.5) / n (|k| < eps: -sigma
log1p(-p_j) inside the logarithm).  With the smoothed x': elpd_loo_i = logsumexp_s(x'_s + l_s) - logsumexp_s(x'_s) (outside
the tail x'_s + l_s is l_min: those draws enter as a count), lppd_i = logsumexp_s(l_s) - log S, p_waic_i = the variance of l_s
over the draws with divisor S, elpd_waic_i = lppd_i - p_waic_i.  Totals are sums over the observations, se = sqrt(N var_i
(elpd_i)) with divisor N, p_loo = lppd - elpd_loo, n_high_k = #{k_i > 0.7}.

Out of scope: returning the smoothed weights (``psislw``) and importance-weighted quantiles, estimating
``reff``, moment matching or refits for high k, K-fold, LOO-PIT, stacking or pseudo-BMA weights, float32 input, a fused
likelihood + PSIS that never forms the (S, N) array."""
import math

import torch

from . import predictive

__all__ = ["loo", "waic", "compare", "normal_log_likelihood", "tail_length"]

MAX_TAIL = 1024                               # include/exoplanet_amd.h EXO_PSIS_MAX_TAIL
EPS = 2.220446049250313e-16
LOG_DBL_MIN = -708.3964185322641
HIGH_K = 0.7


def tail_length(n_draws, reff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / reff))): the largest number of draws the Pareto tail is fitted to"""
    reff = float(reff)
    if not reff > 0 or math.isinf(reff):
        raise ValueError("reff must be a positive number")
    return int(math.ceil(min(n_draws / 5.0, 3.0 * math.sqrt(n_draws / reff)))) if n_draws > 0 else 0


def _statement_block(v, M):
    """the definition for the columns of v (S, n), S >= 1, all at once"""
    S, n_col = v.shape
    dev, f64 = v.device, v.dtype
    bad = ~torch.isfinite(v).all(0)
    v = torch.where(bad[None, :], torch.zeros((), dtype=f64, device=dev), v)
    lmin, lmax = v.min(0).values, v.max(0).values
    x = lmin - v
    xs = torch.sort(x, dim=0).values
    c = torch.clamp(xs[max(S - M - 1, 0)], min=LOG_DBL_MIN)
    ec = torch.exp(c)
    Mt = min(M, S)
    top = xs[S - Mt:]                                                  # (Mt, n) ascending; the tail is its last n rows
    n = (top > c).sum(0)
    pos = torch.arange(Mt, device=dev)[:, None]
    valid = pos < n[None, :]
    xt = top.gather(0, torch.clamp(pos + (Mt - n)[None, :], max=Mt - 1))   # the tail ascending from row 0
    nf = n.to(f64)
    zero, one, inf = (torch.full((), a, dtype=f64, device=dev) for a in (0.0, 1.0, float("inf")))
    u = torch.where(valid, torch.exp(xt) - ec, zero)
    fit = n > 4
    m = 30 + torch.floor(torch.sqrt(nf)).to(torch.int64)
    uq = torch.where(fit, u.gather(0, torch.clamp((n + 2) // 4 - 1, min=0)[None, :])[0], one)
    ul = torch.where(fit, u.gather(0, torch.clamp(n - 1, min=0)[None, :])[0], one)
    m_max = 30 + math.isqrt(Mt)
    i = torch.arange(1, m_max + 1, device=dev)[:, None]
    used = i <= m[None, :]
    b = (1.0 - torch.sqrt(m.to(f64)[None, :] / (i.to(f64) - 0.5))) / (3.0 * uq) + 1.0 / ul          # (m_max, n)
    kk = torch.log1p(-b[:, None, :] * u[None, :, :]).sum(1) / nf
    L = nf * (torch.log(-b / kk) - kk - 1.0)
    w = 1.0 / torch.where(used[None, :, :], torch.exp(L[None, :, :] - L[:, None, :]), zero).sum(1)
    keep = used & (w >= 10.0 * EPS)
    total = torch.where(keep, w, zero).sum(0)
    b_post = torch.where(keep, b * (w / total), zero).sum(0)
    k1 = torch.log1p(-b_post * u).sum(0) / nf
    sigma = -k1 / b_post
    k = torch.where(fit, (nf * k1 + 5.0) / (nf + 10.0), inf)
    smooth = fit & torch.isfinite(k)
    lp = torch.log1p(-(pos.to(f64) + 0.5) / nf)
    q = torch.where(k.abs() < EPS, -sigma * lp, sigma * torch.expm1(-k * lp) / k)
    x_new = torch.where(smooth[None, :] & valid, torch.minimum(torch.log(q + ec), zero), xt)
    body = torch.where(x > c, zero, torch.exp(x)).sum(0)
    lse = torch.log(body + torch.where(valid, torch.exp(x_new), zero).sum(0))
    t = torch.where(valid, x_new + (lmin - xt), -inf)
    outside = n < S
    mx = torch.maximum(t.max(0).values if Mt else -inf.expand(n_col), torch.where(outside, lmin, -inf))
    acc = torch.where(outside, (S - n).to(f64) * torch.exp(lmin - mx), zero) + torch.where(valid, torch.exp(t - mx), zero).sum(0)
    elpd = torch.log(acc) + mx - lse
    lppd = torch.log(torch.exp(v - lmax).sum(0)) + lmax - math.log(S)
    mean = v.sum(0) / S
    var = ((v - mean) ** 2).sum(0) / S
    nan = torch.full((), float("nan"), dtype=f64, device=dev)
    out = {"elpd": elpd, "k": k, "lppd": lppd, "var": var}
    out = {key: torch.where(bad, nan, a) for key, a in out.items()}
    out["n_tail"] = torch.where(bad, torch.zeros_like(n), n).to(torch.int32)
    return out


def _torch_statement(values, M):
    """values (S, N), M -> {"elpd", "k", "lppd", "var": (N,), "n_tail": int32 (N,)}: the definition, on any device, a block of
    columns at a time (the fit's temporaries are trial values x tail x columns)"""
    S, N = values.shape
    if S == 0 or N == 0:
        out = {key: torch.full((N,), float("nan"), dtype=values.dtype, device=values.device) for key in ("elpd", "k", "lppd", "var")}
        out["n_tail"] = torch.zeros(N, dtype=torch.int32, device=values.device)
        return out
    M = max(int(M), 1)
    block = max(1, min((1 << 24) // (62 * min(M, S)), (1 << 26) // S))
    parts = [_statement_block(values[:, lo:lo + block], M) for lo in range(0, N, block)]
    return {key: torch.cat([p[key] for p in parts]) for key in parts[0]}


def _pointwise(rows, reff):
    S = int(rows.shape[0])
    M = max(tail_length(S, reff), 1)
    if M > MAX_TAIL:
        raise ValueError(f"{S} draws at reff = {reff} need a tail of {M} values, more than {MAX_TAIL}: thin with n_draws=")
    if rows.is_cuda:
        from . import ops

        return ops.column_psis(rows, M)
    return _torch_statement(rows, M)


def _log_likelihood_rows(log_likelihood, trace, space, n_draws, chunk):
    if callable(log_likelihood) and not isinstance(log_likelihood, torch.Tensor):
        if trace is None:
            raise ValueError("a callable log-likelihood needs the trace it is evaluated over")
        return predictive._model_over_draws(log_likelihood, trace, space, n_draws, chunk)
    if trace is not None or space is not None:
        raise ValueError("an array of pointwise log-likelihoods takes no trace")
    rows = predictive._as_rows(log_likelihood)
    if n_draws is not None:
        total, S = int(rows.shape[0]), int(n_draws)
        if S < 1 or S > total:
            raise ValueError(f"n_draws must be in 1 .. {total}, the draws of the array")
        rows = rows.index_select(0, (torch.arange(S, dtype=torch.int64, device=rows.device) * total) // S)
    return rows


def _result(kind, log_likelihood, trace, space, n_draws, chunk, reff):
    rows = _log_likelihood_rows(log_likelihood, trace, space, n_draws, chunk)
    S, N = (int(v) for v in rows.shape)
    if S < 1 or N < 1:
        raise ValueError("the pointwise log-likelihood needs at least one draw and one observation")
    with torch.no_grad():
        pw = _pointwise(rows, reff)
        p_waic_i = pw["var"]
        elpd_i = pw["elpd"] if kind == "loo" else pw["lppd"] - p_waic_i
        # the totals: one read from the device
        totals = torch.stack([elpd_i.sum(), ((elpd_i - elpd_i.mean()) ** 2).sum(), pw["lppd"].sum(), p_waic_i.sum(),
                              (pw["k"] > HIGH_K).sum().to(torch.float64)]).tolist()
    elpd, ss, lppd, p_waic, high = totals
    out = {"elpd_i": elpd_i, "pareto_k": pw["k"], "lppd_i": pw["lppd"], "p_waic_i": p_waic_i, "n_tail": pw["n_tail"],
           "elpd_" + kind: elpd, "se": math.sqrt(ss), "p_" + kind: lppd - elpd if kind == "loo" else p_waic,
           "n_high_k": int(high), "n_draws": S, "n_data": N}
    return out


def loo(log_likelihood, trace=None, space=None, *, n_draws=None, chunk=1024, reff=1.0):
    """PSIS-LOO from the pointwise log-likelihood.

    ``log_likelihood``: a float64 tensor (S, N) or (n_draws, chains, N) -- last axis contiguous, any row stride, taken as it
    is --, or a callable with ``trace`` (and ``space``) as `predictive.bands` takes them: it gets the arguments ``bands``'
    ``model`` gets and returns the (chunk, N) pointwise log-likelihood of those draws (`normal_log_likelihood`).  ``n_draws=``
    thins as ``bands`` does; ``reff``: the relative efficiency of the draws, a number (1: independent draws).

    Returns a dict: pointwise device tensors "elpd_i", "pareto_k", "lppd_i", "p_waic_i" (N,) and "n_tail" (int32); the numbers
    "elpd_loo", "se", "p_loo" = lppd - elpd_loo, "n_high_k" = #{k > 0.7}; "n_draws", "n_data".  An observation whose column holds
    a NaN or an infinity is NaN, and so are the totals."""
    return _result("loo", log_likelihood, trace, space, n_draws, chunk, reff)


def waic(log_likelihood, trace=None, space=None, *, n_draws=None, chunk=1024, reff=1.0):
    """WAIC from the pointwise log-likelihood: the arguments and the pointwise entries of `loo`, with "elpd_i" = lppd_i -
    p_waic_i and the numbers "elpd_waic", "se", "p_waic"."""
    return _result("waic", log_likelihood, trace, space, n_draws, chunk, reff)


def compare(results):
    """{name: a result of `loo` (or, all of them, of `waic`)} -> a list of rows, best first: {"name", "rank", "elpd", "se", "p",
    "elpd_diff", "dse", "n_high_k"}.  ``elpd_diff`` is measured against the best model, ``dse = sqrt(N var_i(elpd_i^best -
    elpd_i^other))`` with divisor N.  Results over different numbers of observations are refused."""
    if not isinstance(results, dict) or not results:
        raise ValueError("compare takes a dict {name: result} of at least one model")
    kinds = {"loo" if "elpd_loo" in r else "waic" for r in results.values()}
    if len(kinds) != 1:
        raise ValueError("compare takes results of one kind, loo or waic")
    kind = kinds.pop()
    sizes = {int(r["n_data"]) for r in results.values()}
    if len(sizes) != 1:
        raise ValueError(f"the models were scored on different numbers of observations: {sorted(sizes)}")
    N = sizes.pop()
    order = sorted(results, key=lambda name: -results[name]["elpd_" + kind])
    best = results[order[0]]
    rows = []
    for rank, name in enumerate(order):
        r = results[name]
        d = best["elpd_i"] - r["elpd_i"].to(best["elpd_i"].device)
        dse = math.sqrt(float(((d - d.mean()) ** 2).sum())) if rank else 0.0
        rows.append({"name": name, "rank": rank, "elpd": r["elpd_" + kind], "se": r["se"], "p": r["p_" + kind],
                     "elpd_diff": best["elpd_" + kind] - r["elpd_" + kind], "dse": dse, "n_high_k": r["n_high_k"]})
    return rows


def normal_log_likelihood(y, mu, sigma):
    """The pointwise term of ``pm.Normal("obs", mu=mu, sigma=sigma, observed=y)``: y (N,), mu (chunk, N) -- a model's curves
    --, sigma a number or a tensor that broadcasts ((N,): per-cadence errors; (chunk, 1): a sampled jitter) -> (chunk, N)."""
    sigma = torch.as_tensor(sigma, dtype=mu.dtype, device=mu.device)
    r = (y - mu) / sigma
    return -0.5 * r * r - torch.log(sigma) - 0.5 * math.log(2.0 * math.pi)
