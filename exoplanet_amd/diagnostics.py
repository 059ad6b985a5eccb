"""Convergence diagnostics of a batch of chains: rank-normalised split R-hat, bulk / tail / mean effective sample sizes, the
Monte-Carlo standard error of the mean and the BFMI -- what the reference's tutorials read off ``az.summary(trace)`` before
believing a number -- computed where the draws are.

The definitions are those of Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021), as ArviZ and Stan report them (DESIGN.md
section 16 restates them; agreement with ArviZ itself is unpinned: it is not a dependency).  This module carries the TORCH
STATEMENT of every quantity (`_torch_statement`): it is the definition, runs on any device and is what runs for CPU tensors.
For a ROCm tensor the work goes to the kernels of csrc/exo_diagnostics.hip (`ops.chain_diagnostics`): torch sorts, the library
does the rest.

Every public function takes a float64 tensor of shape (n_draws, chains, *event) and returns one value per event element.
Degenerate input: fewer than four draws, or a value that is not finite in a series -- NaN for that series alone; a constant
series -- ESS = S (the number of split values), R-hat NaN.  A single chain is allowed (two half-chains).  Highest-density
intervals, rank plots and per-chain ESS are out of scope."""
import math

import torch

__all__ = ["rhat", "ess", "mcse_mean", "bfmi", "summary", "Summary"]

LAG_BLOCK = 16
_COLUMNS = ("mean", "sd", "q05", "q50", "q95", "mcse_mean", "ess_bulk", "ess_tail", "ess_mean", "r_hat")
_MAX_T = ("max_t_bulk", "max_t_low", "max_t_high", "max_t_mean")


# ---- the torch statement ---------------------------------------------------------------------------------------------------------
def _ndtri_lower(p):
    """Phi^-1 for 0 < p <= 1/2: torch's, then one Halley step against erfc (full relative accuracy in the lower tail)"""
    z = torch.special.ndtri(p)
    e = 0.5 * torch.special.erfc(-z * math.sqrt(0.5)) - p
    u = e * math.sqrt(2.0 * math.pi) * torch.exp(0.5 * z * z)
    return z - u / (1.0 + 0.5 * z * u)


def _rank_normalise(v):
    """v (K, S) -> z (K, S): z = Phi^-1((r - 3/8) / (S + 1/4)), r the average rank (ties share the mean of their ranks).
    p = (4 (2r) - 3) / (8 S + 2) is formed from whole numbers, on the side of its tail."""
    K, S = v.shape
    sv, perm = torch.sort(v, dim=1)
    sv = sv.contiguous()
    first = torch.searchsorted(sv, sv, right=False)
    last = torch.searchsorted(sv, sv, right=True) - 1
    num = 4 * (first + last + 2) - 3
    den = 8 * S + 2
    lower = 2 * num <= den
    p = torch.where(lower, num, den - num).to(v.dtype) / den
    z = _ndtri_lower(p)
    z = torch.where(lower, z, -z)
    return torch.empty_like(z).scatter_(1, perm, z)


def _quantile_sorted(sv, percent):
    """numpy.quantile's linear interpolation on sorted rows (K, n), the position formed from whole numbers"""
    n = sv.shape[1]
    num = (n - 1) * percent
    lo, rem = num // 100, num % 100
    a = sv[:, lo]
    if rem == 0 or lo + 1 >= n:
        return a.clone()
    return a + (rem / 100.0) * (sv[:, lo + 1] - a)


def _sequence(y):
    """y (K, L, M): K sets of M half-chains of L draws -> (ess (K,), max_t (K,), rhat (K,))"""
    K, L, M = y.shape
    S = M * L
    mean = y.mean(1, keepdim=True)
    d = y - mean
    W = (d * d).sum((1, 2)) / L / M * L / (L - 1)                 # mean_m a_m(0) L / (L - 1): the mean ddof-1 variance
    vb = mean[:, 0, :].var(1, unbiased=True) if M > 1 else torch.zeros_like(W)
    var_plus = W * (L - 1) / L + vb
    rhat = torch.sqrt(var_plus / W)                                # ((L - 1) / L W + B / L) / W, B / L = var of the means
    n_pad = -(-L // LAG_BLOCK) * LAG_BLOCK
    rho = torch.zeros((K, n_pad), dtype=y.dtype, device=y.device)
    have = [0]

    def need(t):                                                    # rho of the lags below t, a block at a time
        while have[0] <= t:
            for k in range(have[0], min(have[0] + LAG_BLOCK, L)):
                abar = (d[:, k:, :] * d[:, :L - k, :]).sum((1, 2)) / L / M
                rho[:, k] = 1.0 - (W - abar) / var_plus
            have[0] += LAG_BLOCK

    need(1)
    rho[:, 0] = 1.0
    re, ro = rho[:, 0].clone(), rho[:, 1].clone()
    active = torch.ones(K, dtype=torch.bool, device=y.device)
    max_t = torch.full((K,), -1, dtype=torch.int64, device=y.device)
    re_end = re.clone()
    t = 1
    while True:                                                     # Geyer's initial positive sequence
        go = active & (re + ro > 0) if t < L - 3 else torch.zeros_like(active)
        ended = active & ~go
        max_t = torch.where(ended, torch.full_like(max_t, t - 2), max_t)
        re_end = torch.where(ended, re, re_end)
        active = go
        if not bool(active.any()):
            break
        need(t + 2)
        re, ro = torch.where(active, rho[:, t + 1], re), torch.where(active, rho[:, t + 2], ro)
        t += 2
    top = int(max_t.max())
    for t in range(1, top - 1, 2):                                  # the initial monotone sequence
        prev = rho[:, t - 1] + rho[:, t]
        fix = (t <= max_t - 2) & (rho[:, t + 1] + rho[:, t + 2] > prev)
        rho[:, t + 1] = torch.where(fix, 0.5 * prev, rho[:, t + 1])
        rho[:, t + 2] = torch.where(fix, 0.5 * prev, rho[:, t + 2])
    keep = torch.arange(n_pad, device=y.device)[None, :] <= max_t[:, None]
    tau = -1.0 + 2.0 * torch.where(keep, rho, torch.zeros_like(rho)).sum(1) + torch.clamp(re_end, min=0.0)
    floor = 1.0 / math.log10(S)
    tau = torch.where(tau >= floor, tau, torch.where(torch.isnan(tau), tau, torch.full_like(tau, floor)))
    # (no variance at all -- an indicator that is the same everywhere: every draw counts, as for a constant series)
    return torch.where(var_plus == 0, torch.full_like(tau, float(S)), S / tau), max_t, rhat


def _torch_statement(x):
    """x (N, C, P) -> dict of (P,) tensors: the columns of a summary, ess_mean, the max_t of the four sequences and the two
    R-hat values"""
    N, C, P = x.shape
    nan = torch.full((P,), float("nan"), dtype=x.dtype, device=x.device)
    out = {k: nan.clone() for k in _COLUMNS + ("r_hat_z", "r_hat_folded")}
    out.update({k: torch.full((P,), -1, dtype=torch.int64, device=x.device) for k in _MAX_T})
    if N < 4 or C < 1 or P == 0:
        return out
    L, M = N // 2, 2 * C
    S = M * L
    flat = x.permute(2, 0, 1).reshape(P, N * C)
    bad = ~torch.isfinite(flat).all(1)
    const = (flat == flat[:, :1]).all(1)
    sf = torch.sort(flat, dim=1).values
    pivot = sf[:, N * C // 2]
    rel = flat - pivot[:, None]
    mean_rel = rel.mean(1)
    sd = torch.sqrt(((rel - mean_rel[:, None]) ** 2).sum(1) / (N * C - 1))
    q05, q50, q95 = (_quantile_sorted(sf, pc) for pc in (5, 50, 95))
    xs = torch.cat([x[:L], x[N - L:]], dim=1).permute(2, 0, 1)                      # (P, L, M)
    v = xs.reshape(P, S)
    sv = torch.sort(v, dim=1).values
    # |v - median| through the two middle order statistics: they themselves stay tied, as they are in exact arithmetic
    fold = 0.5 * ((v - sv[:, (S - 1) // 2][:, None]) + (v - sv[:, S // 2][:, None])).abs()
    z = _rank_normalise(v)
    zf = _rank_normalise(fold)
    low = (v <= q05[:, None]).to(x.dtype)
    high = (v <= q95[:, None]).to(x.dtype)
    raw = v - sv[:, S // 2][:, None]
    sets = torch.stack([z, zf, low, high, raw]).reshape(5 * P, L, M)
    ess_all, max_t, rh = _sequence(sets)
    ess_all, max_t, rh = ess_all.reshape(5, P), max_t.reshape(5, P), rh.reshape(5, P)
    full = torch.full_like(nan, float(S))
    pick = lambda value: torch.where(bad, nan, torch.where(const, full, value))  # noqa: E731
    ess_mean = pick(ess_all[4])
    r = torch.where(torch.isnan(rh[0]) | torch.isnan(rh[1]), nan, torch.maximum(rh[0], rh[1]))
    degenerate = bad | const
    res = dict(mean=pivot + mean_rel, sd=sd, q05=q05, q50=q50, q95=q95, mcse_mean=sd / torch.sqrt(ess_mean),
               ess_bulk=pick(ess_all[0]), ess_tail=pick(torch.minimum(ess_all[2], ess_all[3])), ess_mean=ess_mean,
               r_hat=torch.where(degenerate, nan, r), r_hat_z=torch.where(degenerate, nan, rh[0]),
               r_hat_folded=torch.where(degenerate, nan, rh[1]))
    for k in ("mean", "sd", "q05", "q50", "q95", "mcse_mean"):
        res[k] = torch.where(bad, nan, res[k])
    for name, row in zip(_MAX_T, (0, 2, 3, 4)):
        res[name] = torch.where(degenerate, torch.full_like(max_t[row], -1), max_t[row])
    return res


# ---- the device path -------------------------------------------------------------------------------------------------------------
_SET_BYTES = 1 << 30          # parameters of one library call: their five series sets stay below this


def _device(x):
    from . import ops

    N, C, P = x.shape
    if N < 4 or C < 1 or P == 0:
        return _torch_statement(x)
    L, M = N // 2, 2 * C
    chunk = max(1, min(P, 13000, _SET_BYTES // (8 * ops.DIAG_SETS * L * M)))
    rows = []
    for lo in range(0, P, chunk):
        part = x[:, :, lo:lo + chunk]
        xs = torch.cat([part[:L], part[N - L:]], dim=1).permute(2, 0, 1).contiguous()
        full = None if N % 2 == 0 else part.permute(2, 0, 1).reshape(part.shape[2], N * C).contiguous()
        rows.append(ops.chain_diagnostics(xs, full, M))
    table = torch.cat(rows, dim=0)
    res = {name: table[:, k] for k, name in enumerate(ops.DIAG_COLUMNS)}
    for k in _MAX_T:
        res[k] = res[k].to(torch.int64)
    return res


def _compute(x):
    """(N, C, *event) -> (dict of flat (P,) results, event shape)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 2:
        raise ValueError("need a tensor of shape (n_draws, chains, *event)")
    if x.dtype != torch.float64:
        raise TypeError("diagnostics take float64 draws")
    event = tuple(x.shape[2:])
    x3 = x.detach().reshape(x.shape[0], x.shape[1], -1)
    return (_device(x3) if x3.is_cuda else _torch_statement(x3)), event


def rhat(x):
    """rank-normalised split R-hat: the larger of R-hat of the normal scores and of the scores of |x - median|"""
    res, event = _compute(x)
    return res["r_hat"].reshape(event)


def ess(x, method="bulk"):
    """effective sample size: ``bulk`` (of the normal scores), ``tail`` (the smaller of the 5 % and 95 % indicator ESS) or
    ``mean`` (of the draws themselves)"""
    if method not in ("bulk", "tail", "mean"):
        raise ValueError("method must be 'bulk', 'tail' or 'mean'")
    res, event = _compute(x)
    return res["ess_" + method].reshape(event)


def mcse_mean(x):
    """Monte-Carlo standard error of the posterior mean: sd / sqrt(ess_mean)"""
    res, event = _compute(x)
    return res["mcse_mean"].reshape(event)


def bfmi(energy):
    """Betancourt's Bayesian fraction of missing information per chain: mean_n (E_n - E_{n-1})^2 / var_n(E_n) (ddof 0) of
    ``energy`` (n_draws, chains) -> (chains,).  Plain torch on either device: two reductions over a small array."""
    if energy.dim() != 2:
        raise ValueError("energy must be (n_draws, chains)")
    diff = energy[1:] - energy[:-1]
    return (diff * diff).mean(0) / energy.var(0, unbiased=False)


class Summary:
    """What `summary` returns: ``names`` and, per column of ``columns``, a (len(names),) tensor; from the sampler's
    statistics ``n_divergent`` (int), ``bfmi`` (chains,), ``mean_accept_prob`` and ``mean_depth`` (floats; None without
    statistics).  ``str()`` is the table the tutorials look at."""

    columns = _COLUMNS

    def __init__(self, names, table, n_draws, chains, n_divergent=None, bfmi=None, mean_accept_prob=None, mean_depth=None):
        self.names, self.table, self.n_draws, self.chains = list(names), table, n_draws, chains
        self.n_divergent, self.bfmi, self.mean_accept_prob, self.mean_depth = n_divergent, bfmi, mean_accept_prob, mean_depth

    def __getitem__(self, column):
        return self.table[column]

    def to_dict(self):
        """{name: {column: float}}, plus the sampler's statistics under "_stats" when there are any"""
        cols = {k: self.table[k].detach().cpu().tolist() for k in self.columns}
        res = {name: {k: cols[k][i] for k in self.columns} for i, name in enumerate(self.names)}
        if self.n_divergent is not None:
            res["_stats"] = dict(n_divergent=self.n_divergent, bfmi=self.bfmi.detach().cpu().tolist(),
                                 mean_accept_prob=self.mean_accept_prob, mean_depth=self.mean_depth)
        return res

    def __str__(self):
        d = self.to_dict()
        width = max([len(n) for n in self.names] + [4])
        head = " " * width + "".join("%11s" % k for k in self.columns)
        lines = [head]
        for name in self.names:
            row = d[name]
            lines.append(name.ljust(width) + "".join(("%11.0f" if k.startswith("ess") else "%11.4g") % row[k] for k in self.columns))
        lines.append("%d draws x %d chains" % (self.n_draws, self.chains))
        if self.n_divergent is not None:
            b = self.bfmi
            tail = "divergent transitions: %d; BFMI %.3f .. %.3f; mean accept probability %.3f" % (
                self.n_divergent, float(b.min()), float(b.max()), self.mean_accept_prob)
            if self.mean_depth is not None:
                tail += "; mean tree depth %.2f" % self.mean_depth
            lines.append(tail)
        return "\n".join(lines)


def summary(x, stats=None):
    """The table of a run.  ``x``: a tensor (n_draws, chains, *event) -- named x[0] .. x[n-1] in flat order --, a dict
    {name: tensor (n_draws, chains, *event)} (what ``Trace.constrain`` returns; a name with several elements gets an index),
    or a `sampling.Trace` (its unconstrained draws, and its ``stats`` unless ``stats`` is given).  ``stats``: the dict of a
    trace -- "diverging", "energy", "accept_prob" and, for NUTS, "depth".  No HDIs."""
    if hasattr(x, "draws") and hasattr(x, "stats"):
        stats = x.stats if stats is None else stats
        x = x.draws
    if isinstance(x, dict):
        names, parts = [], []
        for key, v in x.items():
            if v.dim() < 2:
                raise ValueError(f"{key}: need (n_draws, chains, *event)")
            flat = v.reshape(v.shape[0], v.shape[1], -1)
            names += [key] if flat.shape[2] == 1 else ["%s[%d]" % (key, i) for i in range(flat.shape[2])]
            parts.append(flat)
        x3 = torch.cat(parts, dim=2)
    else:
        x3 = x.reshape(x.shape[0], x.shape[1], -1)
        names = ["x[%d]" % i for i in range(x3.shape[2])]
    res, _ = _compute(x3)
    extra = {}
    if stats is not None:
        extra = dict(n_divergent=int(stats["diverging"].sum()), bfmi=bfmi(stats["energy"]),
                     mean_accept_prob=float(stats["accept_prob"].mean()),
                     mean_depth=float(stats["depth"].mean()) if "depth" in stats else None)
    return Summary(names, {k: res[k] for k in _COLUMNS}, int(x3.shape[0]), int(x3.shape[1]), **extra)
