"""What tests/test_sampling_dense.py (CPU) and tests/test_gpu_sampling_dense.py share: the targets, covariances and cases of the
invariance that defines the dense metric -- HMC / NUTS with the mass matrix C^-1 on q IS HMC / NUTS at unit masses on x,
q = c + L x, C = L L^T -- and the comparison of the two samplers transition by transition."""
import numpy as np
import torch

# n, condition number of C, step size, max_depth
CASES = [(1, 1.0, 0.15, 5), (3, 1e2, 0.12, 5), (17, 1e4, 0.2, 4), (64, 1e4, 0.25, 4)]
CHAINS = 65
TRANSITIONS = 25
SEED = 11


def covariance(n, condition, seed=5):
    """C = Q diag(logspace(0, -log10(condition), n)) Q^T with Q from a seeded QR; float64 on the CPU"""
    rng = np.random.RandomState(seed + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    C = (Q * np.logspace(0.0, -np.log10(condition), n)) @ Q.T
    return torch.as_tensor(0.5 * (C + C.T), dtype=torch.float64)


def logp(q):
    """-|q|^2 / 2 - 0.1 q_0^4, and a wall: -inf where q_0 > 1.8"""
    lp = -0.5 * (q * q).sum(1) - 0.1 * q[:, 0] ** 4
    return torch.where(q[:, 0] > 1.8, torch.full_like(lp, -float("inf")), lp)


def setup(n, condition, device="cpu", chains=CHAINS):
    """(C, c, x0) on ``device``: the covariance, a centre and the starting points in x"""
    g = torch.Generator().manual_seed(100 + n)
    C = covariance(n, condition)
    c = 0.3 * torch.randn(n, dtype=torch.float64, generator=g)
    x0 = torch.randn(chains, n, dtype=torch.float64, generator=g)
    return C.to(device), c.to(device), x0.to(device)


def whitened(c, L):
    """the target as a function of x, which the unit-mass sampler of the parent commit is given"""
    return lambda x: logp(c + x @ L.T)


def compare(A, B, c, L, transitions=TRANSITIONS, nuts=True, between=None):
    """step both samplers ``transitions`` times and hold A (dense metric, in q) to B (unit masses, in x) after every one;
    ``between(i)``: called before transition i.  Returns (worst relative position difference, worst accept_prob
    difference, divergences seen)."""
    worst_q = worst_a = 0.0
    n_div = 0
    for i in range(transitions):
        if between is not None:
            between(i)
        ra, rb = A.step(), B.step()
        assert torch.equal(ra, rb), f"transition {i}: {'depths' if nuts else 'accept masks'} differ"
        assert torch.equal(A.last_diverged, B.last_diverged), f"transition {i}: divergence flags differ"
        want = c + B.params[0] @ L.T
        scale = float(want.abs().max())
        dq = float((A.params[0] - want).abs().max()) / scale
        da = float((A.last_accept_prob - B.last_accept_prob).abs().max())
        worst_q, worst_a = max(worst_q, dq), max(worst_a, da)
        assert dq <= 1e-9, f"transition {i}: positions differ by {dq:.3e} of the largest magnitude"
        assert da <= 1e-9, f"transition {i}: accept_prob differs by {da:.3e}"
        n_div += int(A.last_diverged.sum())
    return worst_q, worst_a, n_div
