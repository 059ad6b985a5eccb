"""GPU: GaussianProcess.predict(return_var=True / return_cov=True, kernel=...) against the dense definitions
var = k2(0) - diag(K2(t*, t) A^-1 K2(t, t*)),  cov = K2(t*, t*) - K2(t*, t) A^-1 K2(t, t*),  A = K + diag,
with K2 built from the component term's own coefficients (Term.pair_coefficients), and at full size against the existing
likelihood's gradient with respect to the diagonal."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)


def coefs(term, D):
    """the term's (real (D, Jr, 2), pairs (D, Jc, 4), kind (D, Jc)) as numpy, from its pair_coefficients"""
    ar, cr, pairs, kind = term.pair_coefficients()
    ar, cr = torch.broadcast_tensors(ar, cr)
    real = torch.stack([ar, cr], -1).detach().cpu().numpy()
    pairs = pairs.detach().cpu().numpy()
    kind = np.zeros(pairs.shape[:-1], np.int32) if kind is None else kind.detach().cpu().numpy()
    return (np.broadcast_to(real, (D,) + real.shape[-2:]), np.broadcast_to(pairs, (D,) + pairs.shape[-2:]),
            np.broadcast_to(kind, (D, kind.shape[-1])))


def k_dense(tau, real, pairs, kind):
    tau = np.abs(tau)
    k = np.zeros_like(tau)
    for a, c in real:
        k += a * np.exp(-c * tau)
    for p, kd in zip(pairs, kind):
        if kd:
            k += p[0] * np.exp(-p[1] * tau) + p[2] * np.exp(-p[3] * tau)
        else:
            k += np.exp(-p[2] * tau) * (p[0] * np.cos(p[3] * tau) + p[1] * np.sin(p[3] * tau))
    return k


def dense(t, diag, r, full, comp, tq):
    """(mu of the component without the mean, var, cov, k2(0)) of one draw; full / comp: (real, pairs, kind) of that draw"""
    A = k_dense(t[:, None] - t[None, :], *full) + np.diag(diag)
    K2 = k_dense(tq[:, None] - t[None, :], *comp)
    k0 = k_dense(np.zeros(1), *comp)[0]
    X = np.linalg.solve(A, K2.T)
    cov = k_dense(tq[:, None] - tq[None, :], *comp) - K2 @ X
    return K2 @ np.linalg.solve(A, r), np.diag(cov).copy(), cov, k0


def series(rng, n):
    t = np.sort(rng.uniform(0.0, 20.0, n))
    t[n // 2:] += 3.0      # a gap
    return t


def new_times(rng, t):
    return np.sort(np.concatenate([[t[0] - 2.0, t[0], t[5], t[-1], t[-1] + 1.5], rng.uniform(t[0] - 1, t[-1] + 1, 40),
                                   [t[30] + 1e-3] * 2]))


def make_kernel(name, dev):
    from exoplanet_amd.gp import terms

    S = lambda Q, rho, sigma: terms.SHOTerm(sigma=T(sigma, dev), rho=T(rho, dev), Q=T(Q, dev))
    rot = lambda p: terms.RotationTerm(sigma=T(0.8, dev), period=T(p, dev), Q0=T(1.0, dev), dQ=T(0.5, dev), f=T(0.4, dev))
    return {
        "real": lambda: terms.RealTerm(a=T(1.2, dev), c=T(0.7, dev)),
        "sho_q07": lambda: S(0.7, 3.0, 1.0),
        "sho_q03": lambda: S(0.3, 3.0, 1.0),
        "real_sho": lambda: terms.RealTerm(a=T(0.5, dev), c=T(0.2, dev)) + S(1.5, 2.0, 0.7),
        "mix_j5": lambda: terms.RealTerm(a=T(0.4, dev), c=T(1.0, dev)) + S(0.3, 4.0, 0.6) + S(2.0, 1.5, 0.5),
        "three_sho": lambda: S(2.0, 6.0, 0.5) + S(1.0, 3.0, 0.4) + S(1 / np.sqrt(2), 1.0, 0.3),
        "two_rot_sho": lambda: rot(4.0) + rot(9.0) + S(0.9, 2.0, 0.3),
    }[name]()


def check(gp, y, tq_np, t, diag, full, comp_term, D, kernel=None, mean=0.0):
    """predict's mean, var and cov (at tq_np, None: the data times) against the dense definitions, draw by draw"""
    dev = t.device
    tq = None if tq_np is None else T(tq_np, dev)
    mu, var = gp.predict(y, tq, return_var=True, kernel=kernel)
    mu2, cov = gp.predict(y, tq, return_cov=True, kernel=kernel)
    assert torch.equal(mu, mu2)
    if kernel is None:
        assert torch.equal(mu, gp.predict(y, tq))        # the mean is what the call without the new keywords returns
    tn, yn = t.cpu().numpy(), y.cpu().numpy()
    tqn = tn if tq_np is None else tq_np
    mu, var, cov = (x.cpu().numpy().reshape((D,) + x.shape[-(2 if x is cov else 1):]) for x in (mu, var, cov))
    comp = coefs(comp_term, D)
    for d in range(D):
        fd = tuple(x[d] for x in full)
        cd = tuple(x[d] for x in comp)
        yd = yn if yn.ndim == 1 else yn[d]
        mu_w, var_w, cov_w, k0 = dense(tn, diag[d if diag.shape[0] > 1 else 0], yd - mean, fd, cd, tqn)
        np.testing.assert_allclose(var[d], var_w, rtol=0, atol=1e-9 * k0)
        np.testing.assert_allclose(cov[d], cov_w, rtol=0, atol=1e-7 * k0)
        np.testing.assert_allclose(np.diag(cov[d]), var[d], rtol=0, atol=1e-7 * k0)   # two independent routes
        np.testing.assert_allclose(mu[d], mu_w + mean, rtol=0, atol=1e-8 * np.sqrt(k0) * max(1.0, np.abs(yd).max()))


@pytest.mark.parametrize("name", ["real", "sho_q07", "sho_q03", "real_sho", "mix_j5", "three_sho", "two_rot_sho"])
@pytest.mark.parametrize("noise", ["yerr", "diag"])
@pytest.mark.parametrize("where", ["data", "new"])
def test_predict_var_cov_vs_dense(dev, name, noise, where):
    from exoplanet_amd.gp import GaussianProcess

    rng = np.random.default_rng(zlib.crc32(f"{name}/{noise}/{where}".encode()))
    n = 160
    t = series(rng, n)
    kernel = make_kernel(name, dev)
    if noise == "yerr":
        gp = GaussianProcess(kernel, t=T(t, dev), yerr=0.3, mean=0.25)
        diag = np.full((1, n), 0.09)
    else:
        diag = rng.uniform(0.02, 0.2, (1, n))
        gp = GaussianProcess(kernel, t=T(t, dev), diag=T(diag[0], dev), mean=0.25)
    y = T(0.25 + rng.normal(size=n), dev)
    full = coefs(kernel, 1)
    check(gp, y, None if where == "data" else new_times(rng, t), T(t, dev), diag, full, kernel, 1, mean=0.25)


def test_predict_var_batch_straddles_q_half(dev):
    """D = 3 draws of one SHO term with Q = 0.3, 0.7, 2 (pair slots of both kinds in one call), per-draw diagonals"""
    from exoplanet_amd.gp import GaussianProcess, terms

    rng = np.random.default_rng(5)
    n, D = 150, 3
    t = series(rng, n)
    kernel = terms.SHOTerm(sigma=T([0.7, 1.0, 1.3], dev), rho=T([3.0, 2.0, 5.0], dev), Q=T([0.3, 0.7, 2.0], dev))
    diag = rng.uniform(0.02, 0.2, (D, n))
    gp = GaussianProcess(kernel, t=T(t, dev), diag=T(diag, dev))
    y = T(rng.normal(size=(D, n)), dev)
    kind = kernel.pair_coefficients()[3]
    assert kind.cpu().tolist() == [[1], [0], [0]]
    for where in (None, new_times(rng, t)):
        check(gp, y, where, T(t, dev), diag, coefs(kernel, D), kernel, D)


@pytest.mark.parametrize("layout", ["fused", "concatenated"])
def test_predict_component(dev, layout):
    """kernel=: one term, a RotationTerm inside a sum, a TermSum of terms, the full kernel (= None), a foreign term"""
    from exoplanet_amd.gp import GaussianProcess, terms
    from exoplanet_amd.gp.terms import TermSum

    rng = np.random.default_rng(11)
    n = 170
    t = series(rng, n)
    rot = terms.RotationTerm(sigma=T(0.9, dev), period=T(3.0, dev), Q0=T(1.5, dev), dQ=T(0.3, dev), f=T(0.5, dev))
    sho = terms.SHOTerm(sigma=T(0.5, dev), rho=T(8.0, dev), Q=T(0.3, dev))
    if layout == "fused":
        kernel = rot + sho
        assert kernel._fused_sho() is not None
        comps = [rot, sho]
    else:
        real = terms.RealTerm(a=T(0.3, dev), c=T(0.5, dev))
        kernel = real + rot + sho
        assert kernel._fused_sho() is None
        comps = [real, rot, sho, TermSum(real, sho)]
    gp = GaussianProcess(kernel, t=T(t, dev), yerr=0.2)
    y = T(rng.normal(size=n), dev)
    diag = np.full((1, n), 0.04)
    full = coefs(kernel, 1)
    for comp in comps:
        for where in (None, new_times(rng, t)):
            check(gp, y, where, T(t, dev), diag, full, comp, 1, kernel=comp)
    # the full kernel: the numbers of kernel=None
    for where in (None, T(new_times(rng, t), dev)):
        a = gp.predict(y, where, return_var=True)
        b = gp.predict(y, where, return_var=True, kernel=kernel)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the components add up: the means exactly in exact arithmetic, the covariances do not (cross terms)
    tq = T(new_times(rng, t), dev)
    parts = [gp.predict(y, tq, kernel=c, include_mean=False) for c in comps[:2 if layout == "fused" else 3]]
    np.testing.assert_allclose(sum(parts).cpu().numpy(), gp.predict(y, tq, include_mean=False).cpu().numpy(), rtol=0, atol=1e-10)
    with pytest.raises(ValueError):
        gp.predict(y, tq, return_var=True, kernel=terms.SHOTerm(sigma=T(0.5, dev), rho=T(8.0, dev), Q=T(0.3, dev)))
    with pytest.raises(ValueError):
        gp.predict(y, tq, kernel=rot + terms.RealTerm(a=T(0.3, dev), c=T(0.5, dev)))


def test_predict_shapes_and_errors(dev):
    from exoplanet_amd.gp import GaussianProcess, terms

    rng = np.random.default_rng(2)
    n, m = 90, 13
    t = series(rng, n)
    tq = T(np.sort(rng.uniform(0, 25, m)), dev)
    gp = GaussianProcess(terms.SHOTerm(sigma=T(1.0, dev), rho=T(3.0, dev), Q=T(0.7, dev)), t=T(t, dev), yerr=0.2)
    y = T(rng.normal(size=n), dev)
    mu, var = gp.predict(y, tq, return_var=True)
    assert mu.shape == (m,) and var.shape == (m,)
    mu, cov = gp.predict(y, tq, return_cov=True)
    assert mu.shape == (m,) and cov.shape == (m, m)
    mu, var = gp.predict(y, return_var=True)
    assert mu.shape == (n,) and var.shape == (n,)
    mu, var = gp.predict(y[None].expand(2, n), tq, return_var=True)
    assert mu.shape == (2, m) and var.shape == (2, m)
    _, cov = gp.predict(y[None].expand(2, n), tq, return_cov=True)
    assert cov.shape == (2, m, m)
    assert not var.requires_grad and not cov.requires_grad
    assert bool((var > 0).all()) and bool((var <= 1.0 + 1e-12).all())     # sigma = 1: k(0) = 1
    with pytest.raises(ValueError):
        gp.predict(y, tq, return_var=True, return_cov=True)
    with pytest.raises(ValueError):
        gp.predict(y, tq.flip(0), return_var=True)
    with pytest.raises(ValueError):
        gp.predict(y, tq, return_var=True, kernel=terms.RealTerm(a=T(1.0, dev), c=T(1.0, dev)))


def test_predict_var_full_size_vs_loglike_gradient(dev):
    """N = 150 000, D = 4, at the data times: var = sigma^2 - sigma^4 (A^-1)_nn, and (A^-1)_nn = alpha_n^2 - 2 dloglike/ddiag_n
    from the existing likelihood's autograd -- independent of the new code"""
    from exoplanet_amd.gp import GaussianProcess, celerite_loglike, terms

    rng = np.random.default_rng(9)
    n, D = 150000, 4
    t = np.arange(n) * (2.0 / 1440.0) + 2457000.0
    t[60000:] += 0.5                            # a gap
    cad = 2.0 / 1440.0
    kernel = terms.RealTerm(a=T([1.0, 0.8, 1.2, 1.0], dev), c=T(np.array([0.2, 0.1, 0.3, 0.05]) / cad, dev))
    sig2 = np.array([0.1, 0.2, 0.05, 0.1])[:, None] * np.ones((1, n))
    gp = GaussianProcess(kernel, t=T(t, dev), diag=T(sig2, dev))
    y = T(rng.normal(size=(D, n)), dev)
    _, var = gp.predict(y, return_var=True)
    alpha = gp.apply_inverse(y)
    real, cplx, kind, _, _ = gp._coefficients()
    diag = T(sig2, dev).requires_grad_(True)
    ll = celerite_loglike(T(t, dev), y, diag, real.detach().contiguous(), cplx.detach().contiguous(), pair_kind=kind)
    (g,) = torch.autograd.grad(ll.sum(), diag)
    s2 = T(sig2, dev)
    want = s2 - s2 ** 2 * (alpha ** 2 - 2.0 * g)
    err = ((var - want).abs() / s2).max().item()
    assert err <= 1e-5, err
    assert bool((var < s2).all()) and bool((var > 0.1 * s2).all())
