"""GPU: the conditional half of the celerite GP -- GaussianProcess.apply_inverse, dot_tril, predict (mean at the data and
at new times, return_var, return_cov, kernel=) and sample -- through the public classes, against the multiprecision fixture
tests/golden/gp_cond_mp.npz by the rule of tests/gp_cond_cases.py

    error <= max(16 unit, 1e-13)   in the scales max |alpha|, max |z|, max |mu|, k2(0),

unit = the error of the published recurrences restated in float64 (oracle/numpy_port.py) on the same inputs; the backward
error of the solve; every state width J = 1 .. 16; the draw slices of _predict_var and the blocks of _predict_cov; edges.
Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

import gp_cond_cases as K
from oracle import numpy_port as P

pytestmark = pytest.mark.gpu

D_BATCH = 70            # two waves, the second partly filled


def T(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)


@pytest.fixture(scope="module")
def gold():
    return K.load()


def slot_terms(c, dev):
    """one term per slot of entry ``c``, real slots first: RealTerm; a pair slot through SHOTerm with the entry's
    (sigma, rho, Q) where the cases file has them (the only way to a kind-1 slot), Matern32Term for `matern`, else a
    ComplexTerm of the stored coefficients"""
    from exoplanet_amd.gp import terms

    out = [terms.RealTerm(a=T(a, dev), c=T(cc, dev)) for a, cc in c.coef_real]
    sho = K.SHO.get(c.name)
    for s, p in enumerate(c.pairs):
        if c.name == "matern":
            sigma, rho, eps = K.MATERN
            out.append(terms.Matern32Term(sigma=T(sigma, dev), rho=T(rho, dev), eps=eps))
        elif sho is not None:
            sigma, rho, Q = sho[s]
            out.append(terms.SHOTerm(sigma=T(sigma, dev), rho=T(rho, dev), Q=T(Q, dev)))
        else:
            out.append(terms.ComplexTerm(a=T(p[0], dev), b=T(p[1], dev), c=T(p[2], dev), d=T(p[3], dev)))
    return out


def total(parts):
    from exoplanet_amd.gp.terms import TermSum

    return parts[0] if len(parts) == 1 else TermSum(*parts)


def make_gp(c, dev, diag):
    from exoplanet_amd.gp import GaussianProcess

    parts = slot_terms(c, dev)
    gp = GaussianProcess(total(parts), t=T(c.t, dev), diag=T(diag, dev))
    # the coefficients the device works with are the fixture's (an SHO term's to the rounding of its own algebra)
    real, cplx, kind, _, _ = gp._coefficients()
    assert real.shape[1] == len(c.coef_real) and cplx.shape[1] == len(c.pairs)
    np.testing.assert_allclose(cplx[0].cpu().numpy(), c.pairs, rtol=1e-9, atol=0)
    if kind is not None:
        assert kind[0].cpu().tolist() == c.pair_kind.tolist()
    else:
        assert not c.pair_kind.any()
    comps = [total([p for p, k in zip(parts, m) if k]) for m in c.masks]
    return gp, comps


def everything(gp, comps, c, dev):
    """every quantity of the fixture through the public calls -> dict of device tensors"""
    y, x, tq = T(c.y, dev), T(c.x, dev), T(c.tq, dev)
    got = {"alpha": gp.apply_inverse(y), "z": gp.dot_tril(x)}
    for i, comp in [(None, None)] + list(enumerate(comps)):
        sfx = "" if i is None else f"_m{i}"
        mu_t, var_t = gp.predict(y, return_var=True, kernel=comp)
        mu_q, var_q = gp.predict(y, tq, return_var=True, kernel=comp)
        mu_q2, cov_q = gp.predict(y, tq, return_cov=True, kernel=comp)
        assert torch.equal(mu_t, gp.predict(y, kernel=comp)) and torch.equal(mu_q, gp.predict(y, tq, kernel=comp))
        assert torch.equal(mu_q, mu_q2)
        got.update({"mu_t" + sfx: mu_t, "mu_q" + sfx: mu_q, "var_t" + sfx: var_t, "var_q" + sfx: var_q, "cov_q" + sfx: cov_q})
    return got


@pytest.mark.parametrize("name", K.ENTRIES)
def test_fixture_through_the_public_classes(dev, gold, name):
    """each entry alone and as 70 copies whose diagonals are scaled by 1, 1 + 1e-3, ...: draw 0 is the single call bit for
    bit, and the last draw (second wave) is the single call on ITS diagonal bit for bit.

    Measured on the MI355X: DESIGN.md section 13.2 has the whole table."""
    c = K.Case(gold, name)
    gp, comps = make_gp(c, dev, c.diag)
    one = everything(gp, comps, c, dev)
    got = {q: v.cpu().numpy() for q, v in one.items()}
    assert all(got[q].shape == c.want[q].shape for q in got)
    far = c.far()
    on = np.isin(c.tq, c.t)
    # the batch first, so that a failure of the rule below does not hide a row mix-up
    scale = 1.0 + 1e-3 * np.arange(D_BATCH)
    gpb, compsb = make_gp(c, dev, scale[:, None] * c.diag[None, :])
    many = everything(gpb, compsb, c, dev)
    last = D_BATCH - 1
    gpl, compsl = make_gp(c, dev, scale[last] * c.diag)
    single_last = everything(gpl, compsl, c, dev)
    for q in one:
        assert many[q].shape == (D_BATCH,) + tuple(one[q].shape), q
        assert torch.equal(many[q][0], one[q]), (name, q, "draw 0 of the batch is not the single call")
        assert torch.equal(many[q][last], single_last[q]), (name, q, "the last draw of the batch is not the single call")
    if c.diag[0] > 0:
        assert not torch.equal(many["z"][last], many["z"][0])
    K.check("MI355X", c, got, skip=("alpha",) if name in K.RESIDUAL_ONLY else ())
    for q, v in got.items():
        assert np.all(np.isfinite(v)), (name, q)
        if q.startswith("mu_q"):      # far outside the data: no conditional mean, the prior variance
            assert np.all(np.abs(v[far]) <= K.tol(c, q) * c.scale[q]), (name, q, v[far])
        if q.startswith("var_q"):
            assert np.all(np.abs(v[far] - c.scale[q]) <= K.tol(c, q) * c.scale[q]), (name, q, v[far])
    if name == "diag0":               # on the data the process is known exactly
        assert np.abs(got["var_t"]).max() <= K.tol(c, "var_t") * c.scale["var_t"]
        assert on.sum() >= 5 and np.abs(got["var_q"][on]).max() <= K.tol(c, "var_q") * c.scale["var_q"]


# ------------------------------------------------------------------------------------------------------------------
# the backward error of the solve
RES_N, RES_D = 1500, 6
RES_CASES = ("snr1e3", "snr1e6", "cadence_flagship", "q05001", "bjd_highq", "rot2_sho")


@functools.lru_cache(maxsize=None)
def residual_case(name):
    """(t, diag, slots, y (D, N), A in long double, the yardstick's backward error per draw) at N = 1500: the kernel and
    the noise of fixture entry ``name`` on a longer series of the same kind, y six draws from the process"""
    c = K.Case(K.load(), name)
    rng = np.random.default_rng(700 + K.ENTRIES.index(name))
    if name.startswith("cadence"):
        t = np.arange(RES_N) * (2.0 / 1440.0)
    else:
        t = np.sort(rng.uniform(0.0, 30.0 * RES_N / K.N, RES_N))
        t[RES_N // 3:] += 4.0
        t[RES_N // 2 + 1] = t[RES_N // 2]
        if name == "bjd_highq":
            t = t + K.BJD
    diag = np.full(RES_N, c.diag[0])
    co = c.coeffs()
    y = np.stack([P.celerite_dot_tril(t, diag, co, rng.normal(size=RES_N)) for _ in range(RES_D)])
    tau = np.abs(t[:, None].astype(np.longdouble) - t[None, :].astype(np.longdouble))
    A = np.zeros_like(tau)
    for a, cc in zip(co[0], co[1]):
        A += np.longdouble(a) * np.exp(-np.longdouble(cc) * tau)
    for a, b, cc, d in zip(*co[2:]):
        A += np.exp(-np.longdouble(cc) * tau) * (np.longdouble(a) * np.cos(np.longdouble(d) * tau)
                                                  + np.longdouble(b) * np.sin(np.longdouble(d) * tau))
    A[np.diag_indices(RES_N)] += diag
    yard = residual(A, P.celerite_solve(t, diag, co, y.T).T, y)
    return c, t, diag, y, A, yard


def residual(A, alpha, y):
    """max |A alpha - y| / max |y| per draw, the product in long double"""
    r = alpha.astype(np.longdouble) @ A - y       # (A symmetric)
    return np.array([float(np.abs(r[d]).max() / np.abs(y[d]).max()) for d in range(len(y))])


@pytest.mark.parametrize("plan", ["default", "sequential"])
@pytest.mark.parametrize("name", RES_CASES)
def test_backward_error_of_the_solve(dev, monkeypatch, name, plan):
    """res = max |A alpha - y| / max |y| of apply_inverse, A alpha formed in long double from the dense kernel, against the
    same quantity of the sequential float64 recurrences (celerite_solve): res <= max(16 res_yardstick, 1e-13), with the
    library's own plan and with the sequential recurrences asked for (EXO_GP_CHUNKS=1).  apply_inverse runs
    exo_celerite_solve_f64, which has no plan: both legs must give the same bits.

    Printed beside it, not asserted: the same figure for minus the likelihood's gradient with respect to y, the route
    apply_inverse took before, on the time-parallel plan (42 chunks here) and on the sequential kernels.  Measured on the
    MI355X: the time-parallel plan is at snr1e3 1.4e-8 .. 1.9e-8 against a yardstick of
    7e-12 .. 1.9e-11, at cadence_flagship up to 2.0e-12 against 2e-14, at q05001 1.6e-10 against 7.3e-12."""
    from exoplanet_amd.gp import GaussianProcess, celerite_loglike

    c, t, diag, y, A, yard = residual_case(name)
    if plan == "sequential":
        monkeypatch.setenv("EXO_GP_CHUNKS", "1")
    else:
        monkeypatch.delenv("EXO_GP_CHUNKS", raising=False)
    gp = GaussianProcess(total(slot_terms(c, dev)), t=T(t, dev), diag=T(diag, dev))
    alpha_t = gp.apply_inverse(T(y, dev))
    alpha = alpha_t.cpu().numpy()
    assert alpha.shape == y.shape and np.all(np.isfinite(alpha))
    res = residual(A, alpha, y)
    # the likelihood's reverse pass as a solve, on this leg's plan: measured only
    real, cplx, kind, _, _ = gp._coefficients()
    rep = lambda x: x.detach().expand((RES_D,) + tuple(x.shape[1:])).contiguous()  # noqa: E731
    r = T(y, dev).requires_grad_(True)
    ll = celerite_loglike(T(t, dev), r, T(diag[None], dev), rep(real), rep(cplx), pair_kind=None if kind is None else rep(kind),
                          n_chunks=1 if plan == "sequential" else 0)
    res_like = residual(A, -torch.autograd.grad(ll.sum(), r)[0].cpu().numpy(), y)
    bad = []
    for d in range(RES_D):
        tl = max(K.FACTOR * yard[d], K.FLOOR)
        print(f"MI355X backward error {name} plan {plan} draw {d}: yardstick = {yard[d]:.3g}, tolerance = {tl:.3g}, "
              f"residual = {res[d]:.3g}; the likelihood's reverse pass on this plan: {res_like[d]:.3g}")
        if not res[d] <= tl:
            bad.append((d, res[d], tl))
    assert not bad, (name, plan, bad)
    if plan == "sequential":
        monkeypatch.delenv("EXO_GP_CHUNKS")
        assert torch.equal(alpha_t, gp.apply_inverse(T(y, dev)))


# ------------------------------------------------------------------------------------------------------------------
def k_dense(tau, real, pairs, kind, keep=None):
    tau = np.abs(tau)
    k = np.zeros_like(tau)
    keep = np.ones(len(real) + len(pairs), bool) if keep is None else np.asarray(keep, bool)
    for (a, c), kp in zip(real, keep):
        if kp:
            k += a * np.exp(-c * tau)
    for p, kd, kp in zip(pairs, kind, keep[len(real):]):
        if not kp:
            continue
        if kd:
            k += p[0] * np.exp(-p[1] * tau) + p[2] * np.exp(-p[3] * tau)
        else:
            k += np.exp(-p[2] * tau) * (p[0] * np.cos(p[3] * tau) + p[1] * np.sin(p[3] * tau))
    return k


def device_coefs(gp, D):
    real, cplx, kind, _, _ = gp._coefficients()
    kind = np.zeros((D, cplx.shape[1]), np.int32) if kind is None else kind.cpu().numpy()
    return real.detach().cpu().numpy(), cplx.detach().cpu().numpy(), kind


def width_kernel(J, rng, dev, D=3):
    """a kernel of state width J for D draws: J % 2 (J % 4 == 0: two) real slots, the pair slots alternately an SHO term
    whose draws straddle Q = 1/2 (both kinds in one call) and a ComplexTerm"""
    from exoplanet_amd.gp import terms

    n_real = J % 2 if J % 4 or J < 4 else 2
    parts = [terms.RealTerm(a=T(rng.uniform(0.3, 1.0, D), dev), c=T(rng.uniform(0.05, 2.0, D), dev)) for _ in range(n_real)]
    for s in range((J - n_real) // 2):
        if s % 2 == 0:
            Q = np.where((np.arange(D) + s // 2) % 2 == 0, 0.3, rng.uniform(0.6, 3.0, D))
            parts.append(terms.SHOTerm(sigma=T(rng.uniform(0.4, 0.9, D), dev), rho=T(rng.uniform(1.0, 8.0, D), dev), Q=T(Q, dev)))
        else:
            a, c, d = rng.uniform(0.3, 1.0, D), rng.uniform(0.05, 1.0, D), rng.uniform(0.3, 4.0, D)
            parts.append(terms.ComplexTerm(a=T(a, dev), b=T(rng.uniform(-0.9, 0.9, D) * a * c / d, dev), c=T(c, dev), d=T(d, dev)))
    return total(parts)


@pytest.mark.parametrize("J", range(1, 17))
def test_every_state_width(dev, J):
    """dot_tril, predict at new times and predict(return_var=True) at every state width the kernels are instantiated for
    (with_J<1, 16>), D = 3 draws, against float64 dense linear algebra at the tolerances of tests/test_gpu_gp.py and
    tests/test_gpu_gp_predict_var.py"""
    from exoplanet_amd.gp import GaussianProcess

    rng = np.random.default_rng(900 + J)
    N, D = 96, 3
    t = np.sort(rng.uniform(0.0, 30.0, N))
    t[N // 3:] += 4.0
    diag = rng.uniform(0.05, 0.3, (D, N))
    gp = GaussianProcess(width_kernel(J, rng, dev, D), t=T(t, dev), diag=T(diag, dev))
    real, pairs, kind = device_coefs(gp, D)
    assert real.shape[1] + 2 * pairs.shape[1] == J
    if J >= 2:
        assert kind.any() and not kind.all()
    x, y = rng.normal(size=(D, N)), rng.normal(size=(D, N))
    tq = np.sort(np.concatenate([[t[0] - 2.0, t[0], t[5], t[5], t[-1], t[-1] + 1.5], rng.uniform(t[0], t[-1], 25)]))
    z = gp.dot_tril(T(x, dev)).cpu().numpy()
    mu, var = (v.cpu().numpy() for v in gp.predict(T(y, dev), T(tq, dev), return_var=True))
    for d in range(D):
        co = (real[d], pairs[d], kind[d])
        A = k_dense(t[:, None] - t[None, :], *co) + np.diag(diag[d])
        Kq = k_dense(tq[:, None] - t[None, :], *co)
        k0 = k_dense(np.zeros(1), *co)[0]
        z_w, mu_w = np.linalg.cholesky(A) @ x[d], Kq @ np.linalg.solve(A, y[d])
        var_w = k0 - np.einsum("mn,nm->m", Kq, np.linalg.solve(A, Kq.T))
        print(f"MI355X J = {J} draw {d}: |z - dense| = {np.abs(z[d] - z_w).max():.3g}, |mu - dense| = "
              f"{np.abs(mu[d] - mu_w).max():.3g}, |var - dense| / k(0) = {np.abs(var[d] - var_w).max() / k0:.3g}")
        np.testing.assert_allclose(z[d], z_w, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(mu[d], mu_w, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(var[d], var_w, rtol=0, atol=1e-9 * k0)


# ------------------------------------------------------------------------------------------------------------------
def count_calls(monkeypatch, obj, name):
    n = [0]
    orig = getattr(obj, name)

    def wrapped(*a, **k):
        n[0] += 1
        return orig(*a, **k)

    monkeypatch.setattr(obj, name, wrapped)
    return n


def test_predict_var_draw_slices(dev, gold, monkeypatch):
    """_predict_var with a workspace budget that cuts D = 150 draws into slices of 64 (the last ragged) and into slices of
    one: the result of the default budget (two slices, 128 + 22) bit for bit.  Per-draw diagonals, and a batch whose draws
    fall on either side of Q = 1/2 in no regular order (the slices must take their own rows of the kinds)"""
    from exoplanet_amd import _lib
    from exoplanet_amd.gp import GaussianProcess, celerite, terms

    c = K.Case(gold, "benign")
    rng = np.random.default_rng(31)
    D, N, M = 150, c.t.size, c.tq.size
    Q = np.where(rng.random(D) < 0.5, rng.uniform(0.2, 0.45, D), rng.uniform(0.55, 3.0, D))
    kernel = terms.SHOTerm(sigma=T(rng.uniform(0.5, 1.5, D), dev), rho=T(rng.uniform(2.0, 6.0, D), dev), Q=T(Q, dev))
    gp = GaussianProcess(kernel, t=T(c.t, dev), diag=T(rng.uniform(0.01, 0.3, (D, N)), dev))
    y, tq = T(rng.normal(size=(D, N)), dev), T(c.tq, dev)
    per_draw = 8 * _lib.load().exo_celerite_predict_var_work_doubles(N, M, 0, 1, 1)
    launches = [0]
    check = celerite._lib.check

    def counting(rc, what):
        launches[0] += what == "exo_celerite_predict_var_f64"
        return check(rc, what)

    monkeypatch.setattr(celerite._lib, "check", counting)
    mu, var = gp.predict(y, tq, return_var=True)
    assert launches[0] == 2                 # (the default budget holds all 150: a slice of 128, two waves, and the rest)
    assert var.shape == (D, M) and bool(torch.isfinite(var).all())
    for budget, n_slice in ((70 * per_draw, 3), (per_draw, D)):        # steps of 64 (70 rounded down to a wave) and of 1
        monkeypatch.setattr(celerite, "PREDICT_VAR_WORK_BYTES", budget)
        launches[0] = 0
        mu2, var2 = gp.predict(y, tq, return_var=True)
        assert launches[0] == n_slice, (budget, launches[0])
        assert torch.equal(mu2, mu) and torch.equal(var2, var), budget


def test_predict_cov_blocks(dev, gold, monkeypatch):
    """_predict_cov's blocked branch (K2(t, t*) not held whole; a double loop over row and column blocks): one query time
    per block at the fixture's M = 31, and blocks of 7 at the smallest M for which a budget exists that gives both
    `whole == False` and a block of 7 -- a block of 7 needs 7 x 8 N (3 + J) bytes, `whole == False` fewer than 8 N M, so
    M > 7 (3 + J), 42 here: M = 31 has none for any J >= 2, and no fixture entry has J = 1 -- with M not a multiple of 7; against the unblocked result to 1e-12 k2(0), and
    held to the fixture (real_sho_j3, the whole kernel and both masks; the fixture's query times are among the M)"""
    from exoplanet_amd import _lib
    from exoplanet_amd.gp import celerite

    c = K.Case(gold, "real_sho_j3")
    gp, comps = make_gp(c, dev, c.diag)
    y = T(c.y, dev)
    N = c.t.size
    rng = np.random.default_rng(32)
    per = 8 * (3 * N + _lib.load().exo_celerite_solve_work_doubles(N, len(c.coef_real), len(c.pairs), 1))
    M7 = (15 * per) // (2 * 8 * N) + 2             # 8 N M > 7.5 per
    M7 += 1 if M7 % 7 == 0 else 0
    more = np.sort(np.concatenate([c.tq, rng.uniform(c.t[0] - 1.0, c.t[-1] + 1.0, M7 - c.tq.size)]))
    at = np.searchsorted(more, c.tq)          # (a repeated query time: either copy)
    assert np.array_equal(more[at], c.tq)
    solves = count_calls(monkeypatch, celerite, "_inverse")
    for tq_np, blk, budget in ((c.tq, 1, min(per, 8 * N * c.tq.size) // 2), (more, 7, 7 * per + per // 2)):
        M = tq_np.size
        tq = T(tq_np, dev)
        assert 8 * N * M > budget and budget // per == (0 if blk == 1 else blk) and (blk == 1 or M % blk != 0)
        for i, comp in [(None, None)] + list(enumerate(comps)):
            q = "cov_q" if i is None else f"cov_q_m{i}"
            monkeypatch.setattr(celerite, "PREDICT_COV_WORK_BYTES", 1 << 30)
            solves[0] = 0
            _, cov = gp.predict(y, tq, return_cov=True, kernel=comp)
            assert solves[0] == 2         # (alpha, and every query time at once)
            monkeypatch.setattr(celerite, "PREDICT_COV_WORK_BYTES", budget)
            solves[0] = 0
            _, cov_b = gp.predict(y, tq, return_cov=True, kernel=comp)
            assert solves[0] == 1 + math.ceil(M / blk), (solves[0], M, blk)
            err = float((cov_b - cov).abs().max()) / c.scale[q]
            print(f"MI355X blocks of {blk}, M = {M}, {q}: |blocked - whole| / k2(0) = {err:.3g}")
            assert err <= 1e-12
            sub = cov_b.cpu().numpy()[np.ix_(at, at)] if blk == 7 else cov_b.cpu().numpy()
            K.check(f"MI355X blocks of {blk}", c, {q: sub})


# ------------------------------------------------------------------------------------------------------------------
def sho_dense(sigma, rho, Q):
    return P.sho_coefficients(*P.sho_from_sigma_rho(sigma, rho, Q), Q)


def test_one_datum(dev):
    from exoplanet_amd.gp import GaussianProcess, terms

    sigma, rho, Q, s2, t0, y0 = 0.8, 3.0, 0.7, 0.1, 0.3, 0.7
    gp = GaussianProcess(terms.SHOTerm(sigma=T(sigma, dev), rho=T(rho, dev), Q=T(Q, dev)), t=T([t0], dev), diag=T([s2], dev))
    co = sho_dense(sigma, rho, Q)
    k0 = sigma ** 2
    tq = np.array([-1.0, t0, t0, 2.0])
    kq = P.celerite_kernel(tq - t0, *co)
    y = T([y0], dev)
    np.testing.assert_allclose(gp.apply_inverse(y).cpu().numpy(), [y0 / (k0 + s2)], rtol=1e-14)
    np.testing.assert_allclose(gp.dot_tril(T([1.5], dev)).cpu().numpy(), [1.5 * np.sqrt(k0 + s2)], rtol=1e-14)
    mu, var = gp.predict(y, T(tq, dev), return_var=True)
    _, cov = gp.predict(y, T(tq, dev), return_cov=True)
    np.testing.assert_allclose(mu.cpu().numpy(), kq * y0 / (k0 + s2), rtol=0, atol=1e-14)
    np.testing.assert_allclose(var.cpu().numpy(), k0 - kq ** 2 / (k0 + s2), rtol=0, atol=1e-14 * k0)
    want = P.celerite_kernel(tq[:, None] - tq[None, :], *co) - np.outer(kq, kq) / (k0 + s2)
    np.testing.assert_allclose(cov.cpu().numpy(), want, rtol=0, atol=1e-14 * k0)
    mu, var = gp.predict(y, return_var=True)
    np.testing.assert_allclose(mu.cpu().numpy(), [y0 - s2 * y0 / (k0 + s2)], rtol=1e-14)
    np.testing.assert_allclose(var.cpu().numpy(), [k0 - k0 ** 2 / (k0 + s2)], rtol=0, atol=1e-14 * k0)


def test_query_edges(dev, gold):
    """one query time, none, all before the data, all after: shapes, and the values against the float64 yardstick
    (oracle/numpy_port.py) on those times.  An edge test, not the fixture's rule: the yardstick is no multiprecision
    reference for these query sets, so the allowance is its own unit on the fixture's queries more than the rule's 16"""
    c = K.Case(gold, "real_sho_j3")
    gp, comps = make_gp(c, dev, c.diag)
    y = T(c.y, dev)
    co = c.coeffs()
    alpha = c.want["alpha"]
    k0 = c.scale["var_q"]
    for label, tq in (("one", np.array([0.5 * (c.t[3] + c.t[4])])), ("none", np.zeros(0)),
                      ("before", c.t[0] - np.array([3.0, 1.0, 0.2, 0.2, 1e-6])),
                      ("after", c.t[-1] + np.array([1e-6, 0.2, 0.2, 1.0, 3.0]))):
        mu, var = gp.predict(y, T(tq, dev), return_var=True)
        mu2, cov = gp.predict(y, T(tq, dev), return_cov=True)
        mu_c, var_c = gp.predict(y, T(tq, dev), return_var=True, kernel=comps[1])
        m = tq.size
        assert mu.shape == (m,) and var.shape == (m,) and cov.shape == (m, m) and mu_c.shape == (m,) and var_c.shape == (m,)
        assert torch.equal(mu, mu2)
        mu_w = P.celerite_predict_mean(c.t, co, alpha, tq)
        var_w = P.celerite_predict_var(c.t, c.diag, co, co, tq)
        cov_w = P.celerite_predict_cov(c.t, c.diag, co, co, tq)
        var_cw = P.celerite_predict_var(c.t, c.diag, co, c.coeffs(c.masks[1]), tq)
        if m:
            print(f"MI355X queries {label}: |mu - yardstick| = {np.abs(mu.cpu().numpy() - mu_w).max():.3g}, |var - yardstick| "
                  f"/ k(0) = {np.abs(var.cpu().numpy() - var_w).max() / k0:.3g}")
        # 16 units and one more for the yardstick itself (other query times of the fixture's kinds)
        tl = lambda q: max((K.FACTOR + 1) * c.unit[q], K.FLOOR) * c.scale[q]  # noqa: E731
        np.testing.assert_allclose(mu.cpu().numpy(), mu_w, rtol=0, atol=tl("mu_q"))
        np.testing.assert_allclose(var.cpu().numpy(), var_w, rtol=0, atol=tl("var_q"))
        np.testing.assert_allclose(cov.cpu().numpy(), cov_w, rtol=0, atol=tl("cov_q"))
        np.testing.assert_allclose(var_c.cpu().numpy(), var_cw, rtol=0, atol=tl("var_q_m1"))


def test_not_positive_definite_draw_between_two_good_ones(dev, gold):
    """diag[30] = -50 in the middle draw: NaN in its variance (every query), in its apply_inverse (every cadence) and in its
    dot_tril (from that cadence on); the neighbours are what they are beside a good draw, bit for bit.  An arithmetic NaN,
    not a fault"""
    from exoplanet_amd.gp import GaussianProcess, terms

    c = K.Case(gold, "benign")
    rng = np.random.default_rng(33)
    N = c.t.size
    kernel = terms.SHOTerm(sigma=T([0.7, 1.0, 1.3], dev), rho=T([3.0, 2.0, 5.0], dev), Q=T([0.3, 0.7, 2.0], dev))
    diag = rng.uniform(0.05, 0.3, (3, N))
    bad = diag.copy()
    bad[1, 30] = -50.0
    x, y, tq = T(rng.normal(size=(3, N)), dev), T(rng.normal(size=(3, N)), dev), T(c.tq, dev)
    g_ok = GaussianProcess(kernel, t=T(c.t, dev), diag=T(diag, dev))
    g_bad = GaussianProcess(kernel, t=T(c.t, dev), diag=T(bad, dev))
    z_ok, z_bad = g_ok.dot_tril(x), g_bad.dot_tril(x)
    _, v_ok = g_ok.predict(y, tq, return_var=True)
    _, v_bad = g_bad.predict(y, tq, return_var=True)
    a_ok, a_bad = g_ok.apply_inverse(y), g_bad.apply_inverse(y)
    assert bool(torch.isnan(v_bad[1]).all()) and bool(torch.isnan(z_bad[1, 30:]).all()) and bool(torch.isnan(a_bad[1]).all())
    assert torch.equal(z_bad[1, :30], z_ok[1, :30])
    for d in (0, 2):
        assert torch.equal(z_bad[d], z_ok[d]) and torch.equal(v_bad[d], v_ok[d]) and torch.equal(a_bad[d], a_ok[d])
        assert bool(torch.isfinite(z_bad[d]).all()) and bool(torch.isfinite(v_bad[d]).all())
        assert bool(torch.isfinite(a_bad[d]).all())


@pytest.mark.parametrize("name", ["q045", "rot2_sho"])
def test_sample_second_moments(dev, gold, name):
    """sample(): shapes, and the second moment of 4000 prior draws against K + diag at three lags, for a kind-1 pair slot
    and for J = 10"""
    c = K.Case(gold, name)
    gp, _ = make_gp(c, dev, c.diag)
    g = torch.Generator(device=dev).manual_seed(11)
    s = gp.sample(size=3, generator=g)
    assert s.shape == (3, c.t.size) and bool(torch.isfinite(s).all())
    g.manual_seed(12)
    big = gp.sample(size=4000, generator=g).cpu().numpy()
    A = P.celerite_kernel(c.t[:, None] - c.t[None, :], *c.coeffs()) + np.diag(c.diag)
    i = 60
    for lag in (0, 3, 10):
        emp = np.mean(big[:, i] * big[:, i + lag])
        se = np.sqrt((A[i, i] * A[i + lag, i + lag] + A[i, i + lag] ** 2) / 4000)      # of a product of two Gaussians
        print(f"MI355X sample {name} lag {lag}: second moment {emp:.4g}, K + diag {A[i, i + lag]:.4g}, standard error {se:.3g}")
        assert abs(emp - A[i, i + lag]) < 5 * se
