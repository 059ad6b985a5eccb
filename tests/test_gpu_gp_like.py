"""GPU: the celerite log-likelihood and its reverse pass against the multiprecision fixture tests/golden/gp_like_mp.npz
(tools/make_gp_like_golden.py; entries, quantities, yardstick and tolerance: tests/gp_like_cases.py) -- every state width
J = 1 .. 16 and every route a draw can take, by the rule  error <= max(16 unit, 1e-13)  in the scale of the quantity.

Routes per entry (gp_like_cases.ROUTES; a pair in gp_like_cases.EXCLUDED does not run, or runs with the quantities named there
printed and not asserted, and says why with the measured error: DESIGN.md section 17.4; at most 10 % of the pairs, asserted):
  default           celerite_loglike, one draw, the library's plan
  one_chunk         n_chunks = 1: the sequential kernels; and which route the default plan took: other bits than these for an
                    entry that stays on the time-parallel path, the same bits for one redone sequentially
  forced            n_chunks = 2 and 5
  batch             5 draws, the entry at positions 1 and 3 between benign draws of the same layout on the same time axis,
                    cotangent linspace(0.5, 1.5, D); j03, j08 and j10 also among 70 draws (a ragged last wave)
  obs_minus_model   the observed series minus a per-draw model inside the kernels; d / d model = -gy
  gaussian_process  GaussianProcess(kernel, t, diag=, mean=m).log_likelihood(y) through RealTerm / ComplexTerm / SHOTerm
  no_grad           the value-only call
Every check prints entry, route, quantity, unit, tolerance and error before it asserts (gp_cond_cases.check)."""
import numpy as np
import pytest
import torch

import gp_like_cases as K

pytestmark = pytest.mark.gpu


def T(a, dev, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev).requires_grad_(grad)


def npy(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def gold():
    return K.load()


def benign(c, rng, D):
    """D benign draws of the layout of ``c`` on its time axis: (y, diag, real, pairs), a kind-1 slot two positive real terms"""
    jr, jc, n = len(c.coef_real), len(c.pairs), c.n
    real = np.stack([rng.uniform(0.3, 1.0, (D, jr)), rng.uniform(0.1, 1.0, (D, jr))], -1)
    a, cc, d = rng.uniform(0.3, 1.0, (D, jc)), rng.uniform(0.1, 0.8, (D, jc)), rng.uniform(0.5, 3.0, (D, jc))
    pairs = np.stack([a, 0.3 * a * cc / d, cc, d], -1)
    k1 = np.broadcast_to(c.pair_kind.astype(bool), (D, jc))
    pairs[k1] = np.stack([a, cc, 0.5 * a, d], -1)[k1]
    return rng.normal(size=(D, n)), rng.uniform(0.07, 0.1, (D, n)), real, pairs


def loglike(dev, c, n_chunks=None, D=1, at=(0,), obs=False, grad=True):
    """the entry at the positions ``at`` of a batch of D draws -> per position the quantities of w_d * loglike_d, with w_d"""
    from exoplanet_amd.gp import celerite_loglike

    y, diag, real, pairs = benign(c, np.random.default_rng(7), D)
    for d in at:
        y[d], diag[d], real[d], pairs[d] = c.y, c.diag, c.coef_real, c.pairs
    kind = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(c.pair_kind, (D, len(c.pairs)))), device=dev) if c.pair_kind.any() else None
    # obs - model = y / 2 - (-y / 2): exactly y
    yt, dt, rt, ct = T(-0.5 * y if obs else y, dev, grad), T(diag, dev, grad), T(real, dev, grad), T(pairs, dev, grad)
    kw = dict(obs=T(0.5 * c.y, dev)) if obs else {}
    assert not obs or D == 1
    if not grad:
        with torch.no_grad():
            ll = celerite_loglike(T(c.t, dev), yt, dt, rt, ct, pair_kind=kind, n_chunks=n_chunks, **kw)
        return [({"loglike": npy(ll)[d]}, 1.0) for d in at]
    ll = celerite_loglike(T(c.t, dev), yt, dt, rt, ct, pair_kind=kind, n_chunks=n_chunks, **kw)
    w = torch.linspace(0.5, 1.5, D, dtype=torch.float64, device=dev) if D > 1 else torch.ones(1, dtype=torch.float64, device=dev)
    (ll * w).sum().backward()
    sign = -1.0 if obs else 1.0
    return [({"loglike": npy(ll)[d], "gy": sign * npy(yt.grad)[d], "gdiag": npy(dt.grad)[d], "greal": npy(rt.grad)[d],
              "gpairs": npy(ct.grad)[d]}, float(w[d])) for d in at]


def hold(label, c, results):
    for k, (got, w) in enumerate(results):
        K.check(f"{label}[{k}]" if len(results) > 1 else label, c.weighted(w), got, skip=c.skip)


def case(gold, name, route):
    """the entry for ``route``: None where the pair does not run; ``skip``: its quantities that are printed, not asserted"""
    quantities, reason = K.EXCLUDED.get((name, route), ((), ""))
    if reason:
        print(f"{name} {route}: excluded ({'the pair' if quantities is None else ', '.join(quantities)}) -- {reason}")
    if quantities is None:
        return None
    c = K.Case(gold, name)
    c.skip = quantities
    return c


def test_excluded_pairs_stay_under_their_share():
    pairs = [(e, r) for e in K.ENTRIES for r in K.ROUTES]
    assert set(K.EXCLUDED) <= set(pairs) and all(reason for _, reason in K.EXCLUDED.values())
    print(f"{len(K.EXCLUDED)} of {len(pairs)} (entry, route) pairs excluded, whole or in some quantity")
    assert len(K.EXCLUDED) <= K.MAX_EXCLUDED * len(pairs), (len(K.EXCLUDED), len(pairs))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_default_plan(dev, gold, name):
    c = case(gold, name, "default")
    if c is not None:
        hold("default", c, loglike(dev, c))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_one_chunk_and_which_route_ran(dev, gold, name):
    c = case(gold, name, "one_chunk")
    if c is None:
        return
    seq = loglike(dev, c, n_chunks=1)
    hold("one_chunk", c, seq)
    par = loglike(dev, c)
    same = seq[0][0]["loglike"].tobytes() == par[0][0]["loglike"].tobytes() and seq[0][0]["gy"].tobytes() == par[0][0]["gy"].tobytes()
    print(f"{name}: default plan {'==' if same else '!='} the sequential kernels, bit for bit ({K.route(name)})")
    assert same == (K.route(name) == "seq"), (name, K.route(name))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_forced_chunks(dev, gold, name):
    c = case(gold, name, "forced")
    if c is None:
        assert K.Case(gold, name).n < 64
        return
    for C in K.FORCED:
        hold(f"forced, {C} chunks", c, loglike(dev, c, n_chunks=C))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_batch(dev, gold, name):
    c = case(gold, name, "batch")
    if c is None:
        return
    hold(f"batch of {K.BATCH}", c, loglike(dev, c, D=K.BATCH, at=(1, 3)))
    if name in K.RAGGED:
        hold(f"batch of {K.BATCH_RAGGED}", c, loglike(dev, c, D=K.BATCH_RAGGED, at=(1, 3, K.BATCH_RAGGED - 1)))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_observed_series_minus_model(dev, gold, name):
    c = case(gold, name, "obs_minus_model")
    if c is not None:
        hold("obs_minus_model", c, loglike(dev, c, obs=True))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_no_grad_value(dev, gold, name):
    c = case(gold, name, "no_grad")
    if c is not None:
        hold("no_grad", c, loglike(dev, c, grad=False))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_gaussian_process(dev, gold, name):
    """the user-level classes: value, d / dy, d / d diag, d / d(mean) = -sum gy, and the gradient of every coefficient handed
    to a RealTerm or a ComplexTerm (an SHOTerm's slot is reached through sigma, rho and Q: its coefficients are not leaves)"""
    import exoplanet_amd as xo

    c = case(gold, name, "gaussian_process")
    if c is None:
        return
    leaf = lambda v: torch.tensor(float(v), dtype=torch.float64, device=dev, requires_grad=True)  # noqa: E731
    terms, kern = xo.gp.terms, None
    real = [[leaf(v) for v in row] for row in c.coef_real]
    pairs = [None if q is not None else [leaf(v) for v in row] for row, q in zip(c.pairs, K.sho_of(name))]
    for a, cc in real:
        k1 = terms.RealTerm(a=a, c=cc)
        kern = k1 if kern is None else kern + k1
    for p, q in zip(pairs, K.sho_of(name)):
        if q is None:
            k1 = terms.ComplexTerm(a=p[0], b=p[1], c=p[2], d=p[3])
        else:
            k1 = terms.SHOTerm(sigma=leaf(q[0]), rho=leaf(q[1]), Q=leaf(q[2]))
        kern = k1 if kern is None else kern + k1
    m, yt, dt = leaf(0.0), T(c.y, dev, True), T(c.diag, dev, True)
    gp = xo.gp.GaussianProcess(kern, t=T(c.t, dev), diag=dt, mean=m)
    r_, p_, kind, _, _ = gp._coefficients()
    plain = [i for i, q in enumerate(K.sho_of(name)) if q is None]
    assert np.array_equal(npy(r_)[0], c.coef_real) and np.array_equal(npy(p_)[0][plain], c.pairs[plain])
    assert np.array_equal(np.zeros(len(c.pairs), np.int32) if kind is None else npy(kind)[0], c.pair_kind)
    ll = gp.log_likelihood(yt)
    ll.backward()
    got = {"loglike": npy(ll), "gy": npy(yt.grad), "gdiag": npy(dt.grad),
           "greal": np.array([[npy(v.grad) for v in row] for row in real]).reshape(len(real), 2)}
    K.check("gaussian_process", c, got, skip=c.skip)
    for i in plain:         # one ComplexTerm's four coefficients: the slot's row of gpairs
        ci = K.Case(gold, name)
        ci.want, ci.scale = dict(c.want, gpairs=c.want["gpairs"][i]), dict(c.scale, gpairs=c.scale["gpairs"][i])
        K.check(f"gaussian_process, pair slot {i}", ci, {"gpairs": np.array([npy(v.grad) for v in pairs[i]])}, skip=c.skip)
    dm, want = float(m.grad), -float(c.want["gy"].sum())
    bound = c.n * K.tol(c, "gy") * c.scale["gy"]
    print(f"gaussian_process {name} d/d mean: want {want:.17g}, got {dm:.17g}, error {abs(dm - want):.3g}, bound {bound:.3g}")
    assert abs(dm - want) <= bound
