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
                    cotangent linspace(0.5, 1.5, D); j03, j08 and j10 also among 70 draws (a ragged last wave) and among 130
                    (two full waves and a ragged third)
  obs_minus_model   the observed series minus a per-draw model inside the kernels; d / d model = -gy
  gaussian_process  GaussianProcess(kernel, t, diag=, mean=m).log_likelihood(y) through RealTerm / ComplexTerm / SHOTerm
  no_grad           the value-only call
  cadence_major     the model as the .t() of a contiguous (N, D) tensor (exo_celerite_loglike_obs_{fwd,vjp}_cm_f64): batches of 5, 70
                    and 130, default plan, n_chunks = 1, 2 and 5; through GaussianProcess(mean=) for j03, j08, j10
  sparse_mean       celerite_loglike_sparse on hand-made segments (gp_like_cases.SPARSE_LAYOUTS, both descriptor forms, both forms
                    of ``off``): one draw, batches of 5, 70 and 130 (row_of_draw not the identity), the sparse default plan,
                    n_chunks = 1, 2 and 5, a per-draw and a shared diag; NaN in every value no segment covers; a sentinel in gvals
                    that every uncovered position keeps; through GaussianProcess(mean=) for j03, j08, j10
Both see obs - model: obs = where(H, y / 2, y), an entry's model -y / 2 on H and +0.0 or nothing elsewhere -- exactly y.  Each test
asserts that the route it names ran (the model is cadence-major; the sparse autograd function is in ll.grad_fn) and, where the
default plan can be told from the sequential kernels by its bits, that it took the tree / robust / seq route the entry is there for.
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


def loglike(dev, c, n_chunks=None, D=1, at=(0,), obs=False, grad=True):
    """the entry at the positions ``at`` of a batch of D draws -> per position the quantities of w_d * loglike_d, with w_d"""
    from exoplanet_amd.gp import celerite_loglike

    y, diag, real, pairs = K.batch(c, D, at)
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


def hold(label, c, results, skip=None):
    """results: (quantities, weight) per position, or (quantities, weight, cadences): gy is held at those cadences alone"""
    for k, (got, w, *cad) in enumerate(results):
        ck = K.restricted(c, cad[0]) if cad else c
        K.check(f"{label}[{k}]" if len(results) > 1 else label, ck.weighted(w), got, skip=c.skip if skip is None else skip)


def weights(dev, D):
    return torch.linspace(0.5, 1.5, D, dtype=torch.float64, device=dev) if D > 1 else torch.ones(1, dtype=torch.float64, device=dev)


def same_bits(a, b):
    return a[0][0]["loglike"].tobytes() == b[0][0]["loglike"].tobytes() and a[0][0]["gy"].tobytes() == b[0][0]["gy"].tobytes()


def cadence_major_leaf(y, dev):
    """a contiguous (N, D) leaf holding y (D, N) transposed, with the strides (D, 1) also where N = 1 (numpy gives a one-row
    array the strides of its transpose): its .t() is the cadence-major model"""
    base = torch.empty((y.shape[1], y.shape[0]), dtype=torch.float64, device=dev)
    base.copy_(torch.as_tensor(np.ascontiguousarray(y.T)))
    return base.requires_grad_(True)


def cadence_major(dev, c, n_chunks=None, D=K.BATCH, at=(1, 3)):
    """the entry at the positions ``at`` of D draws whose model is the .t() of a contiguous (N, D) tensor: -y / 2 against
    obs = y / 2, exactly y -> per position the quantities of w_d * loglike_d (gy = minus the model's cotangent), with w_d"""
    from exoplanet_amd import ops
    from exoplanet_amd.gp import celerite_loglike

    y, diag, real, pairs = K.batch(c, D, at)
    y[list(at)] = -0.5 * c.y
    model = cadence_major_leaf(y, dev).t()
    assert ops.is_cadence_major(model) and model.shape == (D, c.n)
    kind = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(c.pair_kind, (D, len(c.pairs)))), device=dev) if c.pair_kind.any() else None
    dt, rt, ct = T(diag, dev, True), T(real, dev, True), T(pairs, dev, True)
    ll = celerite_loglike(T(c.t, dev), model, dt, rt, ct, obs=T(0.5 * c.y, dev), pair_kind=kind, n_chunks=n_chunks)
    w = weights(dev, D)
    gm, gd, gr, gc = torch.autograd.grad((ll * w).sum(), [model, dt, rt, ct])
    assert gm.stride() == model.stride() == (1, D)      # the cotangent in the model's own layout
    return [({"loglike": npy(ll)[d], "gy": -npy(gm)[d], "gdiag": npy(gd)[d], "greal": npy(gr)[d], "gpairs": npy(gc)[d]}, float(w[d]))
            for d in at]


def sparse(dev, c, obs, m, n_chunks, at, shared_diag=False):
    """celerite_loglike_sparse on the hand-made model ``m`` (gp_like_cases.SparseModel) with the entry at the positions ``at``
    -> per position (quantities of w_d * loglike_d with gy = -gvals at the covered cadences, w_d, those cadences).  Every buffer
    the wrapper hands the library -- gvals among them -- holds K.SENTINEL before the call: the positions of gvals that no segment
    covers must still hold it afterwards, bit for bit, in every draw"""
    from exoplanet_amd.gp import celerite as C

    D = m.D
    _, diag, real, pairs = K.batch(c, D, at)
    lc = K.sparse_light_curve(m, dev)
    kind = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(c.pair_kind, (D, len(c.pairs)))), device=dev) if c.pair_kind.any() else None
    dt, rt, ct = T(c.diag[None] if shared_diag else diag, dev, True), T(real, dev, True), T(pairs, dev, True)
    w = weights(dev, D)
    saved = C._POISON[0]
    C._POISON[0] = K.SENTINEL
    try:
        ll = C.celerite_loglike_sparse(T(c.t, dev), lc, dt, rt, ct, T(obs, dev), pair_kind=kind, n_chunks=n_chunks)
        assert type(ll.grad_fn).__name__.startswith("_CeleriteLogLikeSparse")         # the route that ran
        (ll * w).sum().backward()
    finally:
        C._POISON[0] = saved
    if D > 64:      # the kernels took the draws through row_of_draw, and not in the caller's order
        assert C._SORT_DRAWS[0]
        order = npy(C._transit_order(lc))
        assert sorted(order) == list(range(D)) and not np.array_equal(order, np.arange(D))
    gv = npy(lc.values.grad)
    assert gv.shape == m.vals.shape
    for d in range(D):
        keep = m.untouched(d)
        assert np.array_equal(gv[d, keep].view(np.int64), np.full(int(keep.sum()), K.SENTINEL).view(np.int64)), (c.name, d, m.form, m.offs)
    gd = npy(dt.grad)
    return [({"loglike": npy(ll)[d], "gy": -gv[d, m.pos[d]], "gdiag": gd[0 if shared_diag else d], "greal": npy(rt.grad)[d],
              "gpairs": npy(ct.grad)[d]}, float(w[d]), m.cad[d]) for d in at]


SPARSE_PLANS = (("sparse default plan", 0), ("one chunk", 1)) + tuple((f"{C} chunks", C) for C in K.FORCED)


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
        hold(f"batch of {K.BATCH_WAVES}", c, loglike(dev, c, D=K.BATCH_WAVES, at=(1, 64, K.BATCH_WAVES - 1)))


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


# ------------------------------------------------------------------------------------------------------------------
# the two routes the benchmark's configurations take to the likelihood: a cadence-major model, a sparse mean
@pytest.mark.parametrize("name", K.ENTRIES)
def test_cadence_major(dev, gold, name):
    """exo_celerite_loglike_obs_{fwd,vjp}_cm_f64: five draws with the entry at (1, 3) on the default plan, the sequential kernels
    and forced chunk counts; j03, j08, j10 also among 70 and 130 draws (a ragged last wave; two full waves and a ragged third).
    That the model is cadence-major and that its cotangent comes back in its strides is asserted where it is made (cadence_major);
    the default plan took the route the entry is there for (other bits than the sequential kernels', or the same)"""
    c = case(gold, name, "cadence_major")
    default = cadence_major(dev, c)
    hold("cadence_major, default plan", c, default)
    seq = cadence_major(dev, c, n_chunks=1)
    hold("cadence_major, one chunk", c, seq, skip=())
    print(f"{name}: cadence-major default plan {'==' if same_bits(seq, default) else '!='} the sequential kernels ({K.route(name)})")
    assert same_bits(seq, default) == (K.route(name) == "seq"), (name, K.route(name))
    for C in K.FORCED:
        hold(f"cadence_major, {C} chunks", c, cadence_major(dev, c, n_chunks=C))
    if name in K.RAGGED:
        for D in (K.BATCH_RAGGED, K.BATCH_WAVES):
            hold(f"cadence_major, batch of {D}", c, cadence_major(dev, c, D=D, at=(1, 64 if D > 70 else 3, D - 1)))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_sparse_mean(dev, gold, name):
    """exo_celerite_loglike_sparse_{fwd,vjp}_f64 through celerite_loglike_sparse on hand-made segments: one draw carrying the
    entry in every layout of gp_like_cases.SPARSE_LAYOUTS, on the sparse default plan (n_chunks = 0), the sequential kernels
    and forced chunk counts; the uncovered positions of vals hold NaN, those of gvals keep their sentinel (sparse)"""
    c = case(gold, name, "sparse_mean")
    res = {}
    for layout in K.SPARSE_LAYOUTS:
        obs, m = K.sparse_entry(c, layout)
        for label, n_chunks in SPARSE_PLANS:
            res[layout, n_chunks] = sparse(dev, c, obs, m, n_chunks, (0,))
            hold(f"sparse_mean ({layout}, {label})", c, res[layout, n_chunks], skip=() if n_chunks == 1 else None)
    same = same_bits(res["whole", 1], res["whole", 0])
    print(f"{name}: sparse default plan {'==' if same else '!='} the sequential kernels ({K.route(name)})")
    assert same == (K.route(name) == "seq"), (name, K.route(name))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_sparse_mean_descriptor_forms(dev, gold, name):
    """both descriptor forms (the sweep's rows of (lo, a, b, hi) with a, b and the unused runs poisoned; the merged (lo, hi)) and
    both forms of ``off`` (exclusive prefix sums; values that start later and leave holes): whole, comb and blocks for every
    entry, every layout for the ladder"""
    c = case(gold, name, "sparse_mean")
    for layout in (K.SPARSE_LAYOUTS if name in K.LADDER else K.SPARSE_EVERY_ENTRY):
        for form, offs in K.SPARSE_VARIANTS[1:]:       # (sweep, prefix) is test_sparse_mean
            obs, m = K.sparse_entry(c, layout, form, offs)
            for label, n_chunks in SPARSE_PLANS:
                hold(f"sparse_mean ({layout}, {form}, {offs}, {label})", c, sparse(dev, c, obs, m, n_chunks, (0,)),
                     skip=() if n_chunks == 1 else None)


@pytest.mark.parametrize("name", K.ENTRIES)
def test_sparse_mean_batch(dev, gold, name):
    """five draws with another number of segments each: the entry at 1 as blocks and at 3 as padded (the same H) between benign
    draws of layouts none / edges / whole with arbitrary values, a per-draw diag; j03, j08, j10 also among 70 and 130 draws with
    the entry at 1, 64 and D - 1, where the wrapper hands the kernels a row_of_draw that is not the identity (asserted in sparse)"""
    c = case(gold, name, "sparse_mean")
    for (form, offs), (label, n_chunks) in zip(K.SPARSE_VARIANTS, SPARSE_PLANS):
        obs, m = K.sparse_batch(c, K.BATCH, (1, 3), form, offs)
        assert m.nseg[1] == m.nseg[3] and (c.n < 64 or (len(set(m.nseg.tolist())) == 4 and not np.array_equal(m.seg[1], m.seg[3])))
        hold(f"sparse_mean, batch of {K.BATCH} ({form}, {offs}, {label})", c, sparse(dev, c, obs, m, n_chunks, (1, 3)),
             skip=() if n_chunks == 1 else None)
    if name in K.RAGGED:
        for D, (form, offs) in ((K.BATCH_RAGGED, ("sweep", "prefix")), (K.BATCH_WAVES, ("merged", "gaps"))):
            obs, m = K.sparse_batch(c, D, (1, 64, D - 1), form, offs)
            hold(f"sparse_mean, batch of {D} ({form}, {offs})", c, sparse(dev, c, obs, m, 0, (1, 64, D - 1)))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_sparse_mean_shared_diag(dev, gold, name):
    """a diag of shape (1, N) shared by three draws that all carry the entry (blocks, padded, blocks), cotangent
    linspace(0.5, 1.5, 3): its gradient is sum_d w_d gdiag -- three terms, each within the rule, so the sum is held to
    (sum_d w_d) x the tolerance (the sum rule of tests/test_gp_like_host.py); everything else per draw as usual"""
    c = case(gold, name, "sparse_mean")
    obs, m = K.sparse_batch(c, 3, (0, 1, 2))
    res = sparse(dev, c, obs, m, 0, (0, 1, 2), shared_diag=True)
    total = sum(w for _, w, _ in res)
    K.check("sparse_mean, shared diag (sum over the draws)", c.weighted(total), {"gdiag": res[0][0]["gdiag"]}, skip=c.skip)
    hold("sparse_mean, shared diag", c, [({q: v for q, v in got.items() if q != "gdiag"}, w, cad) for got, w, cad in res])


@pytest.mark.parametrize("sparse_model", (False, True))
def test_second_reverse_pass_is_refused(dev, gold, sparse_model):
    """found by test_gaussian_process_mean's first version: the reverse pass of a time-parallel plan works inside the forward call's
    state, and a second backward through the same graph came back with gdiag off by 0.3 of its scale, silently.  Now it is an
    error; the sequential plan (n_chunks = 1), which only reads its state, gives the same bits twice"""
    from exoplanet_amd.gp import celerite as C

    c = K.Case(gold, "j03")
    for n_chunks, again in ((0, False), (1, True)):
        dt, rt, ct = T(c.diag[None], dev, True), T(c.coef_real[None], dev, True), T(c.pairs[None], dev, True)
        if sparse_model:
            obs, m = K.sparse_entry(c, "blocks")
            lc = K.sparse_light_curve(m, dev)
            leaf = lc.values
            ll = C.celerite_loglike_sparse(T(c.t, dev), lc, dt, rt, ct, T(obs, dev), n_chunks=n_chunks)
        else:
            leaf = T(c.y[None], dev, True)
            ll = C.celerite_loglike(T(c.t, dev), leaf, dt, rt, ct, n_chunks=n_chunks)
        first = torch.autograd.grad(ll.sum(), [leaf, dt, rt, ct], retain_graph=True)
        if again:
            second = torch.autograd.grad(ll.sum(), [leaf, dt, rt, ct])
            keep = torch.as_tensor(m.pos[0], device=dev) if sparse_model else slice(None)      # (gvals is defined where a segment covers)
            assert torch.equal(first[0][0, keep], second[0][0, keep]) and all(torch.equal(a, b) for a, b in zip(first[1:], second[1:]))
        else:
            with pytest.raises(RuntimeError, match="consumes the state"):
                torch.autograd.grad(ll.sum(), [leaf, dt, rt, ct])


@pytest.mark.parametrize("mean", ("cadence_major", "sparse_mean"))
@pytest.mark.parametrize("name", K.RAGGED)
def test_gaussian_process_mean(dev, gold, name, mean):
    """GaussianProcess(kernel, t, diag=, mean=<a cadence-major model | a hand-made sparse light curve>).log_likelihood(obs), the
    entry at position 1 of five draws as _prepare takes them: value, gdiag, the coefficient gradients and the mean's cotangent"""
    import exoplanet_amd as xo
    from exoplanet_amd.gp import celerite as C

    c = case(gold, name, mean)
    D, d = K.BATCH, 1
    y, diag, real, pairs = K.batch(c, D, (d,))
    dt, rt, ct = T(diag, dev, True), T(real, dev, True), T(pairs, dev, True)
    terms, kern = xo.gp.terms, None
    for j in range(real.shape[1]):
        k1 = terms.RealTerm(a=rt[:, j, 0], c=rt[:, j, 1])
        kern = k1 if kern is None else kern + k1
    for s in range(pairs.shape[1]):
        k1 = terms.ComplexTerm(a=ct[:, s, 0], b=ct[:, s, 1], c=ct[:, s, 2], d=ct[:, s, 3])
        kern = k1 if kern is None else kern + k1
    assert not c.pair_kind.any()
    if mean == "cadence_major":
        y[d] = -0.5 * c.y
        base = cadence_major_leaf(y, dev)
        model, obs, m = base.t(), 0.5 * c.y, None
    else:
        obs, m = K.sparse_batch(c, D, (d,))
        model = K.sparse_light_curve(m, dev)
    gp = xo.gp.GaussianProcess(kern, t=T(c.t, dev), diag=dt, mean=model)
    r_, p_, kind, _, _ = gp._coefficients()
    assert kind is None and np.array_equal(npy(r_), real) and np.array_equal(npy(p_), pairs)
    taken = gp._prepare(T(obs, dev), fuse=True)[2]
    assert taken is model if m is not None else (xo.ops.is_cadence_major(taken) and taken.data_ptr() == model.data_ptr())
    saved = C._POISON[0]
    C._POISON[0] = K.SENTINEL
    try:
        ll = gp.log_likelihood(T(obs, dev))
        assert ll.shape == (D,)
        assert type(ll.grad_fn).__name__.startswith("_CeleriteLogLikeSparse" if m is not None else "_CeleriteLogLike")
        assert (m is None) == (not type(ll.grad_fn).__name__.startswith("_CeleriteLogLikeSparse"))
        w = weights(dev, D)
        (ll * w).sum().backward()
    finally:
        C._POISON[0] = saved
    if m is None:
        gy, cad = -npy(base.grad)[:, d], []
    else:
        gv = npy(model.values.grad)
        for k in range(D):
            keep = m.untouched(k)
            assert np.array_equal(gv[k, keep].view(np.int64), np.full(int(keep.sum()), K.SENTINEL).view(np.int64)), (name, k)
        gy, cad = -gv[d, m.pos[d]], [m.cad[d]]
    got = {"loglike": npy(ll)[d], "gy": gy, "gdiag": npy(dt.grad)[d], "greal": npy(rt.grad)[d], "gpairs": npy(ct.grad)[d]}
    hold(f"gaussian_process, mean = {mean}", c, [(got, float(w[d]), *cad)])
