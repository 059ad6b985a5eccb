"""CPU: the celerite log-likelihood and its reverse pass against the multiprecision fixture tests/golden/gp_like_mp.npz
(tools/make_gp_like_golden.py; entries, quantities, yardstick and tolerance: tests/gp_like_cases.py).

* the float64 yardstick (oracle.c_port.celerite with grad) reproduces its stored units and stays under the cap;
* oracle.numpy_port.celerite_loglike (the value) and gp_loglike_dense (float64 dense Cholesky) are held to the fixture;
* the lane pipeline the device runs one lane per (draw, chunk), compiled for the host (tests/gp_host_harness.cpp: J <= 6), by the
  rule the GPU tests use -- error <= max(16 unit, 1e-13) in the scale of the quantity -- with the serial reference scans on the
  default plan and with the trees on the forced chunk counts;
* the same pipeline reading the series cadence-major (batches of five, the entry at 1 and 3) and as a sparse model (every layout of
  gp_like_cases.SPARSE_LAYOUTS x both descriptor forms x both forms of ``off``), by the same rule on the default plan and on the
  forced chunk counts: NaN in every value no segment covers, a sentinel in gvals that every uncovered position keeps bit for bit;
* the table of excluded (entry, route) pairs of tests/test_gpu_gp_like.py stays under its share."""
import os

import numpy as np
import pytest

import gp_like_cases as K
from gp_cond_cases import error
from oracle import numpy_port as P
from test_gp_host import harness, run, run_sparse  # noqa: F401

LARGEST_FIXTURE = "diagnostics_mp.npz"


@pytest.fixture(scope="module")
def gold():
    return K.load()


def test_fixture_is_complete(gold):
    assert os.path.getsize(os.path.join(K.GOLD, "gp_like_mp.npz")) < os.path.getsize(os.path.join(K.GOLD, LARGEST_FIXTURE))
    assert not K.ENTRY_FACTOR
    widths = set()
    for name in K.ENTRIES:
        c = K.Case(gold, name)
        want = K.inputs(name)           # the fixture holds the inputs the cases file describes
        for k in ("t", "diag", "coef_real", "pairs", "pair_kind"):
            assert np.array_equal(getattr(c, k), want[k]) and getattr(c, k).dtype == want[k].dtype, (name, k)
        assert c.n == K.SPEC[name].get("n", K.N) and np.all(np.diff(c.t) >= 0)
        assert all(v.dtype == np.float64 and v.ndim <= 2 for k, v in gold.items() if k.startswith(name + "_") and "kind" not in k)
        for q in K.QUANTITIES:
            assert np.all(np.isfinite(c.want[q])) and np.all(c.scale[q] >= 0), (name, q)
            assert np.shape(c.scale[q]) == (c.want[q].shape if q in ("greal", "gpairs") else ()), (name, q)
        # every complex term is a valid kernel; the default plan does with the draw what the entry is there for
        kd0 = c.pair_kind == 0
        assert np.all(np.abs(c.pairs[kd0, 1] * c.pairs[kd0, 3]) <= c.pairs[kd0, 0] * c.pairs[kd0, 2] * (1 + 1e-12)), name
        assert K.expected_route(c) == K.route(name), (name, c.score())
        print(f"{name}: N = {c.n}, J = {c.J}, score = {c.score():.3g}, route = {K.route(name)}")
        if name in K.LADDER:
            assert c.score() < K.SCORE_WIDE and c.n == K.N
            widths.add((len(c.coef_real), len(c.pairs)))
    assert {jr + 2 * jc for jr, jc in widths} == set(range(1, 17)) and {(0, 2), (2, 1), (1, 1)} <= widths
    assert len(K.sho_of("kinds_j6")) == 3 and list(K.Case(gold, "kinds_j6").pair_kind) == [0, 0, 1]


def test_excluded_pairs_stay_under_their_share():
    pairs = [(e, r) for e in K.ENTRIES for r in K.ROUTES]
    assert set(K.EXCLUDED) <= set(pairs) and all(reason for _, reason in K.EXCLUDED.values())
    assert set(K.HOST_EXCLUDED) <= set(K.ENTRIES)
    print(f"{len(K.EXCLUDED)} of {len(pairs)} (entry, route) pairs excluded")
    assert len(K.EXCLUDED) <= K.MAX_EXCLUDED * len(pairs)


@pytest.mark.parametrize("name", K.ENTRIES)
def test_yardstick_reproduces_its_units(gold, name):
    """oracle.c_port.celerite(grad=True): the stored unit is its error, and 16 x unit stays under the cap"""
    c = K.Case(gold, name)
    got = K.yardstick(c)
    for q in K.QUANTITIES:
        err = error(c, q, got[q])
        print(f"{name} {q}: unit = {c.unit[q]:.3g}, measured = {err:.3g}")
        # (the same arithmetic on the same inputs; an exp of another libm may differ in the last bits)
        assert err <= 2 * c.unit[q] + 1e-15, (name, q, err, c.unit[q])
        assert K.FACTOR * c.unit[q] <= K.CAP, (name, q, c.unit[q])


@pytest.mark.parametrize("name", K.ENTRIES)
def test_numpy_ports_hold_the_fixture(gold, name):
    """the value by the recurrences in numpy; value and gradients by float64 dense Cholesky and the analytic dense gradient.

    The dense port evaluates cos and sin of d |t_i - t_j| over the WHOLE span, the recurrences only over single steps: the
    rounding of that argument alone is a phase error of eps * d * span (fast_osc: 2.2e-16 x 53 / d x 34 d = 4e-13), which the
    unit -- a property of the recurrences -- does not know.  So the dense port's unit is max(unit, eps * max d * span)."""
    c = K.Case(gold, name)
    K.check("numpy recurrences", c, {"loglike": np.float64(P.celerite_loglike(c.t, c.y, c.diag, c.coeffs()))})
    rate = c.pairs[c.pair_kind == 0, 3]
    phase = np.finfo(np.float64).eps * (rate.max() if rate.size else 0.0) * (c.t[-1] - c.t[0])
    c.unit = {q: max(u, phase) for q, u in c.unit.items()}
    K.check("numpy dense", c, K.quantities_of(c, *P.gp_loglike_dense(c.t, c.y, c.diag, c.coeffs())))


@pytest.mark.parametrize("name", K.ENTRIES)
def test_lane_pipeline_holds_the_fixture(gold, harness, name):  # noqa: F811
    """elements, scans over the chunks, checkpointed recurrences, adjoint scan, recomputing reverse recurrences -- for every
    entry whose width the harness instantiates (J <= 6) and whose series is cut (N >= 64): the serial reference scans on the
    default plan, the device's scans on the default plan and on forced chunk counts; a draw flagged for the robust route takes
    it, as on the device; one flagged for the sequential kernels has nothing to show here (the harness has none).  The
    quantities of gp_like_cases.HOST_EXCLUDED are printed, not asserted"""
    c = K.Case(gold, name)
    if c.J > K.LANE_MAX_J or c.n < 64:
        assert K.route(name) == "seq" or c.J > K.LANE_MAX_J
        return
    # (the serial reference scans stand in for the trees: a draw on the robust route uses neither)
    modes = [("serial scans", 0, 1)] if K.route(name) == "tree" else []
    for label, n_chunks, serial in modes + [("default plan", 0, 0)] + [(f"{C} chunks", C, 0) for C in K.FORCED]:
        harness.harness_set_serial_scan(serial)
        try:
            ll, flags, C_used, g = run(harness, c.t, c.y[None], c.diag[None], c.coef_real[None], c.pairs[None], c.pair_kind[None],
                                       n_chunks=n_chunks, gll=np.ones(1))
        finally:
            harness.harness_set_serial_scan(0)
        assert flags[0] == {"tree": 0.0, "robust": 1.0, "seq": 2.0}[K.route(name)], (name, flags)
        if flags[0] == 2.0:
            continue
        assert C_used == min(n_chunks, c.n // 32) or n_chunks == 0
        got = {"loglike": ll[0], "gy": g["y"][0], "gdiag": g["diag"][0], "greal": g["real"][0], "gpairs": g["cplx"][0]}
        K.check(f"host pipeline ({label})", c, got, skip=K.HOST_EXCLUDED.get(name, ()))
        # (the sum over the cadences the device returns for a diagonal shared by every draw: N terms, each within the rule)
        assert abs(g["diag_sum"][0] - c.want["gdiag"].sum()) <= c.n * K.tol(c, "gdiag") * c.scale["gdiag"]


def _lane_entry(gold, name):
    """the entry where the harness has something to show for it: its width instantiated, the series cut, the draw not one
    the device redoes sequentially"""
    c = K.Case(gold, name)
    if c.J > K.LANE_MAX_J or c.n < 64 or K.route(name) == "seq":
        return None
    return c


PLANS = (("default plan", 0),) + tuple((f"{C} chunks", C) for C in K.FORCED)


@pytest.mark.parametrize("name", K.ENTRIES)
def test_cadence_major_holds_the_fixture(gold, harness, name):  # noqa: F811
    """the series as a [cadence][draw] array (Series::cm) against the DEFINITION, not against the row-major route: batches of
    five draws with the entry at positions 1 and 3 between benign ones, cotangent linspace(0.5, 1.5, D); the model of an entry
    draw is -y / 2 against obs = y / 2 (exactly y); gy is minus the model's cotangent, read in the model's own layout"""
    c = _lane_entry(gold, name)
    if c is None:
        return
    D, at = K.BATCH, (1, 3)
    y, diag, real, pairs = K.batch(c, D, at)
    model = y.copy()
    model[list(at)] = -0.5 * c.y
    kind = np.broadcast_to(c.pair_kind, (D, len(c.pairs)))
    w = np.linspace(0.5, 1.5, D)
    for label, n_chunks in PLANS:
        ll, flags, C_used, g = run(harness, c.t, model, diag, real, pairs, kind, obs=0.5 * c.y, n_chunks=n_chunks, gll=w,
                                   cadence_major=True)
        assert C_used == min(n_chunks, c.n // 32) or n_chunks == 0
        for k, d in enumerate(at):
            assert flags[d] == {"tree": 0.0, "robust": 1.0}[K.route(name)], (name, flags)
            got = {"loglike": ll[d], "gy": -g["y"][d], "gdiag": g["diag"][d], "greal": g["real"][d], "gpairs": g["cplx"][d]}
            K.check(f"host cadence-major ({label})[{k}]", c.weighted(w[d]), got, skip=K.HOST_EXCLUDED.get(name, ()))


def _sparse_hold(label, harness, c, name, layout, form, offs, n_chunks):  # noqa: F811
    obs, sp = K.sparse_entry(c, layout, form, offs)
    assert np.isnan(sp.vals[0, sp.untouched(0)]).all() and np.array_equal(obs - sp.dense(0), c.y)
    ll, flags, C_used, g = run_sparse(harness, c.t, sp, c.diag[None], c.coef_real[None], c.pairs[None], c.pair_kind[None], obs=obs,
                                      n_chunks=n_chunks, gll=np.ones(1), gfill=K.SENTINEL)
    assert flags[0] == {"tree": 0.0, "robust": 1.0}[K.route(name)], (name, flags)
    assert C_used == min(n_chunks, c.n // 32) or n_chunks == 0
    # positions of gvals no segment covers: as they were, bit for bit; every covered one -- a padded +0.0 too -- holds -gy
    gv = g["y"][0]
    assert np.array_equal(gv[sp.untouched(0)].view(np.int64), np.full(int(sp.untouched(0).sum()), K.SENTINEL).view(np.int64)), \
        (name, layout, form, offs, n_chunks)
    got = {"loglike": ll[0], "gy": -gv[sp.pos[0]], "gdiag": g["diag"][0], "greal": g["real"][0], "gpairs": g["cplx"][0]}
    K.check(f"host sparse ({layout}, {form}, {offs}, {label})", K.restricted(c, sp.cad[0]), got, skip=K.HOST_EXCLUDED.get(name, ()))
    assert abs(g["diag_sum"][0] - c.want["gdiag"].sum()) <= c.n * K.tol(c, "gdiag") * c.scale["gdiag"]


@pytest.mark.parametrize("name", K.ENTRIES)
def test_sparse_mean_holds_the_fixture(gold, harness, name):  # noqa: F811
    """the model as segments of cadences + values (gp::SparseSegs) against the DEFINITION: one draw carrying the entry in every
    layout of gp_like_cases.SPARSE_LAYOUTS x both descriptor forms x both forms of ``off``, on the default plan and on forced
    chunk counts; obs = where(H, y / 2, y), the values -y / 2 on H and +0.0 where a segment is wider than H: obs - model is y
    exactly.  Quantities as for obs_minus_model with gy[n] = -gvals at the covered cadences; gvals is prefilled with a sentinel,
    which every position no segment covers must keep bit for bit; the uncovered positions of vals hold NaN"""
    c = _lane_entry(gold, name)
    if c is None:
        return
    for layout in K.SPARSE_LAYOUTS:
        for form, offs in K.SPARSE_VARIANTS:
            for label, n_chunks in PLANS:
                _sparse_hold(label, harness, c, name, layout, form, offs, n_chunks)


def test_sparse_layouts_are_what_they_say():
    """the builder itself: ascending disjoint segments inside the series at n = 1, 2, 63, 161 and 193; padded covers the H of
    blocks with +0.0 around it; the poison sits where nothing should read"""
    for n in (1, 2, 63, 64, 161, 193):
        for layout in K.SPARSE_LAYOUTS:
            segs, H = K.sparse_segments(layout, n)
            assert all(0 <= lo < hi <= n for lo, hi in segs) and all(a[1] <= b[0] for a, b in zip(segs, segs[1:])), (layout, n)
            cover = np.zeros(n, bool)
            for lo, hi in segs:
                cover[lo:hi] = True
            assert np.array_equal(cover, H) or (layout == "padded" and np.all(cover[H]) and (n < 7 or cover.sum() > H.sum()))
            assert (layout == "none") == (not segs)
        assert np.array_equal(K.sparse_segments("padded", n)[1], K.sparse_segments("blocks", n)[1])
        assert K.sparse_segments("whole", n)[1].all()
    assert K.sparse_segments("touching", 161)[0] == [(0, 40), (40, 41), (41, 161)]
    assert K.sparse_segments("padded", 161)[0][:3] == [(0, 6), (6, 13), (13, 20)]
    for form, offs in K.SPARSE_VARIANTS:
        m = K.sparse_model(161, [("blocks", np.ones(161)), ("none", np.ones(161)), ("comb", np.ones(161))], form, offs)
        assert m.seg.shape[1] == m.nseg.max() + 2 and np.all(m.seg[1] == K.SEG_POISON) and np.all(m.off[1] == K.SEG_POISON)
        if form == "sweep":
            assert np.all(m.seg[:, :, 1:3] == K.SEG_POISON)
        for d in range(3):
            assert np.isnan(m.vals[d, m.untouched(d)]).all() and np.all(m.vals[d, m.pos[d]] == 1.0)
            assert (m.off[d, 0] != 0) == (offs == "gaps") or m.nseg[d] == 0
