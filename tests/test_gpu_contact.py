"""GPU: the contact solver and the in-transit windows -- exo_contact_points_f64, the window slots of exo_pack_records_f64 /
ops.pack_records_cols and of the torch route KeplerianOrbit._transit_window, and what they decide in
get_light_curve(use_in_transit=True) and orbit.in_transit -- against the multiprecision fixture tests/golden/contact_mp.npz
(tools/make_contact_golden.py).  Definition, case table and allowances: tests/contact_cases.py (none from the code under test);
the same header on the host: tests/test_contact_host.py.  Every test prints worst error / allowance before it asserts."""
import numpy as np
import pytest
import torch

import contact_cases as K

pytestmark = pytest.mark.gpu

U = (0.3, 0.2)
U2, SBR = (0.4, 0.1), 0.3
TEXP = 0.02


@pytest.fixture(scope="module")
def g():
    return K.load()


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


def _off(x):
    """the same values in a view that starts 8 bytes into its allocation"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 == 8
    return v


# ------------------------------------------------------------------------------------------------------------------------
# ops.contact_points
# ------------------------------------------------------------------------------------------------------------------------
def contact(dev, inp, off=False):
    from exoplanet_amd import ops

    cols = [T(inp[:, k], dev) for k in range(7)]
    if off:
        cols = [_off(c) for c in cols]
    Ml, Mr, fl = ops.contact_points(*cols)
    return Ml.cpu().numpy(), Mr.cpu().numpy(), fl.cpu().numpy()


def hold(label, g, idx, Ml, Mr, fl):
    want_flag = g["flag"][idx] != 0
    assert np.array_equal(fl != 0, want_flag), [K.NAMES[i] for i in idx[(fl != 0) != want_flag]]
    ok = ~want_flag
    got = np.stack([Ml, Mr], axis=-1)
    err, tol = np.abs(got - g["M"][idx])[ok], K.allow_M(g)[idx][ok]
    K.report(label, lanes=idx.size, solved=ok.sum(), worst_error_over_allowance=err / tol if ok.any() else 0.0,
             worst_error=err if ok.any() else 0.0)
    assert np.all(err <= tol), [K.NAMES[i] for i in idx[ok][np.any(err > tol, axis=1)]]
    assert np.all(got[~ok] == 0.0)


def mixed_order(g):
    """a fixed permutation in which every wave of 64 lanes holds fast-path, bracketing and flagged entries"""
    kind = np.array([2 if f else (0 if K.fast_path(inp) == ("fast", "fast") else 1) for f, inp in zip(g["flag"], g["inputs"])])
    frac = np.zeros(kind.size)
    for k in range(3):                      # each kind dealt evenly over the whole order
        frac[kind == k] = (np.arange((kind == k).sum()) + 0.5) / (kind == k).sum()
    perm = np.argsort(frac, kind="stable")
    for k in range(0, perm.size, 64):
        assert set(kind[perm[k:k + 64]]) == {0, 1, 2}, k
    return perm


def test_contact_points_whole_fixture_in_two_orders(dev, g):
    idx = np.arange(len(K.CASES))
    a = contact(dev, g["inputs"])
    hold("contact_points, fixture order", g, idx, *a)
    perm = mixed_order(g)
    b = contact(dev, g["inputs"][perm])
    hold("contact_points, mixed waves", g, perm, *b)
    for x, y in zip(a, b):
        assert np.array_equal(x[perm], y)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_contact_points_odd_counts_off_alignment(n, dev, g):
    perm = mixed_order(g)
    full = contact(dev, g["inputs"][perm])
    got = contact(dev, g["inputs"][perm[:n]], off=True)
    hold(f"contact_points n={n}, inputs 8 bytes off", g, perm[:n], *got)
    for x, y in zip(full, got):
        assert np.array_equal(x[:n], y)


# ------------------------------------------------------------------------------------------------------------------------
# window slots of the packing kernels and of the torch route
# ------------------------------------------------------------------------------------------------------------------------
def layouts(idx):
    """(label, slots [D, P]) -- entries as draws; as planets (a draw holds EXO_MAX_PLANETS = 16 at the most, so (1, all) is
    one draw of 16 after another, the last wrapping round, and a single draw of 16 on its own); dealt over 5 x 7 blocks, the
    last one wrapping round"""
    n = idx.size
    blocks, rows = -(-n // 35), -(-n // 16)
    dealt = idx[np.arange(blocks * 35) % n].reshape(blocks * 5, 7)
    planets = idx[np.arange(rows * 16) % n].reshape(rows, 16)
    return [("all x 1", idx.reshape(n, 1)), ("all as planets, 16 a draw", planets), ("1 x 16", planets[-1:]), ("5 x 7 dealt", dealt)]


def hold_windows(label, g, slots, rec, secondary, circular):
    """slots TS, TE, TS2, TE2 of rec [D, P, NPAR] against the fixture"""
    from exoplanet_amd import ops

    got = rec[..., [ops.P_TS, ops.P_TE, ops.P_TS2, ops.P_TE2]].reshape(-1, 4)
    idx = slots.reshape(-1)
    if circular:
        want = g["circ_win"][idx].copy()
        tol = (K.allow_circ(g)[idx, None] + K.EPS * g["ctor"][idx, :1] * np.array([0.0, 0.0, 2.0, 2.0]))
    else:
        want, tol = g["win"][idx].copy(), K.allow_t(g)[idx]
    if not secondary:
        want[:, 2], want[:, 3] = -np.inf, np.inf
    fin = np.isfinite(want)
    if circular:
        # degenerate closed form (arg < 0 or x > 1): NaN, or infinite -- either way every cadence is solved
        deg = np.isnan(want)
        assert np.all(np.isnan(got[deg]) | np.isinf(got[deg]))
        want_inf = np.isinf(want)
    else:
        want_inf = ~fin
    assert np.array_equal(got[want_inf], want[want_inf]), label          # -inf / +inf exactly, where mp has no window
    assert np.all(np.isfinite(got[fin])), [K.NAMES[i] for i in idx[np.any(fin & ~np.isfinite(got), axis=1)]]
    with np.errstate(invalid="ignore"):            # (inf - inf in the slots without a window, which are not read)
        err = np.abs(got - want)[fin]
    ratio = err / tol[fin]
    K.report(label, slots=idx.size, windows=fin.sum(), worst_error_over_allowance=ratio, worst_error=err)
    bad = np.zeros_like(fin)
    bad[fin] = ratio > 1.0
    assert not bad.any(), [K.NAMES[i] for i in idx[bad.any(axis=1)]][:8]


@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("secondary", [False, True])
def test_pack_window_slots(dev, g, secondary, circular):
    from exoplanet_amd import ops

    idx = np.nonzero(g["circular"] == 1)[0] if circular else np.arange(len(K.CASES))
    flags = ops.FLAG_WINDOW | (ops.FLAG_SECONDARY if secondary else 0) | (ops.PACK_CIRCULAR if circular else 0)
    ld = [0.3, 0.2] + ([0.4, 0.1] if secondary else [])
    for label, slots in layouts(idx):
        D, Pn = slots.shape
        orbit_in = T(g["ctor"][slots], dev)
        rec, _ = ops.pack_records(orbit_in, T(np.tile(ld, (D, 1)), dev), flags)
        hold_windows(f"pack_records {label} sec={secondary} circ={circular}", g, slots, rec.cpu().numpy(), secondary, circular)
        cols = [orbit_in[..., k].contiguous() for k in range(ops.NIN)]
        rec2, _ = ops.pack_records_cols(cols, [T(x, dev).reshape(()) for x in ld], D, flags)
        hold_windows(f"pack_records_cols {label} sec={secondary} circ={circular}", g, slots, rec2.cpu().numpy(), secondary, circular)


def torch_orbit(dev, g, idx, circular, standard=True):
    """entries ``idx`` as draws of a one-planet orbit; (orbit, r [D, 1])"""
    import exoplanet_amd as xo

    c = g["ctor"][idx]
    col = lambda k: T(c[:, k:k + 1], dev)  # noqa: E731
    kw = dict(period=col(0), t0=col(1), b=col(2), m_star=col(6), r_star=col(7))
    if not circular:
        if standard:
            kw.update(ecc=col(3), omega=col(4))
        else:
            kw.update(ecc=col(3), cos_omega=T(np.cos(c[:, 4:5]), dev), sin_omega=T(np.sin(c[:, 4:5]), dev))
    orbit = xo.KeplerianOrbit(**kw)
    if not standard:
        orbit._standard = False
    return orbit, col(5)


@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("secondary", [False, True])
def test_torch_route_window_slots(dev, g, secondary, circular):
    """KeplerianOrbit._transit_window through kernel_records (a non-standard parameterisation: cos_omega, sin_omega)"""
    idx = np.nonzero(g["circular"] == 1)[0] if circular else np.arange(len(K.CASES))
    orbit, r = torch_orbit(dev, g, idx, circular, standard=False)
    assert not orbit._standard
    rec, _ = orbit.kernel_records(r, use_in_transit=True, secondary_sbr=SBR if secondary else None)
    hold_windows(f"torch route sec={secondary} circ={circular}", g, idx.reshape(-1, 1), rec.detach().cpu().numpy(), secondary, circular)


# ------------------------------------------------------------------------------------------------------------------------
# the consequence: which cadences are solved
# ------------------------------------------------------------------------------------------------------------------------
def batches(g):
    """the entries with contacts, split by what one call can hold: (circular, occultation) -> indices"""
    have = np.isfinite(g["cad_t"][:, 0])
    out = {}
    for circ in (0, 1):
        for sec in (0, 1):
            idx = np.nonzero(have & (g["circular"] == circ) & (g["sec"] == sec))[0]
            if idx.size:
                out[(circ, sec)] = idx
    assert sum(v.size for v in out.values()) == have.sum() >= 150      # no entry with contacts is left out
    return out


@pytest.mark.parametrize("texp", [None, TEXP])
def test_light_curve_in_transit_against_all_cadences(dev, g, texp):
    """get_light_curve(use_in_transit=True) against use_in_transit=False on the cadences the generator placed either side of
    every contact (all entries' cadences in one series: an entry also sees the others' as probes)"""
    import exoplanet_amd as xo

    n_in = n_faint = 0
    for (circ, sec), idx in batches(g).items():
        t = np.unique(g["cad_t"][idx].reshape(-1))
        orbit, r = torch_orbit(dev, g, idx, bool(circ))
        lc = xo.SecondaryEclipseLightCurve(U, U2, SBR) if sec else xo.LimbDarkLightCurve(*U)
        a = lc.get_light_curve(orbit=orbit, r=r, t=T(t, dev), texp=texp, use_in_transit=True)
        b = lc.get_light_curve(orbit=orbit, r=r, t=T(t, dev), texp=texp, use_in_transit=False)
        a, b = a.reshape(idx.size, t.size).cpu().numpy(), b.reshape(idx.size, t.size).cpu().numpy()
        diff = np.abs(a - b).max()
        # the cadences mp puts inside a window by more than the allowance
        lost = []
        for k, i in enumerate(idx):
            pos = np.searchsorted(t, g["cad_t"][i])
            inside = (g["cad_in"][i] != 0) & (g["cad_margin"][i] > K.allow_cadence(g, i, g["cad_t"][i]))
            # (and whose true flux float64 can tell from 0: contact_cases.flux_floor; the centre sample of an exposure carries 1/7)
            faint = inside & ~(K.flux_floor(g, i) / (1 if texp is None else 7) > K.FLUX_RESOLUTION)
            n_faint += int(faint.sum())
            inside &= ~faint
            assert inside.sum() >= 6, K.NAMES[i]                  # every entry keeps cadences that must be non-zero
            n_in += int(inside.sum())
            if np.any(a[k, pos[inside]] == 0.0):
                lost.append((K.NAMES[i], int(np.sum(a[k, pos[inside]] == 0.0)), int(np.sum(b[k, pos[inside]] == 0.0))))
        K.report(f"light curve circ={circ} sec={sec} texp={texp}", draws=idx.size, cadences=t.size, worst_difference=diff,
                 nonzero_windowed=(a != 0).sum(), nonzero_unwindowed=(b != 0).sum(), inside_cadences_lost=len(lost), inside_so_far=n_in, below_float64_so_far=n_faint)
        assert not lost, lost[:8]
        assert np.array_equal(a != 0, b != 0), [K.NAMES[idx[k]] for k in np.nonzero(np.any((a != 0) != (b != 0), axis=1))[0]][:8]
        assert diff <= 4e-15
    assert n_in >= 150 * 20


@pytest.mark.parametrize("texp", [None, TEXP])
def test_in_transit_index_sets(dev, g, texp):
    """orbit.in_transit(t, r, texp) of every entry with contacts, unbatched: the index set of the mp contacts on the cadences at
    least 10 allowances from a (padded) contact -- which excludes none of the placed cadences"""
    import exoplanet_amd as xo

    excluded = n_ent = 0
    worst = 0.0
    for i in np.nonzero(np.isfinite(g["cad_t"][:, 0]))[0]:
        c = g["ctor"][i]
        kw = dict(period=T([c[0]], dev), t0=T([c[1]], dev), b=T([c[2]], dev), m_star=float(c[6]), r_star=float(c[7]))
        if not g["circular"][i]:
            kw.update(ecc=T([c[3]], dev), omega=T([c[4]], dev))
        t = g["cad_t"][i]
        got = np.zeros(K.N_CAD, dtype=bool)
        got[xo.KeplerianOrbit(**kw).in_transit(T(t, dev), r=T([c[5]], dev), texp=texp).cpu().numpy()] = True
        win = g["circ_win"][i] if g["circular"][i] else g["win"][i]
        dt = np.mod(t - c[1] + 0.5 * c[0], c[0]) - 0.5 * c[0]
        h = 0.0 if texp is None else 0.5 * texp
        edge = np.minimum(dt - win[0], win[1] - dt) + h          # + inside the padded transit window
        tol = K.allow_cadence(g, i, t)
        clear = np.abs(edge) >= 10 * tol
        excluded += int((~clear).sum())
        worst = max(worst, float((tol / np.abs(edge)).max()))
        assert np.array_equal(got[clear], (edge > 0)[clear]), K.NAMES[i]
        n_ent += 1
    K.report(f"in_transit texp={texp}", entries=n_ent, excluded=excluded, worst_allowance_over_distance=worst)
    assert n_ent >= 150 and excluded == 0
