"""GPU: the orbit-side kernels -- exo_kepler_f64 with the torch reverse pass of ops.kepler, exo_radial_velocity_{fwd,vjp}_f64,
exo_orbit_vector_{fwd,vjp}_f64 in all three modes -- against the multiprecision fixture tests/golden/orbit_mp.npz
(tools/make_orbit_golden.py) and, for the Kepler op, tests/golden/kepler.npz with all six of its arrays: |M| up to 7e8,
e up to 1 - 1e-12 (Kepler) / 0.999 with gradients and 1 - 1e-8 values only (RV, vectors), BJD-sized times with t_periastron
beside them and at 0.3, omega on the quadrants, edge-on, face-on, circular beside eccentric in one wave; every launch route
of the two elementwise ops (pairs, pairs + tail, scalar; odd counts; inputs and outputs 8 bytes off 16-byte alignment; a
second grid pass) and the grid-stride loop of the RV / vector kernels past their 65 536-block cap.

Tolerances are derived in tests/orbit_mp_cases.py, none from the code under test; every test prints unit, tolerance and error
before it asserts.  exo_contact_points_f64 is exercised for shapes and odd counts here, against the float64 oracle; its values,
flags and the windows built on them are held to tests/golden/contact_mp.npz by tests/test_gpu_contact.py.  The public KeplerianOrbit methods are held for the systems
whose record they reproduce (the RV with K: values of all, gradients where the class's own 2 pi / period equals the record's
mean motion to the bit; the nine vector methods: the edge-on systems without a node rotation); elsewhere only the op level is
covered."""
import numpy as np
import pytest
import torch

import orbit_mp_cases as K
from oracle import numpy_port as P

pytestmark = pytest.mark.gpu

OPS = ("rv",) + K.MODES


@pytest.fixture(scope="module")
def g():
    return K.load()


def T(a, dev, grad=False):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev).requires_grad_(grad)


def run_op(op, t, params):
    from exoplanet_amd import ops

    if op == "rv":
        return ops.radial_velocity(t, params)
    return ops.orbit_vector(t, params, velocity=op == "vel", acceleration=op == "acc")


# ------------------------------------------------------------------------------------------------------------------------
# ops.kepler: values and reverse pass
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["r1", "wide"])
def test_kepler_values_and_reverse(which, dev, g):
    """sin f, cos f and, by torch.autograd.grad with cotangents (1, 0), (0, 1) and a random pair, all four partials entry by
    entry.  Formula of the allowance: orbit_mp_cases (module docstring): 16 x the float64 closed form's own error on the
    same points, floor 8 ulp, widened by the value bound propagated through the closed form (divided by 1 + e cos f where that
    cancels)."""
    from exoplanet_amd import ops

    pts = K.kepler_points(g, which)
    M, e = T(pts[0], dev, True), T(pts[1], dev, True)
    s, c = ops.kepler(M, e)
    vtol = K.kepler_value_tol(pts)
    err = np.maximum(np.abs(s.detach().cpu().numpy() - pts[3]), np.abs(c.detach().cpu().numpy() - pts[4]))
    K.report(f"kepler[{which}] values", n=pts[0].size, worst_error_over_tol=err / vtol, worst_tol=vtol)
    assert np.all(err <= vtol)
    (tsM, tcM, tse, tce), u = K.kepler_partial_tol(pts)
    dsM, dcM, dse, dce = pts[5:]
    rng = np.random.default_rng(41)
    hard = pts[1] >= 1 - 1e-6
    for label, a, b in (("(1,0)", np.ones_like(dsM), np.zeros_like(dsM)), ("(0,1)", np.zeros_like(dsM), np.ones_like(dsM)),
                        ("random", rng.normal(size=dsM.shape), rng.normal(size=dsM.shape))):
        gM, ge = torch.autograd.grad((s * T(a, dev) + c * T(b, dev)).sum(), (M, e), retain_graph=True)
        for name, got, want, tol in (("d/dM", gM, a * dsM + b * dcM, np.abs(a) * tsM + np.abs(b) * tcM),
                                     ("d/de", ge, a * dse + b * dce, np.abs(a) * tse + np.abs(b) * tce)):
            d = np.abs(got.cpu().numpy() - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(tol > 0, d / tol, np.where(d == 0, 0.0, np.inf))
                rel = np.where(want != 0, d / np.abs(want), 0.0)
            K.report(f"kepler[{which}] {label} {name}", closed_form_unit=max(x.max() for x in u), worst_error_over_tol=ratio,
                     worst_relative_error=rel, worst_relative_error_at_e_ge_1m1e6=rel[hard] if hard.any() else 0.0)
            assert np.all(ratio <= 1.0), (label, name, float(ratio.max()), int(ratio.argmax()))


# ------------------------------------------------------------------------------------------------------------------------
# ops.radial_velocity / ops.orbit_vector: any arrangement of the fixture's systems as (draw, planet) slots
# ------------------------------------------------------------------------------------------------------------------------
_UNIT = {}


def unit_of(g, i, op):
    if (i, op) not in _UNIT:
        _UNIT[(i, op)] = K.oracle_unit(g, i, op)
    return _UNIT[(i, op)]


def arrangement(g, op, slots):
    """(t, params [D, P, npar], gout, blocks): the systems of ``slots`` [D, P], each at its own epochs inside the concatenated
    series -- an element off a system's own epochs has no expectation and gets no cotangent"""
    slots = np.asarray(slots)
    D, Pn = slots.shape
    systems = sorted(set(int(i) for i in slots.ravel()))
    N = g["t"].shape[1]
    off = {i: k * N for k, i in enumerate(systems)}
    t = np.concatenate([g["t"][i] for i in systems])
    params = np.stack([[K.case(g, int(i), op)[0] for i in row] for row in slots])
    tail = () if op == "rv" else (3,)
    gout = np.zeros((D, t.size, Pn) + tail)
    for d in range(D):
        for p in range(Pn):
            i = int(slots[d, p])
            gout[d, off[i]:off[i] + N, p] = K.cotangent(i, op, (N,) + tail)
    return t, params, gout, off


def check(dev, g, op, slots, label):
    """values of every slot, VJPs of the slots with e <= 0.999, against the fixture"""
    slots = np.asarray(slots)
    t, params, gout, off = arrangement(g, op, slots)
    N = g["t"].shape[1]
    pt = T(params, dev, True)
    out = run_op(op, T(t, dev), pt)
    (gp,) = torch.autograd.grad((out * T(gout, dev)).sum(), pt)
    out_h, gp = out.detach().cpu().numpy(), gp.cpu().numpy()
    worst = dict(value_error_over_tol=0.0, vjp_error=0.0, vjp_error_over_tol=0.0, unit=0.0)
    bad = []
    for d in range(slots.shape[0]):
        for p in range(slots.shape[1]):
            i = int(slots[d, p])
            rec, want, J = K.case(g, i, op)
            rv = float(np.max(np.abs(out_h[d, off[i]:off[i] + N, p] - want) / K.value_tol(g, i, op)))
            worst["value_error_over_tol"] = max(worst["value_error_over_tol"], rv)
            if not rv <= 1.0:
                bad.append(("value", d, p, i, rv))
            if g["sys_grad"][i]:
                unit = unit_of(g, i, op)
                gw, den = K.vjp_want(J, K.cotangent(i, op, want.shape))
                rg = np.abs(gp[d, p] - gw) / den
                worst["vjp_error"] = max(worst["vjp_error"], float(rg.max()))
                worst["unit"] = max(worst["unit"], float(unit.max()))
                worst["vjp_error_over_tol"] = max(worst["vjp_error_over_tol"], float((rg / K.vjp_tol(unit)).max()))
                if not np.all(rg <= K.vjp_tol(unit)):
                    bad.append(("vjp", d, p, i, rg.tolist()))
    K.report(f"{op} {label} ({slots.shape[0]} x {t.size} x {slots.shape[1]})", vjp_tol_floor=K.VJP_FLOOR, **worst)
    assert not bad, bad[:5]
    return out.detach(), t, params


@pytest.mark.parametrize("op", OPS)
def test_every_system_alone(op, dev, g):
    for i in range(K.n_systems(g)):
        check(dev, g, op, [[i]], f"system {i} alone")


@pytest.mark.parametrize("op", OPS)
def test_all_systems_as_planets_of_one_draw(op, dev, g):
    """circular (e = 0 exactly) and eccentric records alternate inside every wave: kepler_half's vote on e == 0 is false"""
    check(dev, g, op, [list(range(K.n_systems(g)))], "all systems, one draw")


@pytest.mark.parametrize("op", OPS)
def test_all_circular_subset(op, dev, g):
    """only the e = 0 systems: the vote is true in every wave"""
    circ = [i for i in range(K.n_systems(g)) if g["rv_params"][i, 2] == 0.0]
    assert len(circ) == 3
    check(dev, g, op, [circ], "circular systems")


@pytest.mark.parametrize("op", OPS)
def test_draws_times_planets_not_a_round_number(op, dev, g):
    """5 draws x 7 planets = 35 records, the systems dealt round the slots"""
    S = K.n_systems(g)
    slots = (np.arange(35) * 5 % S).reshape(5, 7)
    check(dev, g, op, slots, "5 draws x 7 planets")


# ------------------------------------------------------------------------------------------------------------------------
# the grid-stride loop past the 65 536-block cap of rv_fwd_kernel / ov_fwd_kernel; long reverse reductions
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_forward_beyond_the_block_cap(op, dev, g):
    """7 draws x (209 x 480) epochs x 24 planets = 16 853 760 elements > 65 536 x 256: every draw and every tile of the epochs
    bit-identical to the small call (the same kernel; every wave of either call holds circular and eccentric lanes alike, so
    the vote agrees), which itself is held to the fixture by check()"""
    S = K.n_systems(g)
    small, t, params = check(dev, g, op, [list(range(S))], "small call of the block-cap test")
    D, tiles = 7, 209
    assert D * tiles * t.size * S > 65536 * 256
    big = run_op(op, T(np.tile(t, tiles), dev), T(np.tile(params, (D, 1, 1)), dev))
    torch.cuda.synchronize()
    view = big.view((D, tiles) + tuple(small.shape[1:]))
    same = bool((view == small.unsqueeze(0)).all())
    K.report(f"{op} beyond the block cap", elements=big.numel() // (1 if op == "rv" else 3), bit_identical=float(same))
    assert same


@pytest.mark.parametrize("op", OPS)
def test_reverse_over_3e5_epochs_is_the_sum_of_its_pieces(op, dev, g):
    """the VJP over 300 000 epochs against the sum of the VJPs of five pieces: 16 x 2.3e-16 x sum |terms| (256 lanes of ~1200
    terms each, then the tree: the partial sums differ only by the order of addition)"""
    S = K.n_systems(g)
    t0, params, _, _ = arrangement(g, op, [list(range(S))])
    tiles, pieces = 625, 5
    t = T(np.tile(t0, tiles), dev)
    N = t.numel()
    assert N == 300000
    gen = torch.Generator(device=dev).manual_seed(5)
    tail = () if op == "rv" else (3,)
    gout = torch.randn((1, N, S) + tail, dtype=torch.float64, device=dev, generator=gen)
    pt = T(params, dev, True)
    (full,) = torch.autograd.grad((run_op(op, t, pt) * gout).sum(), pt)
    parts = torch.zeros_like(full)
    step = N // pieces
    for k in range(pieces):
        sl = slice(k * step, (k + 1) * step)
        (gk,) = torch.autograd.grad((run_op(op, t[sl].contiguous(), pt) * gout[:, sl].contiguous()).sum(), pt)
        parts += gk
    # sum |g_n| |d v_n / d p| with the float64 oracle's Jacobian (a magnitude) on the 480 distinct epochs
    if op == "rv":
        _, J = P.radial_velocity(t0, params, jac=True)
    else:
        _, J = P.orbit_vector(t0, params, K.MODES.index(op), jac=True)
    gabs = gout.abs().view((tiles, t0.size, S) + tail).sum(0).cpu().numpy()
    terms = np.einsum("npk,np->pk" if op == "rv" else "npck,npc->pk", np.abs(J[0]), gabs)
    err = np.abs((full - parts).cpu().numpy()[0])
    tol = 16 * K.EPS * terms
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    K.report(f"{op} reverse over {N} epochs", worst_error_over_tol=ratio, worst_error_over_terms=np.where(terms > 0, err / np.where(
        terms > 0, terms, 1), 0.0), tol_over_terms=16 * K.EPS)
    assert np.all(ratio <= 1.0), float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------------
# public-method layer
# ------------------------------------------------------------------------------------------------------------------------
M_STAR, R_STAR, M_PLANET = 1.1, 0.9, 3e-4


def _orbit(dev, g, i, grad=False, **kw):
    """(orbit, [t_periastron, ecc, cos_omega, sin_omega] leaves)"""
    import exoplanet_amd as xo

    rec = g["ov_params"][i]
    one = lambda v, grad=False: T([v], dev, grad)  # noqa: E731
    leaves = [one(rec[k], grad) for k in (1, 2, 3, 4)]
    orbit = xo.KeplerianOrbit(period=one(g["sys_period"][i]), t_periastron=leaves[0], ecc=leaves[1], cos_omega=leaves[2],
                              sin_omega=leaves[3], m_star=M_STAR, r_star=R_STAR, m_planet=one(M_PLANET), **kw)
    return orbit, leaves


def test_get_radial_velocity_with_K(dev, g):
    """KeplerianOrbit(period, t_periastron, ecc, cos_omega, sin_omega).get_radial_velocity(t, K): every slot of the record
    is passed through as given except the mean motion, which the class forms as (1 / period) 2 pi on the device -- one ulp
    from the record's fl(2 pi / period) for most periods.  Values of all systems: the expectation is the fixture moved to the
    orbit's own n to first order, rv + (d rv / d n)(n_orbit - n_record), with the fixture's d rv / d n (the second order is
    (1e-16 |M|)^2); the allowance is unchanged.  Cotangents of (t_periastron, ecc, cos_omega, sin_omega, K) for e <= 0.999:
    only where n is reproduced exactly (one ulp of n moves a gradient of the |M| ~ 3e7 layout by 3e-9 of itself); elsewhere
    only the op level holds them."""
    worst_v = worst_g = 0.0
    exact = 0
    for i in range(K.n_systems(g)):
        rec, want, J = K.case(g, i, "rv")
        orbit, leaves = _orbit(dev, g, i, grad=True, b=0.0)
        dn = float(orbit.n[0]) - rec[0]
        assert abs(dn) <= 2 * K.ULP * rec[0], (i, dn)
        Kt = T([rec[5]], dev, True)
        rv = orbit.get_radial_velocity(T(g["t"][i], dev), K=Kt)
        r = float(np.max(np.abs(rv.detach().cpu().numpy() - (want + J[:, 0] * dn)) / K.value_tol(g, i, "rv")))
        worst_v = max(worst_v, r)
        assert r <= 1.0, (i, r)
        if g["sys_grad"][i] and dn == 0.0:
            exact += 1
            go = K.cotangent(i, "rv", want.shape)
            grads = torch.autograd.grad((rv * T(go, dev)).sum(), leaves + [Kt])
            gw, den = K.vjp_want(J, go)
            unit = unit_of(g, i, "rv")
            rg = np.abs(np.array([float(x[0]) for x in grads]) - gw[1:]) / den[1:]
            worst_g = max(worst_g, float((rg / K.vjp_tol(unit)[1:]).max()))
            assert np.all(rg <= K.vjp_tol(unit)[1:]), (i, rg)
    K.report("get_radial_velocity(K)", value_error_over_tol=worst_v, gradient_systems_with_exact_n=exact, vjp_error_over_tol=worst_g)
    assert exact >= 1


def test_vector_methods_where_the_record_maps(dev, g):
    """the nine get_{star,planet,relative}_{position,velocity,acceleration}: KeplerianOrbit(b=0, Omega=None) gives cos i = 0,
    sin i = 1, no node rotation, so the edge-on systems without a node rotation are reproduced exactly up to the amplitude,
    in which the vector is linear: expectation = fixture x (the orbit's own amplitude / the fixture's), allowance = the value
    tolerance scaled alike + 2 ulp of the expectation for that scaling.  Values only; other systems: op level only."""
    maps = [i for i in range(K.n_systems(g))
            if tuple(g["ov_params"][i, 5:7]) == (0.0, 1.0) and tuple(g["ov_params"][i, 8:10]) == (1.0, 0.0)]
    assert len(maps) >= 4
    worst = 0.0
    for i in maps:
        orbit, _ = _orbit(dev, g, i, b=0.0)
        rec = g["ov_params"][i]
        assert float(orbit.n[0]) == rec[0] and float(orbit.cos_incl[0]) == 0.0 and float(orbit.sin_incl[0]) == 1.0
        t = T(g["t"][i], dev)
        for body, a, m in (("star", orbit.a_star, orbit.m_planet), ("planet", orbit.a_planet, -orbit.m_star),
                           ("relative", -orbit.a, -orbit.m_total)):
            amps = dict(pos=a, vel=orbit.K0 * m, acc=(orbit.K0 * m) ** 2 / a)
            for op, kind in zip(K.MODES, ("position", "velocity", "acceleration")):
                got = torch.stack(getattr(orbit, f"get_{body}_{kind}")(t), dim=-1).cpu().numpy()
                scale = float(amps[op][0]) / rec[7]
                want = K.case(g, i, op)[1] * scale
                tol = K.value_tol(g, i, op) * abs(scale) + 2 * K.ULP * np.abs(want)
                r = float(np.max(np.abs(got - want) / tol))
                worst = max(worst, r)
                assert r <= 1.0, (i, body, kind, r)
    K.report("vector methods", systems=len(maps), value_error_over_tol=worst)


# ------------------------------------------------------------------------------------------------------------------------
# launch routes of exo_kepler_f64 and exo_quad_solution_vector_f64
# ------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 2047, 2048, 2049, 4097]
KEPLER_BIG = 2 * 256 * 16 * 256 + 4099          # past one grid pass of the pair kernel, odd
QUAD_BIG = 2 * 256 * 8 * 256 + 2051


def _off(x):
    """the same values in a view that starts 8 bytes into its allocation"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 == 8
    return v


def _poison(n, dev, blocks=6):
    """leave NaN in the allocator's free blocks of this size: the ops allocate their outputs with torch.empty, and a block
    that still held a previous route's correct values would hide an element that a route never wrote"""
    junk = [torch.full((n,), float("nan"), dtype=torch.float64, device=dev) for _ in range(blocks)]
    del junk


def test_kepler_launch_routes(dev, g):
    """pair kernel, pair kernel + one-element tail, scalar kernel (n / 2 < 1024 or any pointer only 8-byte aligned), second
    grid pass; every element is a fixture point and meets the tolerance of the plain call (no bit equality between routes:
    the compiler contracts multiply-adds per kernel)"""
    from exoplanet_amd import ops

    r1, wide = K.kepler_points(g, "r1"), K.kepler_points(g, "wide")
    pts = tuple(np.concatenate([a, b]) for a, b in zip(r1, wide))
    vtol = K.kepler_value_tol(pts)
    for n in SIZES + [KEPLER_BIG]:
        idx = np.arange(n) % pts[0].size
        M, e = T(pts[0][idx], dev), T(pts[1][idx], dev)
        assert M.data_ptr() % 16 == 0 and e.data_ptr() % 16 == 0
        want_s, want_c, tol = pts[3][idx], pts[4][idx], vtol[idx]
        routes = {"aligned": lambda: ops.kepler(M, e), "M off": lambda: ops.kepler(_off(M), e),
                  "e off": lambda: ops.kepler(M, _off(e))}
        for out_off in ("sinf off", "cosf off"):        # unaligned outputs: only through the C ABI
            def raw(out_off=out_off):
                nan = torch.full_like(M, float("nan"))
                s = _off(nan) if out_off == "sinf off" else nan.clone()
                c = _off(nan) if out_off == "cosf off" else nan.clone()
                ops._call("exo_kepler_f64", dev, ops._ptr(M), ops._ptr(e), ops._ptr(s), ops._ptr(c), n, ops._stream(M))
                return s, c
            routes[out_off] = raw
        for name, fn in routes.items():
            _poison(n, dev)
            s, c = fn()
            err = np.maximum(np.abs(s.cpu().numpy() - want_s), np.abs(c.cpu().numpy() - want_c))
            K.report(f"kepler n={n} {name}", worst_error_over_tol=err / tol)
            assert np.all(err <= tol), (n, name, int(np.argmax(err / tol)))


def test_quad_solution_vector_launch_routes(dev):
    """the same routes of exo_quad_solution_vector_f64, with and without derivatives, on the points of quad_sv.npz tiled;
    tolerances: those of tests/test_oracle.py::test_quad_sv_golden"""
    import os

    from exoplanet_amd import ops

    q = np.load(os.path.join(K.GOLD, "quad_sv.npz"))
    gap = np.minimum.reduce([np.abs(np.abs(q["b"]) - np.abs(1 - q["r"])), np.abs(np.abs(q["b"]) - (1 + q["r"])),
                             np.abs(np.abs(q["b"]) - q["r"]) + 1e-3])
    dtol = (5e-14 + 2e-15 / np.sqrt(np.maximum(gap, 1e-16)))[:, None]

    def raw(b, r, derivs, off):
        n = b.numel()
        outs = [torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev) for _ in range(3 if derivs else 1)]
        if off is not None:
            outs[off] = _off(outs[off])
        ptrs = [ops._ptr(x) for x in outs] + [0] * (3 - len(outs))
        ops._call("exo_quad_solution_vector_f64", dev, ops._ptr(b), ops._ptr(r), *ptrs, n, ops._stream(b))
        return outs

    for n in SIZES + [QUAD_BIG]:
        idx = np.arange(n) % q["b"].size
        b, r = T(q["b"][idx], dev), T(q["r"][idx], dev)
        assert b.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0
        for derivs in (False, True):
            fn = ops.quad_solution_vector_derivs if derivs else (lambda x, y: (ops.quad_solution_vector(x, y),))
            routes = {"aligned": lambda: fn(b, r), "b off": lambda: fn(_off(b), r), "r off": lambda: fn(b, _off(r)),
                      "s off": lambda: raw(b, r, derivs, 0)}
            if derivs:
                routes.update({"dsdb off": lambda: raw(b, r, True, 1), "dsdr off": lambda: raw(b, r, True, 2)})
            for name, route in routes.items():
                _poison(3 * n, dev)
                outs = [x.cpu().numpy() for x in route()]
                es = np.abs(outs[0] - q["s"][idx]).max()
                line = dict(value_error=es, value_tol=5e-15)
                assert es < 5e-15, (n, derivs, name, es)          # (NaN, an element never written, fails this too)
                if derivs:
                    for got, key in zip(outs[1:], ("dsdb", "dsdr")):
                        ratio = np.abs(got - q[key][idx]) / dtol[idx]
                        line[key + "_error_over_tol"] = ratio
                        assert np.all(ratio <= 1.0), (n, name, key)
                K.report(f"quad_sv n={n} derivs={derivs} {name}", **line)


# ------------------------------------------------------------------------------------------------------------------------
# contact_points: shapes and odd counts across its 64-wide blocks (float64 oracle, as tests/test_gpu_ops.py)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1,), (63,), (64,), (65,), (127,), (129,), (1025,), (3, 43), (5, 1, 13)])
def test_contact_points_shapes(shape, dev):
    from exoplanet_amd import ops

    rng = np.random.default_rng(9)
    a = rng.uniform(3, 60, shape); e = rng.uniform(0, 0.9, shape); w = rng.uniform(-np.pi, np.pi, shape)
    cosi = (1 + e * np.sin(w)) / (1 - e * e) * rng.uniform(0, 1.4, shape) / a
    sini = np.sqrt(np.clip(1 - cosi ** 2, 0, None))
    L = 1 + rng.uniform(0.01, 0.2, shape[-1:])            # broadcast over the leading axes
    Ml, Mr, fl = ops.contact_points(*[T(x, dev) for x in (a, e, np.cos(w), np.sin(w), cosi, sini, L)])
    assert Ml.shape == shape and Mr.shape == shape and fl.shape == shape
    Lb = np.broadcast_to(L, shape)
    ml, mr, f0 = P.contact_points(a.ravel(), e.ravel(), np.cos(w).ravel(), np.sin(w).ravel(), cosi.ravel(), sini.ravel(), Lb.ravel())
    assert np.array_equal(fl.cpu().numpy().ravel(), f0)
    ok = f0 == 0
    err = max(np.abs(Ml.cpu().numpy().ravel()[ok] - ml[ok]).max(initial=0.0), np.abs(Mr.cpu().numpy().ravel()[ok] - mr[ok]).max(initial=0.0))
    K.report(f"contact_points {shape}", solved=ok.sum(), worst_error=err, tol=1e-12)
    assert err <= 1e-12
