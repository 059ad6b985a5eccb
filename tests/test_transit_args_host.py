"""CPU: what every transit entry point answers to arguments it must refuse, or has nothing to do for.

The library loads without a GPU and every refusal returns before any launch, so each case hands the entry small fake
pointers that are never followed and asserts the exact return code.  A valid call here always carries a null workspace
(EXO_ERR_WORKSPACE, the last host-side check), so a case that expects EXO_ERR_INVALID_ARGUMENT with everything else valid
also pins that rule's place in front of the workspace check.  No case reaches a launch or an event record: empty series
with draws on the gradient entries, which launch a zero fill, are left to the GPU suite."""
import ctypes

import pytest

OK, INVALID, WORKSPACE = 0, 1, 3

PER_PLANET, WINDOW, SECONDARY, EXACT_SCAN, SPARSE, LIGHT_DELAY, CADENCE_MAJOR, SORTED_TIMES = 1, 2, 4, 16, 32, 64, 128, 256
UNKNOWN = (8, 512, 1 << 31)     # 8 is a packing flag, no sweep flag
MAX_PLANETS, MAX_SUBEXP, MAX_TTV_EDGES, NIN = 16, 63, 65536, 10

P = 0x1000          # a "device pointer": non-null, never followed
N_CAD, N_DRAW = 300, 3
HUGE = 1 << 40

SERIES = ["t", "n_cad", "texp", "n_texp", "stencil_dt", "stencil_w", "n_sub", "params", "ld", "n_draw", "n_planet", "flags"]
TABLES = ["ttv_edges", "ttv_shift", "n_edge"]
WS = ["workspace", "workspace_bytes", "stream"]
NOISE = ["y", "var", "n_var", "mean", "n_mean", "jit2", "n_jit", "chi2", "gmean", "gjit2", "gparams", "gld"]
SHAPE = ["workspace", "workspace_bytes", "n_cad", "n_draw", "n_planet", "flags"]

SIGNATURES = {
    "exo_transit_flux_fwd_f64": SERIES + ["flux"] + WS,
    "exo_transit_flux_fwd_ev_f64": SERIES + ["flux"] + WS + ["ev_start", "ev_stop"],
    "exo_transit_flux_ttv_fwd_f64": SERIES + TABLES + ["flux"] + WS,
    "exo_transit_flux_vjp_f64": SERIES + ["gflux", "flux_out", "gparams", "gld", "flux_dot"] + WS,
    "exo_transit_flux_vjp_ev_f64": SERIES + ["gflux", "flux_out", "gparams", "gld", "flux_dot"] + WS + ["ev_start", "ev_stop"],
    "exo_transit_flux_ttv_vjp_f64": SERIES + TABLES + ["gflux", "flux_out", "gparams", "gld", "gshift", "flux_dot"] + WS,
    "exo_transit_flux_fwd_jac_f64": SERIES + ["flux", "jac", "jac_doubles"] + WS,
    "exo_transit_flux_jac_vjp_f64": ["gflux", "n_cad", "n_draw", "n_planet", "flags", "jac", "workspace", "workspace_bytes",
                                     "gparams", "gld", "flux_dot", "stream"],
    "exo_transit_flux_cols_vjp_f64": ["cols", "draw_stride", "planet_stride", "defaults", "ld_cols", "ld_draw_stride", "pack_flags",
                                      "t", "n_cad", "texp", "n_texp", "stencil_dt", "stencil_w", "n_sub", "n_draw", "n_planet",
                                      "flags", "gflux", "flux_out", "params", "ld", "gparams", "gld", "flux_dot", "fold", "gscale",
                                      "gcols", "gld_cols"] + WS + ["ev_start", "ev_stop"],
    "exo_transit_flux_vjp_sparse_f64": SERIES + ["gvals", "gparams", "gld", "flux_dot", "workspace", "workspace_bytes",
                                                 "reuse_runs", "stream"],
    "exo_transit_flux_sparse_model": SHAPE + ["out"],
    "exo_transit_sparse_scatter_f64": SHAPE + ["clear", "flux", "stream"],
    "exo_sparse_model_merge_f64": SHAPE + ["merge_ws", "merge_ws_bytes", "out", "stream"],
    "exo_sparse_model_merge_vjp_f64": SHAPE + ["merge_ws", "merge_ws_bytes", "gmvals", "gvals", "stream"],
    "exo_sparse_model_merged": ["merge_ws", "merge_ws_bytes", "n_cad", "n_draw", "n_planet", "out"],
    "exo_transit_chi2_vjp_f64": SERIES + ["obs", "ivar", "n_ivar", "chi2", "gparams", "gld"] + WS,
    "exo_transit_chi2_ttv_vjp_f64": SERIES + TABLES + ["obs", "ivar", "n_ivar", "chi2", "gparams", "gld", "gshift"] + WS,
    "exo_transit_noise_vjp_f64": SERIES + NOISE + WS,
    "exo_transit_noise_ttv_vjp_f64": SERIES + TABLES + NOISE + ["gshift"] + WS,
}

# a valid call, but for the null workspace: every pointer set, one planet, no exposure integration
VALID = dict(n_cad=N_CAD, texp=None, n_texp=0, stencil_dt=None, stencil_w=None, n_sub=1, n_draw=N_DRAW, n_planet=1, flags=0,
             n_edge=4, jac_doubles=HUGE, n_ivar=1, n_var=1, n_mean=1, n_jit=1, workspace=None, workspace_bytes=HUGE, stream=None,
             ev_start=None, ev_stop=None, reuse_runs=0, clear=0, fold=0, pack_flags=0, merge_ws_bytes=HUGE)
EXPOSED = dict(texp=P, n_texp=1, stencil_dt=P, stencil_w=P, n_sub=3)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def host_cols():
    """the host-side arrays of the column entry (followed on the host: real memory; their entries are device pointers)"""
    ptrs = (ctypes.c_void_p * NIN)(*([P] * NIN))
    strides = (ctypes.c_int64 * NIN)(*([1] * NIN))
    defaults = (ctypes.c_double * NIN)(*([0.0] * NIN))
    ld = (ctypes.c_void_p * 4)(P, P, P, P)
    ld_gap = (ctypes.c_void_p * 4)(P, None, P, P)
    ld_strides = (ctypes.c_int64 * 4)(2, 2, 2, 2)
    adr = ctypes.addressof
    return dict(cols=adr(ptrs), draw_stride=adr(strides), planet_stride=adr(strides), defaults=adr(defaults), ld_cols=adr(ld),
                ld_draw_stride=adr(ld_strides), gcols=adr(ptrs), gld_cols=adr(ld), _gap=adr(ld_gap),
                _keep=(ptrs, strides, defaults, ld, ld_gap, ld_strides))


def call(lib, name, base=None, **over):
    a = dict(VALID)
    a.update(base or {})
    a.update(over)
    return getattr(lib, name)(*[a.get(k, P) for k in SIGNATURES[name]])


def runs_bytes(lib, n_cad, n_draw):
    """the run-enumeration workspace of (n_cad, n_draw, one planet), to the byte: exo_transit_flux_sparse_model only describes
    that workspace -- it launches nothing -- and accepts it from exactly that size on"""
    from exoplanet_amd import _lib

    out = _lib.SparseModel()
    fits = lambda b: lib.exo_transit_flux_sparse_model(P, b, n_cad, n_draw, 1, 0, ctypes.addressof(out)) == OK  # noqa: E731
    lo, hi = 0, lib.exo_transit_flux_workspace_bytes(n_cad, n_draw, 1)
    assert hi > 0 and fits(hi) and not fits(0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    return hi


@pytest.fixture(scope="module")
def short(lib):
    """a non-null run-enumeration workspace one byte short for the shape of VALID"""
    return dict(workspace=P, workspace_bytes=runs_bytes(lib, N_CAD, N_DRAW) - 1)


# ---- the entries that take a time series --------------------------------------------------------------------------------------------

FWD = ["exo_transit_flux_fwd_f64", "exo_transit_flux_fwd_ev_f64", "exo_transit_flux_ttv_fwd_f64"]
VJP = ["exo_transit_flux_vjp_f64", "exo_transit_flux_vjp_ev_f64", "exo_transit_flux_ttv_vjp_f64"]
CHI2 = ["exo_transit_chi2_vjp_f64", "exo_transit_noise_vjp_f64"]
CHI2_TTV = ["exo_transit_chi2_ttv_vjp_f64", "exo_transit_noise_ttv_vjp_f64"]
JAC, SPARSE_VJP, COLS = "exo_transit_flux_fwd_jac_f64", "exo_transit_flux_vjp_sparse_f64", "exo_transit_flux_cols_vjp_f64"
TIMED = ["exo_transit_flux_ttv_fwd_f64", "exo_transit_flux_ttv_vjp_f64"] + CHI2_TTV
ALL_SERIES = FWD + VJP + [JAC, SPARSE_VJP, COLS] + CHI2 + CHI2_TTV
# exo_transit_flux_ttv_vjp_f64 zero-fills gshift once its arguments pass, before it looks at the workspace, and the column
# entry packs its records before the sweep unless the launches fuse: no valid call of these two without a launch
REACH_WORKSPACE = [e for e in ALL_SERIES if e != "exo_transit_flux_ttv_vjp_f64"]


def base_of(name, host_cols):
    b = {}
    if name == SPARSE_VJP:
        b["flags"] = SPARSE
    if name == COLS:
        b.update({k: v for k, v in host_cols.items() if not k.startswith("_")})
        b["flags"] = SORTED_TIMES       # (the fused path: argument checks, then the workspace)
    return b


@pytest.mark.parametrize("name", REACH_WORKSPACE)
def test_valid_arguments_reach_the_workspace_check(lib, host_cols, short, name):
    b = base_of(name, host_cols)
    assert call(lib, name, b) == WORKSPACE                       # null workspace
    assert call(lib, name, b, **short) == WORKSPACE              # one byte short
    assert call(lib, name, b, **EXPOSED) == WORKSPACE            # one exposure time for all cadences
    assert call(lib, name, b, **EXPOSED, **short) == WORKSPACE
    assert call(lib, name, b, n_planet=MAX_PLANETS, n_sub=MAX_SUBEXP, n_draw=65535) == WORKSPACE     # the last sizes in range


@pytest.mark.parametrize("name", ALL_SERIES)
def test_sizes_flags_and_exposure(lib, host_cols, short, name):
    b = base_of(name, host_cols)
    for bad in (dict(n_cad=-1), dict(n_draw=-1), dict(n_draw=65536), dict(n_planet=0), dict(n_planet=MAX_PLANETS + 1),
                dict(n_planet=-1), dict(n_sub=0), dict(n_sub=MAX_SUBEXP + 1), dict(EXPOSED, n_texp=2), dict(EXPOSED, n_texp=-1),
                dict(EXPOSED, n_texp=N_CAD + 1)):
        assert call(lib, name, b, **bad) == INVALID, bad
        assert call(lib, name, b, **bad, **short) == INVALID, bad
        assert call(lib, name, b, **dict(bad, n_draw=0) if "n_draw" not in bad else bad) == INVALID, bad   # before "no draws"
    for bit in UNKNOWN:
        assert call(lib, name, b, flags=b.get("flags", 0) | bit) == INVALID, bit
        assert call(lib, name, b, flags=b.get("flags", 0) | bit, **short) == INVALID, bit
        assert call(lib, name, b, flags=b.get("flags", 0) | bit, n_draw=0) == INVALID, bit
    # the exposure triple: all three or n_texp == 0
    for missing in ("texp", "stencil_dt", "stencil_w"):
        assert call(lib, name, b, **dict(EXPOSED, **{missing: None})) == INVALID, missing
        assert call(lib, name, b, **dict(EXPOSED, **{missing: None}), **short) == INVALID, missing
    # records and limb darkening
    for missing in ("params", "ld"):
        assert call(lib, name, b, **{missing: None}) == INVALID, missing
        assert call(lib, name, b, **{missing: None}, **short) == INVALID, missing


@pytest.mark.parametrize("name", ALL_SERIES)
def test_no_draws_is_no_work(lib, host_cols, name):
    """n_draw == 0 returns EXO_OK before any pointer is looked at -- but for the timing tables, which come first"""
    nothing = {k: None for k in SIGNATURES[name] if k not in VALID and k not in TABLES and k != "gshift"}
    nothing["flags"] = base_of(name, host_cols).get("flags", 0)
    assert call(lib, name, nothing, n_draw=0) == OK
    assert call(lib, name, nothing, n_draw=0, n_cad=0) == (INVALID if name in CHI2_TTV else OK)      # (these two need a cadence)
    assert call(lib, name, nothing, n_draw=0, **dict(EXPOSED, texp=None, stencil_dt=None, stencil_w=None)) == OK
    if name in TIMED:
        assert call(lib, name, nothing, n_draw=0, ttv_edges=None) == INVALID
    if name in TIMED[1:]:
        assert call(lib, name, nothing, n_draw=0, gshift=None) == INVALID


@pytest.mark.parametrize("name", FWD + [JAC])
def test_forward_entries(lib, name):
    nothing = {k: None for k in SIGNATURES[name] if k not in VALID and k not in TABLES}
    assert call(lib, name, nothing, n_cad=0) == OK                                # no cadences: nothing to do
    assert call(lib, name, nothing, n_cad=0, flags=UNKNOWN[1]) == INVALID
    assert call(lib, name, nothing, n_cad=0, n_planet=0) == INVALID
    assert call(lib, name, t=None) == INVALID
    assert call(lib, name, flux=None) == INVALID
    assert call(lib, name, flux=None, flags=SPARSE) == WORKSPACE                  # the sparse output needs no flux array
    assert call(lib, name, flags=SPARSE | SORTED_TIMES | WINDOW | CADENCE_MAJOR) == WORKSPACE
    assert call(lib, name, flags=CADENCE_MAJOR | PER_PLANET) == INVALID


@pytest.mark.parametrize("name", FWD[:2])
def test_forward_sweeps_off_the_run_enumeration_path(lib, short, name):
    """per-cadence exposure times and the exact scan take the list path: its own workspace, and no sparse, light-delay or
    cadence-major output"""
    per_cadence = dict(EXPOSED, n_texp=N_CAD)
    for off in (per_cadence, dict(flags=EXACT_SCAN)):
        assert call(lib, name, **off) == WORKSPACE
        assert call(lib, name, **dict(off, workspace=P, workspace_bytes=0)) == WORKSPACE
        for flag in (SPARSE, LIGHT_DELAY, CADENCE_MAJOR):
            assert call(lib, name, **dict(off, flags=off.get("flags", 0) | flag)) == INVALID, flag
            assert call(lib, name, **dict(off, flags=off.get("flags", 0) | flag), **short) == INVALID, flag
    assert call(lib, name, flags=LIGHT_DELAY) == WORKSPACE
    # (the list path's workspace is the smaller of the two and no entry reports its size alone: "one byte short" of it cannot
    # be written down here without risking a launch)


@pytest.mark.parametrize("name", TIMED)
def test_timing_tables(lib, short, name):
    for bad in (dict(ttv_edges=None), dict(ttv_shift=None), dict(n_edge=0), dict(n_edge=-1), dict(n_edge=MAX_TTV_EDGES + 1)):
        assert call(lib, name, **bad) == INVALID, bad
        assert call(lib, name, **bad, **short) == INVALID, bad
    if name != "exo_transit_flux_ttv_fwd_f64":
        assert call(lib, name, gshift=None) == INVALID
        assert call(lib, name, gshift=None, **short) == INVALID
    if name != "exo_transit_flux_ttv_vjp_f64":
        assert call(lib, name, n_edge=MAX_TTV_EDGES) == WORKSPACE
        assert call(lib, name, n_edge=1) == WORKSPACE


def test_timed_forward_sweep_paths(lib, short):
    """timing tables with occultations or light delay leave the run-enumeration path (and light delay has no other)"""
    name = "exo_transit_flux_ttv_fwd_f64"
    assert call(lib, name, flags=SECONDARY) == WORKSPACE
    assert call(lib, name, flags=SECONDARY | SPARSE) == INVALID
    assert call(lib, name, flags=SECONDARY | CADENCE_MAJOR, **short) == INVALID
    assert call(lib, name, flags=LIGHT_DELAY) == INVALID
    assert call(lib, name, flags=SPARSE, flux=None) == WORKSPACE
    assert call(lib, name, flags=CADENCE_MAJOR | PER_PLANET) == INVALID


@pytest.mark.parametrize("name", VJP + [COLS])
def test_gradient_entries(lib, host_cols, short, name):
    b = base_of(name, host_cols)
    for missing in ("t", "gflux", "gparams", "gld"):
        assert call(lib, name, b, **{missing: None}) == INVALID, missing
        assert call(lib, name, b, **{missing: None}, **short) == INVALID, missing
    if name != "exo_transit_flux_ttv_vjp_f64":      # (which has zero-filled gshift by the time the sweep looks at the layout)
        assert call(lib, name, b, flags=b.get("flags", 0) | CADENCE_MAJOR | PER_PLANET) == INVALID
        assert call(lib, name, b, flags=b.get("flags", 0) | CADENCE_MAJOR | PER_PLANET, **short) == INVALID
        assert call(lib, name, b, flux_out=None, flux_dot=None) == WORKSPACE          # both optional
        assert call(lib, name, b, flags=b.get("flags", 0) | SPARSE | LIGHT_DELAY | WINDOW) == WORKSPACE


@pytest.mark.parametrize("name", VJP[:2])
def test_gradient_sweeps_off_the_run_enumeration_path(lib, short, name):
    for off in (dict(EXPOSED, n_texp=N_CAD), dict(flags=EXACT_SCAN)):
        assert call(lib, name, **off) == WORKSPACE
        for flag in (SPARSE, LIGHT_DELAY, CADENCE_MAJOR):
            assert call(lib, name, **dict(off, flags=off.get("flags", 0) | flag)) == INVALID, flag


def test_column_entry(lib, host_cols, short):
    b = base_of(COLS, host_cols)
    for missing in ("cols", "draw_stride", "planet_stride", "defaults", "ld_cols", "ld_draw_stride"):
        assert call(lib, COLS, b, **{missing: None}) == INVALID, missing
        assert call(lib, COLS, b, **{missing: None}, **short) == INVALID, missing
    # the column cotangents are asked for with fold
    assert call(lib, COLS, b, gcols=None, gld_cols=None, gscale=None) == WORKSPACE
    assert call(lib, COLS, b, fold=1, gscale=None) == WORKSPACE
    assert call(lib, COLS, b, fold=1, gcols=None) == INVALID
    assert call(lib, COLS, b, fold=1, gld_cols=None, **short) == INVALID
    # one answer to "occultations?"
    assert call(lib, COLS, b, pack_flags=SECONDARY) == INVALID
    assert call(lib, COLS, b, flags=SORTED_TIMES | SECONDARY, **short) == INVALID
    assert call(lib, COLS, b, pack_flags=SECONDARY, flags=SORTED_TIMES | SECONDARY) == WORKSPACE
    assert call(lib, COLS, b, pack_flags=8) == WORKSPACE                               # (the packing's own flag)
    # a limb-darkening column the packing would read is missing (two without occultations, four with)
    assert call(lib, COLS, b, ld_cols=host_cols["_gap"]) == INVALID
    assert call(lib, COLS, b, ld_cols=host_cols["_gap"], **short) == INVALID
    gap3 = (ctypes.c_void_p * 4)(P, P, None, P)
    assert call(lib, COLS, b, ld_cols=ctypes.addressof(gap3)) == WORKSPACE
    assert call(lib, COLS, b, ld_cols=ctypes.addressof(gap3), pack_flags=SECONDARY, flags=SORTED_TIMES | SECONDARY) == INVALID


@pytest.mark.parametrize("name", [JAC, "exo_transit_flux_jac_vjp_f64"])
def test_jacobian_entries(lib, short, name):
    for flag in (PER_PLANET, EXACT_SCAN, LIGHT_DELAY):
        assert call(lib, name, flags=flag) == INVALID, flag
        assert call(lib, name, flags=flag, **short) == INVALID, flag
        assert call(lib, name, flags=flag, n_draw=0) == INVALID, flag
    assert call(lib, name, jac=None) == INVALID
    assert call(lib, name, jac=None, **short) == INVALID
    assert call(lib, name, flags=SECONDARY | WINDOW | SPARSE | CADENCE_MAJOR | SORTED_TIMES) == WORKSPACE


def test_jacobian_forward(lib, short):
    assert call(lib, JAC, **dict(EXPOSED, n_texp=N_CAD)) == INVALID                   # run-enumeration sweeps only
    need = lib.exo_transit_flux_jac_doubles(N_CAD, N_DRAW, 1)
    assert need == 16 * N_CAD * N_DRAW
    ample = dict(workspace=P, workspace_bytes=HUGE)                                     # (never reached: jac comes first)
    assert call(lib, JAC, jac_doubles=need - 1, **ample) == WORKSPACE
    assert call(lib, JAC, jac_doubles=need - 1, jac=None, **ample) == INVALID
    assert call(lib, JAC, jac_doubles=need, **short) == WORKSPACE
    assert call(lib, JAC, jac_doubles=0, n_draw=0) == OK


def test_jacobian_contraction(lib, short):
    name = "exo_transit_flux_jac_vjp_f64"
    assert call(lib, name) == WORKSPACE and call(lib, name, **short) == WORKSPACE
    assert call(lib, name, n_planet=MAX_PLANETS, n_draw=65535) == WORKSPACE
    for bad in (dict(n_cad=-1), dict(n_draw=-1), dict(n_draw=65536), dict(n_planet=0), dict(n_planet=MAX_PLANETS + 1)):
        assert call(lib, name, **bad) == INVALID, bad
        assert call(lib, name, **bad, **short) == INVALID, bad
    for bit in UNKNOWN:
        assert call(lib, name, flags=bit) == INVALID
        assert call(lib, name, flags=bit, n_draw=0) == INVALID
    for missing in ("gflux", "gparams", "gld"):
        assert call(lib, name, **{missing: None}) == INVALID, missing
        assert call(lib, name, **{missing: None}, **short) == INVALID, missing
    assert call(lib, name, flux_dot=None) == WORKSPACE
    nothing = dict(gflux=None, jac=None, gparams=None, gld=None, flux_dot=None)
    assert call(lib, name, nothing, n_draw=0) == OK
    assert call(lib, name, nothing, n_draw=0, n_cad=0) == OK


def test_sparse_cotangent_entry(lib, short):
    name, b = SPARSE_VJP, dict(flags=SPARSE)
    assert call(lib, name, flags=0) == INVALID                                         # the sparse output's layout or none
    assert call(lib, name, flags=0, n_draw=0) == INVALID
    for flag in (PER_PLANET, CADENCE_MAJOR, EXACT_SCAN):
        assert call(lib, name, flags=SPARSE | flag) == INVALID, flag
        assert call(lib, name, flags=SPARSE | flag, **short) == INVALID, flag
    assert call(lib, name, b, **dict(EXPOSED, n_texp=N_CAD)) == INVALID                # run-enumeration sweeps only
    assert call(lib, name, b, **dict(EXPOSED, n_texp=N_CAD), n_draw=0) == INVALID
    for missing in ("t", "gvals", "gparams", "gld"):
        assert call(lib, name, b, **{missing: None}) == INVALID, missing
        assert call(lib, name, b, **{missing: None}, **short) == INVALID, missing
    assert call(lib, name, b, flux_dot=None, reuse_runs=1) == WORKSPACE
    assert call(lib, name, flags=SPARSE | LIGHT_DELAY | SECONDARY | WINDOW | SORTED_TIMES, **short) == WORKSPACE


@pytest.mark.parametrize("name", CHI2 + CHI2_TTV)
def test_likelihood_entries(lib, short, name):
    timed, noise = name in CHI2_TTV, "noise" in name
    for flag in (PER_PLANET, SPARSE, EXACT_SCAN):
        assert call(lib, name, flags=flag) == INVALID, flag
        assert call(lib, name, flags=flag, **short) == INVALID, flag
        assert call(lib, name, flags=flag, n_draw=0) == INVALID, flag
    for flag in (SECONDARY, LIGHT_DELAY):
        assert call(lib, name, flags=flag) == (INVALID if timed else WORKSPACE), flag
        assert call(lib, name, flags=flag, **short) == (INVALID if timed else WORKSPACE), flag
        assert call(lib, name, flags=flag, n_draw=0) == (INVALID if timed else OK), flag
    assert call(lib, name, flags=WINDOW | CADENCE_MAJOR | SORTED_TIMES) == WORKSPACE
    assert call(lib, name, **dict(EXPOSED, n_texp=N_CAD)) == INVALID                   # run-enumeration sweeps only ...
    assert call(lib, name, **dict(EXPOSED, n_texp=N_CAD), **short) == INVALID
    assert call(lib, name, **dict(EXPOSED, n_texp=N_CAD), n_draw=0) == OK              # ... asked after "no draws"
    required = ["t", "chi2", "gparams", "gld"] + (["y", "var", "mean", "jit2", "gmean", "gjit2"] if noise else ["obs", "ivar"])
    for missing in required:
        assert call(lib, name, **{missing: None}) == INVALID, missing
        assert call(lib, name, **{missing: None}, **short) == INVALID, missing
        assert call(lib, name, **{missing: None}, n_draw=0) == OK, missing
    # extents: one value or one per cadence (per draw), and no jitter at all
    extent = "n_var" if noise else "n_ivar"
    assert call(lib, name, **{extent: N_CAD}) == WORKSPACE
    for n in (0, 2, N_DRAW, -1):
        assert call(lib, name, **{extent: n}) == INVALID, n
        assert call(lib, name, **{extent: n}, **short) == INVALID, n
        assert call(lib, name, **{extent: n}, n_draw=0) == INVALID, n
    if noise:
        assert call(lib, name, n_mean=N_DRAW, n_jit=N_DRAW) == WORKSPACE
        assert call(lib, name, n_jit=0, jit2=None) == WORKSPACE
        for bad in (dict(n_mean=0), dict(n_mean=2), dict(n_mean=N_CAD), dict(n_jit=2), dict(n_jit=N_CAD), dict(n_jit=-1)):
            assert call(lib, name, **bad) == INVALID, bad
            assert call(lib, name, **bad, **short) == INVALID, bad
            assert call(lib, name, **bad, n_draw=0) == (OK if bad == dict(n_mean=0) else INVALID), bad     # (one mean per draw)
    # an empty series: the timed entries refuse it; the others go on to the workspace (and, valid, to a launch: not here)
    empty = dict(n_cad=0, t=None, **({"y": None} if noise else {"obs": None, "ivar": None}))
    assert call(lib, name, **empty) == (INVALID if timed else WORKSPACE)


# ---- the entries that describe, scatter or merge a sparse output: a shape and a workspace, no series -------------------------------

def test_sparse_model(lib, short):
    from exoplanet_amd import _lib

    name, out = "exo_transit_flux_sparse_model", _lib.SparseModel()
    b = dict(out=ctypes.addressof(out))
    exact = dict(workspace=P, workspace_bytes=short["workspace_bytes"] + 1)
    assert call(lib, name, b, **exact) == OK
    assert out.nseg and out.seg and out.off and out.vals and (out.seg_step, out.hi_at) == (4, 3) and out.val_row == N_CAD
    assert call(lib, name, b, **short) == WORKSPACE and call(lib, name, b) == WORKSPACE
    for bad in (dict(n_cad=-1), dict(n_cad=1 << 31), dict(n_draw=-1), dict(n_planet=0), dict(n_planet=MAX_PLANETS + 1), dict(out=None)):
        assert call(lib, name, b, **bad) == INVALID, bad
        assert call(lib, name, b, **bad, **short) == INVALID, bad
    # one list per draw: several planets or occultations need the merged form
    assert call(lib, name, b, n_planet=2) == INVALID
    assert call(lib, name, b, flags=SECONDARY, **short) == INVALID
    assert call(lib, name, b, flags=UNKNOWN[1] | PER_PLANET) == WORKSPACE               # (no other flag is looked at)
    # the draws are not bounded here, and an empty series still has a (small) workspace
    # (n_draw == 0 is not asked: this entry and the two merge entries divide by it while carving the workspace)
    assert call(lib, name, b, n_draw=65536) == WORKSPACE
    assert call(lib, name, b, n_cad=0) == WORKSPACE
    assert call(lib, name, b, n_cad=0, workspace=P) == OK


def test_sparse_scatter(lib, short):
    name = "exo_transit_sparse_scatter_f64"
    assert call(lib, name) == WORKSPACE and call(lib, name, **short) == WORKSPACE
    assert call(lib, name, clear=1, flags=SECONDARY, n_planet=MAX_PLANETS, n_draw=65535) == WORKSPACE
    for bad in (dict(n_cad=-1), dict(n_draw=-1), dict(n_draw=65536), dict(n_planet=0), dict(n_planet=MAX_PLANETS + 1),
                dict(flags=PER_PLANET), dict(flags=SPARSE), dict(flags=UNKNOWN[1]), dict(flux=None)):
        assert call(lib, name, **bad) == INVALID, bad
        assert call(lib, name, **bad, **short) == INVALID, bad
    assert call(lib, name, n_cad=0, flux=None) == OK and call(lib, name, n_draw=0, flux=None) == OK
    assert call(lib, name, n_draw=0, flags=SPARSE) == INVALID


@pytest.mark.parametrize("name", ["exo_sparse_model_merge_f64", "exo_sparse_model_merge_vjp_f64"])
def test_sparse_merge(lib, short, name):
    need = lib.exo_sparse_merge_workspace_bytes(N_CAD, N_DRAW, 1)
    assert need > 0
    b = dict(merge_ws=P, merge_ws_bytes=need, out=None)
    assert call(lib, name, b) == WORKSPACE and call(lib, name, b, **short) == WORKSPACE
    ample = dict(workspace=P, workspace_bytes=HUGE)
    assert call(lib, name, b, merge_ws=None, **ample) == WORKSPACE
    assert call(lib, name, b, merge_ws_bytes=need - 1, **ample) == WORKSPACE
    for bad in (dict(n_cad=-1), dict(n_cad=1 << 31), dict(n_draw=-1), dict(n_draw=65536), dict(n_planet=0),
                dict(n_planet=MAX_PLANETS + 1), dict(flags=PER_PLANET), dict(flags=UNKNOWN[1])):
        assert call(lib, name, b, **bad) == INVALID, bad
        assert call(lib, name, b, **bad, **short) == INVALID, bad
    # nothing to merge: EXO_OK once both workspaces are there, whatever else is null
    for empty in (dict(n_cad=0),):
        fit = dict(merge_ws_bytes=lib.exo_sparse_merge_workspace_bytes(empty.get("n_cad", N_CAD), empty.get("n_draw", N_DRAW), 1))
        assert call(lib, name, b, **empty, **fit, **ample, gmvals=None, gvals=None) == OK
        assert call(lib, name, b, **empty, **fit, gmvals=None, gvals=None) == WORKSPACE
        assert call(lib, name, b, **empty, **fit, **ample, flags=SPARSE) == INVALID
    if name.endswith("vjp_f64"):
        # (the cotangent arrays are looked at last: only a call that would otherwise launch gets that far)
        assert call(lib, name, b, gmvals=None, **short) == WORKSPACE


def test_sparse_merged_description(lib):
    from exoplanet_amd import _lib

    name, out = "exo_sparse_model_merged", _lib.SparseModel()
    need = lib.exo_sparse_merge_workspace_bytes(N_CAD, N_DRAW, 2)
    b = dict(merge_ws=P, merge_ws_bytes=need, n_planet=2, out=ctypes.addressof(out))
    assert call(lib, name, b) == OK
    assert out.nseg == P and (out.seg_step, out.hi_at) == (2, 1) and out.val_row == N_CAD
    assert call(lib, name, b, merge_ws_bytes=need - 1) == WORKSPACE
    assert call(lib, name, b, merge_ws=None) == WORKSPACE
    for bad in (dict(n_cad=-1), dict(n_draw=-1), dict(n_planet=0), dict(n_planet=MAX_PLANETS + 1), dict(out=None)):
        assert call(lib, name, b, **bad) == INVALID, bad
        assert call(lib, name, b, **bad, merge_ws=None) == INVALID, bad
    assert call(lib, name, b, n_draw=65536, merge_ws_bytes=HUGE) == OK                  # (the draws are not bounded here)
    assert call(lib, name, b, n_draw=0) == OK
