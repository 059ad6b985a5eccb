"""Device ops behind the reference's ``exoplanet.compat.ops`` names.

Drop-in for the three callables the reference imports from exoplanet_core
(/root/reference/src/exoplanet/compat.py:27,56):

    ops.kepler(M, ecc) -> (sinf, cosf)                 keplerian.py:333,818
    ops.quad_solution_vector(b, r) -> s[..., 3]        limb_dark.py:24
    ops.contact_points(a, e, cosw, sinw, cosi, sini, L)
        -> (M_left, M_right, flag)                     keplerian.py:744-753

plus the fused ops that replace whole sub-graphs: ``transit_flux`` (everything between
the time array and the flux array; ``ttv=`` for a TTVOrbit's timing tables),
``transit_flux_dot`` / ``transit_flux_value_and_vjp`` (value and gradient in one sweep),
``pack_records`` (the constructor algebra) and ``radial_velocity``.  All take float64 ROCm tensors and
run hand-written HIP kernels through the C ABI (include/exoplanet_amd.h); each
has value + gradient (torch.autograd).  There is no CPU / eager fallback.
"""
import ctypes
import os
import warnings
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

NPAR = 20
(P_N, P_TP, P_ECC, P_COSW, P_SINW, P_COSI, P_SINI, P_AOR, P_ROR, P_T0, P_PERIOD, P_TS, P_TE,
 P_FRATIO, P_TS2, P_TE2, P_CLIGHT) = range(17)
FLAG_PER_PLANET = 1
FLAG_WINDOW = 2
FLAG_SECONDARY = 4
PACK_CIRCULAR = 8
FLAG_EXACT_SCAN = 16
FLAG_SPARSE = 32
FLAG_LIGHT_DELAY = 64
FLAG_CADENCE_MAJOR = 128   # summed dense flux / its cotangent as [cadence][draw] arrays (include/exoplanet_amd.h)
FLAG_SORTED_TIMES = 256    # t has been checked to be non-decreasing (known_sorted): windows and runs in one launch
NIN = 10
(IN_PERIOD, IN_T0, IN_B, IN_ECC, IN_OMEGA, IN_R, IN_MSTAR, IN_RSTAR, IN_MPLANET, IN_SBR) = range(10)
MAX_PLANETS = 16
MAX_SUBEXP = 63


_SORTED = {}
_VOUCHED = {}


def _capturing():
    """whether the current stream is being captured into a hipGraph (the one place that asks)"""
    return torch.cuda.is_current_stream_capturing()


def needs_grad(x):
    """whether autograd will want a gradient with respect to ``x``"""
    return isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled()


def _refuse_data_grad(what, differentiates, instead, **named):
    """the data of the likelihood ``what`` carry no gradient through its fused kernels: one of ``named`` that requires grad
    is refused rather than answered with a partial gradient"""
    for name, x in named.items():
        if needs_grad(x):
            raise NotImplementedError(f"{what}: `{name}` requires grad, and the fused kernels differentiate {differentiates} "
                                      f"only; use {instead}")


def _series_key(t):
    return (t.device.index, t.data_ptr(), t.numel(), t.stride(0) if t.dim() else 0)


def vouch_sorted(t):
    """The caller's word that the device tensor ``t`` is non-decreasing (no NaN) and STAYS so for as long as this buffer is
    a time array -- whatever is written into it later, by whatever means.  (Keyed by device, address and extent; at most
    sixteen series are held: a seventeenth releases the oldest, with a RuntimeWarning.)  The sweeps then carry FLAG_SORTED_TIMES
    (windows and runs in one launch) also where the torch layer cannot see for itself: inside a hipGraph capture, whose
    launches keep their flags at every replay.  The array is looked at once, now (one host synchronisation; not during a
    capture); ValueError if it is not sorted.  A sampler's time array is the use: fixed for the whole run.
    ``release_sorted(t)`` takes the word back."""
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError("vouch_sorted: a device tensor, please")
    if _capturing():
        raise RuntimeError("vouch_sorted looks at the array (a host synchronisation): call it before the capture")
    if t.numel() > 1 and not bool((t[1:] >= t[:-1]).all()):
        raise ValueError("vouch_sorted: the times are not non-decreasing (or hold a NaN)")
    key = _series_key(t)
    _VOUCHED.pop(key, None)
    if len(_VOUCHED) >= 16:
        # the table holds sixteen series (an entry keeps its time array alive): the OLDEST word is taken back, with a warning --
        # that series falls back to the sweep's own device check inside later captures (slower, never wrong)
        oldest = next(iter(_VOUCHED))
        _VOUCHED.pop(oldest)
        warnings.warn("vouch_sorted: more than 16 vouched series; the oldest one's word has been released (release_sorted "
                      "what you no longer use)", RuntimeWarning, stacklevel=2)
    _VOUCHED[key] = t        # (keeps the storage alive: the address cannot pass to another series meanwhile)
    return t


def release_sorted(t):
    _VOUCHED.pop(_series_key(t), None)


def known_sorted(t, unknown=True, nan_ok=True):
    """True if ``t`` is non-decreasing.  A device tensor is looked at once (one host synchronisation) and remembered
    by storage and version -- the entry keeps the tensor alive, so its address cannot be handed to another series
    meanwhile: a sampler evaluates on the same time array every step, and a step that is being captured into a hipGraph
    must not synchronise (``unknown``: the answer then, for a tensor never looked at).  ``nan_ok=False``: every
    neighbouring pair must compare as ordered -- a NaN among the times makes the answer False (what the sweep's own
    device check says: it then solves every cadence instead of searching).  A tensor without a version counter
    (inference mode) is ``unknown``.  The version counter sees torch's own in-place writes only: a buffer that is
    written behind torch's back (``t.data.copy_``, DLPack / ctypes consumers) must not rely on this cache -- see
    ``vouch_sorted`` and INTEGRATION.md."""
    if not t.is_cuda:
        return bool((t[1:] >= t[:-1]).all()) if not nan_ok else not bool((t[1:] < t[:-1]).any())
    # (by storage address, extent and version: `t.detach()` is a new object on the same storage with the same version
    # counter; the entry holds a tensor on that storage, so the address is not reused while it is here)
    try:
        key = _series_key(t) + (t._version,)
    except RuntimeError:                 # inference tensors do not track versions
        return unknown
    hit = _SORTED.get(key)
    if hit is None:
        if _capturing():
            return unknown   # cannot look during a capture; the warm-up runs before it did
        both = torch.stack([~(t[1:] < t[:-1]).any(), (t[1:] >= t[:-1]).all()]).cpu()     # one synchronisation
        if len(_SORTED) >= 8:      # (an entry keeps its time array alive: a handful of series, not dozens -- ADVICE r2)
            _SORTED.clear()
        hit = _SORTED[key] = (bool(both[0]), bool(both[1]), t)
    return hit[0] if nan_ok else hit[1]


def _sorted_flag(t):
    """FLAG_SORTED_TIMES when the sweep may skip its own check of ``t``: never on a guess, never with a NaN among the times,
    and -- ADVICE r3 -- never baked into a captured launch on the strength of the version cache (a replay runs on whatever
    the buffer holds THEN; the cache saw what it held at capture): inside a capture only a series the caller vouched for
    (``vouch_sorted``) gets the flag, everything else keeps the device's own check, every replay."""
    if os.environ.get("EXO_CHECK_SORTED_ON_DEVICE") == "1":     # (A/B: the sweep's own check, every call)
        return 0
    if t.numel() <= 1:
        return 0
    if _series_key(t) in _VOUCHED:
        return FLAG_SORTED_TIMES
    if _capturing():
        return 0
    return FLAG_SORTED_TIMES if known_sorted(t, unknown=False, nan_ok=False) else 0


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(
            f"{name} lives on {x.device}: exoplanet_amd ops run only on a ROCm device "
            "(HIP kernels through libexoplanet_amd.so); there is no CPU fallback"
        )
    if x.dtype != torch.float64:
        raise TypeError(f"{name} must be float64 (the reference casts everything to float64, utils.py:18)")
    return x.contiguous()


def _ptr(x):
    return 0 if x is None else x.data_ptr()


def _call(name, device, *args):
    """the library entry ``name`` on ``device`` (None: a host-side query, no device to select); a failure is reported
    under the same ``name``"""
    fn = getattr(_lib.load(), name)
    if device is None:
        status = fn(*args)
    else:
        with torch.cuda.device(device):
            status = fn(*args)
    _lib.check(status, name)


def _ptr_array(xs, n):
    """a host array of ``n`` pointers: those of ``xs`` (None: null), the rest null"""
    return (ctypes.c_void_p * n)(*[_ptr(x) for x in xs])


def _workspace_bytes(N, D, P):
    return _lib.load().exo_transit_flux_workspace_bytes(N, D, P)


def _workspace(N, D, P, device, zero=False):
    """(a sweep's workspace, its size in bytes).  The size need not be a multiple of 8 and the tensor is float64 (the
    values of a sparse sweep are views of it): one double more than the bytes round down to"""
    nbytes = _workspace_bytes(N, D, P)
    return (torch.zeros if zero else torch.empty)(max(nbytes // 8 + 1, 1), dtype=torch.float64, device=device), nbytes


def _layout(name, N, D, P):
    lay = (ctypes.c_int64 * 5)()
    _call(name, None, N, D, P, lay)
    return list(lay)


def _sparse_layout(N, D, P):
    """byte offsets of (run counts, runs, prefix sums, values) in a sparse sweep's workspace, and the runs a list can hold"""
    return _layout("exo_transit_flux_sparse_layout", N, D, P)


def _merge_layout(N, D, P):
    """byte offsets of (segment counts, segments, value offsets, values) in a merge workspace, and the segments a draw can hold"""
    return _layout("exo_sparse_merge_layout", N, D, P)


def is_cadence_major(x):
    """a (D, N) float64 device tensor laid out [cadence][draw] -- the transposed view of a contiguous (N, D) array: what
    the light-curve sweep returns under FLAG_CADENCE_MAJOR and what the celerite kernels read (and write the cotangent
    of) with every wave's accesses contiguous, a lane being a draw"""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.shape[0] > 1
            and x.stride() == (1, x.shape[0]))


# ------------------------------------------------------------------------------
# kepler
# ------------------------------------------------------------------------------
class _Kepler(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, ecc):
        M = _dev(M, "M")
        ecc = _dev(ecc, "ecc")
        if M.shape != ecc.shape:
            raise ValueError("kepler: M and ecc must have the same shape (the caller broadcasts, keplerian.py:333)")
        sinf = torch.empty_like(M)
        cosf = torch.empty_like(M)
        _call("exo_kepler_f64", M.device, _ptr(M), _ptr(ecc), _ptr(sinf), _ptr(cosf), M.numel(), _stream(M))
        ctx.save_for_backward(sinf, cosf, ecc)
        return sinf, cosf

    @staticmethod
    def backward(ctx, gs, gc):
        sinf, cosf, e = ctx.saved_tensors
        # df/dM = (1+e cosf)^2/(1-e^2)^{3/2},  df/de = (2+e cosf) sinf/(1-e^2)
        ome2 = (1 - e) * (1 + e)      # not 1 - e^2, which loses the digits of 1 - e as e -> 1
        gf = gs * cosf - gc * sinf
        dfdM = (1 + e * cosf) ** 2 / ome2 ** 1.5
        dfde = (2 + e * cosf) * sinf / ome2
        return gf * dfdM, gf * dfde


def kepler(M, ecc):
    """sin and cos of the true anomaly; same shape as ``M`` (= shape of ``ecc``)."""
    return _Kepler.apply(M, ecc)


# ------------------------------------------------------------------------------
# quad_solution_vector
# ------------------------------------------------------------------------------
def _quad_sv(b, r, derivs):
    """(s, ds/db, ds/dr) of exo_quad_solution_vector_f64; the derivatives are None unless ``derivs``"""
    b = _dev(b, "b")
    r = _dev(r, "r")
    if b.shape != r.shape:
        raise ValueError("quad_solution_vector: b and r must have the same shape")
    s = torch.empty(b.shape + (3,), dtype=torch.float64, device=b.device)
    dsdb = torch.empty_like(s) if derivs else None
    dsdr = torch.empty_like(s) if derivs else None
    _call("exo_quad_solution_vector_f64", b.device, _ptr(b), _ptr(r), _ptr(s), _ptr(dsdb), _ptr(dsdr), b.numel(), _stream(b))
    return s, dsdb, dsdr


class _QuadSV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, r):
        need = any(ctx.needs_input_grad)   # (not .requires_grad: forward runs under no_grad and .contiguous() may copy)
        s, dsdb, dsdr = _quad_sv(b, r, need)
        if need:
            ctx.save_for_backward(dsdb, dsdr)
        return s

    @staticmethod
    def backward(ctx, gs):
        dsdb, dsdr = ctx.saved_tensors
        return (gs * dsdb).sum(-1), (gs * dsdr).sum(-1)


def quad_solution_vector(b, r):
    """s[..., 3] for separations ``b`` (|b| is used) and radius ratios ``r``."""
    return _QuadSV.apply(b, r)


@torch.no_grad()
def quad_solution_vector_derivs(b, r):
    """(s, ds/db, ds/dr), each [..., 3], as plain tensors -- for callers that carry their own
    differentiation (the PyTensor Op of compat_pytensor.py)."""
    return _quad_sv(b, r, True)


# ------------------------------------------------------------------------------
# contact_points (no gradient: it only selects cadences, keplerian.py:769-775)
# ------------------------------------------------------------------------------
@torch.no_grad()
def contact_points(a, e, cosw, sinw, cosi, sini, L):
    args = torch.broadcast_tensors(*[x.detach() for x in (a, e, cosw, sinw, cosi, sini, L)])
    args = [_dev(x, n) for x, n in zip(args, ("a", "e", "cosw", "sinw", "cosi", "sini", "L"))]
    ref = args[0]
    Ml = torch.empty_like(ref)
    Mr = torch.empty_like(ref)
    flag = torch.empty(ref.shape, dtype=torch.int32, device=ref.device)
    _call("exo_contact_points_f64", ref.device, *[_ptr(x) for x in args], _ptr(Ml), _ptr(Mr), _ptr(flag), ref.numel(),
          _stream(ref))
    return Ml, Mr, flag


# ------------------------------------------------------------------------------
# fused transit flux
# ------------------------------------------------------------------------------
class _Sweep(NamedTuple):
    """what every light-curve sweep of the C ABI takes first (include/exoplanet_amd.h), validated by _transit_args"""
    t: torch.Tensor
    texp: Optional[torch.Tensor]
    n_texp: int
    sdt: Optional[torch.Tensor]
    sw: Optional[torch.Tensor]
    n_sub: int
    params: torch.Tensor
    ld: torch.Tensor
    D: int
    P: int
    N: int

    def head(self, flags):
        """the twelve leading arguments of a sweep"""
        return (_ptr(self.t), self.N, _ptr(self.texp), self.n_texp, _ptr(self.sdt), _ptr(self.sw), self.n_sub,
                _ptr(self.params), _ptr(self.ld), self.D, self.P, flags)

    def ttv(self, ttv):
        """(edges (D, P, E), shift (D, P, E + 1), E) of a timing-variation table (include/exoplanet_amd.h); E = 0: none"""
        if ttv is None:
            return _NO_TTV
        edges, shift = ttv
        edges = _dev(edges, "ttv edges")
        shift = _dev(shift, "ttv shift")
        if edges.dim() != 3 or tuple(edges.shape[:2]) != (self.D, self.P) or edges.shape[2] < 1:
            raise ValueError("ttv edges must be (n_draw, n_planet, n_edge >= 1)")
        if tuple(shift.shape) != (self.D, self.P, edges.shape[2] + 1):
            raise ValueError("ttv shift must be (n_draw, n_planet, n_edge + 1)")
        return edges, shift, int(edges.shape[2])


_NO_TTV = (None, None, 0)


def _exposure_args(t, texp, stencil_dt, stencil_w):
    """(texp, n_texp, stencil_dt, stencil_w, n_sub) of a sweep over the cadences ``t``"""
    if texp is None:
        return None, 0, None, None, 1
    texp = _dev(texp, "texp").reshape(-1)
    stencil_dt = _dev(stencil_dt, "stencil_dt")
    stencil_w = _dev(stencil_w, "stencil_w")
    n_texp, n_sub = texp.numel(), stencil_dt.numel()
    if n_texp not in (1, t.numel()):
        raise ValueError("texp must be a scalar or have one entry per cadence")
    if stencil_w.numel() != n_sub or not 1 <= n_sub <= MAX_SUBEXP:
        raise ValueError(f"stencil must have 1..{MAX_SUBEXP} points")
    return texp, n_texp, stencil_dt, stencil_w, n_sub


def _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags):
    t = _dev(t, "t")
    params = _dev(params, "params")
    ld = _dev(ld, "ld")
    if t.dim() != 1:
        raise ValueError("t must be 1-D (n_cad,)")
    if params.dim() != 3 or params.shape[-1] != NPAR:
        raise ValueError(f"params must be (n_draw, n_planet, {NPAR})")
    D, P, _ = params.shape
    nld = 6 if flags & FLAG_SECONDARY else 3
    if ld.shape != (D, nld):
        raise ValueError(f"ld must be (n_draw, {nld})")
    if not 1 <= P <= MAX_PLANETS:
        raise ValueError(f"1 <= n_planet <= {MAX_PLANETS}")
    texp, n_texp, stencil_dt, stencil_w, n_sub = _exposure_args(t, texp, stencil_dt, stencil_w)
    return _Sweep(t, texp, n_texp, stencil_dt, stencil_w, n_sub, params, ld, D, P, t.numel())


def _flux_shape(N, D, P, flags):
    return (D, N, P) if flags & FLAG_PER_PLANET else (D, N)


def _flux_out(N, D, P, flags, device):
    """the dense flux array a sweep writes: rows, or under FLAG_CADENCE_MAJOR (D, N) with the draws innermost"""
    if flags & FLAG_CADENCE_MAJOR:
        return torch.empty((N, D), dtype=torch.float64, device=device).t()
    return torch.empty(_flux_shape(N, D, P, flags), dtype=torch.float64, device=device)


def _cotangent_layout(gflux, flags, cm_sweep, transpose):
    """(gflux, flags) for a sweep that reads a cotangent.  It is taken as it comes: cadence-major (the celerite kernels'
    gradient of a cadence-major model) or rows.  Only the run-enumeration sweeps read it cadence-major
    (include/exoplanet_amd.h; ``cm_sweep``: this is one): anything else gets rows.  Rows under FLAG_CADENCE_MAJOR are
    transposed if the caller lets them be (``transpose``), otherwise the flag goes."""
    if is_cadence_major(gflux) and cm_sweep:
        return gflux, flags | FLAG_CADENCE_MAJOR
    if flags & FLAG_CADENCE_MAJOR and transpose and cm_sweep:
        return _dev(gflux, "gflux").t().contiguous().t(), flags
    return _dev(gflux, "gflux"), flags & ~FLAG_CADENCE_MAJOR


# the Jacobian route of _TransitFlux: on from this many samples per cadence (with one sample a cadence the rows cost as much
# HBM traffic as the second sweep costs arithmetic: C3 gains nothing), up to this many bytes of rows (EXO_JAC_ROUTE=0: A/B)
_JAC_ROUTE = [os.environ.get("EXO_JAC_ROUTE", "1") != "0"]
_JAC_MIN_SUB = 2
_JAC_MAX_BYTES = 8 << 30


_JAC_DECISIONS = {}     # (device index, bytes of rows) -> bool: the first answer stands (warm-up, capture and replay agree)


def _jac_fits(nbytes, device):
    """the rows of derivatives are worst-case sized (16 doubles per (draw, planet, cadence), a few per cent touched): take the
    route only if they fit the cap AND half of what the device can still give (a smaller-memory device must fall
    back to the two-sweep route rather than run out).  "Can still give" = the driver's free bytes + what torch's caching
    allocator holds but has not handed out -- a warm sampler's reserved pool would otherwise read as a full device and flip
    the route between steps.  The decision is remembered per (device, size): a capture takes what its warm-up took."""
    if nbytes > _JAC_MAX_BYTES:
        return False
    key = (torch.device(device).index, int(nbytes))
    hit = _JAC_DECISIONS.get(key)
    if hit is not None:
        return hit
    try:
        if _capturing():
            return True          # (no warm-up call asked before this capture: nothing to agree with; not remembered)
        free, _ = torch.cuda.mem_get_info(device)
        free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        fits = 2 * nbytes <= free
    except Exception:
        fits = True
    _JAC_DECISIONS[key] = fits
    return fits


_JAC_CALLS = [0]        # forward sweeps that took the route (tests look at it)


def _use_jac(a, flags, wanted, n_edge=0, excluded=0):
    """the Jacobian route (include/exoplanet_amd.h, exo_transit_flux_fwd_jac_f64): when the gradient will be asked for
    (``wanted``) and a cadence is several samples, the value sweep keeps every solved cadence's row of derivatives and
    backward() is a contraction instead of a second sweep.  Returns the doubles the rows take, None for the two-sweep route.
    Per-cadence exposure times, per-planet / exact-scan / light-delay sweeps have no Jacobian form (without these exclusions
    the library refuses -- ADVICE r5: fall back to the two-sweep route instead); what else rules it out is the caller's:
    _TransitFlux passes its timing tables (``n_edge``) and FLAG_SPARSE (``excluded``), _TransitFluxSparse has neither."""
    if not (_JAC_ROUTE[0] and wanted and a.n_sub >= _JAC_MIN_SUB and not n_edge and a.n_texp <= 1
            and not flags & (FLAG_PER_PLANET | FLAG_EXACT_SCAN | FLAG_LIGHT_DELAY | excluded)):
        return None
    n_jac = _lib.load().exo_transit_flux_jac_doubles(a.N, a.D, a.P)
    # (the memory question last: it is a driver call -- ADVICE r5)
    return n_jac if _jac_fits(8 * n_jac, a.t.device) else None


def _forward_sweep(a, flags, ttv, flux, ws, nbytes, n_jac=None):
    """the value sweep: with timing tables, on the Jacobian route (``n_jac`` doubles of rows: allocated here and returned)
    or plain.  ``flux`` None: a sparse sweep, the values stay in the workspace."""
    edges, shift, n_edge = ttv
    dev, tail = a.t.device, (_ptr(ws), nbytes, _stream(a.t))
    if n_jac is not None:
        _JAC_CALLS[0] += 1
        jac = torch.empty(n_jac, dtype=torch.float64, device=dev)
        _call("exo_transit_flux_fwd_jac_f64", dev, *a.head(flags), _ptr(flux), _ptr(jac), n_jac, *tail)
        return jac
    if n_edge:
        _call("exo_transit_flux_ttv_fwd_f64", dev, *a.head(flags), _ptr(edges), _ptr(shift), n_edge, _ptr(flux), *tail)
    else:
        _call("exo_transit_flux_fwd_f64", dev, *a.head(flags), _ptr(flux), *tail)
    return None


def _jac_vjp(g, t, D, P, flags, jac, ws, nbytes, params, ld):
    """(gparams, gld): the rows a Jacobian-route forward sweep left, contracted with the cotangent ``g``"""
    gparams, gld = torch.empty_like(params), torch.empty_like(ld)
    _call("exo_transit_flux_jac_vjp_f64", t.device, _ptr(g), t.numel(), D, P, flags, _ptr(jac), _ptr(ws), nbytes,
          _ptr(gparams), _ptr(gld), 0, _stream(t))
    return gparams, gld


class _TransitFlux(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, params, ld, flags, ttv_edges, ttv_shift, grad_mode=True):
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        flags |= _sorted_flag(a.t)
        ttv = a.ttv(None if ttv_edges is None else (ttv_edges, ttv_shift))
        if flags & FLAG_CADENCE_MAJOR and flags & FLAG_PER_PLANET:
            raise ValueError("FLAG_CADENCE_MAJOR is a layout of the summed flux")
        flux = _flux_out(a.N, a.D, a.P, flags, a.t.device)
        ws, nbytes = _workspace(a.N, a.D, a.P, a.t.device)
        n_jac = _use_jac(a, flags, grad_mode and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]), ttv[2], FLAG_SPARSE)
        jac = _forward_sweep(a, flags, ttv, flux, ws, nbytes, n_jac)
        ctx.jac = None if jac is None else (jac, ws, nbytes)
        ctx.save_for_backward(a.t, a.texp, a.sdt, a.sw, a.params, a.ld, ttv[0], ttv[1])
        ctx.meta = (a.n_texp, a.n_sub, a.D, a.P, flags)
        return flux

    @staticmethod
    def backward(ctx, gflux):
        t, texp, sdt, sw, params, ld, edges, shift = ctx.saved_tensors
        n_texp, n_sub, D, P, flags = ctx.meta
        if ctx.jac is not None:
            gflux, flags = _cotangent_layout(gflux, flags, True, False)
            gparams, gld = _jac_vjp(gflux, t, D, P, flags, *ctx.jac, params, ld)
            return None, None, None, None, gparams, gld, None, None, None, None
        a = _Sweep(t, texp, n_texp, sdt, sw, n_sub, params, ld, D, P, t.numel())
        _, gparams, gld, _, gshift = _vjp(a, flags, gflux, False, ttv=None if edges is None else (edges, shift))
        return None, None, None, None, gparams, gld, None, None, gshift, None


def _vjp(a, flags, gflux, want_flux, events=(None, None), ttv=None, ws=None):
    """the value + VJP sweep -> (flux | SparseFlux | None, gparams, gld, dot, gshift | None).  ``ws``: a caller's
    (workspace, its bytes)"""
    N, D, P, dev = a.N, a.D, a.P, a.t.device
    flags |= _sorted_flag(a.t)
    shape = _flux_shape(N, D, P, flags)
    if isinstance(gflux, torch.Tensor) and tuple(gflux.shape) != shape:
        raise ValueError(f"gflux must have shape {shape}")
    edges, shift, n_edge = a.ttv(ttv)
    cm_sweep = (a.n_texp <= 1 and not flags & (FLAG_EXACT_SCAN | FLAG_PER_PLANET)
                and not (n_edge and flags & (FLAG_SECONDARY | FLAG_LIGHT_DELAY)))
    gflux, flags = _cotangent_layout(gflux, flags, cm_sweep, want_flux)
    ws, nbytes = ws or _workspace(N, D, P, dev)
    gparams = torch.empty_like(a.params)
    gld = torch.empty_like(a.ld)
    dot = torch.empty(D, dtype=torch.float64, device=dev)
    flux = _flux_out(N, D, P, flags, dev) if want_flux and not flags & FLAG_SPARSE else None
    gshift = torch.empty_like(shift) if n_edge else None
    tail = (_ptr(ws), nbytes, _stream(a.t))
    if n_edge:
        _call("exo_transit_flux_ttv_vjp_f64", dev, *a.head(flags), _ptr(edges), _ptr(shift), n_edge, _ptr(gflux), _ptr(flux),
              _ptr(gparams), _ptr(gld), _ptr(gshift), _ptr(dot), *tail)
    else:
        _call("exo_transit_flux_vjp_ev_f64", dev, *a.head(flags), _ptr(gflux), _ptr(flux), _ptr(gparams), _ptr(gld), _ptr(dot),
              *tail, events[0], events[1])
    if flags & FLAG_SPARSE:
        flux = _sparse_from_ws(ws, N, D, P, flags)
    return flux, gparams, gld, dot, gshift


def _sparse_from_ws(ws, N, D, P, flags):
    """the sweep's output lives in its workspace (include/exoplanet_amd.h, EXO_FLAG_SPARSE)"""
    return SparseFlux(ws, _sparse_layout(N, D, P), N, D, P, 2 if flags & FLAG_SECONDARY else 1)


def transit_flux(t, params, ld, texp=None, stencil_dt=None, stencil_w=None, flags=0, ttv=None):
    """Fused light curve for ``n_draw`` parameter sets.

    t (n_cad,), params (n_draw, n_planet, 20) (slot meaning: include/exoplanet_amd.h),
    ld (n_draw, 3|6).  Returns (n_draw, n_cad) or, with FLAG_PER_PLANET,
    (n_draw, n_cad, n_planet).  Differentiable w.r.t. ``params`` and ``ld``.
    ``ttv = (edges (n_draw, n_planet, E), shift (n_draw, n_planet, E + 1))``: transit-timing
    variations (every time is measured from the transit of its bin); differentiable
    w.r.t. ``shift`` as well.
    """
    edges, shift = (None, None) if ttv is None else ttv
    return _TransitFlux.apply(t, texp, stencil_dt, stencil_w, params, ld, int(flags),
                              None if edges is None else edges.detach(), shift, torch.is_grad_enabled())


@torch.no_grad()
def transit_flux_value_and_vjp(t, params, ld, gflux, texp=None, stencil_dt=None, stencil_w=None, flags=0,
                               events=(None, None), ttv=None):
    """One sweep over t: flux AND the cotangents of (params, ld) for a given
    ``gflux`` -- 24 B per (draw, cadence).  Returns (flux, gparams, gld), plus the
    cotangent of the shift table when ``ttv`` is given.
    ``events``: optional (hipEvent_t, hipEvent_t) handles (ints) recorded around
    the dominant kernel (profiling hook of the C ABI)."""
    flags = int(flags)
    a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
    out = _vjp(a, flags, gflux, True, events, ttv=ttv)
    return out[:3] if ttv is None else out[:3] + (out[4],)


class _TransitFluxDot(torch.autograd.Function):
    """(flux, L) with L[d] = sum_n gflux[d, n] * flux[d, n]: because the cotangent
    is known up front, forward runs the one-sweep value+vjp kernel and stores
    the parameter cotangents; backward only scales them by dL."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, params, ld, gflux, flags, events, ttv_edges, ttv_shift):
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        ttv = None if ttv_edges is None else (ttv_edges, ttv_shift)
        flux, gparams, gld, dot, gshift = _vjp(a, flags, gflux, True, events, ttv=ttv)
        ctx.save_for_backward(gparams, gld, gshift)
        ctx.set_materialize_grads(False)  # never build a (D, N) zero cotangent for the detached flux
        if isinstance(flux, SparseFlux):
            flux = flux._ws      # the workspace travels as a (non-differentiable) output; the wrapper rebuilds the views
        ctx.mark_non_differentiable(flux)
        return flux, dot

    @staticmethod
    def backward(ctx, _gflux_unused, gdot):
        gparams, gld, gshift = ctx.saved_tensors
        if gdot is None:
            return (None,) * 11
        return (None, None, None, None, gdot[:, None, None] * gparams, gdot[:, None] * gld, None, None, None, None,
                None if gshift is None else gdot[:, None, None] * gshift)


def transit_flux_dot(t, params, ld, gflux, texp=None, stencil_dt=None, stencil_w=None, flags=0,
                     events=(None, None), ttv=None):
    """One-sweep value + gradient for a cotangent known in advance: returns
    ``(flux, L)`` with ``L[d] = (gflux[d] * flux[d]).sum()``; ``L`` is
    differentiable w.r.t. ``params`` and ``ld`` (and the ``ttv`` shift table);
    flux itself is returned detached.  With ``flags | FLAG_SPARSE`` no dense flux array is written:
    the first return value is a :class:`SparseFlux` (runs of cadences + their values)."""
    edges, shift = (None, None) if ttv is None else ttv
    out = _TransitFluxDot.apply(t, texp, stencil_dt, stencil_w, params, ld, gflux, int(flags), events,
                                None if edges is None else edges.detach(), shift)
    if int(flags) & FLAG_SPARSE:
        return _sparse_from_ws(out[0], t.numel(), params.shape[0], params.shape[1], int(flags)), out[1]
    return out


def _chi2_launch(a, flags, ttv_edges, ttv_shift, obs, ivar):
    """exo_transit_chi2[_ttv]_vjp_f64 -> (chi2 (D,), gparams, gld, gshift | None)"""
    flags |= _sorted_flag(a.t)
    edges, shift, n_edge = a.ttv(None if ttv_edges is None else (ttv_edges, ttv_shift))
    dev = a.t.device
    ws, nbytes = _workspace(a.N, a.D, a.P, dev)
    chi2 = torch.empty(a.D, dtype=torch.float64, device=dev)
    gparams = torch.empty_like(a.params)
    gld = torch.empty_like(a.ld)
    gshift = torch.empty_like(shift) if n_edge else None
    data = (_ptr(obs), _ptr(ivar), ivar.numel(), _ptr(chi2), _ptr(gparams), _ptr(gld))
    tail = (_ptr(ws), nbytes, _stream(a.t))
    if n_edge:
        _call("exo_transit_chi2_ttv_vjp_f64", dev, *a.head(flags), _ptr(edges), _ptr(shift), n_edge, *data, _ptr(gshift), *tail)
    else:
        _call("exo_transit_chi2_vjp_f64", dev, *a.head(flags), *data, *tail)
    return chi2, gparams, gld, gshift


class _TransitChi2(torch.autograd.Function):
    """chi2[d] = sum_n w_n ((f[d, n] - obs[n])^2 - obs[n]^2) over the cadences solved for draw d, and -- computed in the
    same call, like transit_flux_dot -- its gradient with respect to params and ld (exo_transit_chi2_vjp_f64)."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, params, ld, obs, ivar, flags, ttv_edges, ttv_shift):
        if ctx.needs_input_grad[6] or ctx.needs_input_grad[7]:
            # (the kernels never hold the per-cadence residuals of every draw; see white_noise_loglike for what is offered)
            raise NotImplementedError(
                "transit_chi2 is not differentiable with respect to obs / ivar: per-draw error bars go through "
                "white_noise_loglike(yerr=(n_draw, 1) tensor), anything else through get_light_curve(total=True) and torch")
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        obs = _dev(obs, "obs")
        ivar = _dev(ivar, "ivar").reshape(-1)
        if tuple(obs.shape) != (a.N,):
            raise ValueError("obs must have shape (n_cad,)")
        if ivar.numel() not in (1, a.N):
            raise ValueError("ivar must be a scalar or have one entry per cadence")
        chi2, gparams, gld, gshift = _chi2_launch(a, flags, ttv_edges, ttv_shift, obs, ivar)
        ctx.save_for_backward(gparams, gld, *([] if gshift is None else [gshift]))
        return chi2

    @staticmethod
    def backward(ctx, gchi2):
        gparams, gld, *rest = ctx.saved_tensors
        gshift = gchi2[:, None, None] * rest[0] if rest else None
        return (None, None, None, None, gchi2[:, None, None] * gparams, gchi2[:, None] * gld, None, None, None, None, gshift)


class _SeriesCache:
    """What a likelihood derives from the data alone (residuals, variances, cos / sin of the angles, int32 instruments), made
    once per series: a sampler calls with the same series thousands of times.  One rule for every likelihood:

    * the key is (address, version, shape, strides, device) of every source tensor and the value of every number; the entry
      holds its sources, so an address cannot pass to another series while the entry lives;
    * at most ``capacity`` entries are kept; a further one empties the store first (a few series at most: no LRU);
    * a miss while the stream is being captured into a hipGraph is made and returned but not kept: its arrays belong to the
      graph's pool;
    * a hit while capturing -- GraphedStep warms up eagerly, so the series is here before the capture -- is in the graph by
      its addresses and held by nothing else, so the entry moves to ``pinned``, which is never emptied: a replay after any
      number of other series reads the arrays it captured (a few kB per captured series, for the life of the process).

    ``capturing``: the question, injectable so that the rule can be tested without a device."""

    def __init__(self, capacity=4, capturing=_capturing):
        self.capacity, self.capturing = capacity, capturing
        self.kept, self.pinned = {}, {}

    @staticmethod
    def key(sources):
        return tuple((x.data_ptr(), x._version, x.shape, x.stride(), x.device) if isinstance(x, torch.Tensor)
                     else x if x is None or isinstance(x, str) else float(x) for x in sources)

    def get(self, sources, make):
        """the entry of ``sources`` (tensors, numbers, None): ``.value`` is what ``make()`` returned, ``.sources`` the sources"""
        key = self.key(sources)
        entry = self.pinned.get(key)
        if entry is not None:
            return entry
        entry = self.kept.get(key)
        capturing = self.capturing()
        if entry is None:
            entry = SimpleNamespace(sources=sources, value=make())
            if not capturing:
                if len(self.kept) >= self.capacity:
                    self.kept.clear()
                self.kept[key] = entry
        elif capturing:
            self.pinned[key] = self.kept.pop(key)
        return entry


_CONSTS = _SeriesCache(capacity=256)    # a handful of error bars in practice: never let a sweep over values grow it
_WN_TERMS = _SeriesCache()     # white_noise_loglike: (series, error bars, mean) -> residuals, weights, constants
_NZ_DATA = _SeriesCache()      # sampled mean / jitter: (series, error bars) -> _NoiseData
_RV_SERIES = _SeriesCache()    # rv_loglike: (epochs, error bars, reference time, instruments) -> tau, variances, int32 instruments
_AST_SERIES = _SeriesCache()   # astrometry_loglike: (position angles, error bars) -> cos theta, sin theta, the two variances


def _const(value, device):
    """a one-element float64 device tensor holding ``value`` (cached per device: created once, outside any capture; one that
    a capture was handed stays for good, like a captured series)"""
    value = float(value)
    return _CONSTS.get((value, str(device)), lambda: torch.tensor([value], dtype=torch.float64, device=device)).value


def transit_chi2(t, params, ld, obs, ivar, texp=None, stencil_dt=None, stencil_w=None, flags=0, ttv=None):
    """White-noise misfit of ONE observed series ``obs`` (n_cad,) against the light curves of ``n_draw`` parameter
    sets, relative to an empty light curve, without any (n_draw, n_cad) array:
    ``chi2[d] = sum_n ivar_n ((flux[d, n] - obs[n])**2 - obs[n]**2)`` -- the sum runs over the cadences in which a
    planet of draw d can overlap the disk, everything else cancels.  Differentiable w.r.t. ``params`` and ``ld``
    (the gradient is computed in the same call).  ``ivar``: scalar or (n_cad,).  The Gaussian log-likelihood is
    ``-0.5 * (chi2 + (ivar * obs**2).sum()) + 0.5 * log(ivar / 2 pi).sum()``: :func:`white_noise_loglike`.
    ``ttv = (edges, shift)``: timing tables (transits only); differentiable w.r.t. ``shift`` as well."""
    edges, shift = (None, None) if ttv is None else ttv
    return _TransitChi2.apply(t, texp, stencil_dt, stencil_w, params, ld, obs, ivar, int(flags), edges, shift)


def _white_noise_terms(y, yerr, mean):
    """(y - mean, weights, sum w (y - mean)^2, sum log(w / 2 pi), and the likelihood's constant term (the last minus the
    one before, halved)) of a white-noise likelihood"""
    number = isinstance(yerr, (int, float))

    def make():
        if number:
            ivar = _const(1.0 / (float(yerr) * float(yerr)), y.device)      # cached: no upload inside a hipGraph capture
        else:
            err = _dev(yerr, "yerr")
            ivar = (1.0 / (err * err)).reshape(-1)
        obs = y - mean
        n = y.numel()
        const = (ivar * obs * obs).sum() if ivar.numel() == n else ivar[0] * (obs * obs).sum()
        lognorm = torch.log(ivar / (2.0 * torch.pi)).sum() * (1.0 if ivar.numel() == n else float(n))
        return obs, ivar, const, lognorm, 0.5 * (lognorm - const)

    # what depends on the data alone is computed once per (y, yerr, mean) -- where nothing of it requires grad
    if isinstance(mean, (int, float)) and not y.requires_grad and (number or not yerr.requires_grad):
        return _WN_TERMS.get((y, yerr, mean), make).value
    return make()


def per_draw_yerr(yerr, n_cad):
    """``yerr`` as a per-draw error bar: a tensor that broadcasts against a (n_draw, n_cad) light curve along the
    draws only -- 0-d, or last dimension 1 -- flattened to (n_draw | 1,); None for anything else (a number, a
    per-cadence vector)."""
    if not isinstance(yerr, torch.Tensor):
        return None
    if yerr.dim() == 0 or yerr.shape[-1] == 1 or (yerr.numel() == 1 and n_cad != 1):
        return yerr.reshape(-1)
    return None


_WN = "white-noise likelihood"
_WN_INSTEAD = ("LimbDarkLightCurve.white_noise_log_likelihood (it falls back to the dense light curve) or "
               "get_light_curve(total=True) with torch")


def _check_data_terms(y, yerr, mean):
    """the data-side terms of the white-noise likelihood carry no gradient through the fused kernels: refuse rather than
    return a partial gradient (jitter per chain: a (n_draw, 1) ``yerr``; anything else: the dense light curve + torch)"""
    _refuse_data_grad(_WN, "the orbit, the limb darkening and per-draw error bars (yerr of shape (n_draw, 1))", _WN_INSTEAD,
                      y=y, yerr=yerr, mean=mean)


def _scaled_loglike(unit_fn, y, yerr_d, mean):
    """log-likelihood for per-draw error bars from the unit-weight misfit: with w_d = 1 / yerr_d^2,
    ll_d = -w_d / 2 (chi2_1[d] + sum obs^2) + n / 2 log(w_d / 2 pi) -- differentiable in yerr_d through torch, in
    everything else through the kernels' own gradient; ``unit_fn(obs, one)`` returns chi2 at unit weights"""
    _check_data_terms(y, None, mean)
    obs, one, s2, _, _ = _white_noise_terms(y, 1.0, mean)
    w = 1.0 / (yerr_d * yerr_d)
    n = float(y.numel())
    chi2 = unit_fn(obs, one)
    if chi2.numel() != 1 and yerr_d.numel() not in (1, chi2.numel()):
        raise ValueError(f"white-noise likelihood: yerr holds {yerr_d.numel()} per-draw error bars, the parameters "
                         f"{chi2.numel()} draws -- one error bar, one per draw, or one system with many error bars")
    # (one system, many error bars -- a jitter chain per entry of yerr: the result has yerr's draws)
    return -0.5 * w * (chi2 + s2) + 0.5 * n * torch.log(w / (2.0 * torch.pi))


_NOISE_SERIES = 8  # doubles of exo_white_noise_terms_f64's `series`
_LOG_2PI = 1.8378770664093453


class _NoiseData:
    """what depends on (y, yerr) alone: the variances yerr^2 ((1,) or (n_cad,)) and the buffer of per-series sums that
    exo_white_noise_terms_f64 fills on its first eager call on a stream and reads in every later call on THAT stream
    (one buffer per stream: a call on another stream never reads sums that are still being written)"""

    def __init__(self, y, var):
        self.y, self.var = y, var
        self.series = {}     # stream -> filled buffer


def _noise_data(y, yerr):
    """the :class:`_NoiseData` of a series and its error bars (a number or a per-cadence tensor), made once per (y, yerr)"""
    def make():
        if isinstance(yerr, (int, float)):
            return _NoiseData(y, _const(float(yerr) * float(yerr), y.device))
        err = _dev(yerr, "yerr")
        var = (err * err).reshape(-1)
        if var.numel() not in (1, y.numel()):
            raise ValueError("yerr must be a number, one entry per cadence, or per draw: (n_draw, 1)")
        return _NoiseData(y, var)

    return _NZ_DATA.get((y, yerr), make).value


def _dev_or_number(x, name):
    return x if isinstance(x, (int, float)) else _dev(x, name)


def _per_draw(x, name, D, device, what, columns=False):
    """``x`` -- a number, or a 0-d / (1,) / (D,) / (D, 1) / (1, 1) device tensor -- as a 1-D tensor of 1 or D entries, one
    per draw of the likelihood ``what``; ``columns``: a (D, k) tensor as well, and the result is 2-D, of 1 or D rows"""
    if isinstance(x, (int, float)):
        x = _const(x, device)
        return x.reshape(1, 1) if columns else x
    if x.dim() > 2 or (x.dim() == 2 and not columns and x.shape[1] != 1):
        raise ValueError(f"{what}: `{name}` has shape {tuple(x.shape)} -- a number, one value per draw, or "
                         + ("(draws, instruments)" if columns else "(draws,) or (draws, 1)"))
    n = x.shape[0] if x.dim() == 2 else x.numel()
    if n not in (1, D):
        raise ValueError(f"{what}: `{name}` holds {n} draws, the parameters {D} -- one value, or one per draw")
    if columns:
        return x if x.dim() == 2 else x.reshape(-1, 1)
    return x if x.dim() == 1 else x.reshape(-1)


def _noise_launch(a, flags, ttv_edges, ttv_shift, data, var, mean, jit2):
    """exo_transit_noise[_ttv]_vjp_f64 + exo_white_noise_terms_f64 -> (loglike (D,), d/dmean (D,), d/djit2 (D,), gparams and
    gld of the MISFIT (d loglike = -1/2 of them), gshift | None)"""
    flags |= _sorted_flag(a.t)
    edges, shift, n_edge = a.ttv(None if ttv_edges is None else (ttv_edges, ttv_shift))
    dev = a.t.device
    y = data.y
    ws, nbytes = _workspace(a.N, a.D, a.P, dev)
    sums = torch.empty(3, a.D, dtype=torch.float64, device=dev)          # chi2, gmean, gjit2
    gparams = torch.empty_like(a.params)
    gld = torch.empty_like(a.ld)
    gshift = torch.empty_like(shift) if n_edge else None
    n_jit = 0 if jit2 is None else jit2.numel()
    noise = (_ptr(y), _ptr(var), var.numel(), _ptr(mean), mean.numel(), _ptr(jit2), n_jit,
             _ptr(sums[0]), _ptr(sums[1]), _ptr(sums[2]), _ptr(gparams), _ptr(gld))
    tail = (_ptr(ws), nbytes, _stream(a.t))
    if n_edge:
        _call("exo_transit_noise_ttv_vjp_f64", dev, *a.head(flags), _ptr(edges), _ptr(shift), n_edge, *noise, _ptr(gshift), *tail)
    else:
        _call("exo_transit_noise_vjp_f64", dev, *a.head(flags), *noise, *tail)
    # the sums over all cadences: per-series sums once per (y, yerr) and stream where the weight separates
    separable = n_jit == 0 or var.numel() == 1
    terms = torch.empty(5, a.D, dtype=torch.float64, device=dev)
    tws, tbytes = None, 0
    if not separable:
        tbytes = int(_lib.load().exo_white_noise_workspace_bytes(a.N, a.D))
        tws = torch.empty(tbytes // 8, dtype=torch.float64, device=dev)
    stream = _stream(a.t)
    capturing = _NZ_DATA.capturing()
    keep = separable and data.var is var
    series = None
    if keep and capturing:
        # sums that an eager call (the warm-up) filled before the capture began -- torch.cuda.graph waits for the device on
        # entry; the graph holds their address, and the entry that holds them is pinned (_SeriesCache).  A capture without a
        # warm-up gets a buffer from the graph's own pool and fills it on every replay.
        series = next(iter(data.series.values()), None)
    elif keep:
        series = data.series.get(stream)
    ready = series is not None
    if not ready:
        series = torch.empty(_NOISE_SERIES, dtype=torch.float64, device=dev)
    _call("exo_white_noise_terms_f64", dev, _ptr(y), _ptr(var), a.N, var.numel(), _ptr(mean), mean.numel(), _ptr(jit2), n_jit, a.D,
          _ptr(series), 1 if ready else 0, _ptr(terms), _ptr(tws), tbytes, stream)
    if keep and not ready and not capturing:
        data.series[stream] = series
    ll = torch.add(terms[0] + terms[1], sums[0]).mul_(-0.5).sub_(0.5 * a.N * _LOG_2PI)
    dmean = terms[2] - sums[1]
    djit2 = (terms[3] + sums[2] - terms[4]).mul_(0.5)
    return ll, dmean, djit2, gparams, gld, gshift


def _refuse_data_grads(ctx, first, names):
    for k, name in enumerate(names):
        if ctx.needs_input_grad[first + k]:
            raise NotImplementedError(
                f"white-noise likelihood: `{name}` requires grad, and the fused kernels differentiate the orbit, the limb "
                "darkening, `mean` and `jitter` only; use get_light_curve(total=True) with torch")


def _draw_cotangent(g, n):
    """cotangent of a (1,) or (D,) per-draw input from its per-draw contributions"""
    return g.sum().reshape(1) if n == 1 and g.numel() != 1 else g


class _TransitNoise(torch.autograd.Function):
    """White-noise log-likelihood with a per-draw mean and jitter (``jit2`` = jitter^2, or None): value and every gradient
    from one pass of the sweep (exo_transit_noise[_ttv]_vjp_f64) and the data terms (exo_white_noise_terms_f64)."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, params, ld, data, var, mean, jit2, flags, ttv_edges, ttv_shift):
        _refuse_data_grads(ctx, 7, ("yerr",))
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        ll, dmean, djit2, gparams, gld, gshift = _noise_launch(a, flags, ttv_edges, ttv_shift, data, var, mean, jit2)
        ctx.n_mean, ctx.n_jit = mean.numel(), 0 if jit2 is None else jit2.numel()
        ctx.save_for_backward(gparams, gld, dmean, djit2, *([] if gshift is None else [gshift]))
        return ll

    @staticmethod
    def backward(ctx, gll):
        gparams, gld, dmean, djit2, *rest = ctx.saved_tensors
        half = -0.5 * gll
        gshift = half[:, None, None] * rest[0] if rest else None
        gjit2 = _draw_cotangent(gll * djit2, ctx.n_jit) if ctx.n_jit else None
        return (None, None, None, None, half[:, None, None] * gparams, half[:, None] * gld, None, None,
                _draw_cotangent(gll * dmean, ctx.n_mean), gjit2, None, None, gshift)


def sampled_noise(mean, jitter):
    """whether (``mean``, ``jitter``) take the sampled-mean / jitter kernels: any jitter, a per-draw ``mean``, a ``mean``
    that requires grad.  A number, and a one-element tensor that is a constant of the call, stay where they always went
    (:func:`_white_noise_terms`, :func:`_scaled_loglike`): same launches, same bits as before those kernels existed."""
    if jitter is not None:
        return True
    return isinstance(mean, torch.Tensor) and (mean.numel() > 1 or (mean.requires_grad and torch.is_grad_enabled()))


def _noise_inputs(y, yerr, mean, jitter, D):
    """(data, var, mean, jit2) of the sampled-mean / jitter likelihood for ``D`` draws: a per-draw ``yerr`` is a jitter on
    top of a zero variance"""
    yd = per_draw_yerr(yerr, y.numel())
    _refuse_data_grad(_WN, "the orbit, the limb darkening, `mean`, `jitter` and per-draw error bars", _WN_INSTEAD,
                      y=y, yerr=yerr if yd is None else None)
    dev = y.device

    def per_draw(x, name):      # (any shape that holds one value or one per draw, as this likelihood always took them)
        if isinstance(x, torch.Tensor) and x.dim() > 1 and tuple(x.shape[1:]) != (1,):
            x = x.reshape(-1)
        return _per_draw(_dev_or_number(x, name), name, D, dev, _WN)

    mean = per_draw(mean, "mean")
    jit2 = None
    if jitter is not None:
        jit2 = per_draw(jitter, "jitter")
        jit2 = jit2 * jit2 if isinstance(jitter, torch.Tensor) else _const(float(jitter) ** 2, dev)
    if yd is not None:
        yd = per_draw(yd, "yerr")
        jit2 = yd * yd if jit2 is None else yd * yd + jit2
        data = _noise_data(y, 0.0)
    else:
        data = _noise_data(y, yerr)
    return data, data.var, mean, jit2


def white_noise_loglike(t, params, ld, y, yerr, mean=0.0, texp=None, stencil_dt=None, stencil_w=None, flags=0, ttv=None,
                        jitter=None):
    """Gaussian log-likelihood (n_draw,) of the observed series ``y`` with independent errors ``yerr`` (a number, a
    per-cadence vector, or PER DRAW: a 0-d / (n_draw, 1) tensor, differentiable -- a jitter term sampled per chain)
    given ``mean + light curve`` -- the reference's ``pm.Normal("obs", mu=mean + lc, sigma=yerr, observed=y)`` for a
    batch of parameter sets, value and gradient in one call (:func:`transit_chi2`).

    ``mean``: a number, or PER DRAW -- a 0-d, (n_draw,) or (n_draw, 1) tensor -- and ``jitter`` (None, a number or per
    draw likewise), added to ``yerr`` in quadrature: ``sigma = sqrt(yerr**2 + jitter**2)``.  Both are differentiable and
    stay on the sparse light curve (exo_transit_noise_vjp_f64 + exo_white_noise_terms_f64): the reference's
    ``pm.Normal("obs", mu=mean + lc, sigma=sqrt(yerr**2 + exp(2 * log_jitter)), observed=y)`` with ``mean`` and
    ``log_jitter`` sampled.  ``y`` and a per-cadence ``yerr`` are data: one that requires grad is refused, not silently
    dropped."""
    y = _dev(y, "y")
    kw = dict(texp=texp, stencil_dt=stencil_dt, stencil_w=stencil_w, flags=flags, ttv=ttv)
    if sampled_noise(mean, jitter):
        params = _dev(params, "params")
        if tuple(y.shape) != (_dev(t, "t").numel(),):
            raise ValueError("y must have shape (n_cad,)")
        data, var, mean, jit2 = _noise_inputs(y, yerr, mean, jitter, params.shape[0])
        edges, shift = (None, None) if ttv is None else ttv
        return _TransitNoise.apply(t, texp, stencil_dt, stencil_w, params, ld, data, var, mean, jit2, int(flags), edges, shift)
    yd = per_draw_yerr(yerr, y.numel())
    if yd is not None:
        return _scaled_loglike(lambda obs, one: transit_chi2(t, params, ld, obs, one, **kw), y, _dev(yd, "yerr"), mean)
    _check_data_terms(y, yerr, mean)
    obs, ivar, const, lognorm, _ = _white_noise_terms(y, yerr, mean)
    chi2 = transit_chi2(t, params, ld, obs, ivar, **kw)
    return -0.5 * (chi2 + const) + 0.5 * lognorm


class SparseFlux:
    """Output of a sparse sweep (include/exoplanet_amd.h, EXO_FLAG_SPARSE): for every list
    (draw, planet, event) the runs of cadences in which the planet can overlap the disk, and the
    flux of exactly those cadences; every other cadence has flux 0.  Tensors are views into the
    sweep's workspace (kept alive here)."""

    def __init__(self, ws, layout, n_cad, D, P, n_ev):
        off_nrun, off_runs, off_pre, off_vals, r_max = layout
        i32 = ws.view(torch.int32)
        n_list = D * P * n_ev
        self.n_cad, self.n_draw, self.n_planet, self.n_ev, self.r_max = n_cad, D, P, n_ev, r_max
        self.nrun = i32[off_nrun // 4: off_nrun // 4 + n_list].view(D, P, n_ev)
        self.runs = i32[off_runs // 4: off_runs // 4 + n_list * r_max * 4].view(D, P, n_ev, r_max, 4)
        self.pre_all = i32[off_pre // 4: off_pre // 4 + n_list * (r_max + 1)].view(D, P, n_ev, r_max + 1)
        self.vals = ws[off_vals // 8: off_vals // 8 + D * P * n_cad].view(D, P, n_cad)
        self._ws = ws

    def n_solved(self):
        """cadences in runs, summed over all lists (one host synchronisation)"""
        k = self.nrun.long().unsqueeze(-1)
        return int(torch.gather(self.pre_all.long(), -1, k).sum().item())

    def to_dense(self, per_planet=False):
        """(D, N) summed flux, or (D, N, P): rebuilt on the host (tests / plots)"""
        nrun, runs = self.nrun.cpu().numpy(), self.runs.cpu().numpy()
        pre, vals = self.pre_all.cpu().numpy(), self.vals.cpu().numpy()
        out = np.zeros((self.n_draw, self.n_cad, self.n_planet))
        for d in range(self.n_draw):
            for p in range(self.n_planet):
                base = 0
                for e in range(self.n_ev):
                    for k in range(nrun[d, p, e]):
                        lo, _, _, hi = runs[d, p, e, k]
                        out[d, lo:hi, p] = vals[d, p, base + pre[d, p, e, k]: base + pre[d, p, e, k] + hi - lo]
                    base += pre[d, p, e, nrun[d, p, e]]
        return out if per_planet else out.sum(-1)


@torch.no_grad()
def transit_flux_sparse(t, params, ld, gflux=None, texp=None, stencil_dt=None, stencil_w=None, flags=0, ttv=None, ws=None):
    """Sparse sweep: no dense flux array is written.  Returns a :class:`SparseFlux`, and with
    ``gflux`` (dense cotangent, read only at the solved cadences) also (gparams, gld, dot[, gshift]).
    Needs sorted times, a scalar (or no) exposure time and no FLAG_EXACT_SCAN; ``ttv = (edges, shift)``:
    timing tables (transits only)."""
    flags = int(flags) | FLAG_SPARSE
    a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
    if ttv is not None and flags & FLAG_SECONDARY:
        raise ValueError("the sparse sweep takes timing tables for transits only")
    N, D, P = a.N, a.D, a.P
    if ws is None:
        ws, nbytes = _workspace(N, D, P, a.t.device)
    else:
        nbytes = _workspace_bytes(N, D, P)
        if ws.dtype != torch.float64 or ws.numel() * 8 < nbytes or not ws.is_contiguous() or ws.device != a.t.device:
            raise ValueError("ws: a contiguous float64 tensor of at least exo_transit_flux_workspace_bytes on the device of t")
    if gflux is None:
        _forward_sweep(a, flags | _sorted_flag(a.t), a.ttv(ttv), None, ws, nbytes)
        return _sparse_from_ws(ws, N, D, P, flags)
    # (the cotangent in rows and no dense flux: the sweep reads it at the solved cadences only)
    out = _vjp(a, flags, _dev(gflux, "gflux"), False, ttv=ttv, ws=(ws, nbytes))
    return out[:4] if ttv is None else out


# ------------------------------------------------------------------------------
# the light curve as a SPARSE model of a GP (round 5): segments of cadences + their values, differentiable
# ------------------------------------------------------------------------------
_SPARSE_MEAN = [os.environ.get("EXO_SPARSE_MEAN", "1") != "0"]     # (0: A/B -- get_light_curve(sparse=True) returns the dense array)


_MULTI_LIST_MEAN = [os.environ.get("EXO_SPARSE_MULTI_LIST", "1") != "0"]    # (0: several lists per draw keep the dense mean -- A/B)


def sparse_mean_supported(n_texp, n_edge, flags, P):
    """can this light curve travel to the celerite kernels as segments + values?  A run-enumeration sweep of the summed flux
    without timing tables or light delay.  One list per draw (one planet, no occultations): the sweep's runs ARE the segments
    (exo_transit_flux_sparse_model); several lists -- planets, occultations -- are merged on the device first
    (exo_sparse_model_merge_f64, round 6)"""
    n_ev = 2 if flags & FLAG_SECONDARY else 1
    return (_SPARSE_MEAN[0] and (P * n_ev == 1 or _MULTI_LIST_MEAN[0]) and n_texp <= 1 and not n_edge
            and not flags & (FLAG_PER_PLANET | FLAG_EXACT_SCAN | FLAG_LIGHT_DELAY | FLAG_CADENCE_MAJOR))


class _TransitFluxSparse(torch.autograd.Function):
    """the EXO_FLAG_SPARSE sweep as a differentiable op: returns (values (D, P * N) -- a view of the value array inside the
    sweep's workspace --, workspace).  The cotangent of `values` comes back in the same layout (the sparse celerite entry
    writes it at the positions of the values) and goes to the reverse sweep as it is -- or, on the Jacobian route, to the
    contraction: no dense (draw, cadence) array in either direction."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, params, ld, flags, box, grad_mode):
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        flags = (flags | FLAG_SPARSE | _sorted_flag(a.t)) & ~FLAG_CADENCE_MAJOR
        N, D, P = a.N, a.D, a.P
        ws, nbytes = _workspace(N, D, P, a.t.device)
        off_vals = _sparse_layout(N, D, P)[3]
        # (grad_mode: torch.is_grad_enabled() of the CALLER -- inside forward() it is always off; under no_grad the rows of
        # derivatives would be written for nothing: ADVICE r4)
        n_jac = _use_jac(a, flags, grad_mode and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]))
        ctx.jac = _forward_sweep(a, flags, _NO_TTV, None, ws, nbytes, n_jac)
        vals = ws[off_vals // 8: off_vals // 8 + D * P * N].view(D, P * N)
        ctx.save_for_backward(a.t, a.texp, a.sdt, a.sw, a.params, a.ld)
        ctx.meta = (a.n_texp, a.n_sub, D, P, flags, nbytes)
        ctx.ws = ws
        box.append(ws)      # (the workspace is not an autograd output -- `vals` is a view of it: the caller's box keeps it)
        return vals

    @staticmethod
    def backward(ctx, gvals):
        t, texp, sdt, sw, params, ld = ctx.saved_tensors
        n_texp, n_sub, D, P, flags, nbytes = ctx.meta
        N = t.numel()
        if gvals is None:
            return (None,) * 9
        if not gvals.is_contiguous() or tuple(gvals.shape) != (D, P * N):
            raise ValueError("the cotangent of a sparse light curve's values must be a contiguous (n_draw, n_planet * n_cad) array")
        if ctx.jac is not None:
            gparams, gld = _jac_vjp(gvals, t, D, P, flags, ctx.jac, ctx.ws, nbytes, params, ld)
        else:
            gparams, gld = torch.empty_like(params), torch.empty_like(ld)
            a = _Sweep(t, texp, n_texp, sdt, sw, n_sub, params, ld, D, P, N)
            _call("exo_transit_flux_vjp_sparse_f64", t.device, *a.head(flags), _ptr(gvals), _ptr(gparams), _ptr(gld), 0,
                  _ptr(ctx.ws), nbytes, 1, _stream(t))
        return None, None, None, None, gparams, gld, None, None, None


def _expand_runs(lo, hi, count, vstart, draw):
    """flat index lists (position in values.view(-1), cadence, draw) of every cadence in runs [lo, hi) -- tensors (..., K) of
    which the first ``count`` (...,) of a row are live --, ``vstart`` the position of a run's first value, ``draw`` its draw
    (broadcast against lo); built with torch ops"""
    dev = lo.device
    live = torch.arange(lo.shape[-1], device=dev) < count.unsqueeze(-1)
    flat_len = torch.where(live, hi - lo, torch.zeros_like(lo)).reshape(-1)
    total = int(flat_len.sum().item())
    rid = torch.repeat_interleave(torch.arange(flat_len.numel(), device=dev), flat_len, output_size=total)
    start = torch.cumsum(flat_len, 0) - flat_len
    within = torch.arange(total, device=dev) - start[rid]
    return vstart.reshape(-1)[rid] + within, lo.reshape(-1)[rid] + within, draw.expand_as(lo).reshape(-1)[rid]


class _SparseToDense(torch.autograd.Function):
    """(D, N) dense summed flux of a sparse light curve, differentiable (the fallback for uses the sparse celerite entry does
    not cover): scatter forward, gather of the cotangent at the solved cadences backward -- both on the host-side indices of
    the runs, a handful of torch kernels (not a hot path)"""

    @staticmethod
    def forward(ctx, vals, sp):
        idx_val, idx_cad, idx_draw = sp._indices()
        out = torch.zeros(sp.n_draw, sp.n_cad, dtype=torch.float64, device=vals.device)
        # the lists of a draw (planets, occultations) may cover the same cadence, and their values add up; a merged light
        # curve's segments are disjoint: plain assignment
        if sp._lists_overlap:
            out.index_put_((idx_draw, idx_cad), vals.reshape(-1)[idx_val], accumulate=True)
        else:
            out[idx_draw, idx_cad] = vals.reshape(-1)[idx_val]
        ctx.sp = sp
        return out

    @staticmethod
    def backward(ctx, gout):
        sp = ctx.sp
        idx_val, idx_cad, idx_draw = sp._indices()
        # (the cotangent in the layout of `values`: the sweep's (D, P * N), or (D, N) of a merged light curve)
        g = torch.zeros(sp.n_draw, sp._values_per_draw(), dtype=torch.float64, device=gout.device)
        g.view(-1)[idx_val] = gout[idx_draw, idx_cad]
        return g, None


class SparseLightCurve:
    """What ``get_light_curve(total=True, sparse=True)`` returns for a batch of draws: the summed light curve as the runs
    of cadences in which a planet can overlap the disk and the flux of exactly those cadences (every other cadence: 0),
    differentiable through ``values``.  It is the ``mean`` of a ``GaussianProcess``: the celerite kernels read the
    segments and write the mean's cotangent back at the values, and the (draws, cadences) array -- 97 % zeros -- never
    exists (C3: 3.8 -> ~3.1 ms per value + gradient).  ``dense()`` gives the ordinary (draws, cadences) tensor."""

    def __init__(self, values, ws, n_cad, n_draw, n_planet, flags):
        self.values, self._ws = values, ws
        self.n_cad, self.n_draw, self.n_planet, self.flags = n_cad, n_draw, n_planet, flags
        self.shape = (n_draw, n_cad)

    def layout(self):
        return _sparse_from_ws(self._ws, self.n_cad, self.n_draw, self.n_planet, self.flags)

    def model_struct(self):
        """exo_sparse_model for the celerite entries (a host struct of device pointers: keep ``self`` alive while it is used)"""
        m = _lib.SparseModel()
        n_ev = 2 if self.flags & FLAG_SECONDARY else 1
        if self.n_planet * n_ev != 1:
            raise ValueError("a sparse GaussianProcess mean is one list of segments per draw; this light curve has "
                             f"{self.n_planet} planet(s) x {n_ev} event(s): use .merged() (or .dense())")
        _call("exo_transit_flux_sparse_model", None, _ptr(self._ws), _workspace_bytes(self.n_cad, self.n_draw, self.n_planet),
              self.n_cad, self.n_draw, self.n_planet, self.flags & FLAG_SECONDARY, ctypes.addressof(m))
        return m

    _lists_overlap = True       # (several lists per draw: _SparseToDense)

    def _values_per_draw(self):
        return self.n_planet * self.n_cad

    def _indices(self):
        """(position in values.view(-1), cadence, draw) of every solved cadence -- built with torch ops from the runs"""
        lay = self.layout()
        D, P, N = self.n_draw, self.n_planet, self.n_cad
        nrun = lay.nrun.long()                                   # (D, P, n_ev)
        K = int(nrun.max().item()) if nrun.numel() else 0
        dev = self.values.device
        if K == 0:
            z = torch.zeros(0, dtype=torch.long, device=dev)
            return z, z, z
        runs = lay.runs[..., :K, :].long()                       # (D, P, n_ev, K, 4)
        pre = lay.pre_all[..., :K].long()
        tot = torch.gather(lay.pre_all.long(), -1, nrun.unsqueeze(-1)).squeeze(-1)          # (D, P, n_ev)
        evbase = torch.cumsum(tot, -1) - tot                      # occultations behind the transits
        d_i = torch.arange(D, device=dev).view(D, 1, 1, 1)
        p_i = torch.arange(P, device=dev).view(1, P, 1, 1)
        vbase = (d_i * P + p_i) * N + evbase.unsqueeze(-1) + pre  # first value of every run
        return _expand_runs(runs[..., 0], runs[..., 3], nrun, vbase, d_i)

    def dense(self):
        """the (draws, cadences) summed flux, differentiable"""
        return _SparseToDense.apply(self.values, self)

    def merged(self):
        """this light curve with ONE list of segments per draw (what the celerite kernels take): itself when it already is
        (one planet, no occultations), otherwise the lists merged on the device -- union of the runs, values summed over the
        planets / events per cadence -- as a :class:`MergedSparseLightCurve`, differentiable through ``values``"""
        n_ev = 2 if self.flags & FLAG_SECONDARY else 1
        if self.n_planet * n_ev == 1:
            return self
        box = []
        mvals = _MergeSparse.apply(self.values, self, box)
        return MergedSparseLightCurve(mvals, box[0], self.n_cad, self.n_draw, self.n_planet, self.flags)

    def detach(self):
        return SparseLightCurve(self.values.detach(), self._ws, self.n_cad, self.n_draw, self.n_planet, self.flags)

    # Arithmetic: a sparse light curve in an expression -- ``offset + lc``, ``lc * depth`` -- becomes the ordinary
    # (draws, cadences) tensor (``dense()``: differentiable), so code written for the dense return type keeps working whatever
    # get_light_curve(sparse=True) could return for the model; only a GaussianProcess mean stays sparse.
    def __add__(self, other): return self.dense() + other
    def __radd__(self, other): return other + self.dense()
    def __sub__(self, other): return self.dense() - other
    def __rsub__(self, other): return other - self.dense()
    def __mul__(self, other): return self.dense() * other
    def __rmul__(self, other): return other * self.dense()
    def __truediv__(self, other): return self.dense() / other
    def __neg__(self): return -self.dense()


_POISON = [None]    # tests: fill the merge workspace and its cotangent buffer with this value first (nothing may depend on what they
                    # held before the call -- under hipGraph replay that is the previous step's: gp/celerite.py has the same hook)


def _merge_bytes(N, D, P):
    return _lib.load().exo_sparse_merge_workspace_bytes(N, D, P)


def _scratch(n, device):
    x = torch.empty(n, dtype=torch.float64, device=device)
    if _POISON[0] is not None:
        x.fill_(_POISON[0])
    return x


class _MergeSparse(torch.autograd.Function):
    """values of a several-list sparse light curve (D, P * N: the sweep's layout) -> values of the merged model (D, N), of which
    row d's first off[d][nseg[d]] entries are defined (exo_sparse_model_merge_f64); backward: the cotangent of the merged values
    back at the lists' value positions (exo_sparse_model_merge_vjp_f64).  `box` receives the merge workspace."""

    @staticmethod
    def forward(ctx, vals, sp, box):
        N, D, P = sp.n_cad, sp.n_draw, sp.n_planet
        nbytes, mbytes = _workspace_bytes(N, D, P), _merge_bytes(N, D, P)
        mws = _scratch(max(mbytes // 8 + 1, 1), vals.device)
        _call("exo_sparse_model_merge_f64", vals.device, _ptr(sp._ws), nbytes, N, D, P, sp.flags & FLAG_SECONDARY, _ptr(mws),
              mbytes, None, _stream(vals))
        off_vals = _merge_layout(N, D, P)[3]
        ctx.sp, ctx.mws, ctx.sizes = sp, mws, (nbytes, mbytes)
        box.append(mws)
        return mws[off_vals // 8: off_vals // 8 + D * N].view(D, N)

    @staticmethod
    def backward(ctx, gm):
        sp = ctx.sp
        N, D, P = sp.n_cad, sp.n_draw, sp.n_planet
        nbytes, mbytes = ctx.sizes
        if not gm.is_contiguous() or tuple(gm.shape) != (D, N):
            raise ValueError("the cotangent of a merged sparse light curve's values must be a contiguous (n_draw, n_cad) array")
        # (only the positions the lists cover are defined, as in `vals` itself -- gp/celerite.py, _CeleriteLogLikeSparse.backward)
        gvals = _scratch(D * P * N, gm.device).view(D, P * N)
        _call("exo_sparse_model_merge_vjp_f64", gm.device, _ptr(sp._ws), nbytes, N, D, P, sp.flags & FLAG_SECONDARY,
              _ptr(ctx.mws), mbytes, _ptr(gm), _ptr(gvals), _stream(gm))
        return gvals, None, None


class MergedSparseLightCurve(SparseLightCurve):
    """A sparse light curve of several lists per draw (planets, occultations) merged into one list of disjoint segments per
    draw, a cadence's value the sum over the lists: the ``mean`` of a ``GaussianProcess`` for multi-planet and
    secondary-eclipse models (round 6).  ``values`` is (draws, cadences) with the first ``off[nseg]`` entries of a row defined."""

    def merged(self):
        return self

    def model_struct(self):
        m = _lib.SparseModel()
        _call("exo_sparse_model_merged", None, _ptr(self._ws), _merge_bytes(self.n_cad, self.n_draw, self.n_planet), self.n_cad,
              self.n_draw, self.n_planet, ctypes.addressof(m))
        return m

    def segments(self):
        """(nseg (D,), seg (D, cap, 2), off (D, cap + 1)) int32 views of the merge workspace"""
        o_nseg, o_seg, o_off, _, cap = _merge_layout(self.n_cad, self.n_draw, self.n_planet)
        raw = self._ws.view(torch.int32)
        D = self.n_draw
        nseg = raw[o_nseg // 4: o_nseg // 4 + D]
        seg = raw[o_seg // 4: o_seg // 4 + D * cap * 2].view(D, cap, 2)
        off = raw[o_off // 4: o_off // 4 + D * (cap + 1)].view(D, cap + 1)
        return nseg, seg, off

    def layout(self):
        raise NotImplementedError("a merged light curve has segments(), not the sweep's per-list runs")

    _lists_overlap = False      # (disjoint segments: _SparseToDense)

    def _values_per_draw(self):
        return self.n_cad

    def _indices(self):
        nseg, seg, off = self.segments()
        D, N = self.n_draw, self.n_cad
        K = int(nseg.max().item()) if nseg.numel() else 0
        if K == 0:
            z = torch.zeros(0, dtype=torch.long, device=self.values.device)
            return z, z, z
        d_i = torch.arange(D, device=self.values.device).view(D, 1)
        return _expand_runs(seg[:, :K, 0].long(), seg[:, :K, 1].long(), nseg.long(), d_i * N + off[:, :K].long(), d_i)

    def detach(self):
        return MergedSparseLightCurve(self.values.detach(), self._ws, self.n_cad, self.n_draw, self.n_planet, self.flags)


def transit_flux_sparse_model(t, params, ld, texp=None, stencil_dt=None, stencil_w=None, flags=0):
    """the summed light curve of ``n_draw`` parameter sets as a :class:`SparseLightCurve` with one list of segments per draw
    (differentiable w.r.t. ``params`` and ``ld``): the sweep's own runs for one planet without occultations, the merged form
    (:class:`MergedSparseLightCurve`) otherwise; see :func:`sparse_mean_supported` for what qualifies"""
    box = []
    vals = _TransitFluxSparse.apply(t, texp, stencil_dt, stencil_w, params, ld, int(flags), box, torch.is_grad_enabled())
    return SparseLightCurve(vals, box[0], t.numel(), params.shape[0], params.shape[1], int(flags) | FLAG_SPARSE).merged()


class KeptDenseFlux:
    """A dense (D, N) flux array KEPT ACROSS STEPS (include/exoplanet_amd.h, exo_transit_sparse_scatter_f64).

    The dense sweep zero-fills every cadence of every draw on every call (1.2 GB at 1024 draws x 150 000 cadences) although a
    step of a sampler solves the same few per cent of them as the step before.  This object owns the flux array and the
    sweep's workspace: ``step`` zeroes the cadences the LAST step solved, runs the sparse sweep, and writes the cadences THIS
    step solved -- after every step ``flux`` holds what ``transit_flux`` / ``transit_flux_vjp`` would have returned, bit for
    bit, for the price of the sparse sweep.  The state is this object's, not the library's; ``flux`` must not be written by
    anyone else.  Total flux, run-enumeration sweeps (sorted times, a scalar or no exposure time), no timing tables."""

    def __init__(self, t, n_draw, n_planet, texp=None, stencil_dt=None, stencil_w=None, flags=0):
        if int(flags) & (FLAG_PER_PLANET | FLAG_CADENCE_MAJOR | FLAG_EXACT_SCAN | FLAG_SPARSE):
            raise ValueError("KeptDenseFlux: the summed flux in rows, run-enumeration sweeps")
        self.t = _dev(t, "t")
        self.texp, self.stencil = texp, (stencil_dt, stencil_w)
        self.flags = int(flags)
        self.D, self.P, self.N = int(n_draw), int(n_planet), self.t.numel()
        # zeroed: a workspace without runs (the first step has nothing to clear), a flux array without a transit
        self._ws, self._nbytes = _workspace(self.N, self.D, self.P, self.t.device, zero=True)
        self.flux = torch.zeros(self.D, self.N, dtype=torch.float64, device=self.t.device)

    def _scatter(self, clear):
        _call("exo_transit_sparse_scatter_f64", self.t.device, _ptr(self._ws), self._nbytes, self.N, self.D, self.P,
              self.flags & FLAG_SECONDARY, 1 if clear else 0, _ptr(self.flux), _stream(self.t))

    @torch.no_grad()
    def step(self, params, ld, gflux=None):
        """-> flux (D, N) [, gparams, gld, dot with a cotangent ``gflux`` (D, N)]; ``flux`` is this object's array"""
        if params.shape[0] != self.D or params.shape[1] != self.P:
            raise ValueError("params: (n_draw, n_planet, NPAR) as this object was made for")
        self._scatter(True)
        out = transit_flux_sparse(self.t, params, ld, gflux, self.texp, self.stencil[0], self.stencil[1], self.flags, ws=self._ws)
        self._scatter(False)
        return self.flux if gflux is None else (self.flux,) + tuple(out[1:])


# ------------------------------------------------------------------------------
# timing tables of a TTVOrbit given O-C offsets
# ------------------------------------------------------------------------------
class _TtvTables(torch.autograd.Function):
    """(edges, shift) of exo_ttv_tables_f64 from period (D|1, P), t0 (D|1, P) and one (D|1, n_p) tensor of offsets per
    planet; differentiable in the offsets and the period (the edges carry no gradient, t0 none through the tables)"""

    @staticmethod
    def forward(ctx, period, t0, n_draw, *ttvs):
        period, t0 = _dev(period.detach(), "period"), _dev(t0.detach(), "t0")
        ttvs = [_dev(x.detach(), "ttvs") for x in ttvs]
        P, D = len(ttvs), int(n_draw)
        counts = [int(x.shape[-1]) for x in ttvs]
        n_edge = max(counts) + 1
        edges = torch.empty(D, P, n_edge, dtype=torch.float64, device=period.device)
        shift = torch.empty(D, P, n_edge + 1, dtype=torch.float64, device=period.device)
        _call("exo_ttv_tables_f64", period.device, *_TtvTables._args(period, t0, ttvs, counts), D, P, n_edge, _ptr(edges),
              _ptr(shift), _stream(period))
        ctx.save_for_backward(period, t0, *ttvs)
        ctx.meta = (D, P, n_edge, counts)
        ctx.mark_non_differentiable(edges)
        return edges, shift

    @staticmethod
    def _args(period, t0, ttvs, counts):
        def strides(x):      # (rows, P) -> element strides of (draw, planet); one row: broadcast over draws
            return (x.stride(0) if x.shape[0] > 1 else 0, x.stride(1) if x.shape[1] > 1 else 0)

        P = len(ttvs)
        tp = _ptr_array(ttvs, P)
        td = (ctypes.c_int64 * P)(*[(x.stride(0) if x.shape[0] > 1 else 0) for x in ttvs])
        tn = (ctypes.c_int32 * P)(*counts)
        return (_ptr(period), *strides(period), _ptr(t0), *strides(t0), tp, td, tn)

    @staticmethod
    def backward(ctx, _gedges, gshift):
        period, t0, *ttvs = ctx.saved_tensors
        D, P, n_edge, counts = ctx.meta
        if gshift is None:
            return (None,) * (3 + P)
        gshift = _dev(gshift, "gshift")
        need_p = ctx.needs_input_grad[0]
        gper = torch.empty(D, P, dtype=torch.float64, device=gshift.device) if need_p else None
        gt = [torch.empty(D, n, dtype=torch.float64, device=gshift.device) if ctx.needs_input_grad[3 + p] else None
              for p, n in enumerate(counts)]
        _call("exo_ttv_tables_vjp_f64", gshift.device, *_TtvTables._args(period, t0, ttvs, counts), D, P, n_edge, _ptr(gshift),
              _ptr_array(gt, P), _ptr(gper), _stream(gshift))
        if gper is not None:
            gper = gper.sum_to_size(period.shape)
        gt = [None if g is None else g.sum_to_size(x.shape) for g, x in zip(gt, ttvs)]
        return (gper, None, None, *gt)


def ttv_tables(period, t0, ttvs, n_draw):
    """Timing tables ``(edges (D, P, E), shift (D, P, E + 1))`` of a TTVOrbit whose transits are all labelled and given as
    offsets from the linear ephemeris: ``period``, ``t0`` (1 | D, P), ``ttvs`` a list of (1 | D, n_p) tensors.  One
    launch each way (exo_ttv_tables_f64); differentiable in ``ttvs`` and ``period``."""
    return _TtvTables.apply(period, t0, int(n_draw), *ttvs)


# ------------------------------------------------------------------------------
# radial velocity
# ------------------------------------------------------------------------------
RV_NPAR = 6
OV_NPAR = 10          # include/exoplanet_amd.h EXO_OV_*
OV_VELOCITY = 1
OV_ACCELERATION = 2
RV_N, RV_TP, RV_ECC, RV_COSW, RV_SINW, RV_AMP = range(6)


class _RadialVelocity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, params):
        t = _dev(t, "t")
        params = _dev(params, "params")
        if t.dim() != 1:
            raise ValueError("t must be 1-D (n_cad,)")
        if params.dim() != 3 or params.shape[-1] != RV_NPAR:
            raise ValueError(f"params must be (n_draw, n_planet, {RV_NPAR})")
        D, P, _ = params.shape
        rv = torch.empty(D, t.numel(), P, dtype=torch.float64, device=t.device)
        _call("exo_radial_velocity_fwd_f64", t.device, _ptr(t), t.numel(), _ptr(params), D, P, _ptr(rv), _stream(t))
        ctx.save_for_backward(t, params)
        return rv

    @staticmethod
    def backward(ctx, grv):
        t, params = ctx.saved_tensors
        D, P, _ = params.shape
        grv = _dev(grv, "grv")
        gparams = torch.empty_like(params)
        _call("exo_radial_velocity_vjp_f64", t.device, _ptr(t), t.numel(), _ptr(params), D, P, _ptr(grv), _ptr(gparams),
              _stream(t))
        return None, gparams


class _OrbitVector(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, params, flags):
        t = _dev(t, "t")
        params = _dev(params, "params")
        if t.dim() != 1:
            raise ValueError("t must be 1-D (n_cad,)")
        if params.dim() != 3 or params.shape[-1] != OV_NPAR:
            raise ValueError(f"params must be (n_draw, n_planet, {OV_NPAR})")
        D, P, _ = params.shape
        out = torch.empty(D, t.numel(), P, 3, dtype=torch.float64, device=t.device)
        _call("exo_orbit_vector_fwd_f64", t.device, _ptr(t), t.numel(), _ptr(params), D, P, flags, _ptr(out), _stream(t))
        ctx.save_for_backward(t, params)
        ctx.flags = flags
        return out

    @staticmethod
    def backward(ctx, gout):
        t, params = ctx.saved_tensors
        D, P, _ = params.shape
        gout = _dev(gout, "gout")
        gparams = torch.empty_like(params)
        _call("exo_orbit_vector_vjp_f64", t.device, _ptr(t), t.numel(), _ptr(params), D, P, ctx.flags, _ptr(gout),
              _ptr(gparams), _stream(t))
        return None, gparams, None


def orbit_vector(t, params, velocity=False, acceleration=False):
    """Position (or, ``velocity=True`` / ``acceleration=True``, velocity / acceleration) vectors in the observer frame for ``n_draw`` parameter sets, one
    fused launch each way: t (n_cad,), params (n_draw, n_planet, 10) with slots EXO_OV_* (n, t_periastron, ecc,
    cos / sin omega, cos / sin incl, amplitude, cos / sin Omega) -> (n_draw, n_cad, n_planet, 3) = (X, Y, Z).
    Differentiable with respect to ``params``.  (keplerian.py:380-409, :572-578, :283-322)"""
    return _OrbitVector.apply(t, params, OV_ACCELERATION if acceleration else (OV_VELOCITY if velocity else 0))


def radial_velocity(t, params):
    """Stellar reflex radial velocity, one column per planet: t (n_cad,), params
    (n_draw, n_planet, 6) = (n, t_periastron, ecc, cos omega, sin omega, amplitude)
    (include/exoplanet_amd.h EXO_RV_*) -> (n_draw, n_cad, n_planet); differentiable
    w.r.t. ``params``.  One launch each way (keplerian.py:633-677)."""
    return _RadialVelocity.apply(t.detach(), params)


# ------------------------------------------------------------------------------
# radial-velocity likelihood: value and every gradient from one launch
# ------------------------------------------------------------------------------
RV_MAX_TREND = 4      # include/exoplanet_amd.h EXO_RV_MAX_TREND
RV_MAX_INST = 8       # EXO_RV_MAX_INST


class _DrawLoglike(torch.autograd.Function):
    """A likelihood whose value (n_draw,) and every gradient come from ONE library call: the forward pass makes the call and
    keeps the gradients that will be asked for, the reverse pass scales each by the incoming cotangent.  ``entry``: the
    library entry; ``args(ll, grads)``: its arguments up to the stream, ``grads`` holding a tensor or None per pair of
    ``wanted`` -- (index into ``inputs``, shape of that input's gradient), first dimension the draws; ``inputs``: the time
    array, then what is differentiated (None: absent)."""

    @staticmethod
    def forward(ctx, entry, args, wanted, n_draw, *inputs):
        t = inputs[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=t.device)  # noqa: E731
        ll = new(n_draw)
        grads = [new(*shape) if inputs[i] is not None and ctx.needs_input_grad[4 + i] else None for i, shape in wanted]
        _call(entry, t.device, *args(ll, grads), _stream(t))
        ctx.slots = [4 + i for (i, _), g in zip(wanted, grads) if g is not None]
        ctx.n_in = 4 + len(inputs)
        ctx.save_for_backward(*[g for g in grads if g is not None])
        return ll

    @staticmethod
    def backward(ctx, gll):
        gll = gll.contiguous()
        out = [None] * ctx.n_in
        for slot, g in zip(ctx.slots, ctx.saved_tensors):
            out[slot] = gll.reshape((-1,) + (1,) * (g.dim() - 1)) * g
        return tuple(out)


def _rv_data(t, rv_err, t_ref, instrument):
    """the per-series arrays of exo_rv_loglike_vjp_f64 -- (tau = t - t_ref, var = rv_err^2 as (1,) or (n_cad,), int32
    instruments | None, their largest index | None if unchecked) -- made once per series (the indices are checked on the
    host, a device synchronisation; inside a capture nothing is checked: the kernel answers an index outside its tables
    with NaN)"""
    def make():
        tau = t - float(t_ref)
        if isinstance(rv_err, torch.Tensor):
            err = _dev(rv_err.detach(), "rv_err").reshape(-1)
            if err.numel() not in (1, t.numel()):
                raise ValueError("rv_err must be a number or one value per epoch")
            var = err * err
        else:
            var = _const(float(rv_err) ** 2, t.device)
        inst, hi = None, None
        if instrument is not None:
            if instrument.is_floating_point() or tuple(instrument.shape) != (t.numel(),):
                raise ValueError("instrument must be an integer tensor with one entry per epoch")
            inst = instrument.to(device=t.device, dtype=torch.int32).contiguous()
            if not _RV_SERIES.capturing() and inst.numel():
                lo, hi = int(inst.min()), int(inst.max())
                if lo < 0 or hi >= RV_MAX_INST:
                    raise ValueError(f"instrument indices must lie in [0, {RV_MAX_INST}): got {lo} .. {hi}")
        return tau, var, inst, hi

    return _RV_SERIES.get((t, rv_err, t_ref, instrument), make).value


def rv_loglike(t, params, rv, rv_err, trend=None, t_ref=0.0, offset=None, jitter=None, instrument=None):
    """Gaussian log-likelihood (n_draw,) of the observed radial velocities ``rv`` (n_cad,) with independent errors ``rv_err``
    (a number or one value per epoch) for ``n_draw`` parameter sets, value and every gradient in ONE launch
    (exo_rv_loglike_vjp_f64) -- the reference tutorials' ``pm.Normal("obs", mu=zero_point + trend +
    orbit.get_radial_velocity(t, K=K), sigma=sqrt(rv_err**2 + exp(2 * log_jitter)), observed=rv)``:

        model = sum over planets of radial_velocity(t, params) + sum_k trend[:, k] (t - t_ref)**k + offset[:, instrument]
        sigma**2 = rv_err**2 + jitter[:, instrument]**2

    ``params`` (n_draw, n_planet, 6) as for :func:`radial_velocity`; ``trend`` None or (n_draw, T), T <= 4, powers
    increasing; ``offset`` and ``jitter`` None, a number, one value per draw or (n_draw, n_inst), n_inst <= 8; ``instrument``
    None (one instrument) or an integer tensor (n_cad,) of indices into those columns.  Differentiable in ``params``,
    ``trend``, ``offset`` and ``jitter`` (which enters the kernel squared; the chain rule to it is torch's).  ``rv`` and
    ``rv_err`` are data: one that requires grad is refused, not silently dropped
    (KeplerianOrbit.rv_log_likelihood takes the composed route for those)."""
    t, params, rv = _dev(t, "t").detach(), _dev(params, "params"), _dev(rv, "rv")
    if t.dim() != 1 or tuple(rv.shape) != tuple(t.shape):
        raise ValueError("t and rv must be 1-D with one entry per epoch")
    if params.dim() != 3 or params.shape[-1] != RV_NPAR:
        raise ValueError(f"params must be (n_draw, n_planet, {RV_NPAR})")
    D, P, _ = params.shape
    if not 1 <= P <= MAX_PLANETS:
        raise ValueError(f"between 1 and {MAX_PLANETS} planets")
    what = "radial-velocity likelihood"
    _refuse_data_grad(what, "the orbit, the trend, the zero points and the jitter",
                      "KeplerianOrbit.rv_log_likelihood (it falls back to get_radial_velocity and torch)", rv=rv, rv_err=rv_err)
    tau, var, inst, hi = _rv_data(t, rv_err, t_ref, instrument)
    if trend is not None:
        trend = _dev(trend, "trend")
        if trend.dim() != 2 or trend.shape[0] not in (1, D) or trend.shape[1] > RV_MAX_TREND:
            raise ValueError(f"trend must be (n_draw, T) with T <= {RV_MAX_TREND}; got {tuple(trend.shape)} for {D} draws")
        trend = trend.expand(D, -1).contiguous() if trend.shape[1] else None
    offset = None if offset is None else _per_draw(_dev_or_number(offset, "offset"), "offset", D, t.device, what, columns=True)
    jitter = None if jitter is None else _per_draw(_dev_or_number(jitter, "jitter"), "jitter", D, t.device, what, columns=True)
    # one column everywhere: the instruments share every parameter, and which epoch is whose does not matter
    widths = {x.shape[1] for x in (offset, jitter) if x is not None and x.shape[1] > 1}
    n_inst = max(widths) if widths else 1
    if len(widths) > 1 or n_inst > RV_MAX_INST or (n_inst > 1 and (inst is None or (hi is not None and hi >= n_inst))):
        raise ValueError(f"offset / jitter with {sorted(widths)} columns need `instrument` with indices below that one number of "
                         f"columns (at most {RV_MAX_INST}); the indices go up to {hi}")
    if n_inst == 1:
        inst = None
    offset = None if offset is None else offset.expand(D, n_inst).contiguous()
    jit2 = None if jitter is None else (jitter * jitter).expand(D, n_inst).contiguous()
    rv, T = rv.detach(), 0 if trend is None else trend.shape[1]

    def args(ll, grads):
        return (_ptr(t), _ptr(tau), _ptr(inst), _ptr(rv), _ptr(var), t.numel(), var.numel(), _ptr(params), D, P, _ptr(trend), T,
                _ptr(offset), _ptr(jit2), n_inst, _ptr(ll), *map(_ptr, grads))

    wanted = [(1, (D, P, RV_NPAR)), (2, (D, T)), (3, (D, n_inst)), (4, (D, n_inst))]
    return _DrawLoglike.apply("exo_rv_loglike_vjp_f64", args, wanted, D, t, params, trend, offset, jit2)


# ------------------------------------------------------------------------------
# astrometric likelihood (separation and position angle): value and every gradient from one launch
# ------------------------------------------------------------------------------
def _astrometry_data(theta, rho_err, theta_err):
    """the per-series arrays of exo_astrometry_loglike_vjp_f64 -- (cos theta, sin theta, var_rho, var_theta), the variances
    as (1,) or (n_cad,) -- made once per series"""
    def variance(err, name):
        if isinstance(err, torch.Tensor):
            err = _dev(err.detach(), name).reshape(-1)
            if err.numel() not in (1, theta.numel()):
                raise ValueError(f"{name} must be a number or one value per epoch")
            return err * err
        return _const(float(err) ** 2, theta.device)

    def make():
        return torch.cos(theta), torch.sin(theta), variance(rho_err, "rho_err"), variance(theta_err, "theta_err")

    return _AST_SERIES.get((theta, rho_err, theta_err), make).value


def astrometry_loglike(t, params, rho, rho_err, theta, theta_err, rho_jitter=None, theta_jitter=None):
    """Gaussian log-likelihood (n_draw,) of the observed separations ``rho`` and position angles ``theta`` (n_cad,) of ONE
    companion, with independent errors ``rho_err`` / ``theta_err`` (each a number or one value per epoch), for ``n_draw``
    parameter sets, value and every gradient in ONE launch (exo_astrometry_loglike_vjp_f64) -- the reference tutorial's

        rho_model, theta_model = orbit.get_relative_angles(t, parallax)
        pm.Normal("rho_obs", mu=rho_model, sd=sqrt(rho_err**2 + rho_jitter**2), observed=rho)
        theta_diff = arctan2(sin(theta_model - theta), cos(theta_model - theta))
        pm.Normal("theta_obs", mu=theta_diff, sd=sqrt(theta_err**2 + theta_jitter**2), observed=0)

    ``params`` (n_draw, 10) with slots EXO_OV_* as for :func:`orbit_vector` (amplitude -a, times parallax au_per_R_sun for
    arcseconds).  ``theta`` in any 2 pi convention: the kernel sees its cosine and sine, formed once per series.  Each
    jitter None, a number or one value per draw.  Differentiable in ``params`` and the jitters (which enter the kernel
    squared; the chain rule to them is torch's).  ``rho``, ``theta`` and the error bars are data: one that requires grad is
    refused, not silently dropped (KeplerianOrbit.astrometry_log_likelihood takes the composed route for those)."""
    t, params, rho, theta = _dev(t, "t").detach(), _dev(params, "params"), _dev(rho, "rho"), _dev(theta, "theta")
    if t.dim() != 1 or tuple(rho.shape) != tuple(t.shape) or tuple(theta.shape) != tuple(t.shape):
        raise ValueError("t, rho and theta must be 1-D with one entry per epoch")
    if params.dim() != 2 or params.shape[-1] != OV_NPAR:
        raise ValueError(f"params must be (n_draw, {OV_NPAR}): one companion per call")
    D = params.shape[0]
    what = "astrometric likelihood"
    _refuse_data_grad(what, "the orbit and the jitters",
                      "KeplerianOrbit.astrometry_log_likelihood (it falls back to get_relative_angles and torch)",
                      rho=rho, theta=theta, rho_err=rho_err, theta_err=theta_err)
    cos_theta, sin_theta, var_rho, var_theta = _astrometry_data(theta.detach(), rho_err, theta_err)
    jit2 = []
    for name, x in (("rho_jitter", rho_jitter), ("theta_jitter", theta_jitter)):
        x = None if x is None else _per_draw(_dev_or_number(x, name), name, D, t.device, what)
        jit2.append(None if x is None else (x * x).expand(D).contiguous())
    rho = rho.detach()

    def args(ll, grads):
        return (_ptr(t), _ptr(rho), _ptr(cos_theta), _ptr(sin_theta), _ptr(var_rho), var_rho.numel(), _ptr(var_theta),
                var_theta.numel(), t.numel(), _ptr(params), D, _ptr(jit2[0]), _ptr(jit2[1]), _ptr(ll), *map(_ptr, grads))

    wanted = [(1, (D, OV_NPAR)), (2, (D,)), (3, (D,))]
    return _DrawLoglike.apply("exo_astrometry_loglike_vjp_f64", args, wanted, D, t, params, jit2[0], jit2[1])


# ------------------------------------------------------------------------------
# record packing: KeplerianOrbit.__init__ algebra + get_cl + windows as one kernel
# ------------------------------------------------------------------------------
class _PackRecords(torch.autograd.Function):
    @staticmethod
    def forward(ctx, orbit_in, ld_in, flags):
        orbit_in = _dev(orbit_in, "orbit_in")
        ld_in = _dev(ld_in, "ld_in")
        if orbit_in.dim() != 3 or orbit_in.shape[-1] != NIN:
            raise ValueError(f"orbit_in must be (n_draw, n_planet, {NIN})")
        D, P, _ = orbit_in.shape
        nset = 2 if flags & FLAG_SECONDARY else 1
        if ld_in.shape != (D, 2 * nset):
            raise ValueError(f"ld_in must be (n_draw, {2 * nset})")
        params = torch.empty(D, P, NPAR, dtype=torch.float64, device=orbit_in.device)
        ld = torch.empty(D, 3 * nset, dtype=torch.float64, device=orbit_in.device)
        _call("exo_pack_records_f64", orbit_in.device, _ptr(orbit_in), _ptr(ld_in), D, P, flags, _ptr(params), _ptr(ld),
              _stream(orbit_in))
        ctx.save_for_backward(orbit_in, ld_in)
        ctx.flags = flags
        return params, ld

    @staticmethod
    def backward(ctx, gparams, gld):
        orbit_in, ld_in = ctx.saved_tensors
        D, P, _ = orbit_in.shape
        gparams = _dev(gparams, "gparams")
        gld = _dev(gld, "gld")
        go = torch.empty_like(orbit_in)
        gl = torch.empty_like(ld_in)
        _call("exo_pack_records_vjp_f64", orbit_in.device, _ptr(orbit_in), _ptr(ld_in), D, P, ctx.flags, _ptr(gparams),
              _ptr(gld), _ptr(go), _ptr(gl), _stream(orbit_in))
        return go, gl, None


SHO_SIGMA, SHO_RHO, SHO_TAU = 1, 2, 4   # include/exoplanet_amd.h EXO_SHO_*


class _ShoCoefficients(torch.autograd.Function):
    @staticmethod
    def forward(ctx, amp, freq, damp, flags, eps):
        amp, freq, damp = (_dev(x, "SHO parameter").contiguous() for x in (amp, freq, damp))
        if not (amp.shape == freq.shape == damp.shape) or amp.dim() != 1:
            raise ValueError("amp, freq, damp must be 1-D tensors of one length")
        n = amp.numel()
        coef = torch.empty(n, 4, dtype=torch.float64, device=amp.device)
        kind = torch.empty(n, dtype=torch.int32, device=amp.device)
        _call("exo_sho_coefficients_f64", amp.device, _ptr(amp), _ptr(freq), _ptr(damp), flags, eps, n, _ptr(coef), _ptr(kind),
              _stream(amp))
        ctx.save_for_backward(amp, freq, damp)
        ctx.flags, ctx.eps = flags, eps
        ctx.mark_non_differentiable(kind)
        ctx.set_materialize_grads(False)      # (no zero-filled int32 "gradient" of `kind` per backward call: a launch each)
        return coef, kind

    @staticmethod
    def backward(ctx, gcoef, _gkind):
        amp, freq, damp = ctx.saved_tensors
        n = amp.numel()
        if gcoef is None:
            return None, None, None, None, None
        gcoef = _dev(gcoef, "gcoef").contiguous()
        ga, gf, gd = (torch.empty_like(amp) for _ in range(3))
        _call("exo_sho_coefficients_vjp_f64", amp.device, _ptr(amp), _ptr(freq), _ptr(damp), ctx.flags, ctx.eps, n,
              _ptr(gcoef), _ptr(ga), _ptr(gf), _ptr(gd), _stream(amp))
        return ga, gf, gd, None, None


def sho_coefficients(amp, freq, damp, flags=0, eps=1e-5):
    """celerite2's SHOTerm in any of its parameterisations (``flags``: SHO_SIGMA | SHO_RHO | SHO_TAU say that ``amp``
    is sigma rather than S0, ``freq`` the undamped period rho rather than w0, ``damp`` tau rather than Q) -> the
    term's pair slot ``coef`` (n, 4) and ``kind`` (n,) int32 (1: two real terms, Q < 1/2), one fused launch each way."""
    return _ShoCoefficients.apply(amp, freq, damp, int(flags), float(eps))


SHO_MAX_TERMS = 8


class _ShoCoefficientsMulti(torch.autograd.Function):
    """several SHO terms in one launch each way (include/exoplanet_amd.h, exo_sho_coefficients_multi_f64): inputs
    (flags tuple, eps, amp_0, freq_0, damp_0, amp_1, ...) -> coef (n, T, 4), kind (n, T)"""

    @staticmethod
    def forward(ctx, flags, eps, *cols):
        T = len(flags)
        cols = [_dev(x, "SHO parameter").contiguous() for x in cols]
        n = cols[0].numel()
        if len(cols) != 3 * T or not 1 <= T <= SHO_MAX_TERMS or any(c.dim() != 1 or c.numel() != n for c in cols):
            raise ValueError("three 1-D tensors of one length per term, at most %d terms" % SHO_MAX_TERMS)
        coef = torch.empty(n, T, 4, dtype=torch.float64, device=cols[0].device)
        kind = torch.empty(n, T, dtype=torch.int32, device=cols[0].device)
        arr = lambda q: _ptr_array(cols[q::3], T)  # noqa: E731
        fl = (ctypes.c_uint32 * T)(*[int(f) for f in flags])
        _call("exo_sho_coefficients_multi_f64", coef.device, arr(0), arr(1), arr(2), fl, T, eps, n, _ptr(coef), _ptr(kind),
              _stream(coef))
        ctx.save_for_backward(*cols)
        ctx.flags, ctx.eps = tuple(int(f) for f in flags), eps
        ctx.mark_non_differentiable(kind)
        ctx.set_materialize_grads(False)
        return coef, kind

    @staticmethod
    def backward(ctx, gcoef, _gkind):
        cols = ctx.saved_tensors
        T = len(ctx.flags)
        if gcoef is None:
            return (None,) * (2 + 3 * T)
        n = cols[0].numel()
        gcoef = _dev(gcoef, "gcoef").contiguous()
        grads = [torch.empty_like(c) for c in cols]
        arr = lambda xs, q: _ptr_array(xs[q::3], T)  # noqa: E731
        fl = (ctypes.c_uint32 * T)(*ctx.flags)
        _call("exo_sho_coefficients_multi_vjp_f64", gcoef.device, arr(cols, 0), arr(cols, 1), arr(cols, 2), fl, T, ctx.eps, n,
              _ptr(gcoef), arr(grads, 0), arr(grads, 1), arr(grads, 2), _stream(gcoef))
        return (None, None) + tuple(grads)


def sho_coefficients_multi(terms, eps=1e-5):
    """``terms``: [(amp, freq, damp, flags), ...] of one length n each -> coef (n, T, 4), kind (n, T) int32: a sum of SHO terms
    in one launch each way (and no concatenation of the terms' slots)"""
    flat = [x for amp, freq, damp, _ in terms for x in (amp, freq, damp)]
    return _ShoCoefficientsMulti.apply(tuple(int(f) for *_, f in terms), float(eps), *flat)


class PriorTable:
    """the block table of a ParameterSpace as the kernels take it (include/exoplanet_amd.h, exo_prior_block): ``rows`` --
    dicts of kind, offset, count, link, out, flags, p; ``n_free`` columns of z; ``out_cols``: the columns of every output array"""

    def __init__(self, rows, n_free, out_cols):
        self.n_block, self.n_free, self.out_cols = len(rows), int(n_free), [int(c) for c in out_cols]
        self.blocks = (_lib.PriorBlock * max(self.n_block, 1))()
        for b, row in zip(self.blocks, rows):
            b.kind, b.offset, b.count, b.link, b.out, b.flags = (int(row[k]) for k in ("kind", "offset", "count", "link", "out", "flags"))
            for i, v in enumerate(row["p"]):
                b.p[i] = float(v)


class _PriorTransform(torch.autograd.Function):
    """exo_prior_transform_f64 / _vjp_f64: (table, z) -> (log prior (D,), one (D, columns) array per output); the reverse
    recomputes from z and takes missing cotangents as null pointers"""

    @staticmethod
    def forward(ctx, table, z):
        z = _dev(z, "z")
        if z.dim() != 2 or z.shape[1] != table.n_free:
            raise ValueError(f"z must have shape (n_chain, {table.n_free})")
        D = z.shape[0]
        outs = [torch.empty(D, c, dtype=torch.float64, device=z.device) for c in table.out_cols]
        log_prior = torch.empty(D, dtype=torch.float64, device=z.device)
        _call("exo_prior_transform_f64", z.device, _ptr(z), D, table.n_free, table.blocks, table.n_block,
              _ptr_array(outs, len(outs)), _ptr(log_prior), _stream(z))
        ctx.save_for_backward(z)
        ctx.table = table
        ctx.set_materialize_grads(False)
        return (log_prior, *outs)

    @staticmethod
    def backward(ctx, glp, *gouts):
        (z,) = ctx.saved_tensors
        table = ctx.table
        if glp is None and all(g is None for g in gouts):
            return None, None
        glp, *gouts = (None if g is None else _dev(g, "cotangent") for g in (glp, *gouts))
        gz = torch.empty_like(z)
        _call("exo_prior_transform_vjp_f64", z.device, _ptr(z), z.shape[0], table.n_free, table.blocks, table.n_block,
              _ptr_array(gouts, len(gouts)), _ptr(glp), _ptr(gz), _stream(z))
        return None, gz


def prior_transform(z, table):
    """``z`` (D, n_free) on the device, ``table``: a PriorTable -> (log prior (D,), the constrained parameters, one (D, columns)
    tensor each): one launch each way (exoplanet_amd.distributions.ParameterSpace.constrain)"""
    return _PriorTransform.apply(table, z)


_PACK_DEFAULTS = (float("nan"), 0.0, 0.0, 0.0, 0.0, float("nan"), 1.0, 1.0, 0.0, 0.0)   # EXO_IN_* order; period, r: required


def _cols_vjp(t, texp, stencil_dt, stencil_w, host, D, P, nset, flags, pack_flags, gflux, events=(None, None), fold=None):
    """exo_transit_flux_cols_vjp_f64: the constructor's columns (``host`` = the six host arrays of _cols_host) -> records, the
    value + VJP sweep and, ``fold = (gscale | None, gcols, gld_cols)`` (host arrays of output pointers), the packing VJP in
    the same call.  Returns (flux | SparseFlux, gparams, gld, dot)."""
    t = _dev(t, "t")
    N, dev = t.numel(), t.device
    if t.dim() != 1:
        raise ValueError("t must be 1-D (n_cad,)")
    texp, n_texp, sdt, sw, n_sub = _exposure_args(t, texp, stencil_dt, stencil_w)
    if not 1 <= P <= MAX_PLANETS:
        raise ValueError(f"1 <= n_planet <= {MAX_PLANETS}")
    flags = int(flags) | _sorted_flag(t)
    shape = _flux_shape(N, D, P, flags)
    if isinstance(gflux, torch.Tensor) and tuple(gflux.shape) != shape:
        raise ValueError(f"gflux must have shape {shape}")
    gflux, flags = _cotangent_layout(gflux, flags, n_texp <= 1 and not flags & (FLAG_EXACT_SCAN | FLAG_PER_PLANET), True)
    ws, nbytes = _workspace(N, D, P, dev)
    params = torch.empty(D, P, NPAR, dtype=torch.float64, device=dev)
    ld = torch.empty(D, 3 * nset, dtype=torch.float64, device=dev)
    gparams, gld = torch.empty_like(params), torch.empty_like(ld)
    dot = torch.empty(D, dtype=torch.float64, device=dev)
    flux = None if flags & FLAG_SPARSE else _flux_out(N, D, P, flags, dev)
    gscale, gcp, glp = (None, None, None) if fold is None else fold
    _call("exo_transit_flux_cols_vjp_f64", dev, *host, int(pack_flags), _ptr(t), N, _ptr(texp), n_texp, _ptr(sdt), _ptr(sw),
          n_sub, D, P, flags, _ptr(gflux), _ptr(flux), _ptr(params), _ptr(ld), _ptr(gparams), _ptr(gld), _ptr(dot),
          0 if fold is None else 1, _ptr(gscale), gcp, glp, _ptr(ws), nbytes, _stream(t), events[0], events[1])
    if flags & FLAG_SPARSE:
        flux = _sparse_from_ws(ws, N, D, P, flags)
    return flux, gparams, gld, dot


def _cols_batch(ocols, lcols, n_draw=None):
    """(D, P) of a set of columns: what their shapes imply, or -- ``n_draw`` -- the caller's D and the planets of the orbit
    columns"""
    D, P = (1, 1) if n_draw is None else (int(n_draw), 1)
    for c in ocols:
        if c is not None:
            if c.dim() > 2:
                raise ValueError("orbit parameters may carry at most one draw dimension here")
            P = max(P, c.shape[-1] if c.dim() >= 1 else 1)
            if n_draw is None:
                D = max(D, c.shape[0] if c.dim() == 2 else 1)
    if n_draw is None:
        for c in lcols:
            if c.dim() > 1:
                raise ValueError("limb-darkening coefficients may carry at most one draw dimension")
            D = max(D, c.shape[0] if c.dim() == 1 else 1)
    return D, P


def _cols_host(ocols, lcols, D, P):
    """the host arrays exo_pack_records_cols_f64 / exo_transit_flux_cols_vjp_f64 take for a list of NIN orbit columns (None = the
    constructor's default) and the limb-darkening columns, + the expanded views (kept alive by the caller)"""
    keep = []
    for c in ocols:
        if c is None:
            continue
        c = _dev(c.detach(), "orbit parameter")
        v = c.reshape(1, 1) if c.dim() == 0 else (c.unsqueeze(0) if c.dim() == 1 else c)
        keep.append(v.expand(D, P))
    for c in lcols:
        c = _dev(c.detach(), "limb-darkening coefficient")
        keep.append((c.reshape(1) if c.dim() == 0 else c).expand(D))
    return _cols_host_saved(keep, [c is not None for c in ocols], len(lcols)), keep


def _cols_host_saved(keep, present, n_ld):
    """the six host arrays from the expanded views of _cols_host (``present[k]``: orbit column k was given): also what the
    reverse pass rebuilds them with"""
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    cp, ds, ps, df = (vp * NIN)(), (i64 * NIN)(), (i64 * NIN)(), (ctypes.c_double * NIN)(*_PACK_DEFAULTS)
    lp, ls = (vp * 4)(), (i64 * 4)()
    it = iter(keep)
    for k in range(NIN):
        if present[k]:
            v = next(it)
            cp[k], ds[k], ps[k] = v.data_ptr(), v.stride(0), v.stride(1)
    for k in range(n_ld):
        v = next(it)
        lp[k], ls[k] = v.data_ptr(), v.stride(0)
    return cp, ds, ps, df, lp, ls


def _cols_meta(D, P, pack_flags, n_ld, cols):
    """what the reverse pass of a column-form packing needs besides the views: the batch, which orbit columns were given,
    every column's own shape"""
    return D, P, pack_flags, n_ld, [c is not None for c in cols[:NIN]], [None if c is None else tuple(c.shape) for c in cols]


def _to_col_shape(g, shape):
    """a dense (D, P) / (D,) cotangent back to the shape the caller passed (sums over what was broadcast)"""
    if g is None:
        return None
    return g.reshape(shape) if g.numel() == _numel(shape) else g.sum_to_size(_bshape(shape, g.dim())).reshape(shape)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _bshape(shape, ndim):
    """`shape` left-padded with ones to `ndim` dimensions (what sum_to_size reduces to)"""
    return (1,) * (ndim - len(shape)) + tuple(shape)


@torch.no_grad()
def orbit_flux_value_and_grad(t, gflux, orbit_cols, ld_cols, flags=0, pack_flags=0, texp=None, stencil_dt=None, stencil_w=None,
                              gscale=None, events=(None, None), wanted=None):
    """Value AND gradient of ``L[d] = sum_n gflux[d, n] flux[d, n]`` for orbits in the standard parameterisation given column
    by column (as :func:`orbit_flux_dot`), WITHOUT autograd: returns ``(flux, L, gcols, gld_cols)`` -- ``gcols[k]`` the
    gradient of ``sum_d gscale[d] L[d]`` (``gscale`` None: of ``sum_d L[d]``) with respect to orbit column k in that
    column's own shape (None where the column was None), ``gld_cols`` likewise for (u1, u2[, u1s, u2s]).  What a sampler's
    leapfrog step needs, in ONE call of the library (exo_transit_flux_cols_vjp_f64): the packing rides on the windows +
    enumeration launch, then the sweep, then the packing VJP -- three launches at >= 512 draws, no autograd graph.
    ``wanted``: one bool per orbit column -- False: no gradient for it (None in ``gcols``)."""
    ocols, lcols = list(orbit_cols), list(ld_cols)
    if len(ocols) != NIN or len(lcols) not in (2, 4):
        raise ValueError(f"{NIN} orbit columns (None = default) and 2 or 4 limb-darkening columns")
    D, P = _cols_batch(ocols, lcols)
    host, keep = _cols_host(ocols, lcols, D, P)
    dev = keep[0].device
    wanted = [True] * NIN if wanted is None else list(wanted)
    outs = [None if (c is None or not w) else torch.empty(D, P, dtype=torch.float64, device=dev) for c, w in zip(ocols, wanted)]
    louts = [torch.empty(D, dtype=torch.float64, device=dev) for _ in lcols]
    if gscale is not None:
        gscale = _dev(gscale, "gscale")
        if tuple(gscale.shape) != (D,):
            raise ValueError("gscale: one factor per draw")
    flux, _, _, dot = _cols_vjp(t, texp, stencil_dt, stencil_w, host, D, P, len(lcols) // 2, flags, pack_flags, gflux, events,
                                fold=(gscale, _ptr_array(outs, NIN), _ptr_array(louts, 4)))
    return (flux, dot, [None if g is None else _to_col_shape(g, tuple(c.shape)) for g, c in zip(outs, ocols)],
            [_to_col_shape(g, tuple(c.shape)) for g, c in zip(louts, lcols)])


class _OrbitFluxDot(torch.autograd.Function):
    """Record packing (column form: every constructor argument its own tensor), the one-sweep value + VJP light
    curve, and -- backward -- the packing VJP with the cotangent of L folded in (``gscale``): the whole
    user-level step of a standard-parameterisation orbit is the sweep plus TWO small kernels, where the
    composition pack_records -> transit_flux_dot costs seven (two concatenations, the pack, two scalings of
    the saved cotangents, the pack VJP, and whatever produced the cotangent of L)."""

    @staticmethod
    def forward(ctx, t, gflux, texp, stencil_dt, stencil_w, flags, pack_flags, events, n_ld, *cols):
        t = _dev(t, "t")
        ocols, lcols = list(cols[:NIN]), list(cols[NIN:NIN + n_ld])
        D, P = _cols_batch(ocols, lcols)
        host, keep = _cols_host(ocols, lcols, D, P)
        # (packing, windows + enumeration in ONE launch, then the sweep: exo_transit_flux_cols_vjp_f64; the packing VJP stays in
        # backward() -- the cotangent of L is not known before)
        flux, gparams, gld, dot = _cols_vjp(t, texp, stencil_dt, stencil_w, host, D, P, n_ld // 2, flags, pack_flags, gflux,
                                            events)
        ctx.save_for_backward(gparams, gld, *keep)
        ctx.meta = _cols_meta(D, P, pack_flags, n_ld, cols)
        ctx.set_materialize_grads(False)
        if isinstance(flux, SparseFlux):
            shape = torch.tensor([D, P], dtype=torch.int64)      # (host tensor: the wrapper needs the batch the columns implied)
            ctx.mark_non_differentiable(flux._ws, shape)
            return flux._ws, dot, shape
        ctx.mark_non_differentiable(flux)
        return flux, dot

    @staticmethod
    def backward(ctx, _gflux_unused, gdot, *_shape_unused):
        nfix = 9
        if gdot is None:
            return (None,) * (nfix + len(ctx.meta[5]))
        gparams, gld, *keep = ctx.saved_tensors
        return (None,) * nfix + tuple(_pack_cols_backward(keep, ctx.meta, gparams, gld, _dev(gdot, "gdot"),
                                                          ctx.needs_input_grad[nfix:]))


def orbit_flux_dot(t, gflux, orbit_cols, ld_cols, flags=0, pack_flags=0, texp=None, stencil_dt=None, stencil_w=None,
                   events=(None, None)):
    """``transit_flux_dot(t, *pack_records(stack(orbit_cols), stack(ld_cols)), gflux)`` without the stacking, the
    intermediate autograd nodes and the separate scaling of the cotangents: ``orbit_cols`` are the EXO_IN_* inputs
    (period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr), each a tensor of shape (), (P,), (D, 1) or (D, P)
    -- or None for the constructor default -- and ``ld_cols`` are (u1, u2[, u1s, u2s]) of shape () or (D,).
    Returns ``(flux, L)`` like :func:`transit_flux_dot`; L is differentiable w.r.t. every column."""
    out = _OrbitFluxDot.apply(t, gflux, texp, stencil_dt, stencil_w, int(flags), int(pack_flags), events, len(ld_cols),
                              *orbit_cols, *ld_cols)
    if int(flags) & FLAG_SPARSE:
        D, P = (int(x) for x in out[2])
        return _sparse_from_ws(out[0], t.numel(), D, P, int(flags)), out[1]
    return out


def _pack_cols_forward(cols, n_ld, n_draw, pack_flags):
    """exo_pack_records_cols_f64 on a list of NIN orbit columns (None = constructor default) + n_ld limb-darkening
    columns: (params (D, P, 20), ld (D, 3|6), the expanded views to keep for the reverse call, meta)"""
    ocols, lcols = list(cols[:NIN]), list(cols[NIN:NIN + n_ld])
    ref = next(c for c in ocols + lcols if c is not None)
    D, P = _cols_batch(ocols, lcols, n_draw)
    host, keep = _cols_host(ocols, lcols, D, P)
    params = torch.empty(D, P, NPAR, dtype=torch.float64, device=ref.device)
    ld = torch.empty(D, 3 * (n_ld // 2), dtype=torch.float64, device=ref.device)
    _call("exo_pack_records_cols_f64", ref.device, *host, D, P, pack_flags, _ptr(params), _ptr(ld), _stream(params))
    return params, ld, keep, _cols_meta(D, P, pack_flags, n_ld, cols)


def _pack_cols_backward(keep, meta, gparams, gld, gscale, needs):
    """exo_pack_records_cols_vjp_f64: cotangents of (params, ld), optionally scaled per draw by ``gscale``, back to the
    columns' own shapes; ``needs[k]``: whether column k wants one"""
    D, P, pack_flags, n_ld, present, shapes = meta
    dev = keep[0].device
    host = _cols_host_saved(keep, present, n_ld)
    outs = [None] * len(shapes)
    for k in range(NIN):
        if present[k] and needs[k]:
            outs[k] = torch.empty(D, P, dtype=torch.float64, device=dev)
    for k in range(n_ld):
        if needs[NIN + k]:
            outs[NIN + k] = torch.empty(D, dtype=torch.float64, device=dev)
    _call("exo_pack_records_cols_vjp_f64", dev, *host, D, P, pack_flags, _ptr(gparams), _ptr(gld), _ptr(gscale),
          _ptr_array(outs[:NIN], NIN), _ptr_array(outs[NIN:NIN + n_ld], 4), _stream(gparams))
    return [_to_col_shape(g, shp) for g, shp in zip(outs, shapes)]


class _PackCols(torch.autograd.Function):
    """exo_pack_records_cols_f64 on its own: every constructor argument its own tensor (shape (), (P,), (D, 1) or
    (D, P); None = the constructor default), limb-darkening coefficients () or (D,) -> records (D, P, 20), ld (D, 3|6).
    No stacking pass forward, one packing-VJP launch in the reverse pass (the composition stack -> pack_records costs
    a concatenation each way plus a slice and a reduction per broadcast column)."""

    @staticmethod
    def forward(ctx, pack_flags, n_ld, n_draw, *cols):
        params, ld, keep, ctx.meta = _pack_cols_forward(cols, n_ld, n_draw, pack_flags)
        ctx.save_for_backward(*keep)
        return params, ld

    @staticmethod
    def backward(ctx, gparams, gld):
        D, P, _, n_ld = ctx.meta[:4]
        keep = ctx.saved_tensors
        dev = keep[0].device
        gparams = torch.zeros(D, P, NPAR, dtype=torch.float64, device=dev) if gparams is None else _dev(gparams, "gparams")
        gld = torch.zeros(D, 3 * (n_ld // 2), dtype=torch.float64, device=dev) if gld is None else _dev(gld, "gld")
        return (None,) * 3 + tuple(_pack_cols_backward(keep, ctx.meta, gparams, gld, None, ctx.needs_input_grad[3:]))


class _OrbitLoglike(torch.autograd.Function):
    """The white-noise log-likelihood of a batch of standard-parameterisation orbits straight from the constructor
    arguments: column-form packing, the one-call misfit + gradient (exo_transit_chi2[_ttv]_vjp_f64), and -- backward --
    the packing VJP with the likelihood's cotangent folded in (gscale = -gll / 2).  Seven launches for value and
    gradient where pack_records_cols -> transit_chi2 -> torch algebra takes eleven."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, obs, ivar, cterm, flags, pack_flags, n_ld, n_draw, ttv_edges, ttv_shift,
                *cols):
        params, ld, keep, meta = _pack_cols_forward(cols, n_ld, n_draw, pack_flags)
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        chi2, gparams, gld, gshift = _chi2_launch(a, flags, ttv_edges, ttv_shift, obs, ivar)
        ctx.meta = meta
        ctx.n_keep = len(keep)
        ctx.save_for_backward(gparams, gld, *keep, *([] if gshift is None else [gshift]))
        return torch.add(cterm, chi2, alpha=-0.5)

    @staticmethod
    def backward(ctx, gll):
        saved = ctx.saved_tensors
        gparams, gld, keep = saved[0], saved[1], saved[2:2 + ctx.n_keep]
        gscale = -0.5 * _dev(gll, "gll")
        nfix = 13
        grads = _pack_cols_backward(keep, ctx.meta, gparams, gld, gscale, ctx.needs_input_grad[nfix:])
        gshift = gscale[:, None, None] * saved[2 + ctx.n_keep] if len(saved) > 2 + ctx.n_keep else None
        return (None,) * 11 + (None, gshift) + tuple(grads)


class _OrbitNoiseLoglike(torch.autograd.Function):
    """:class:`_OrbitLoglike` with a per-draw mean and jitter: column-form packing, the sweep and the data terms of
    :class:`_TransitNoise`, and -- backward -- the packing VJP with the likelihood's cotangent folded in."""

    @staticmethod
    def forward(ctx, t, texp, stencil_dt, stencil_w, data, var, mean, jit2, flags, pack_flags, n_ld, n_draw, ttv_edges, ttv_shift,
                *cols):
        _refuse_data_grads(ctx, 5, ("yerr",))
        params, ld, keep, meta = _pack_cols_forward(cols, n_ld, n_draw, pack_flags)
        a = _transit_args(t, texp, stencil_dt, stencil_w, params, ld, flags)
        ll, dmean, djit2, gparams, gld, gshift = _noise_launch(a, flags, ttv_edges, ttv_shift, data, var, mean, jit2)
        ctx.meta = meta
        ctx.n_keep = len(keep)
        ctx.n_mean, ctx.n_jit = mean.numel(), 0 if jit2 is None else jit2.numel()
        ctx.save_for_backward(gparams, gld, dmean, djit2, *keep, *([] if gshift is None else [gshift]))
        return ll

    @staticmethod
    def backward(ctx, gll):
        saved = ctx.saved_tensors
        gparams, gld, dmean, djit2, keep = saved[0], saved[1], saved[2], saved[3], saved[4:4 + ctx.n_keep]
        gll = _dev(gll, "gll")
        gscale = -0.5 * gll
        nfix = 14
        grads = _pack_cols_backward(keep, ctx.meta, gparams, gld, gscale, ctx.needs_input_grad[nfix:])
        gshift = gscale[:, None, None] * saved[4 + ctx.n_keep] if len(saved) > 4 + ctx.n_keep else None
        gjit2 = _draw_cotangent(gll * djit2, ctx.n_jit) if ctx.n_jit else None
        return (None,) * 6 + (_draw_cotangent(gll * dmean, ctx.n_mean), gjit2) + (None,) * 5 + (gshift,) + tuple(grads)


def orbit_white_noise_loglike(t, y, yerr, orbit_cols, ld_cols, n_draw, mean=0.0, flags=0, pack_flags=0, texp=None,
                              stencil_dt=None, stencil_w=None, ttv=None, jitter=None):
    """:func:`white_noise_loglike` for orbits in the standard parameterisation given column by column (the EXO_IN_*
    inputs of :func:`pack_records_cols`): Gaussian log-likelihood (n_draw,), differentiable w.r.t. every column, the
    timing shifts, a per-draw ``mean`` and ``jitter``, value and gradient in seven launches (nine with the data terms of
    a sampled mean / jitter)."""
    t = _dev(t, "t")
    y = _dev(y, "y")
    if tuple(y.shape) != (t.numel(),):
        raise ValueError("y must have shape (n_cad,)")
    edges, shift = (None, None) if ttv is None else ttv
    if sampled_noise(mean, jitter):
        data, var, mean, jit2 = _noise_inputs(y, yerr, mean, jitter, int(n_draw))
        return _OrbitNoiseLoglike.apply(t, texp, stencil_dt, stencil_w, data, var, mean, jit2, int(flags), int(pack_flags),
                                        len(ld_cols), int(n_draw), edges, shift, *orbit_cols, *ld_cols)

    def run(obs, ivar, cterm):
        return _OrbitLoglike.apply(t, texp, stencil_dt, stencil_w, obs, ivar, cterm, int(flags), int(pack_flags),
                                   len(ld_cols), int(n_draw), edges, shift, *orbit_cols, *ld_cols)

    yd = per_draw_yerr(yerr, y.numel())
    if yd is not None:
        # (_OrbitLoglike returns cterm - chi2 / 2: with cterm = 0 the unit-weight misfit is -2 x that)
        zero = _const(0.0, t.device)
        return _scaled_loglike(lambda obs, one: -2.0 * run(obs, one, zero), y, _dev(yd, "yerr"), mean)
    _check_data_terms(y, yerr, mean)
    obs, ivar, _, _, cterm = _white_noise_terms(y, yerr, mean)
    if ivar.numel() not in (1, t.numel()):
        raise ValueError("yerr must be a number, one entry per cadence, or per draw: (n_draw, 1)")
    return run(obs, ivar, cterm)


def pack_records_cols(orbit_cols, ld_cols, n_draw, pack_flags=0):
    """:func:`pack_records` without the stacking: ``orbit_cols`` are the EXO_IN_* inputs (period, t0, b, ecc, omega, r,
    m_star, r_star, m_planet, sbr), each a tensor of shape (), (P,), (D, 1) or (D, P) -- or None for the constructor
    default -- and ``ld_cols`` (u1, u2[, u1s, u2s]) of shape () or (D,).  Returns records (D, P, 20) and ld (D, 3|6),
    differentiable w.r.t. every column (one launch each way)."""
    return _PackCols.apply(int(pack_flags), len(ld_cols), int(n_draw), *orbit_cols, *ld_cols)


def pack_records(orbit_in, ld_in, flags=0):
    """(period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr) per (draw, planet) and
    (u1, u2[, u1s, u2s]) per draw -> kernel records (n_draw, n_planet, 20) and Green's-basis
    limb-darkening coefficients (n_draw, 3|6): KeplerianOrbit.__init__ + get_cl + windows in
    one kernel, differentiable.  Slot order: include/exoplanet_amd.h EXO_IN_*."""
    return _PackRecords.apply(orbit_in, ld_in, int(flags))


# ---- chain diagnostics (exo_diag_*_f64; the quantities are stated in exoplanet_amd/diagnostics.py) ------------------------------
DIAG_LAG_BLOCK = 16   # include/exoplanet_amd.h EXO_DIAG_LAG_BLOCK
DIAG_SETS = 5         # EXO_DIAG_SETS
DIAG_MOMENTS = 8      # EXO_DIAG_MOMENTS
DIAG_OUT = 16         # EXO_DIAG_OUT
DIAG_COLUMNS = ("mean", "sd", "q05", "q50", "q95", "mcse_mean", "ess_bulk", "ess_tail", "ess_mean", "r_hat", "max_t_bulk",
                "max_t_low", "max_t_high", "max_t_mean", "r_hat_z", "r_hat_folded")


def diag_workspace_bytes(P, M, L):
    return _lib.load().exo_diag_workspace_bytes(P, M, L)


def chain_diagnostics(x_split, x_full, n_half, check_every=4, timings=None):
    """The split diagnostics of P parameters: ``x_split`` (P, L, n_half) -- the half-chains of every parameter, innermost --
    and ``x_full`` (P, n) with ALL draws of a parameter (None: no middle draw was dropped, the split values are all there
    are).  Returns (P, DIAG_OUT), columns DIAG_COLUMNS.  The sorts are torch's, everything else the library's; the host
    reads the device once per ``check_every`` lag blocks ("is every sequence truncated?").  ``timings``: a dict that receives
    device events around the stages (tools/time_diagnostics.py)."""
    x_split = _dev(x_split, "x_split")
    P, L, M = (int(v) for v in x_split.shape)
    if M != int(n_half) or M % 2 or L < 2:
        raise ValueError("x_split must be (P, L, n_half) with an even n_half and L >= 2")
    dev, S = x_split.device, L * M
    out = torch.empty((P, DIAG_OUT), dtype=torch.float64, device=dev)
    if P == 0 or M == 0:
        return out
    nbytes = diag_workspace_bytes(P, M, L)
    if nbytes < 0:
        raise ValueError("too many parameters for one call, or sizes that cannot be")
    stream = _stream(x_split)

    def mark(name):
        if timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            timings.setdefault("events", []).append((name, ev))

    mark("start")
    flat = x_split.reshape(P, S)
    sv, perm = torch.sort(flat, dim=1)
    if x_full is None:
        sf = sv
    else:
        sf = torch.sort(_dev(x_full, "x_full").reshape(P, -1), dim=1).values
    mark("sort")
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    sets = torch.empty((P, DIAG_SETS, S), dtype=torch.float64, device=dev)
    folded = torch.empty((P, S), dtype=torch.float64, device=dev)
    moments = torch.empty((P, DIAG_MOMENTS), dtype=torch.float64, device=dev)
    done = torch.zeros(P * DIAG_SETS, dtype=torch.int32, device=dev)
    _call("exo_diag_prepare_f64", dev, _ptr(flat), _ptr(sv), _ptr(sf), int(sf.shape[1]), P, M, L, _ptr(folded), _ptr(sets),
          _ptr(moments), stream)
    _call("exo_diag_rank_f64", dev, _ptr(sv), _ptr(perm), P, M, L, 0, _ptr(sets), stream)
    mark("prepare + rank")
    fsv, fperm = torch.sort(folded, dim=1)
    mark("sort (folded)")
    _call("exo_diag_rank_f64", dev, _ptr(fsv), _ptr(fperm), P, M, L, 1, _ptr(sets), stream)
    mark("rank (folded)")
    n_blocks = -(-L // DIAG_LAG_BLOCK)
    check_every = max(int(check_every), 1)
    used = 0
    for block in range(n_blocks):
        if block and block % check_every == 0 and bool(done.all()):
            break
        _call("exo_diag_autocov_f64", dev, _ptr(sets), P, M, L, block, _ptr(done), _ptr(ws), nbytes, stream)
        _call("exo_diag_finish_f64", dev, P, M, L, block, 0, 0, _ptr(done), _ptr(ws), nbytes, stream)
        used += 1
    mark("autocovariance blocks + finish")
    _call("exo_diag_finish_f64", dev, P, M, L, -1, _ptr(moments), _ptr(out), _ptr(done), _ptr(ws), nbytes, stream)
    mark("assemble")
    if timings is not None:
        timings["lag_blocks"] = used
    return out


# ---- quantiles along the strided axis (exo_column_quantiles_f64; the definition is stated in exoplanet_amd/predictive.py) ----------
QUANTILE_MAX_Q = 16   # include/exoplanet_amd.h EXO_QUANTILE_MAX_Q


def column_quantiles(values, num, den, return_count=False):
    """Per column of ``values`` (S, N) -- float64 on a ROCm device, last axis contiguous, any row stride >= N (no copy) -- the
    quantiles at the exact fractions ``num[q] / den[q]`` (whole numbers, 0 <= num <= den <= 1e9) of its values that are not
    NaN: (Q, N), and with ``return_count`` the int32 (N,) number of those values.  Selection by counting passes in the
    library: no sort, no copy of ``values``.  More than QUANTILE_MAX_Q fractions go in groups of that many."""
    if not isinstance(values, torch.Tensor) or values.dim() != 2:
        raise ValueError("values must be a tensor of shape (S, N)")
    if not values.is_cuda:
        _dev(values, "values")
    if values.dtype != torch.float64:
        raise TypeError("values must be float64")
    S, N = (int(v) for v in values.shape)
    num, den = [int(v) for v in num], [int(v) for v in den]
    if len(num) != len(den) or not num:
        raise ValueError("num and den must be two lists of one length, at least one fraction")
    if any(b < 1 or b > 10 ** 9 or a < 0 or a > b for a, b in zip(num, den)):
        raise ValueError("a fraction num / den needs 0 <= num <= den <= 1e9")
    if S >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    values = values.detach()
    if (N > 1 and values.stride(1) != 1) or (S > 1 and values.stride(0) < N):
        values = values.contiguous()
    stride = int(values.stride(0)) if S > 1 else N
    dev, Q = values.device, len(num)
    out = torch.empty((Q, N), dtype=torch.float64, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev) if return_count else None
    for lo in range(0, Q, QUANTILE_MAX_Q):
        n_q = min(QUANTILE_MAX_Q, Q - lo)
        a, b = (ctypes.c_int64 * n_q)(*num[lo:lo + n_q]), (ctypes.c_int64 * n_q)(*den[lo:lo + n_q])
        _call("exo_column_quantiles_f64", dev, _ptr(values), S, N, stride, ctypes.addressof(a), ctypes.addressof(b), n_q,
              _ptr(out[lo:lo + n_q]), _ptr(count) if lo == 0 else 0, _stream(values))
    return (out, count) if return_count else out


# ---- PSIS-LOO and WAIC per column (exo_column_psis_f64; the definition is stated in exoplanet_amd/comparison.py) --------------------
PSIS_MAX_TAIL = 1024   # include/exoplanet_amd.h EXO_PSIS_MAX_TAIL


def column_psis(values, n_tail_max):
    """Per column of ``values`` (S, N) -- pointwise log-likelihoods, float64 on a ROCm device, last axis contiguous, any row
    stride >= N (no copy) -- the PSIS leave-one-out density, the Pareto k, the lppd, the variance over the draws and the
    length of the fitted tail, with the tail's largest length ``n_tail_max`` = M (1 .. PSIS_MAX_TAIL): a dict of (N,) tensors
    "elpd", "k", "lppd", "var" (float64) and "n_tail" (int32).  One kernel of the library: no sort and no copy of ``values``."""
    if not isinstance(values, torch.Tensor) or values.dim() != 2:
        raise ValueError("values must be a tensor of shape (S, N)")
    if not values.is_cuda:
        _dev(values, "values")
    if values.dtype != torch.float64:
        raise TypeError("values must be float64")
    S, N = (int(v) for v in values.shape)
    n_tail_max = int(n_tail_max)
    if n_tail_max < 1 or n_tail_max > PSIS_MAX_TAIL:
        raise ValueError(f"n_tail_max must be in 1 .. {PSIS_MAX_TAIL}")
    if S >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    values = values.detach()
    if (N > 1 and values.stride(1) != 1) or (S > 1 and values.stride(0) < N):
        values = values.contiguous()
    stride = int(values.stride(0)) if S > 1 else N
    dev = values.device
    out = {k: torch.empty(N, dtype=torch.float64, device=dev) for k in ("elpd", "k", "lppd", "var")}
    out["n_tail"] = torch.empty(N, dtype=torch.int32, device=dev)
    _call("exo_column_psis_f64", dev, _ptr(values), S, N, stride, n_tail_max, _ptr(out["elpd"]), _ptr(out["k"]), _ptr(out["lppd"]),
          _ptr(out["var"]), _ptr(out["n_tail"]), _stream(values))
    return out
