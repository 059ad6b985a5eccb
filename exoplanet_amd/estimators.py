"""Period search and the other pre-fit estimators of the reference's ``exoplanet.estimators``: where ``period0`` and ``t00``
come from.  The periodograms are HIP kernels (csrc/exo_estimators.hip) and are computed exactly on an unthinned grid, for
many series on one time axis at once; the glue around them keeps the reference's names, arguments, defaults and dictionary
keys.  Definitions: DESIGN.md section 9, and section 18 for transit least squares -- the box search's twin with a
limb-darkened template in place of the box, whose ``depth`` is the mid-transit depth and therefore a starting ``r`` (not in
the reference).  Before the search comes the detrending (csrc/exo_detrend.hip): a time-windowed running
median, MAD or biweight location, divided out of the series, since real photometry is not flat (not in the reference either;
wotan's biweight and lightkurve's ``flatten`` are the CPU counterparts); with ``order=1`` or ``2`` a robust local line or
parabola in place of the location (csrc/exo_trend.hip).

After the search come the transits one by one (csrc/exo_timing.hip): the same template slid over a
grid of shifts of every single transit's mid-time, which gives the times a ``TTVOrbit`` starts from and the per-transit depths
behind the odd/even test (not in the reference).

For radial velocities the search is the Keplerian periodogram (csrc/exo_keplerian.hip): at every
frequency a grid of eccentricities and times of periastron, each candidate a linear fit with one constant per instrument,
which gives the ``ecc``, ``omega``, ``t_periastron``, ``K`` and zero points an RV model starts from (not in the reference).

Whether a peak of either periodogram is a detection is the question of :func:`false_alarm`: the highest
peak of shuffled or bootstrapped series, for the Keplerian periodogram through :func:`keplerian_max_power`, a kernel in which a
group of series shares every solve of Kepler's equation and only the arg-max leaves the device (not in the reference).

For relative astrometry it is the search on the Thiele-Innes constants (csrc/exo_astrometric.hip): the
same grid of candidates, each a linear fit of four constants to the sky-plane positions, which gives the seven elements
``astrometry_log_likelihood`` starts from (not in the reference).

Low level (device tensors in and out, float64): :func:`bls_power`, :func:`tls_power` (its templates:
:func:`transit_template`), :func:`lomb_scargle_power`, :func:`keplerian_power`, :func:`keplerian_max_power`,
:func:`false_alarm` (its pieces: :func:`resample_indices`, :func:`series_chi2_0`, :func:`false_alarm_probability`,
:func:`false_alarm_level`), :func:`astrometric_power`, :func:`running_location` (its windows:
:func:`location_plan`),
:func:`transit_times` (its windows: :func:`timing_plan`), and the
grids :func:`bls_autoperiod`, :func:`lomb_scargle_autofrequency` (host arithmetic).

High level (numpy arrays or tensors in, numpy out, ``peaks`` hold Python floats): :func:`flatten`, :func:`bls_estimator`,
:func:`tls_estimator`, :func:`ttv_estimator`, :func:`lomb_scargle_estimator`, :func:`keplerian_estimator`, :func:`astrometric_estimator`,
:func:`autocorr_estimator`, :func:`find_peaks`, :func:`sde`,
:func:`estimate_semi_amplitude`, :func:`estimate_minimum_mass`.  Plain numbers throughout: days, m/s and solar masses in, m/s and
Jupiter masses out.

Synchronisation: ``periods``, ``durations`` and ``frequencies`` given as numpy arrays (or lists) never leave the host -- the grid
sizes and the choice of kernel need them there -- and their device copies are cached, so that a call repeated with the same grid
enqueues kernels only and can be captured into a graph after one eager call.  Given as device tensors they are copied to the
host once per call, which waits for the stream; that is the only synchronisation in the periodograms.  The detrending has one
of its own: :func:`location_plan` reads the widest window (the kernel's LDS is sized by it) and whether ``t`` is sorted back to
the host.  :func:`running_location` given that ``plan`` enqueues kernels only and can be captured.  :func:`timing_plan` and
:func:`transit_times` divide the per-transit fit the same way.

Run-to-run differences: the box search and the template search sum each phase bin with fp64 atomic adds, whose order is not
fixed; ``power`` and the other outputs may differ in their last bits between two runs on the same input (and a near-tie
between two boxes may then resolve differently).  The Lomb-Scargle sums have a fixed order and are bitwise reproducible, and so
are the running filters (no atomics: selection does no arithmetic, the biweight sums run in the window's order) and the
per-transit fit (sums in the window's order, a fixed-shape reduction), a row of a batch being bitwise what the single call gives;
the same holds for the Keplerian periodogram and the astrometric search (a lane sums its candidate over the epochs in order; the
only reduction is an arg-max).
"""
import collections
import ctypes
import types

import numpy as np
import torch

from . import _lib

__all__ = [
    "bls_power", "tls_power", "transit_template", "lomb_scargle_power", "keplerian_power", "keplerian_max_power", "astrometric_power",
    "resample_indices", "series_chi2_0", "false_alarm_probability", "false_alarm_level", "false_alarm", "bls_autoperiod", "lomb_scargle_autofrequency",
    "LocationPlan", "location_plan", "running_location", "flatten", "sde",
    "TimingPlan", "timing_plan", "transit_times", "ttv_estimator",
    "find_peaks", "bls_estimator", "tls_estimator", "lomb_scargle_estimator", "keplerian_estimator", "astrometric_estimator", "autocorr_function", "autocorr_estimator", "estimate_semi_amplitude", "estimate_minimum_mass",
]

MAX_DURATIONS = 16      # EXO_BLS_MAX_DURATIONS
MAX_TEMPLATE = 8192     # EXO_TLS_MAX_TEMPLATE: bins of all templates of a call together
_OBJECTIVES = {None: 0, "likelihood": 0, "snr": 1}
BLS_FIELDS = ("power", "depth", "depth_err", "depth_snr", "log_likelihood", "duration", "transit_time")


class BLSResult(dict):
    """the outputs of :func:`bls_power`, by key and by attribute: ``period`` and the seven of ``BLS_FIELDS``"""

    __getattr__ = dict.__getitem__


# ---- arguments ---------------------------------------------------------------------------------------------------------------

def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise ValueError("the estimators run on a ROCm device and none is available; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to(x, device):
    return None if x is None else torch.as_tensor(x, dtype=torch.float64, device=device)


def _on_device(name, x):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor on a ROCm device")
    if not x.is_cuda:
        raise ValueError(f"{name} lives on {x.device}: the estimators run HIP kernels on a ROCm device; there is no CPU fallback")


def _time_axis(t):
    """the rule of a time axis: a device tensor of shape (N,), N >= 1"""
    _on_device("t", t)
    if t.ndim != 1 or t.numel() < 1:
        raise ValueError(f"t must have shape (N,), got {tuple(t.shape)}")


def _device_series(t, y, yerr):
    """-> t (N,), y (B, N), yerr None / (1, N) / (B, N), all contiguous float64 on t's device, and whether y was batched"""
    _time_axis(t)
    _on_device("y", y)
    n = t.numel()
    if y.ndim not in (1, 2) or y.shape[-1] != n:
        raise ValueError(f"y must have shape (N,) or (B, N) with N = {n}, got {tuple(y.shape)}")
    batched = y.ndim == 2
    t = t.to(torch.float64).contiguous()
    y = y.to(device=t.device, dtype=torch.float64).reshape(-1, n).contiguous()
    if y.shape[0] < 1:
        raise ValueError("y holds no series")
    if yerr is not None:
        if isinstance(yerr, torch.Tensor) and not yerr.is_cuda and yerr.ndim > 0:
            raise ValueError(f"yerr lives on {yerr.device}: there is no CPU fallback")
        if not isinstance(yerr, torch.Tensor) or yerr.ndim == 0:
            yerr = torch.full((1, n), float(yerr), dtype=torch.float64, device=t.device)
        if yerr.shape not in ((n,), (1, n), tuple(y.shape)):
            raise ValueError(f"yerr must be a scalar or have shape (N,) or that of y, got {tuple(yerr.shape)}")
        yerr = yerr.to(device=t.device, dtype=torch.float64).reshape(-1, n).contiguous()
    return t, y, yerr, batched


_grid_cache = collections.OrderedDict()


def _grid(x, name, device):
    """-> (host float64 array, device tensor) of a 1-D grid.  Host input: the device copy is cached by content."""
    if isinstance(x, torch.Tensor):
        if x.ndim != 1:
            raise ValueError(f"{name} must be one-dimensional")
        dev = x.to(device=device, dtype=torch.float64).contiguous()
        return dev.cpu().numpy(), dev
    host = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64)))
    if host.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    key = (str(device), host.shape, hash(host.tobytes()))
    hit = _grid_cache.get(key)
    if hit is not None and np.array_equal(hit[0], host):
        _grid_cache.move_to_end(key)
        return hit
    dev = torch.as_tensor(host, device=device)
    _grid_cache[key] = (host.copy(), dev)
    while len(_grid_cache) > 16:
        _grid_cache.popitem(last=False)
    return host, dev


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _workspace(nbytes, device):
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def _exclude_rows(exclude, B, N, device):
    """-> ``exclude`` (bool, (N,), (1, N) or (B, N), on a device) as contiguous rows (1, N) or (B, N).  Contiguous because
    :func:`running_location` hands the kernel its address; :func:`transit_times` only does torch arithmetic with it, where the
    call costs nothing."""
    if not isinstance(exclude, torch.Tensor):
        raise ValueError("exclude must be a torch.Tensor on a ROCm device")
    if not exclude.is_cuda:
        raise ValueError(f"exclude lives on {exclude.device}: there is no CPU fallback")
    if exclude.dtype != torch.bool or tuple(exclude.shape) not in ((N,), (1, N), (B, N)):
        raise ValueError(f"exclude must be bool of shape (N,) or that of y, got {exclude.dtype} {tuple(exclude.shape)}")
    return exclude.to(device).reshape(-1, N).contiguous()


def _plan_widest(info, t, check_sorted, cap, cap_name, argument):
    """The read-back of a plan, its one device-to-host copy: ``info`` (int32, (2,)) holds the widest window, and with
    ``check_sorted`` receives the count of places where ``t`` is unsorted or not finite.  -> the widest window"""
    if check_sorted:
        info[1] = (~(t[1:] >= t[:-1])).sum() + (~torch.isfinite(t)).sum()
    widest, unsorted = (int(v) for v in info.cpu())
    if unsorted:
        raise ValueError("t must be finite and non-decreasing (sort the series first)")
    if widest > cap:
        raise ValueError(f"the widest window holds {widest} cadences, more than the {cap} a window may hold "
                         f"({cap_name}): shorten {argument} or bin the series")
    return widest


def _check_plan(plan, t):
    if plan.n != t.numel() or plan.device != t.device:
        raise ValueError(f"plan was made for {plan.n} cadences on {plan.device}, t has {t.numel()} on {t.device}")


def _fields(planes, names, batched):
    """-> the output planes (F, B, ...) by name, without the series axis unless ``batched``"""
    return {name: plane if batched else plane[0] for name, plane in zip(names, planes)}


# ---- the periodograms ----------------------------------------------------------------------------------------------------------

def bls_plan(periods, durations, oversample):
    """host arithmetic of a box search: delta, the boxes' widths in bins, and every period's bin count"""
    periods, durations = np.asarray(periods, dtype=np.float64), np.asarray(durations, dtype=np.float64)
    if int(oversample) != oversample or oversample < 1:
        raise ValueError(f"oversample must be an integer >= 1, got {oversample}")
    if periods.size and not np.all(periods > 0):
        raise ValueError("periods must be positive")
    if durations.size < 1 or not np.all(durations > 0):
        raise ValueError("durations must be positive (and at least one is needed)")
    if durations.size > MAX_DURATIONS:
        raise ValueError(f"at most {MAX_DURATIONS} durations per call")
    if periods.size and durations.max() >= periods.min():
        raise ValueError("the longest duration must be shorter than the shortest period")
    delta = float(durations.min()) / int(oversample)
    m = np.round(durations / delta).astype(np.int32)
    n_bins = np.ceil(periods / delta).astype(np.int64) + int(oversample)
    return delta, m, n_bins


def bls_power(t, y, yerr=None, *, periods, durations, oversample=10, objective="likelihood"):
    """Box-least-squares periodogram (the binned method) of ``y`` (N,) or (B, N) at times ``t`` (N,), any order.

    ``yerr``: None (unit weights), a scalar, (N,) or (B, N).  ``periods`` (P,), ``durations`` (K,): numpy arrays or device
    tensors (see the module docstring).  Returns a :class:`BLSResult` of (P,) or (B, P) device tensors: ``power`` -- the
    maximum over durations and phases of the objective, the box's log likelihood (``"likelihood"``) or the depth's signal to
    noise (``"snr"``) -- and ``depth, depth_err, depth_snr, log_likelihood, duration, transit_time`` of that box, plus ``period``.
    A period with no admissible box (no weight inside or none outside every box) has ``power = -inf`` and NaN elsewhere."""
    return _period_search("bls_power", t, y, yerr, periods, durations, oversample, objective)


def _period_search(name, t, y, yerr, periods, durations, oversample, objective, extra=lambda m, device: ()):
    """The body of :func:`bls_power` and :func:`tls_power`, whose entry point is ``exo_<name>_f64``.  ``extra(m, device)``
    gives what that entry point takes between ``objective`` and ``out``: device tensors and numpy arrays, passed by address."""
    if objective not in _OBJECTIVES:
        raise ValueError(f"unknown objective {objective!r}: 'likelihood' or 'snr'")
    t, y, yerr, batched = _device_series(t, y, yerr)
    p_host, p_dev = _grid(periods, "periods", t.device)
    d_host = np.atleast_1d(_np(durations))
    if d_host.ndim != 1:
        raise ValueError("durations must be one-dimensional")
    delta, m, n_bins = bls_plan(p_host, d_host, oversample)
    more = extra(m, t.device)
    B, N, P = y.shape[0], y.shape[1], p_host.size
    out = torch.empty((7, B, P), dtype=torch.float64, device=t.device)
    if P:
        lib = _lib.load()
        lo, hi = int(n_bins.min()), int(n_bins.max())
        nbytes = lib.exo_bls_workspace_bytes(N, B, P, hi)
        if nbytes < 0:
            raise ValueError(f"{name}: invalid sizes")
        ws = _workspace(nbytes, t.device)
        ptr = lambda x: x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        entry = f"exo_{name}_f64"
        _lib.check(getattr(lib, entry)(t.data_ptr(), y.data_ptr(), 0 if yerr is None else yerr.data_ptr(),
                                       0 if yerr is None else yerr.shape[0], N, B, p_dev.data_ptr(), P, lo, hi, ptr(m), m.size, delta,
                                       int(oversample), _OBJECTIVES[objective], *(ptr(x) for x in more), out.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8, _stream(t)), entry)
    return BLSResult(period=p_dev, **_fields(out, BLS_FIELDS, batched))


_template_cache = collections.OrderedDict()


def transit_template(m, ror=0.1, b=0.0, u=(0.4804, 0.1867)):
    """The shape of a quadratically limb-darkened transit for :func:`tls_power`: the flux deficit of a straight-line transit of
    impact parameter ``b`` and radius ratio ``ror`` from first to fourth contact, sampled at the ``m`` bin centres
    ``x_j = (2 j + 1) / m - 1`` and divided by the deficit at mid-transit, so that the fitted ``depth`` is the mid-transit depth:
    ``z = sqrt(b^2 + ((1 + ror)^2 - b^2) x^2)``, ``g = lc(z, ror; u) / lc(b, ror; u)``.  A numpy array (m,).  The flux comes from
    the package's own solution-vector kernel (``ops.quad_solution_vector``), so a ROCm device is needed; results are remembered
    per argument set, and a repeated call touches no device."""
    if int(m) != m or m < 1:
        raise ValueError(f"m must be an integer >= 1, got {m}")
    ror, b = float(ror), float(b)
    if not ror > 0:
        raise ValueError(f"ror must be positive, got {ror}")
    if not 0 <= b < 1:
        raise ValueError(f"b must lie in [0, 1), got {b}")
    u = tuple(float(v) for v in np.atleast_1d(np.asarray(u, dtype=np.float64)))
    if len(u) != 2:
        raise ValueError(f"u must hold the two quadratic limb-darkening coefficients, got {u}")
    key = (int(m), ror, b, u)
    hit = _template_cache.get(key)
    if hit is not None:
        _template_cache.move_to_end(key)
        return hit.copy()
    from . import ops

    dev = _device_of()
    x = (2.0 * np.arange(int(m)) + 1.0) / int(m) - 1.0
    z = np.sqrt(b * b + ((1.0 + ror) ** 2 - b * b) * x * x)
    zd = torch.as_tensor(np.append(z, b), dtype=torch.float64, device=dev)
    s = ops.quad_solution_vector(zd, torch.full_like(zd, ror)).cpu().numpy()
    c = np.array([1.0 - u[0] - 1.5 * u[1], u[0] + 2.0 * u[1], -0.25 * u[1]])
    lc = s @ (c / (np.pi * (c[0] + c[1] / 1.5))) - 1.0
    g = lc[:-1] / lc[-1]
    _template_cache[key] = g.copy()
    while len(_template_cache) > 64:
        _template_cache.popitem(last=False)
    return g


def _template_table(templates, m, ror, b, u):
    """-> the flat host table of the K templates and its K + 1 offsets (int32)"""
    if templates is None:
        templates = [transit_template(int(mk), ror, b, u) for mk in m]
    elif isinstance(templates, (torch.Tensor, np.ndarray)) and templates.ndim != 1:
        raise ValueError(f"templates must be a list of {len(m)} one-dimensional arrays, got an array of shape {tuple(templates.shape)}")
    elif isinstance(templates, (torch.Tensor, np.ndarray)):
        templates = [templates]
    if len(templates) != len(m):
        raise ValueError(f"templates must hold one array per duration ({len(m)}), got {len(templates)}")
    rows = [np.atleast_1d(_np(g)) for g in templates]
    for k, (g, mk) in enumerate(zip(rows, m)):
        if g.ndim != 1 or g.size != mk:
            raise ValueError(f"template {k} must have shape ({int(mk)},), the duration in bins, got {tuple(g.shape)}")
        if not np.all(np.isfinite(g)):
            raise ValueError(f"template {k} is not finite: {g[~np.isfinite(g)][:3]}")
    offsets = np.concatenate([[0], np.cumsum([g.size for g in rows])])
    if offsets[-1] > MAX_TEMPLATE:
        raise ValueError(f"the templates hold {int(offsets[-1])} bins in all, more than the {MAX_TEMPLATE} a call takes")
    return np.ascontiguousarray(np.concatenate(rows)), offsets.astype(np.int32)


def tls_power(t, y, yerr=None, *, periods, durations, templates=None, ror=0.1, b=0.0, u=(0.4804, 0.1867), oversample=10,
              objective="likelihood"):
    """Transit-least-squares periodogram on the bins of :func:`bls_power`: every box is replaced by a template ``g_k`` of
    ``m_k = round(d_k / delta)`` bins, and the level and the depth of the model ``c - depth * g_k`` inside the window, ``c``
    outside, are fitted jointly by weighted least squares.

    Arguments and results as :func:`bls_power`, with ``templates``: a list of K arrays of lengths ``m_k`` (``bls_plan`` gives
    them), finite; None: :func:`transit_template` of ``ror``, ``b`` and ``u`` for every duration.  ``depth`` is the factor of the
    template (the mid-transit depth for a template that is 1 there), ``depth_err = 1 / sqrt(D)``, ``log_likelihood`` exactly half
    the drop in chi-squared against a constant.  With all-ones templates the depth, its error and its signal to noise are
    :func:`bls_power`'s.  Host templates are cached on the device by content, as the grids are."""
    def table(m, device):
        flat, offsets = _template_table(templates, m, ror, b, u)
        return _grid(flat, "templates", device)[1], offsets

    return _period_search("tls_power", t, y, yerr, periods, durations, oversample, objective, extra=table)


def lomb_scargle_power(t, y, yerr=None, *, frequencies):
    """Floating-mean Lomb-Scargle periodogram, exact sums, "psd" normalisation: ``(chi2_0 - chi2(f)) / 2`` with ``chi2(f)`` the
    weighted least-squares misfit of ``a sin(2 pi f t) + b cos(2 pi f t) + c``.  ``y`` (N,) or (B, N) -> (F,) or (B, F)."""
    t, y, yerr, batched = _device_series(t, y, yerr)
    f_host, f_dev = _grid(frequencies, "frequencies", t.device)
    B, N, F = y.shape[0], y.shape[1], f_host.size
    out = torch.empty((B, F), dtype=torch.float64, device=t.device)
    if F:
        lib = _lib.load()
        ws = _workspace(lib.exo_bls_workspace_bytes(N, B, 0, 0), t.device)
        _lib.check(lib.exo_lomb_scargle_power_f64(t.data_ptr(), y.data_ptr(), 0 if yerr is None else yerr.data_ptr(),
                                                  0 if yerr is None else yerr.shape[0], N, B, f_dev.data_ptr(), F, out.data_ptr(),
                                                  ws.data_ptr(), ws.numel() * 8, _stream(t)), "exo_lomb_scargle_power_f64")
    return out if batched else out[0]


MAX_INSTRUMENTS = 8     # EXO_KEP_MAX_INSTRUMENTS
MAX_ECC = 64            # EXO_KEP_MAX_ECC: eccentricities of a grid
MAX_PHASES = 4096       # EXO_KEP_MAX_PHASES
KEPLERIAN_FIT = ("ecc", "omega", "t_periastron", "K", "zero_point")


def _keplerian_grid(ecc, n_phase):
    """-> the eccentricity grid as a host array and ``n_phase``, checked"""
    ecc = np.linspace(0.0, 0.9, 10) if ecc is None else np.ascontiguousarray(np.atleast_1d(_np(ecc)))
    if ecc.ndim != 1 or ecc.size < 1:
        raise ValueError("ecc must be one-dimensional and hold at least one eccentricity")
    if not np.all((ecc >= 0.0) & (ecc < 1.0)):
        raise ValueError("every eccentricity must lie in [0, 1)")
    if ecc.size > MAX_ECC:
        raise ValueError(f"at most {MAX_ECC} eccentricities per call")
    if int(n_phase) != n_phase or not 1 <= n_phase <= MAX_PHASES:
        raise ValueError(f"n_phase must be an integer in [1, {MAX_PHASES}], got {n_phase}")
    return ecc, int(n_phase)


def _instrument_segments(instrument, n):
    """-> (order, offsets) of the ``n`` epochs sorted by instrument, stably: ``order`` a host int64 array (None without
    ``instrument``: one instrument, the epochs as they are), ``offsets`` int32 of length n_inst + 1"""
    if instrument is None:
        return None, np.array([0, n], dtype=np.int32)
    inst = instrument.detach().cpu().numpy() if isinstance(instrument, torch.Tensor) else np.asarray(instrument)
    if inst.ndim != 1 or inst.size != n:
        raise ValueError(f"instrument must have shape (N,) with N = {n}, got {tuple(inst.shape)}")
    if inst.dtype == bool:
        inst = inst.astype(np.int64)
    if not np.issubdtype(inst.dtype, np.integer):
        if not np.all(inst == np.round(inst)):
            raise ValueError("instrument must hold integers")
        inst = inst.astype(np.int64)
    if inst.min() < 0:
        raise ValueError("instrument must not be negative")
    counts = np.bincount(inst)
    if np.count_nonzero(counts) > MAX_INSTRUMENTS:
        raise ValueError(f"at most {MAX_INSTRUMENTS} instruments per call")
    if not np.all(counts > 0):
        raise ValueError("the instruments must be numbered 0 .. n_inst - 1 without gaps: "
                         f"none of the epochs belongs to instrument {int(np.flatnonzero(counts == 0)[0])}")
    return np.argsort(inst, kind="stable"), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _keplerian_arguments(t, y, yerr, frequencies, ecc, n_phase, instrument):
    """What :func:`keplerian_power` and :func:`keplerian_max_power` do alike before their entry point: the grids checked, the
    series on the device with the epochs sorted by instrument, and ``lead``, the entry's arguments before the frequencies.  ->
    a namespace that also keeps alive what ``lead`` points to"""
    e_host, n_phase = _keplerian_grid(ecc, n_phase)
    n_given = t.shape[-1] if hasattr(t, "shape") and len(t.shape) else 0
    order, offsets = _instrument_segments(instrument, int(n_given))
    t, y, yerr, batched = _device_series(t, y, yerr)
    _, f_dev = _grid(frequencies, "frequencies", t.device)
    t_min = t.min()
    if order is not None:                                      # the epochs by instrument (the sums need no time order)
        order = torch.as_tensor(order, device=t.device)
        t, y = t[order].contiguous(), y[:, order].contiguous()
        yerr = None if yerr is None else yerr[:, order].contiguous()
    lead = (t.data_ptr(), y.data_ptr(), 0 if yerr is None else yerr.data_ptr(), 0 if yerr is None else yerr.shape[0], y.shape[1],
            y.shape[0], offsets.ctypes.data_as(ctypes.c_void_p), offsets.size - 1)
    return types.SimpleNamespace(t=t, y=y, yerr=yerr, batched=batched, f_dev=f_dev, e_host=e_host, n_phase=n_phase, offsets=offsets,
                                 t_min=t_min, lead=lead)


def keplerian_power(t, y, yerr=None, *, frequencies, ecc=None, n_phase=64, instrument=None, return_fit=False):
    """Keplerian periodogram of the radial velocities ``y`` (N,) or (B, N) at the epochs ``t`` (N,), any order: at every
    frequency the largest ``(chi2_0 - chi2) / 2`` over a grid of eccentricities ``ecc`` (default ``linspace(0, 0.9, 10)``) and
    ``n_phase`` times of periastron ``t.min() + (k / n_phase) / f``, where ``chi2`` is the weighted least-squares misfit of
    ``c_inst + A cos nu + B sin nu`` (``nu``: the true anomaly) and ``chi2_0`` that of the constants alone (DESIGN.md section
    22).  ``instrument``: integers 0 .. n_inst - 1 (at most 8), one per epoch, each instrument with a constant of its own; None:
    one instrument.  ``yerr`` as in :func:`lomb_scargle_power`; ``frequencies`` (F,), ``ecc``: numpy arrays or tensors.
    Returns the power, (F,) or (B, F); with ``ecc=[0]`` and one instrument it is :func:`lomb_scargle_power`, and with 0 in the
    grid it is never below it.

    ``return_fit=True``: also a dict of tensors ``ecc, omega, t_periastron, K`` (..., F) and ``zero_point`` (..., F, n_inst) of
    the winning candidate's fit (and ``candidate``, its number ``j * n_phase + k`` in the grids, int64), in the convention of
    ``KeplerianOrbit.get_radial_velocity(t, K=K)`` and ``rv_log_likelihood(K=, zero_point=, instrument=)``: ``period = 1 / f``,
    and the model is ``zero_point[instrument] + K (cos omega (cos nu + ecc) - sin omega sin nu)``.  Every sum has a fixed
    order: the results are bitwise reproducible."""
    a = _keplerian_arguments(t, y, yerr, frequencies, ecc, n_phase, instrument)
    t_min, f_dev, n_phase = a.t_min, a.f_dev, a.n_phase

    def fit(cand, c, e, coef):
        # the elements of the winner: A = K cos w, B = -K sin w, c_k = zero_point_k + e A
        phi = (c % n_phase).to(torch.float64) / n_phase
        t_p = torch.where(cand >= 0, t_min + phi / f_dev, torch.full_like(e, float("nan")))
        A, Bs = coef[..., 0], coef[..., 1]
        return dict(ecc=e, omega=torch.atan2(-Bs, A), t_periastron=t_p, K=torch.hypot(A, Bs),
                    zero_point=coef[..., 2:] - (e * A)[..., None], candidate=cand.to(torch.int64))

    return _orbit_search("keplerian", a.t, a.lead, tuple(a.y.shape), f_dev, a.e_host, n_phase, 2 + a.offsets.size - 1, a.batched,
                         fit if return_fit else None)


def _orbit_search(name, t, lead, shape, f_dev, e_host, n_phase, n_coef, batched, fit):
    """What :func:`keplerian_power` and :func:`astrometric_power` do alike around ``exo_<name>_power_f64``: the outputs, the
    workspace and the call (``lead``: the entry's arguments before the frequencies; ``shape``: (B, N)); then the power, (F,)
    or (B, F) -- with ``fit`` also ``fit(candidate, c, ecc, coef)`` of the winners' records, unbatched alike: ``candidate``
    int32 (-1: none), ``c`` the same clamped to the grid (int64), ``ecc`` the winner's eccentricity, NaN where there is none."""
    (B, N), F = shape, f_dev.numel()
    power = torch.empty((B, F), dtype=torch.float64, device=t.device)
    cand = torch.empty((B, F), dtype=torch.int32, device=t.device)
    coef = torch.empty((B, F, n_coef), dtype=torch.float64, device=t.device)
    if F:
        lib = _lib.load()
        nbytes = getattr(lib, f"exo_{name}_workspace_bytes")(N, B)
        if nbytes < 0:
            raise ValueError(f"{name}_power: invalid sizes")
        ws = _workspace(nbytes, t.device)
        entry = f"exo_{name}_power_f64"
        _lib.check(getattr(lib, entry)(*lead, f_dev.data_ptr(), F, e_host.ctypes.data_as(ctypes.c_void_p), e_host.size, n_phase,
                                       power.data_ptr(), cand.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(t)),
                   entry)
    if fit is None:
        return power if batched else power[0]
    c = cand.clamp(min=0).to(torch.int64)
    e = torch.where(cand >= 0, _grid(e_host, "ecc", t.device)[1][c // n_phase], torch.full_like(power, float("nan")))
    out = fit(cand, c, e, coef)
    if not batched:
        power, out = power[0], {k: v[0] for k, v in out.items()}
    return power, out


KEPLERIAN_MAX_GROUP = 8  # series that share a solve in exo_keplerian_max_f64 (csrc/exo_keplerian.hip: kGroup)
MAX_SERIES = 65535       # series of one call of the orbit searches


def keplerian_max_power(t, y, yerr=None, *, frequencies, ecc=None, n_phase=64, instrument=None, frequencies_per_block=None):
    """The highest peak of :func:`keplerian_power` for every series of ``y`` (N,) or (B, N), without the periodogram: a dict of
    ``power``, the largest power over the grid, ``frequency_index``, the lowest index at which it is reached, and ``candidate``,
    the winner's number there (int64), each (B,) or a scalar tensor; ``-inf, -1, -1`` for a series without a finite power.  The
    numbers are bit for bit those of ``keplerian_power(..., return_fit=True)`` and its row maximum, for any batch; what makes
    it several times cheaper for a large one is that ``KEPLERIAN_MAX_GROUP`` series share every solve of Kepler's equation
    (DESIGN.md section 26).  The other arguments are :func:`keplerian_power`'s; ``frequencies_per_block``: consecutive
    frequencies searched by one workgroup (None: chosen to fill the device; the results do not depend on it)."""
    per_block = 0 if frequencies_per_block is None else frequencies_per_block
    if int(per_block) != per_block or (frequencies_per_block is not None and per_block < 1):
        raise ValueError(f"frequencies_per_block must be a positive integer or None, got {frequencies_per_block}")
    a = _keplerian_arguments(t, y, yerr, frequencies, ecc, n_phase, instrument)
    (B, N), F, device = a.y.shape, a.f_dev.numel(), a.t.device
    power = torch.full((B,), float("-inf"), dtype=torch.float64, device=device)
    index = torch.full((B,), -1, dtype=torch.int32, device=device)
    cand = torch.full((B,), -1, dtype=torch.int32, device=device)
    if F:
        lib = _lib.load()
        nbytes = lib.exo_keplerian_max_workspace_bytes(N, B, F, int(per_block))
        if nbytes < 0:
            raise ValueError("keplerian_max_power: invalid sizes")
        ws = _workspace(nbytes, device)
        _lib.check(lib.exo_keplerian_max_f64(*a.lead, a.f_dev.data_ptr(), F, a.e_host.ctypes.data_as(ctypes.c_void_p), a.e_host.size,
                                             a.n_phase, int(per_block), power.data_ptr(), index.data_ptr(), cand.data_ptr(),
                                             ws.data_ptr(), ws.numel() * 8, _stream(a.t)), "exo_keplerian_max_f64")
    out = dict(power=power, frequency_index=index.to(torch.int64), candidate=cand.to(torch.int64))
    return out if a.batched else {k: v[0] for k, v in out.items()}


# ---- false-alarm probabilities by resampling ------------------------------------------------------------

def _instrument_of(instrument, n):
    """-> the instrument of every epoch as a host int64 array (zeros without ``instrument``), checked as the searches check it"""
    if instrument is None:
        return np.zeros(n, dtype=np.int64)
    _instrument_segments(instrument, n)
    inst = instrument.detach().cpu().numpy() if isinstance(instrument, torch.Tensor) else np.asarray(instrument)
    return inst.astype(np.int64)


def resample_indices(n, n_resample, *, instrument=None, replace=False, seed=0):
    """A resampling table (R, N), int64, made on the host with ``np.random.default_rng(seed)``, row by row: resampled series
    ``r`` takes ``y[idx[r, i]]`` at epoch ``i``.  Every index stays within its epoch's instrument, so the segments and the free
    constants keep their meaning.  ``replace=False``: each instrument's entries of a row are a permutation of its epochs (the
    shuffle of the radial-velocity literature); ``replace=True``: drawn from them with replacement (the bootstrap)."""
    if int(n) != n or n < 1 or int(n_resample) != n_resample or n_resample < 1:
        raise ValueError(f"n and n_resample must be positive integers, got {n} and {n_resample}")
    inst = _instrument_of(instrument, int(n))
    members = [np.flatnonzero(inst == k) for k in np.unique(inst)]
    rng = np.random.default_rng(seed)
    idx = np.empty((int(n_resample), int(n)), dtype=np.int64)
    for row in idx:
        for m in members:
            row[m] = rng.choice(m, size=m.size, replace=True) if replace else rng.permutation(m)
    return idx


def _check_resamples(resamples, inst):
    """-> a caller's table as a host int64 array (R, N), or ValueError: shape, dtype, range, and no index across instruments"""
    idx = resamples.detach().cpu().numpy() if isinstance(resamples, torch.Tensor) else np.asarray(resamples)
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] != inst.size:
        raise ValueError(f"resamples must have shape (R, N) with R >= 1 and N = {inst.size}, got {tuple(idx.shape)}")
    if idx.dtype != np.int64:
        raise ValueError(f"resamples must be int64, got {idx.dtype}")
    if idx.min() < 0 or idx.max() >= inst.size:
        raise ValueError(f"resamples holds an index outside 0 .. {inst.size - 1}")
    if not np.array_equal(inst[idx], np.broadcast_to(inst, idx.shape)):
        raise ValueError("resamples takes an epoch's value from another instrument: resample within the instruments")
    return np.ascontiguousarray(idx)


def _ordered_sum(x):
    """the sum over the last axis by a tree of one fixed shape, whatever the batch: ``torch.sum`` chooses its order by the
    tensor's shape, and a row of a batch must give bit for bit what the single series gives"""
    n = x.shape[-1]
    x = torch.nn.functional.pad(x, (0, (1 << max(n - 1, 0).bit_length()) - n))
    while x.shape[-1] > 1:
        half = x.shape[-1] // 2
        x = x[..., :half] + x[..., half:]
    return x[..., 0]


def series_chi2_0(y, yerr=None, instrument=None):
    """``chi2_0 = sum w (y - ybar_inst)^2`` of every row of ``y`` (N,) or (B, N), ``ybar_inst`` the weighted mean of the epoch's
    instrument: the misfit of the constants alone, which ``2 power / chi2_0`` of a periodogram is relative to.  ``yerr``: None, a
    scalar, (N,) or the shape of ``y``.  Plain torch, on the device of ``y`` (a CPU tensor too); every sum has one fixed order, so a
    row of a batch is bit for bit the single series."""
    y = torch.as_tensor(y)
    y = y.to(torch.float64)
    w = torch.ones_like(y) if yerr is None else (1.0 / torch.as_tensor(yerr, dtype=torch.float64, device=y.device) ** 2).expand_as(y)
    inst = _instrument_of(instrument, y.shape[-1])
    total = torch.zeros(y.shape[:-1], dtype=torch.float64, device=y.device)
    for k in range(int(inst.max()) + 1):
        members = torch.as_tensor(np.flatnonzero(inst == k), device=y.device)
        wk, yk = w[..., members], y[..., members]
        ybar = (_ordered_sum(wk * yk) / _ordered_sum(wk))[..., None]
        total = total + _ordered_sum(wk * (yk - ybar) ** 2)
    return total


def false_alarm_probability(z_null, z):
    """``FAP(z) = (1 + #{r : z_null[r] >= z}) / (R + 1)`` for the maxima ``z_null`` (R,) of R resamplings: never zero; a NaN in
    ``z_null`` never counts (and stays in R).  ``z``: any shape; NaN gives NaN.  Tensors give a tensor, arrays an array."""
    if isinstance(z_null, torch.Tensor) or isinstance(z, torch.Tensor):
        zn = torch.as_tensor(z_null).to(torch.float64).reshape(-1)
        zz = torch.as_tensor(z).to(device=zn.device, dtype=torch.float64)
        fap = (1 + (zn >= zz[..., None]).sum(-1)).to(torch.float64) / (zn.numel() + 1)
        return torch.where(torch.isnan(zz), zz, fap)
    zn, zz = np.asarray(z_null, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fap = (1.0 + (zn >= zz[..., None]).sum(-1)) / (zn.size + 1.0)
    return np.where(np.isnan(zz), zz, fap)


def false_alarm_level(z_null, alpha):
    """The level of the false-alarm probability ``alpha`` from the maxima ``z_null`` (R,) of R resamplings: with ``k = floor(alpha
    (R + 1))`` the k-th largest of them (a NaN ranks below every number), so that a peak strictly above it has ``FAP <= alpha``;
    NaN when ``k < 1``: R resamplings resolve no level below ``1 / (R + 1)``.  -> a float"""
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"a false-alarm level must lie in (0, 1), got {alpha}")
    zn = np.sort(_np(z_null).reshape(-1))[::-1]                 # (descending: np.sort puts NaN last, reversed they come first ...)
    zn = np.concatenate([zn[~np.isnan(zn)], zn[np.isnan(zn)]])  # (... and belong behind the numbers)
    k = int(np.floor(alpha * (zn.size + 1) + 1e-9))             # (1e-9: 0.29 * 100 is 28.999999999999996 in binary)
    return float(zn[k - 1]) if k >= 1 else float("nan")


def _default_chunk(method, n, n_freq):
    """rows of the resampling table searched per call: under the entry points' series limit, about 256 MiB of workspace and
    output, whole groups of the Keplerian kernel"""
    per_row = 8 * (4 * n + n_freq) if method == "lomb_scargle" else 8 * 4 * n + 4096     # (the columns; the partials)
    chunk = max(1, min(MAX_SERIES, (256 << 20) // per_row))
    return chunk - chunk % KEPLERIAN_MAX_GROUP if chunk > KEPLERIAN_MAX_GROUP else chunk


def false_alarm(t, y, yerr=None, *, frequencies, method="keplerian", n_resample=1000, replace=False, seed=0, resamples=None,
                ecc=None, n_phase=64, instrument=None, power=None, levels=(0.1, 0.01, 0.001), chunk=None):
    """False-alarm probability of the highest peak of one series' periodogram, by resampling (Cumming 2004; astropy's
    ``method="bootstrap"``): the velocities ``y`` (N,) are shuffled (``replace=False``) or drawn with replacement on their
    epochs ``t``, within each instrument, ``n_resample`` times (:func:`resample_indices`; ``resamples``: a table (R, N) of the
    caller's instead), a per-epoch ``yerr`` travelling with its velocity, and the highest peak of every resampled series is
    recorded as ``z = 2 max_f power(f) / chi2_0``, ``chi2_0`` the resampled series' own (:func:`series_chi2_0`; NaN where it is
    zero).  ``method="keplerian"``: the peak of :func:`keplerian_power` (``ecc``, ``n_phase``, ``instrument``), found by
    :func:`keplerian_max_power`; ``"lomb_scargle"``: that of :func:`lomb_scargle_power` (one instrument).  ``chunk``: rows of
    the table searched per call (None: bounded by the kernels' series limit and a modest memory budget; the results do not
    depend on it).

    Returns a dict: ``z``, ``max_power``, ``frequency_index`` (R,), device tensors; ``observed``, the same three for the data
    itself; ``fap``, the probability of the observed peak (a float) or, with ``power=`` raw powers of that periodogram, of each
    of them (an array); ``levels`` ``{alpha: z}`` (:func:`false_alarm_level`) and ``power_levels`` ``{alpha: z chi2_0 / 2}``, the
    lines to draw on the data's own :func:`keplerian_power` plot; ``resamples``, the table.  The same seed gives the same
    numbers bit for bit."""
    if method not in ("keplerian", "lomb_scargle"):
        raise ValueError(f"method must be 'keplerian' or 'lomb_scargle', got {method!r}")
    if method == "lomb_scargle" and instrument is not None:
        raise ValueError("method='lomb_scargle' fits one constant: instrument must be None")
    if not hasattr(y, "shape") or len(y.shape) != 1 or not hasattr(t, "shape") or tuple(t.shape) != tuple(y.shape):
        raise ValueError("false_alarm takes one series: t and y must have the same shape (N,)")
    n = y.shape[0]
    levels = tuple(float(a) for a in levels)
    for alpha in levels:
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"a false-alarm level must lie in (0, 1), got {alpha}")
    inst = _instrument_of(instrument, n)
    if resamples is not None:
        idx = _check_resamples(resamples, inst)
    elif int(n_resample) != n_resample or n_resample < 1:
        raise ValueError(f"n_resample must be a positive integer (or give resamples=), got {n_resample}")
    else:
        idx = resample_indices(n, n_resample, instrument=instrument, replace=replace, seed=seed)
    if chunk is not None and (int(chunk) != chunk or not 1 <= chunk <= MAX_SERIES):
        raise ValueError(f"chunk must be an integer in [1, {MAX_SERIES}], got {chunk}")

    dev = _device_of(t, y)
    td, yd = _to(t, dev), _to(y, dev)
    per_epoch = yerr is not None and len(getattr(yerr, "shape", ())) > 0
    ed = _to(yerr, dev) if per_epoch else yerr
    f_host, _ = _grid(frequencies, "frequencies", dev)
    chunk = _default_chunk(method, n, f_host.size) if chunk is None else int(chunk)

    def peaks(rows):
        """rows (C, N) of indices on the device (None: the data itself) -> z, max_power, frequency_index, each (C,)"""
        ys = yd[None] if rows is None else yd[rows]
        es = ed if rows is None or not per_epoch else ed[rows]
        if method == "keplerian":
            res = keplerian_max_power(td, ys, es, frequencies=frequencies, ecc=ecc, n_phase=n_phase, instrument=instrument)
            top, where = res["power"], res["frequency_index"]
        else:
            top, where = lomb_scargle_power(td, ys, es, frequencies=frequencies).max(dim=1)
        chi2_0 = series_chi2_0(ys, es, inst)
        return torch.where(chi2_0 == 0, torch.full_like(top, float("nan")), 2.0 * top / chi2_0), top, where, chi2_0

    z_obs, top_obs, where_obs, chi2_obs = (v[0] for v in peaks(None))
    idx_dev = torch.as_tensor(idx, device=dev)
    parts = [peaks(idx_dev[r:r + chunk])[:3] for r in range(0, idx.shape[0], chunk)]
    z, top, where = (torch.cat(col) for col in zip(*parts))
    z_host, half = _np(z), 0.5 * float(chi2_obs)
    fap = float(false_alarm_probability(z_host, float(z_obs))) if power is None else false_alarm_probability(z_host, _np(power) / half)
    z_levels = {alpha: false_alarm_level(z_host, alpha) for alpha in levels}
    return dict(z=z, max_power=top, frequency_index=where, observed=dict(z=z_obs, max_power=top_obs, frequency_index=where_obs),
                fap=fap, levels=z_levels, power_levels={alpha: v * half for alpha, v in z_levels.items()}, resamples=idx)


AST_NCOEF = 10          # EXO_AST_NCOEF
ASTROMETRIC_FIT = ("TA", "TB", "TF", "TG", "a_angular", "incl", "omega", "Omega", "t_periastron", "chi2")   # the record's order


def _astrometric_error(name, err, shape, device):
    """-> an error bar (a scalar, (N,) or the shape of the series) as contiguous rows (1, N) or (B, N) on the device"""
    n = shape[-1]
    if err is None:
        raise ValueError(f"{name} is required: the weights of the fit are 1 / {name}^2")
    if isinstance(err, torch.Tensor) and not err.is_cuda and err.ndim > 0:
        raise ValueError(f"{name} lives on {err.device}: there is no CPU fallback")
    if not isinstance(err, torch.Tensor) or err.ndim == 0:
        return torch.full((1, n), float(err), dtype=torch.float64, device=device)
    if tuple(err.shape) not in ((n,), (1, n), tuple(shape)):
        raise ValueError(f"{name} must be a scalar or have shape (N,) or that of rho, got {tuple(err.shape)}")
    return err.to(device=device, dtype=torch.float64).reshape(-1, n).contiguous()


def astrometric_power(t, rho, rho_err, theta, theta_err, *, frequencies, ecc=None, n_phase=64, parallax=None, return_fit=False):
    """Astrometric orbit search of the separations ``rho`` and position angles ``theta`` (radians), each (N,) or (B, N), at
    the epochs ``t`` (N,), any order: at every frequency the largest ``(chi2_0 - chi2) / 2`` over a grid of eccentricities
    ``ecc`` (default ``linspace(0, 0.9, 10)``) and ``n_phase`` times of periastron ``t.min() + (k / n_phase) / f``.  At a
    fixed period, eccentricity and time of periastron the sky-plane position is linear in the four Thiele-Innes constants,
    ``X = TA xi + TF eta``, ``Y = TB xi + TG eta`` with ``xi = cos E - ecc``, ``eta = sqrt(1 - ecc^2) sin E``; ``chi2`` is the
    misfit of that least-squares fit with the radial error ``rho_err`` and the tangential error ``rho theta_err`` (the
    measured ``rho``), and ``chi2_0`` that of no companion.  ``rho_err``, ``theta_err``: a scalar,
    (N,) or (B, N); ``frequencies`` (F,), ``ecc``: numpy arrays or tensors.  Returns the power, (F,) or (B, F); a frequency
    at which every candidate's normal equations are singular has power 0.

    ``return_fit=True``: also a dict of tensors (..., F) of the winning candidate: ``candidate`` (its number ``j * n_phase +
    k`` in the grids, int64, -1 where there is none), ``ecc, t_periastron, omega, Omega, incl, a_angular``, the constants
    ``TA, TB, TF, TG`` and ``chi2``; with ``parallax`` (arcseconds) also ``a = a_angular / (parallax au_per_R_sun)`` in R_sun.
    The elements are in the convention of ``KeplerianOrbit(period=1 / f, t_periastron=, ecc=, omega=, Omega=, incl=, a=)``,
    whose ``get_relative_position(t, parallax)`` then is ``(X, Y)`` and whose ``astrometry_log_likelihood`` they start.
    Astrometry alone cannot tell ``(omega, Omega)`` from ``(omega + pi, Omega + pi)``: ``Omega`` is given in ``[0, pi)``, the
    usual rule, and ``omega`` in ``(-pi, pi]``.  Every sum has a fixed order: the results are bitwise reproducible."""
    e_host, n_phase = _keplerian_grid(ecc, n_phase)
    t, rho, _, batched = _device_series(t, rho, None)
    _on_device("theta", theta)
    if theta.ndim not in (1, 2) or (theta.ndim == 2) != batched or theta.shape[-1] != t.numel():
        raise ValueError(f"theta must have the shape of rho, got {tuple(theta.shape)}")
    theta = theta.to(device=t.device, dtype=torch.float64).reshape(-1, t.numel()).contiguous()
    if theta.shape != rho.shape:
        raise ValueError(f"theta must have the shape of rho, got {tuple(theta.shape)}")
    rho_err = _astrometric_error("rho_err", rho_err, rho.shape, t.device)
    theta_err = _astrometric_error("theta_err", theta_err, rho.shape, t.device)
    _, f_dev = _grid(frequencies, "frequencies", t.device)
    B, N = rho.shape
    lead = (t.data_ptr(), rho.data_ptr(), rho_err.data_ptr(), rho_err.shape[0], theta.data_ptr(), theta_err.data_ptr(),
            theta_err.shape[0], N, B)

    def fit(cand, c, e, coef):
        out = dict(candidate=cand.to(torch.int64), ecc=e, **{k: coef[..., i] for i, k in enumerate(ASTROMETRIC_FIT)})
        if parallax is not None:
            from .orbits.constants import au_per_R_sun

            out["a"] = out["a_angular"] / (parallax * au_per_R_sun)
        return out

    return _orbit_search("astrometric", t, lead, (B, N), f_dev, e_host, n_phase, AST_NCOEF, batched, fit if return_fit else None)


# ---- detrending: running median, MAD and biweight location --------------------------------------------------------------------

MAX_WINDOW = 8192       # EXO_LOCATION_MAX_WINDOW: cadences in one window
MAX_TREND_WINDOW = 4096  # EXO_TREND_MAX_WINDOW: the same for order 1 and 2, whose kernel stages the times beside the values
_METHODS = {"median": 0, "biweight": 1}


class LocationPlan:
    """The windows of :func:`running_location` on one time axis, from :func:`location_plan`: device tensors ``lo`` and ``hi``
    (int32, (N,): cadence i's window is ``lo[i] .. hi[i]``, both included), ``edge`` (bool, (N,): cut by ``edge_cutoff``), and
    ``max_window``, the widest window in cadences, a Python int."""

    __slots__ = ("lo", "hi", "edge", "max_window", "n", "device")

    def __init__(self, lo, hi, edge, max_window):
        self.lo, self.hi, self.edge, self.max_window = lo, hi, edge, int(max_window)
        self.n, self.device = lo.numel(), lo.device

    def __repr__(self):
        return f"LocationPlan(n={self.n}, max_window={self.max_window}, device={self.device})"


def location_plan(t, window_length, break_tolerance=None, edge_cutoff=0.0, check_sorted=True):
    """The windows of a running filter of ``window_length`` (in the units of ``t``) on the device time axis ``t`` (N,), finite
    and non-decreasing: cadence i's window holds the cadences j of its segment with ``t[i] - h <= t[j] <= t[i] + h``,
    ``h = 0.5 * window_length``; a new segment opens where ``t[i] - t[i-1] > break_tolerance`` (None: one segment); cadences
    closer than ``edge_cutoff`` to their segment's first or last time are flagged and get NaN.  Returns a
    :class:`LocationPlan`.

    This is the one synchronisation of the detrending functions: the widest window (and, with ``check_sorted``, whether
    ``t`` is sorted and finite) is read back.  ValueError: an unsorted ``t``, or a window wider than ``MAX_WINDOW`` cadences."""
    _time_axis(t)
    window_length, edge_cutoff = float(window_length), float(edge_cutoff)
    if not window_length >= 0:
        raise ValueError(f"window_length must be at least 0, got {window_length}")
    if not edge_cutoff >= 0:
        raise ValueError(f"edge_cutoff must be at least 0, got {edge_cutoff}")
    if break_tolerance is not None and not float(break_tolerance) > 0:
        raise ValueError(f"break_tolerance must be None or positive, got {break_tolerance}")
    t = t.to(torch.float64).contiguous()
    n = t.numel()
    lo = torch.empty(n, dtype=torch.int32, device=t.device)
    hi = torch.empty(n, dtype=torch.int32, device=t.device)
    edge = torch.empty(n, dtype=torch.bool, device=t.device)
    info = torch.zeros(2, dtype=torch.int32, device=t.device)
    lib = _lib.load()
    _lib.check(lib.exo_location_windows_f64(t.data_ptr(), n, 0.5 * window_length,
                                            float("inf") if break_tolerance is None else float(break_tolerance), edge_cutoff,
                                            lo.data_ptr(), hi.data_ptr(), edge.data_ptr(), info.data_ptr(), _stream(t)),
               "exo_location_windows_f64")
    return LocationPlan(lo, hi, edge, _plan_widest(info, t, check_sorted, MAX_WINDOW, "EXO_LOCATION_MAX_WINDOW", "window_length"))


def _check_trend_window(widest):
    if widest > MAX_TREND_WINDOW:
        raise ValueError(f"the widest window holds {widest} cadences, more than the {MAX_TREND_WINDOW} a window may hold with order "
                         f"1 or 2 (EXO_TREND_MAX_WINDOW): shorten window_length or bin the series")


def running_location(t, y, window_length=None, *, method="biweight", exclude=None, break_tolerance=None, edge_cutoff=0.0, cval=5.0,
                     n_iter=10, return_scale=False, plan=None, order=0, rescale=1):
    """Running robust location of ``y`` (N,) or (B, N) over time windows of ``window_length`` on ``t`` (N,), finite and
    non-decreasing: the trend that :func:`flatten` divides by (definition: DESIGN.md section 19).  Device tensors in and out.

    ``method``: ``"median"``, or ``"biweight"`` -- Tukey's biweight location with tuning constant ``cval``, started at the median
    and scaled by the window's median absolute deviation, **exactly** ``n_iter`` steps.  The iteration converges linearly (a
    contraction of about 0.8 per step at worst on noisy photometry): ``n_iter`` is the accuracy knob, and going from 10 to 40
    moves the result by up to 1e-5 where the noise is 1e-3; a fixed count keeps the result independent of the order of
    summation.  ``exclude``: bool, (N,) or (B, N): cadences left out of every window, which still receive a trend value (mask
    known transits with it).  ``break_tolerance``, ``edge_cutoff``: see :func:`location_plan`.  A window with no cadence left,
    and a cadence cut by ``edge_cutoff``, give NaN.

    ``order``: 0 (the default) is the location above, a polynomial of degree 0.  1 or 2 (``method="biweight"`` only; DESIGN.md
    section 21; csrc/exo_trend.hip) fits a polynomial of that degree in time to the window with the same biweight weights --
    ``n_iter`` weighted least-squares steps from the median, then ``rescale`` times (an integer >= 0, read only here) the median
    absolute residual as the new scale and ``n_iter`` more steps -- and returns its value at the cadence's own time.  A line
    removes the location's bias next to a gap or a segment's end, about ``slope * window / 4``, so that ``edge_cutoff`` need not
    throw those cadences away; a parabola also removes its undershoot of every extremum, ``curvature * window**2 / 24``, so
    that the window may be twice as long.  A window holds at most ``MAX_TREND_WINDOW`` cadences then.

    Returns ``trend``, (N,) or (B, N); with ``return_scale`` also the windows' MAD (unscaled; for ``order`` 1 and 2 the last scale
    used).  With ``plan`` (a :class:`LocationPlan` of the same ``t``; ``window_length``, ``break_tolerance`` and ``edge_cutoff`` are
    then not read) the call enqueues kernels only and may be captured into a graph.  Bitwise reproducible; a row of a batch is
    bitwise the single call."""
    if method not in _METHODS:
        raise ValueError(f"unknown method {method!r}: 'median' or 'biweight'")
    if not float(cval) > 0:
        raise ValueError(f"cval must be positive, got {cval}")
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError(f"n_iter must be an integer >= 0, got {n_iter}")
    if order not in (0, 1, 2):
        raise ValueError(f"order must be 0, 1 or 2, got {order}")
    if order:
        if method != "biweight":
            raise ValueError(f"order {order} needs method 'biweight', got {method!r}")
        if int(rescale) != rescale or rescale < 0:
            raise ValueError(f"rescale must be an integer >= 0, got {rescale}")
        if plan is not None:
            _check_trend_window(plan.max_window)
    t, y, _, batched = _device_series(t, y, None)
    B, N = y.shape
    if exclude is not None:
        exclude = _exclude_rows(exclude, B, N, t.device)
    if plan is None:
        if window_length is None:
            raise ValueError("running_location needs window_length or plan")
        plan = location_plan(t, window_length, break_tolerance=break_tolerance, edge_cutoff=edge_cutoff)
    else:
        _check_plan(plan, t)
    trend = torch.empty((B, N), dtype=torch.float64, device=t.device)
    scale = torch.empty((B, N), dtype=torch.float64, device=t.device) if return_scale else None
    lib = _lib.load()
    if order:
        _check_trend_window(plan.max_window)
        _lib.check(lib.exo_running_trend_f64(t.data_ptr(), y.data_ptr(), 0 if exclude is None else exclude.data_ptr(),
                                             0 if exclude is None else exclude.shape[0], N, B, plan.lo.data_ptr(), plan.hi.data_ptr(),
                                             plan.edge.data_ptr(), plan.max_window, int(order), float(cval), int(n_iter), int(rescale),
                                             trend.data_ptr(), 0 if scale is None else scale.data_ptr(), _stream(t)),
                   "exo_running_trend_f64")
    else:
        _lib.check(lib.exo_running_location_f64(y.data_ptr(), 0 if exclude is None else exclude.data_ptr(),
                                                0 if exclude is None else exclude.shape[0], N, B, plan.lo.data_ptr(), plan.hi.data_ptr(),
                                                plan.edge.data_ptr(), plan.max_window, _METHODS[method], float(cval), int(n_iter),
                                                trend.data_ptr(), 0 if scale is None else scale.data_ptr(), _stream(t)),
                   "exo_running_location_f64")
    if not batched:
        trend, scale = trend[0], None if scale is None else scale[0]
    return (trend, scale) if return_scale else trend


def flatten(t, y, window_length, *, return_trend=False, **kwargs):
    """Remove the slow variability of a light curve before the period search: ``y / trend`` with ``trend`` the
    :func:`running_location` of ``y`` over windows of ``window_length`` (``kwargs``: its ``method``, ``exclude``,
    ``break_tolerance``, ``edge_cutoff``, ``cval``, ``n_iter``, ``order``, ``rescale``).  ``t`` sorted, (N,); ``y`` (N,) or (B, N);
    numpy arrays or tensors in, numpy out.  A window some three times the longest transit keeps the transits' depth; ``exclude``
    masks the transits already found before a second search.  ``order=2`` follows the variability's extrema and the ramps at
    a segment's ends with a window twice as long, e.g. ``flatten(t, y, 1.5, order=2, break_tolerance=0.5)``.  With
    ``return_trend``: ``(flat, trend)``."""
    dev = _device_of(t, y)
    if "exclude" in kwargs and kwargs["exclude"] is not None:
        kwargs["exclude"] = torch.as_tensor(kwargs["exclude"], dtype=torch.bool, device=dev)
    yd = _to(y, dev)
    trend = running_location(_to(t, dev), yd, window_length, **kwargs)
    flat = _np(yd / trend)
    return (flat, _np(trend)) if return_trend else flat


def sde(power, window=151):
    """Signal detection efficiency of a periodogram ``power`` (P,): ``(power - trend) / std(power - trend)`` with ``trend`` the
    running median of ``power`` over ``window`` grid points (the same kernel on the index axis) and the population standard
    deviation over the finite entries.  Entries that are ``-inf`` or NaN (periods without a fit) take no part and come back
    NaN.  A device tensor gives a device tensor; anything else a numpy array."""
    if int(window) != window or window < 1:
        raise ValueError(f"window must be an integer >= 1, got {window}")
    as_tensor = isinstance(power, torch.Tensor) and power.is_cuda
    p = _to(power, _device_of(power))
    if p.ndim != 1 or p.numel() < 1:
        raise ValueError(f"power must have shape (P,), got {tuple(p.shape)}")
    out = ~torch.isfinite(p)
    axis = torch.arange(p.numel(), dtype=torch.float64, device=p.device)
    trend = running_location(axis, torch.where(out, torch.zeros_like(p), p), float(window - 1), method="median", exclude=out)
    resid = p - trend
    ok = torch.isfinite(resid) & ~out
    r = resid[ok]
    res = torch.where(ok, resid / torch.sqrt(((r - r.mean()) ** 2).mean()), torch.full_like(p, float("nan")))
    return res if as_tensor else _np(res)


# ---- the transits one by one: times and depths -----------------------------------------------------------------------------------

MAX_TIMING_WINDOW = 4096     # EXO_TIMING_MAX_WINDOW: cadences in one transit's window
MAX_TIMING_TEMPLATE = 1024   # EXO_TIMING_MAX_TEMPLATE: bins of the template
MAX_TIMING_SHIFTS = 4097     # EXO_TIMING_MAX_SHIFTS: trial shifts
TIMING_FIELDS = ("transit_time", "shift", "time_err", "depth", "depth_err", "log_likelihood", "depth_snr")
TIMING_COUNTS = ("n_window", "n_in", "valid", "at_edge")


class TimingPlan:
    """The transits of a linear ephemeris on one time axis, from :func:`timing_plan`: ``transit_ind`` (host int64, (K,): the
    epoch numbers ``n_k``) and its device copy ``epochs``, the device tensors ``linear_time`` (``T_k = t0 + period n_k``), ``lo`` and
    ``hi`` (int32: transit k's window is the cadences ``lo[k] .. hi[k]``, both included) and ``shifts`` (M,), the widest window
    ``max_window`` in cadences, a Python int, and the numbers it was made with."""

    __slots__ = ("period", "t0", "duration", "max_shift", "n_shift", "window", "transit_ind", "epochs", "linear_time", "lo", "hi",
                 "shifts", "max_window", "n", "device")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return (f"TimingPlan(transits={len(self.transit_ind)}, n_shift={self.n_shift}, max_window={self.max_window}, n={self.n}, "
                f"device={self.device})")


def _timing_numbers(period, t0, duration, max_shift, n_shift, window):
    for name, v in (("period", period), ("t0", t0), ("duration", duration)):
        if v is None:
            raise ValueError(f"the per-transit fit needs {name} (or a plan)")
    period, t0, duration = float(period), float(t0), float(duration)
    if not period > 0:
        raise ValueError(f"period must be positive, got {period}")
    if not np.isfinite(t0):
        raise ValueError(f"t0 must be finite, got {t0}")
    if not duration > 0:
        raise ValueError(f"duration must be positive, got {duration}")
    max_shift = duration / 2 if max_shift is None else float(max_shift)
    if not max_shift >= 0:
        raise ValueError(f"max_shift must be at least 0, got {max_shift}")
    window = 3 * duration + 2 * max_shift if window is None else float(window)
    if not window >= duration + 2 * max_shift:
        raise ValueError(f"window must hold the template at every shift: at least duration + 2 max_shift = {duration + 2 * max_shift}, "
                         f"got {window}")
    if int(n_shift) != n_shift or n_shift < 3 or n_shift % 2 == 0:
        raise ValueError(f"n_shift must be an odd integer >= 3, got {n_shift}")
    if n_shift > MAX_TIMING_SHIFTS:
        raise ValueError(f"n_shift = {n_shift}: more than the {MAX_TIMING_SHIFTS} shifts a call takes (EXO_TIMING_MAX_SHIFTS)")
    return period, t0, duration, max_shift, int(n_shift), window


def timing_plan(t, period, t0, duration, max_shift=None, n_shift=201, window=None, check_sorted=True):
    """The transits of the linear ephemeris ``t0 + period n`` on the device time axis ``t`` (N,), finite and non-decreasing, and
    their windows for :func:`transit_times`: every integer ``n`` with ``t0 + period n`` inside ``[t[0] - window / 2, t[-1] +
    window / 2]``, and for each the cadences with ``|t_i - T_k| <= window / 2``.  ``duration``: first to fourth contact, as in
    :func:`transit_template`.  The ``n_shift`` (odd) trial shifts of a mid-time run from ``-max_shift`` to ``max_shift`` (default
    ``duration / 2``); ``window`` defaults to ``3 duration + 2 max_shift``, one duration of baseline beyond the furthest position of
    the template on each side.  Returns a :class:`TimingPlan`; no epoch in range gives one without transits.

    This is the one synchronisation of the per-transit fit: ``t[0]`` and ``t[-1]``, the widest window (the kernel's LDS is sized
    by it) and, with ``check_sorted``, whether ``t`` is sorted and finite are read back.  ValueError: an unsorted ``t``, or a
    window of more than ``MAX_TIMING_WINDOW`` cadences."""
    _time_axis(t)
    period, t0, duration, max_shift, n_shift, window = _timing_numbers(period, t0, duration, max_shift, n_shift, window)
    t = t.to(torch.float64).contiguous()
    n = t.numel()
    first, last = (float(v) for v in torch.stack([t[0], t[-1]]).cpu())
    if not (np.isfinite(first) and np.isfinite(last)):
        raise ValueError("t must be finite and non-decreasing (sort the series first)")
    a, b = first - window / 2, last + window / 2
    cand = np.arange(int(np.floor((a - t0) / period)) - 1, int(np.ceil((b - t0) / period)) + 2, dtype=np.int64)
    T_k = t0 + period * cand.astype(np.float64)
    transit_ind = cand[(T_k >= a) & (T_k <= b)]
    K = transit_ind.size
    h = 2.0 * max_shift / (n_shift - 1)
    _, shifts = _grid(-max_shift + np.arange(n_shift, dtype=np.float64) * h, "shifts", t.device)
    epochs = torch.as_tensor(transit_ind, device=t.device)
    linear_time = torch.empty(K, dtype=torch.float64, device=t.device)
    lo = torch.empty(K, dtype=torch.int32, device=t.device)
    hi = torch.empty(K, dtype=torch.int32, device=t.device)
    info = torch.zeros(2, dtype=torch.int32, device=t.device)
    if K:
        lib = _lib.load()
        _lib.check(lib.exo_timing_windows_f64(t.data_ptr(), n, epochs.data_ptr(), K, period, t0, window, linear_time.data_ptr(),
                                              lo.data_ptr(), hi.data_ptr(), info.data_ptr(), _stream(t)), "exo_timing_windows_f64")
    widest = _plan_widest(info, t, check_sorted, MAX_TIMING_WINDOW, "EXO_TIMING_MAX_WINDOW", "window")
    return TimingPlan(period=period, t0=t0, duration=duration, max_shift=max_shift, n_shift=n_shift, window=window,
                      transit_ind=transit_ind, epochs=epochs, linear_time=linear_time, lo=lo, hi=hi, shifts=shifts,
                      max_window=max(widest, 1), n=n, device=t.device)


def transit_times(t, y, yerr=None, *, period=None, t0=None, duration=None, max_shift=None, n_shift=201, window=None, template=None,
                  ror=0.1, b=0.0, u=(0.4804, 0.1867), n_template=256, depth=None, min_in_transit=3, exclude=None, return_curve=False,
                  plan=None):
    """The mid-time and the depth of every single transit of ``y`` (N,) or (B, N) at times ``t`` (N,), finite and non-decreasing,
    around the linear ephemeris ``t0 + period n`` (definition: DESIGN.md section 20).  Device tensors in and out.

    In the window of transit k (see :func:`timing_plan` for ``duration``, ``max_shift``, ``n_shift`` and ``window``) the template
    -- ``template``, a finite array of at most ``MAX_TIMING_TEMPLATE`` samples at the bin centres of :func:`transit_template`, or
    None: ``transit_template(n_template, ror, b, u)`` -- is made continuous by linear interpolation and placed at every trial
    shift; the level and the depth of ``c - depth g`` are fitted by weighted least squares (weights ``1 / yerr^2``; ``yerr``: None, a
    scalar, (N,) or (B, N); ``exclude``: bool, (N,) or (B, N), cadences of weight 0, another planet's transits for instance), and
    ``log_likelihood`` is half the drop in chi-squared against a constant.  ``depth`` (a number or (B,)) holds the depth at that
    value instead; ``depth_err`` is then NaN.  A shift needs ``min_in_transit`` weighted cadences inside the template and one
    outside.  The highest shift is refined by the parabola through it and its neighbours, whose curvature is ``time_err``
    (a change of chi-squared by 1); a maximum at an end of the grid, beside a shift without a fit, or without curvature has
    ``at_edge`` set, ``shift`` the grid's and ``time_err`` NaN.

    Returns a :class:`BLSResult` of (K,) or (B, K) device tensors: ``transit_time`` (``linear_time + shift``), ``shift``, ``time_err``,
    ``depth``, ``depth_err``, ``log_likelihood``, ``depth_snr``, ``n_window`` and ``n_in`` (int32: the cadences of the window, and the
    weighted ones inside the template at the maximum), ``valid`` and ``at_edge`` (bool); ``transit_ind`` (K,), the epoch numbers
    ``n_k``, and ``linear_time`` (K,); with ``return_curve`` also ``curve`` (..., K, M), the log likelihood of every shift (``-inf``
    without a fit), and ``shifts`` (M,).  A transit without any fit is not ``valid`` and holds NaN (``n_in`` 0).

    With ``plan`` (a :class:`TimingPlan` of the same ``t``; ``period`` ... ``window`` are then not read) the call enqueues kernels
    only and may be captured into a graph, once the template is known (a host template is cached on the device by content).
    Bitwise reproducible; a row of a batch is bitwise the single call."""
    t, y, yerr, batched = _device_series(t, y, yerr)
    B, N = y.shape
    if int(min_in_transit) != min_in_transit or min_in_transit < 1:
        raise ValueError(f"min_in_transit must be an integer >= 1, got {min_in_transit}")
    if exclude is not None:
        exclude = _exclude_rows(exclude, B, N, t.device)
    if depth is not None:
        if isinstance(depth, torch.Tensor) and depth.ndim > 0:
            if not depth.is_cuda:
                raise ValueError(f"depth lives on {depth.device}: there is no CPU fallback")
            if tuple(depth.shape) not in ((1,), (B,)):
                raise ValueError(f"depth must be a number or have shape (B,) with B = {B}, got {tuple(depth.shape)}")
            depth = depth.to(device=t.device, dtype=torch.float64).contiguous()
        else:
            depth = torch.full((1,), float(depth), dtype=torch.float64, device=t.device)
    if template is None:
        if int(n_template) != n_template or not 1 <= n_template <= MAX_TIMING_TEMPLATE:
            raise ValueError(f"n_template must be an integer in [1, {MAX_TIMING_TEMPLATE}], got {n_template}")
        template = transit_template(int(n_template), ror, b, u)
    g_host, g_dev = _grid(template, "template", t.device)
    if not 1 <= g_host.size <= MAX_TIMING_TEMPLATE:
        raise ValueError(f"the template holds {g_host.size} bins: a call takes 1 to {MAX_TIMING_TEMPLATE} (EXO_TIMING_MAX_TEMPLATE)")
    if not np.all(np.isfinite(g_host)):
        raise ValueError(f"the template is not finite: {g_host[~np.isfinite(g_host)][:3]}")
    if plan is None:
        plan = timing_plan(t, period, t0, duration, max_shift=max_shift, n_shift=n_shift, window=window)
    else:
        _check_plan(plan, t)
    K, M = len(plan.transit_ind), plan.n_shift
    ivar = None
    if yerr is not None:
        ivar = 1.0 / yerr ** 2
    if exclude is not None:
        keep = (~exclude).to(torch.float64)
        ivar = keep if ivar is None else torch.where(exclude, torch.zeros_like(ivar), ivar)
    if ivar is not None:
        ivar = ivar.contiguous()
    out = torch.empty((7, B, K), dtype=torch.float64, device=t.device)
    iout = torch.empty((4, B, K), dtype=torch.int32, device=t.device)
    curve = torch.empty((B, K, M), dtype=torch.float64, device=t.device) if return_curve else None
    if K:
        lib = _lib.load()
        _lib.check(lib.exo_transit_timing_f64(t.data_ptr(), y.data_ptr(), 0 if ivar is None else ivar.data_ptr(),
                                              0 if ivar is None else ivar.shape[0], N, B, plan.linear_time.data_ptr(),
                                              plan.lo.data_ptr(), plan.hi.data_ptr(), K, plan.max_window, plan.duration, plan.max_shift,
                                              M, plan.window, g_dev.data_ptr(), g_host.size, 0 if depth is None else depth.data_ptr(),
                                              0 if depth is None else depth.numel(), int(min_in_transit), out.data_ptr(),
                                              iout.data_ptr(), 0 if curve is None else curve.data_ptr(), _stream(t)),
                   "exo_transit_timing_f64")
    res = BLSResult(transit_ind=plan.epochs, linear_time=plan.linear_time, **_fields(out, TIMING_FIELDS, batched))
    res.update(_fields((iout[0], iout[1], iout[2] != 0, iout[3] != 0), TIMING_COUNTS, batched))
    if return_curve:
        res.update(_fields((curve,), ("curve",), batched), shifts=plan.shifts)
    return res


def ttv_estimator(x, y, yerr=None, period=None, t0=None, duration=None, **kwargs):
    """Measure the time and the depth of every transit of one light curve around the linear ephemeris of a period search, and
    from them the two questions asked of a peak: do the times follow a line, and are odd and even transits equally deep?
    ``x`` sorted, (N,); ``y`` (N,); numpy arrays or tensors in, numpy arrays and Python floats out.  ``period``, ``t0`` and
    ``duration`` as :func:`bls_estimator` / :func:`tls_estimator` report them; ``kwargs``: those of :func:`transit_times`
    (``max_shift``, ``n_shift``, ``window``, ``ror``, ``b``, ``u``, ``template``, ``depth``, ``min_in_transit``, ``exclude`` ...).

    Returns ``timing`` (the arrays of :func:`transit_times`) and, over the transits that are valid and not at an edge of the
    grid: ``transit_times`` and ``transit_time_err``; ``transit_inds``, zero-based and counted from the first of them; ``period``
    and ``t0`` of the line through the times weighted by ``1 / time_err^2`` (``t0``: the line at index 0; fewer than two
    transits: the input's); ``ttvs``, observed minus that line; ``ttv_chi2 = sum (ttv / err)^2`` and ``ttv_dof``, the count less 2;
    ``depth_odd`` and ``depth_even``, the inverse-variance means of the depths over odd and even epoch numbers, and
    ``odd_even_sigma``, their difference over its error (NaN with a held depth or without transits of both kinds).

    The hand-over to a model with free transit times::

        res = ttv_estimator(x, y, yerr, period=peak["period"], t0=peak["transit_time"], duration=peak["duration"])
        orbit = TTVOrbit(transit_times=[res["transit_times"]], transit_inds=[res["transit_inds"]], b=..., duration=...)
    """
    dev = _device_of(x, y)
    if kwargs.get("exclude") is not None:
        kwargs["exclude"] = torch.as_tensor(kwargs["exclude"], dtype=torch.bool, device=dev)
    if isinstance(kwargs.get("depth"), np.ndarray):
        kwargs["depth"] = _to(kwargs["depth"], dev)
    yd = _to(y, dev)
    if yd.ndim != 1:
        raise ValueError(f"ttv_estimator takes one series, y of shape (N,), got {tuple(yd.shape)}")
    ed = _to(yerr, dev)
    res = transit_times(_to(x, dev), yd, ed if ed is None or ed.ndim else float(ed), period=period, t0=t0, duration=duration,
                        **kwargs)
    timing = BLSResult((k, v.cpu().numpy()) for k, v in res.items())
    use = timing["valid"] & ~timing["at_edge"]
    n_k = timing["transit_ind"][use]
    times, err = timing["transit_time"][use], timing["time_err"][use]
    inds = (n_k - n_k[0]) if n_k.size else n_k
    period_fit, t0_fit = float(period), float(times[0]) if n_k.size else float(t0)
    if n_k.size >= 2:
        wt = 1.0 / err ** 2
        ibar = (wt * inds).sum() / wt.sum()
        tbar = (wt * times).sum() / wt.sum()
        period_fit = float((wt * (inds - ibar) * (times - tbar)).sum() / (wt * (inds - ibar) ** 2).sum())
        t0_fit = float(tbar - period_fit * ibar)
    ttvs = times - (t0_fit + period_fit * inds)
    results = dict(timing=timing, transit_inds=inds.astype(np.int64), transit_times=times, transit_time_err=err, period=period_fit,
                   t0=t0_fit, ttvs=ttvs, ttv_chi2=float(((ttvs / err) ** 2).sum()), ttv_dof=int(n_k.size) - 2)
    means = {}
    for name, odd in (("odd", 1), ("even", 0)):
        sel = timing["valid"] & (timing["transit_ind"] % 2 == odd) & np.isfinite(timing["depth_err"])
        wd = 1.0 / timing["depth_err"][sel] ** 2
        means[name] = ((wd * timing["depth"][sel]).sum() / wd.sum(), 1.0 / wd.sum()) if sel.any() else (float("nan"), float("nan"))
        results[f"depth_{name}"] = float(means[name][0])
    results["odd_even_sigma"] = float((means["odd"][0] - means["even"][0]) / np.sqrt(means["odd"][1] + means["even"][1]))
    return results


def _span(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    return float(t.max() - t.min())


def bls_autoperiod(t, durations, minimum_period=None, maximum_period=None, minimum_n_transit=3, frequency_factor=1.0):
    """The box search's period grid, even in frequency with step ``frequency_factor * min(durations) / T^2``, from
    ``maximum_period`` (default ``T / (minimum_n_transit - 1)``) down to ``minimum_period`` (default ``2 max(durations)``);
    returned shortest period first.  A numpy array."""
    durations = np.atleast_1d(np.asarray(durations, dtype=np.float64))
    if not np.all(durations > 0):
        raise ValueError("durations must be positive")
    T = _span(t)
    if not T > 0:
        raise ValueError("the times span no baseline")
    if minimum_n_transit < 2:
        raise ValueError("minimum_n_transit must be at least 2")
    df = frequency_factor * durations.min() / T ** 2
    if maximum_period is None:
        maximum_period = T / (minimum_n_transit - 1)
    if minimum_period is None:
        minimum_period = 2.0 * durations.max()
    if not 0 < minimum_period <= maximum_period:
        raise ValueError("need 0 < minimum_period <= maximum_period")
    f_hi, f_lo = 1.0 / minimum_period, 1.0 / maximum_period
    n = 1 + int(np.round((f_hi - f_lo) / df))
    return 1.0 / (f_hi - df * np.arange(n))


def lomb_scargle_autofrequency(t, samples_per_peak=5, nyquist_factor=5, minimum_frequency=None, maximum_frequency=None):
    """The periodogram's frequency grid: step ``1 / (T samples_per_peak)`` from ``minimum_frequency`` (default half a step) to
    ``maximum_frequency`` (default ``nyquist_factor`` times the mean Nyquist frequency ``N / 2T``).  A numpy array."""
    T = _span(t)
    if not T > 0:
        raise ValueError("the times span no baseline")
    n_t = t.numel() if isinstance(t, torch.Tensor) else np.asarray(t).size
    df = 1.0 / (T * samples_per_peak)
    if minimum_frequency is None:
        minimum_frequency = 0.5 * df
    if maximum_frequency is None:
        maximum_frequency = nyquist_factor * 0.5 * n_t / T
    n = 1 + int(np.round((maximum_frequency - minimum_frequency) / df))
    return minimum_frequency + df * np.arange(n)


# ---- the reference's estimators -------------------------------------------------------------------------------------------------

def find_peaks(freq, power, max_peaks=0):
    """Local maxima of a periodogram, highest first, each refined by the parabola through the three ``log(power)`` samples
    around it.  ``max_peaks = 0``: the highest peak as a dictionary ``index, log_power, period, period_uncert`` (ValueError if
    there is none); ``max_peaks > 0``: a list of at most that many."""
    freq, power = _np(freq), _np(power)
    inner = power[1:-1]
    inds = np.arange(1, len(power) - 1)[(inner > power[:-2]) & (inner > power[2:])]
    inds = inds[np.argsort(power[inds])][::-1]
    peaks = []
    for i in inds[: max(1, max_peaks)]:
        w = np.linalg.solve(np.vander(freq[i - 1:i + 2], 3), np.log(power[i - 1:i + 2]))
        sigma2 = -0.5 / w[0]
        freq0 = w[1] * sigma2
        peaks.append(dict(index=int(i + 1), log_power=float(w[2] + 0.5 * freq0 ** 2 / sigma2), period=float(1.0 / freq0),
                          period_uncert=float(np.sqrt(sigma2 / freq0 ** 4))))
    if max_peaks:
        return peaks
    if not peaks:
        raise ValueError("no peaks were found")
    return peaks[0]


def _estimator_periods(xc, durations, min_period, max_period, minimum_n_transit, frequency_factor):
    """the period grid of the transit estimators; ``frequency_factor=None``: doubled until there are no more periods than cadences"""
    grid = lambda ff: bls_autoperiod(xc, durations, minimum_period=min_period, maximum_period=max_period,  # noqa: E731
                                     minimum_n_transit=minimum_n_transit, frequency_factor=ff)
    if frequency_factor is not None:
        return grid(frequency_factor)
    frequency_factor = 1.0
    periods = grid(frequency_factor)
    while len(periods) > len(xc):
        frequency_factor *= 2
        periods = grid(frequency_factor)
    return periods


def _estimator_front(x, y, yerr, duration, min_period, max_period, minimum_n_transit, frequency_factor):
    """What the two transit estimators do before the search.  -> ``x_ref``, the middle of the times; the times about it, the
    series less its median and ``yerr`` as device tensors; and ``periods`` and ``durations``, the search's grid"""
    dev = _device_of(x, y)
    xh = _np(x)
    x_ref = 0.5 * (xh.min() + xh.max())
    durations = np.atleast_1d(np.asarray(duration, dtype=np.float64))
    periods = _estimator_periods(xh - x_ref, durations, min_period, max_period, minimum_n_transit, frequency_factor)
    yd = _to(y, dev)
    return x_ref, _to(xh - x_ref, dev), yd - torch.median(yd), _to(yerr, dev), dict(periods=periods, durations=durations)


def _estimator_back(res, x_ref, objective, **spectra):
    """... and after it.  -> the periodogram as numpy arrays, its transit times on the input's axis again, with ``spectra`` and
    ``objective`` added; and its peaks (at most one)"""
    pg = BLSResult((k, _np(v)) for k, v in res.items())
    pg["transit_time"] = pg["transit_time"] + x_ref
    pg.update(spectra, objective=objective)
    return pg, find_peaks(1.0 / pg["period"], pg["power"], max_peaks=1)


def bls_estimator(x, y, yerr=None, duration=0.2, min_period=None, max_period=None, objective=None, method=None, oversample=10,
                  frequency_factor=None, minimum_n_transit=3):
    """Estimate the period of a transit signal by box least squares.  Returns ``bls`` (the periodogram: numpy arrays under the
    keys of :class:`BLSResult`), ``peaks`` (at most one, from ``find_peaks(1 / period, power)``) and ``peak_info``.

    ``frequency_factor=None`` thins the grid as the reference does (doubled until there are no more periods than cadences), so
    that results compare; ``frequency_factor=1.0`` searches the full grid.  ``method`` is accepted and ignored."""
    objective = "likelihood" if objective is None else objective
    x_ref, td, yd, ed, grid = _estimator_front(x, y, yerr, duration, min_period, max_period, minimum_n_transit, frequency_factor)
    res = bls_power(td, yd, ed, oversample=oversample, objective=objective, **grid)
    pg, peaks = _estimator_back(res, x_ref, objective)
    results = dict(bls=pg, peaks=peaks, peak_info=None)
    if peaks:
        ind = peaks[0]["index"]
        results["peak_info"] = dict((k, float(v[ind])) for k, v in pg.items() if k != "objective")
    return results


def tls_estimator(x, y, yerr=None, duration=0.2, min_period=None, max_period=None, objective=None, oversample=10,
                  frequency_factor=None, minimum_n_transit=3, ror=0.1, b=0.0, u=(0.4804, 0.1867)):
    """Estimate the period, the mid-transit depth and from it the radius ratio of a transit signal by transit least squares:
    :func:`bls_estimator`'s twin on :func:`tls_power` with the :func:`transit_template` of ``ror``, ``b`` and ``u`` (the same grid
    and thinning rule, the median subtracted).  Returns ``tls`` (the periodogram: numpy arrays under the keys of
    :class:`BLSResult`, and ``sr`` and ``sde_spectrum``), ``peaks`` and ``peak_info``.

    ``sr = min chi2 / chi2(p)`` with ``chi2(p) = chi2_0 - 2 log_likelihood(p)``, ``chi2_0 = sum w (y - ybar)^2``, over the periods
    of finite power (NaN elsewhere); ``sde_spectrum = (sr - mean) / std``.  ``peak_info`` holds the periodogram's values at the
    peak, ``sde = (1 - mean) / std``, and ``ror`` from ``LimbDarkLightCurve(*u).get_ror_from_approx_transit_depth(depth, b)``: a
    starting value for ``r`` (NaN for a brightening)."""
    from .light_curves.limb_dark import LimbDarkLightCurve

    objective = "likelihood" if objective is None else objective
    x_ref, td, yd, ed, grid = _estimator_front(x, y, yerr, duration, min_period, max_period, minimum_n_transit, frequency_factor)
    res = tls_power(td, yd, ed, ror=ror, b=b, u=u, oversample=oversample, objective=objective, **grid)
    # the signal residue and its detection efficiency, over the periods with a fit
    w = torch.ones_like(yd) if ed is None else 1.0 / ed.expand_as(yd) ** 2
    chi2_0 = (w * (yd - (w * yd).sum() / w.sum()) ** 2).sum()
    chi2 = chi2_0 - 2.0 * res["log_likelihood"]
    ok = torch.isfinite(res["power"])
    nan = torch.full_like(chi2, float("nan"))
    sr = torch.where(ok, chi2[ok].min() / chi2, nan) if bool(ok.any()) else nan
    mean, std = sr[ok].mean(), sr[ok].std()
    pg, peaks = _estimator_back(res, x_ref, objective, sr=_np(sr), sde_spectrum=_np((sr - mean) / std))
    results = dict(tls=pg, peaks=peaks, peak_info=None)
    if peaks:
        ind = peaks[0]["index"] - 1           # (find_peaks counts from one: this is the grid's highest sample itself)
        info = dict((k, float(pg[k][ind])) for k in ("period",) + BLS_FIELDS)
        info["sde"] = float((1.0 - mean) / std)
        star = LimbDarkLightCurve(torch.tensor(u[0], dtype=torch.float64), torch.tensor(u[1], dtype=torch.float64))
        info["ror"] = float(star.get_ror_from_approx_transit_depth(torch.tensor(info["depth"], dtype=torch.float64),
                                                                   torch.tensor(float(b), dtype=torch.float64)))
        results["peak_info"] = info
    return results


def _period_bounds(kwargs, min_period, max_period):
    """``min_period`` / ``max_period`` into the keywords of :func:`lomb_scargle_autofrequency`, in place"""
    if min_period is not None:
        kwargs["maximum_frequency"] = 1.0 / min_period
    if max_period is not None:
        kwargs["minimum_frequency"] = 1.0 / max_period


def _grid_maxima(peaks, max_peaks, freq, power):
    """every peak of :func:`find_peaks` with the index ``i`` of the grid's local maximum itself, where a search's fit is read"""
    for peak in peaks if max_peaks else [peaks]:
        i = peak["index"] - 1                 # (find_peaks counts from one)
        assert 1 <= i < len(freq) - 1 and power[i] > power[i - 1] and power[i] > power[i + 1], peak
        yield peak, i


def _peak_false_alarms(results, peaks, raw, n, **kwargs):
    """``fap`` into every peak ((peak, i) pairs, ``i`` the grid index of its maximum) and ``power_levels`` into ``results``, in
    the normalisation of the estimators' ``periodogram`` (``/ n``), from :func:`false_alarm` on the same grid; ``raw``: the
    periodogram as the kernel gives it"""
    peaks = list(peaks)
    fa = false_alarm(power=raw[[i for _, i in peaks]], **kwargs)
    for (peak, _), fap in zip(peaks, fa["fap"]):
        peak["fap"] = float(fap)
    results["power_levels"] = {alpha: v / n for alpha, v in fa["power_levels"].items()}


def lomb_scargle_estimator(x, y, yerr=None, min_period=None, max_period=None, filter_period=None, max_peaks=2, n_resample=0,
                           replace=False, seed=0, **kwargs):
    """Estimate the period of a series from its Lomb-Scargle periodogram on the automatic grid (``kwargs``: those of
    :func:`lomb_scargle_autofrequency`).  Returns ``periodogram = (freq, power / len(x))`` and ``peaks``, found after the
    optional high-pass weight ``1 / sqrt(1 + (f0 / f)^6)``, ``f0 = 1 / filter_period``.  ``n_resample > 0``: every peak also
    carries ``fap``, the false-alarm probability of the unfiltered power at its grid maximum from that many resamplings
    (:func:`false_alarm` with ``replace`` and ``seed``), and the result ``power_levels`` ``{0.1, 0.01, 0.001: power}``, the
    lines to draw on ``periodogram``."""
    _period_bounds(kwargs, min_period, max_period)
    dev = _device_of(x, y)
    xh = _np(x)
    freq = lomb_scargle_autofrequency(xh, **kwargs)
    raw = _np(lomb_scargle_power(_to(xh, dev), _to(y, dev), _to(yerr, dev), frequencies=freq))
    power = raw / len(xh)
    power_est = np.array(power)
    if filter_period is not None:
        power = power / np.sqrt(1 + ((1.0 / filter_period) / freq) ** 6)
    results = dict(periodogram=(freq, power_est), peaks=find_peaks(freq, power, max_peaks=max_peaks))
    if n_resample:
        _peak_false_alarms(results, _grid_maxima(results["peaks"], max_peaks, freq, power), raw, len(xh), t=_to(xh, dev), y=_to(y, dev),
                           yerr=_to(yerr, dev), frequencies=freq, method="lomb_scargle", n_resample=n_resample, replace=replace,
                           seed=seed)
    return results


def keplerian_estimator(x, y, yerr=None, min_period=None, max_period=None, max_peaks=2, ecc=None, n_phase=64, instrument=None,
                        n_resample=0, replace=False, seed=0, **kwargs):
    """Estimate the period and the orbital elements of a radial-velocity signal from its Keplerian periodogram
    (:func:`keplerian_power`) on :func:`lomb_scargle_estimator`'s grid (``kwargs``: those of
    :func:`lomb_scargle_autofrequency`).  Returns ``periodogram = (freq, power / len(x))``, the normalisation of
    :func:`lomb_scargle_estimator`, and ``peaks`` from :func:`find_peaks`; each peak also carries ``ecc, omega, t_periastron,
    K, zero_point`` and ``power`` at the grid frequency of the local maximum itself (``power`` as in ``periodogram``;
    ``zero_point`` a float, or with ``instrument`` a list of one float per instrument).  They go straight into
    ``KeplerianOrbit(period=, ecc=, omega=, t_periastron=)`` and ``rv_log_likelihood(K=, zero_point=, instrument=)``.
    ``n_resample > 0``: every peak also carries ``fap`` and the result ``power_levels``, as in :func:`lomb_scargle_estimator`,
    from resamplings searched with the same grids (:func:`false_alarm`, ``method="keplerian"``)."""
    _period_bounds(kwargs, min_period, max_period)
    dev = _device_of(x, y)
    xh = _np(x)
    freq = lomb_scargle_autofrequency(xh, **kwargs)
    power, fit = keplerian_power(_to(xh, dev), _to(y, dev), _to(yerr, dev), frequencies=freq, ecc=ecc, n_phase=n_phase,
                                 instrument=instrument, return_fit=True)
    if power.ndim != 1:
        raise ValueError("keplerian_estimator takes one series: y must have shape (N,)")
    raw = _np(power)
    power = raw / len(xh)
    fit = {k: _np(v) for k, v in fit.items()}
    peaks = find_peaks(freq, power, max_peaks=max_peaks)
    for peak, i in _grid_maxima(peaks, max_peaks, freq, power):
        peak.update({k: float(fit[k][i]) for k in KEPLERIAN_FIT[:4]}, power=float(power[i]))
        peak["zero_point"] = float(fit["zero_point"][i, 0]) if instrument is None else [float(v) for v in fit["zero_point"][i]]
    results = dict(periodogram=(freq, power), peaks=peaks)
    if n_resample:
        _peak_false_alarms(results, _grid_maxima(peaks, max_peaks, freq, power), raw, len(xh), t=_to(xh, dev), y=_to(y, dev),
                           yerr=_to(yerr, dev), frequencies=freq, method="keplerian", n_resample=n_resample, replace=replace,
                           seed=seed, ecc=ecc, n_phase=n_phase, instrument=instrument)
    return results


def astrometric_estimator(t, rho, rho_err, theta, theta_err, min_period=None, max_period=None, periods=None, max_peaks=2, ecc=None,
                          n_phase=64, parallax=None):
    """Estimate the period and the orbital elements of a visual binary or a directly imaged companion from the astrometric
    orbit search (:func:`astrometric_power`) of its separations ``rho`` and position angles ``theta``.  The grid is
    ``lomb_scargle_autofrequency(t, samples_per_peak=10, minimum_frequency=1 / max_period, maximum_frequency=1 / min_period)``
    with the defaults ``max_period = 4 x baseline`` and ``min_period = 4 x baseline / N`` (astrometric orbits are often
    covered only in part); an explicit ``periods`` (descending, so that the frequencies ascend -- a logarithmic grid, say)
    overrides them.  Returns ``periodogram = (freq, power)`` and ``peaks`` from :func:`find_peaks`; each peak also carries
    ``period, ecc, t_periastron, omega, Omega, incl, a_angular`` (with ``parallax`` also ``a``), ``chi2`` and ``power`` at the
    grid frequency of the local maximum itself, ``period`` included (``period_refined`` keeps the parabola's).  They go straight into ``KeplerianOrbit(period=,
    t_periastron=, ecc=, omega=, Omega=, incl=, a=)`` and its ``astrometry_log_likelihood``."""
    th = _np(t)
    if periods is not None:
        freq = 1.0 / np.atleast_1d(_np(periods))
        if freq.ndim != 1 or freq.size < 3 or not np.all(np.diff(freq) > 0):
            raise ValueError("periods must be one-dimensional, descending and hold at least three periods")
    else:
        T = _span(th)
        if not T > 0:
            raise ValueError("the times span no baseline")
        max_period = 4.0 * T if max_period is None else max_period
        min_period = 4.0 * T / th.size if min_period is None else min_period
        if not 0 < min_period < max_period:
            raise ValueError("need 0 < min_period < max_period")
        freq = lomb_scargle_autofrequency(th, samples_per_peak=10, minimum_frequency=1.0 / max_period,
                                          maximum_frequency=1.0 / min_period)
    dev = _device_of(t, rho, theta)
    err = lambda e: _to(e, dev) if isinstance(e, (torch.Tensor, np.ndarray, list, tuple)) else e   # noqa: E731
    power, fit = astrometric_power(_to(th, dev), _to(rho, dev), err(rho_err), _to(theta, dev), err(theta_err), frequencies=freq,
                                   ecc=ecc, n_phase=n_phase, parallax=parallax, return_fit=True)
    if power.ndim != 1:
        raise ValueError("astrometric_estimator takes one series: rho and theta must have shape (N,)")
    power = _np(power)
    fit = {k: _np(v) for k, v in fit.items()}
    peaks = find_peaks(freq, power, max_peaks=max_peaks)
    keys = ("ecc", "t_periastron", "omega", "Omega", "incl", "a_angular") + (("a",) if parallax is not None else ()) + ("chi2",)
    for peak, i in _grid_maxima(peaks, max_peaks, freq, power):
        peak.update({k: float(fit[k][i]) for k in keys}, period_refined=peak["period"], period=float(1.0 / freq[i]),
                    power=float(power[i]))
    return dict(periodogram=(freq, power), peaks=peaks)


def autocorr_function(x):
    """The normalised autocorrelation function of a 1-D series (by FFT, zero padded to twice the next power of two)"""
    as_numpy = not isinstance(x, torch.Tensor)
    x = torch.atleast_1d(torch.as_tensor(x, dtype=torch.float64))
    if x.ndim != 1:
        raise ValueError("invalid dimensions for 1D autocorrelation function")
    n = 1
    while n < x.numel():
        n <<= 1
    f = torch.fft.fft(x - x.mean(), n=2 * n)
    acf = torch.fft.ifft(f * torch.conj(f))[: x.numel()].real
    acf = acf / acf[0]
    return acf.cpu().numpy() if as_numpy else acf


def _interp(xx, x, y):
    """numpy.interp for increasing x, in torch"""
    i = torch.searchsorted(x, xx, right=True).clamp(1, x.numel() - 1)
    x0, x1 = x[i - 1], x[i]
    return y[i - 1] + (y[i] - y[i - 1]) * ((xx - x0) / (x1 - x0)).clamp(0.0, 1.0)


def _gaussian_filter(a, sigma, truncate=4.0):
    """a Gaussian of standard deviation ``sigma`` samples, cut at ``truncate`` sigma, edges reflected (d c b a | a b c d | d c b a)"""
    if not sigma > 0:
        return a
    r = int(truncate * sigma + 0.5)
    k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=a.dtype, device=a.device) / sigma) ** 2)
    k = k / k.sum()
    idx = torch.arange(-r, a.numel() + r, device=a.device)
    period = 2 * a.numel()
    idx = idx % period
    idx = torch.where(idx >= a.numel(), period - 1 - idx, idx)
    return torch.nn.functional.conv1d(a[idx][None, None], k[None, None])[0, 0]


def autocorr_estimator(x, y, yerr=None, min_period=None, max_period=None, oversample=2.0, smooth=2.0, max_peaks=10):
    """Estimate the period of a series from the first (or, if higher, second) peak of its autocorrelation function.  The
    series is interpolated to an even grid ``oversample`` times finer than its closest cadences, and the function smoothed by
    a Gaussian of ``smooth * min_period``.  Returns ``autocorr = (tau, acor)`` and ``peaks`` (one entry or none)."""
    dev = _device_of(x, y)
    x, y = _to(x, dev), _to(y, dev)
    gap = float(torch.diff(x).min())
    if min_period is None:
        min_period = gap
    if max_period is None:
        max_period = float(x.max() - x.min())
    dx = gap / float(oversample)
    xx = torch.arange(float(x.min()), float(x.max()), dx, dtype=torch.float64, device=dev)
    tau = _np(xx - x[0])
    acor = _np(_gaussian_filter(autocorr_function(_interp(xx, x, y)), smooth * min_period / dx))
    inds = np.arange(1, len(acor) - 1)[(acor[1:-1] > acor[:-2]) & (acor[1:-1] > acor[2:])]
    inds = inds[tau[inds] >= min_period]
    result = dict(autocorr=(tau, acor), peaks=[])
    if len(inds) == 0 or tau[inds[0]] > max_period:
        return result
    if len(inds) > 1 and acor[inds[1]] > acor[inds[0]]:
        inds = inds[1:]
    if tau[inds[0]] > max_period:
        return result
    result["peaks"] = [dict(period=float(tau[inds[0]]), period_uncert=float("nan"))]
    return result


def _design_matrix(periods, t0s, x):
    two_pi = 2 * np.pi
    if t0s is not None:
        cols = [torch.cos(two_pi * (x - (t0s[i] - 0.25 * periods[i])) / periods[i]) for i in range(len(periods))]
    else:
        cols = [fn(two_pi * x / periods[i]) for i in range(len(periods)) for fn in (torch.sin, torch.cos)]
    return torch.stack(cols + [torch.ones_like(x)], dim=1)


def estimate_semi_amplitude(periods, x, y, yerr=None, t0s=None):
    """Estimate the radial-velocity semi-amplitude of each planet (m/s) by weighted linear least squares: a sine and a cosine per
    period and a constant, or, with the reference transit times ``t0s``, one cosine of known phase per planet.  A numpy array."""
    dev = _device_of(x, y)
    periods = np.atleast_1d(_np(periods))
    t0s = None if t0s is None else np.atleast_1d(_np(t0s))
    x, y = torch.atleast_1d(_to(x, dev)), torch.atleast_1d(_to(y, dev))
    ivar = torch.ones_like(y) if yerr is None else 1.0 / torch.atleast_1d(_to(yerr, dev)).expand_as(y) ** 2
    D = _design_matrix(periods, t0s, x)
    w = torch.linalg.solve(D.T @ (D * ivar[:, None]), D.T @ (y * ivar))[:-1]
    K = w if t0s is not None else torch.sqrt(w[::2] ** 2 + w[1::2] ** 2)
    return _np(K)


def estimate_minimum_mass(periods, x, y, yerr=None, t0s=None, m_star=1):
    """Estimate the minimum mass ``m sin i`` of each planet in Jupiter masses from :func:`estimate_semi_amplitude`, for a star of
    ``m_star`` solar masses and circular orbits: ``K / 28.4329 m/s * m_star^(2/3) * (P / yr)^(1/3)``."""
    periods = np.atleast_1d(_np(periods))
    K = estimate_semi_amplitude(periods, x, y, yerr=yerr, t0s=t0s)
    return K / 28.4329 * float(m_star) ** (2.0 / 3) * (periods / 365.25) ** (1.0 / 3)
