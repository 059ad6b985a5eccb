#!/usr/bin/env python
"""bench.py -- light-curve evaluations / s (value + gradient) at 150 000 cadences.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it
is launched under torch.distributed.run, one rank per GPU (RCCL).  Rank 0
prints ONE JSON line.

Default workload = BASELINE.json configs[1] ("C2"): single planet, e = 0.3,
omega = 1.1, P = 3.5 d, t0 = 1, b = 0.3, r = 0.1, (u1, u2) = (0.3, 0.2), 150 000
two-minute cadences, float64, cotangent gbar ~ N(0,1), use_in_transit=False: the
output is the DENSE flux array [draws][150 000]; every cadence is classified on
the device (binary search of the conjunction windows in the sorted time array),
the ~3 % that can overlap the stellar disk are solved (Kepler + solution vector
+ reverse sweep), the rest are written as zeros.  One
*evaluation* = forward flux for all 150 000 cadences of one posterior draw + the
VJP of gbar back to all orbit / limb-darkening parameters.  One *step* = one
pass of the hot path over a batch of `--draws-per-gpu` draws (base parameters x
(1 + 1e-3 N(0,1))): leaf parameters -> record-packing kernel (KeplerianOrbit
algebra + get_cl) -> window + run-enumeration + heavy + finish kernels (value +
VJP in one sweep; the heavy kernel zero-fills the dense flux array while it
solves) -> packing VJP -> leaf gradients, replayed as one hipGraph.  With N > 1
ranks each own their draws and exchange only the per-draw scalar (sum(gbar*flux),
or the log-likelihood of a GP config): ONE collective per step
(exoplanet_amd.distributed.LoglikeExchange), whose result -- the full vector of the
previous step -- is consumed inside the timed loop.

`--config c2|c3|c4|c5` selects the BASELINE config whose step is timed (`workload_c2` ..
`workload_c5` below build exactly the step each `extras` leg reports, and
tests/test_gpu_timed_config.py holds those same steps to the oracle):
  c2 (default)  weak scaling, `--draws-per-gpu` draws on every GPU;
  c3            C2 + SHO-term celerite GP log-likelihood, weak scaling;
  c4            4 planets, 200 000 cadences, `--global-draws` (default 512) draws sharded over the GPUs: strong scaling;
  c5            65 000 long cadences x 7 sub-exposures, secondary eclipse, 3-term GP (J = 6),
                `--global-draws` (default 1024) chains sharded over the GPUs: strong scaling.
`--global-draws G` fixes the total for any config.  Inputs are resident in HBM before the timed region.

Timing: `value` comes from EXACTLY --steps steps between barrier + synchronize
on both sides (max over ranks), after the un-timed setup steps and --warmup.

A plain run does only that: set up, warm up, time the --steps steps, print the
line (`roofline`, `cpu_baseline` null; `configs_ms` holds the timed config only).
`--full` adds everything else: the same W + K timed once before the setup steps
(`value_after_contract_warmup_only`), `timing` (median / p10 / p90 per step over
>= 100 steps and >= 2 s, SURVEY.md 8d, independently of --steps), the per-kernel
figures of `roofline`, the `extras` legs (C2, one GPU), the CPU baseline, and the
full record in a side file; --no-stats / --no-extras / --no-cpu-baseline drop
parts of it.

`--dump-outputs DIR`: after the timed steps, what the last of them computed --
the arrays the caller of the step receives -- goes to DIR/<name>.npy (float64;
dump_outputs below).  The inputs are seeded: the same arguments give the same
inputs on every run, so two builds can be compared output for output.
"""
import argparse
import ctypes
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_CAD = 150_000
CADENCE = 2.0 / 1440.0
SURVEY_BYTES_PER_UNIT = 24       # SURVEY.md 8d count: read t 8 + read gbar 8 + write flux 8 per (draw, cadence)
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md


def hip_runtime():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("libamdhip64 not found")


class HipEvents:
    """K (start, stop) hipEvent pairs recorded by the C ABI around the kernels of one sweep,
    on the stream they are launched on."""

    def __init__(self, k):
        self.hip = hip_runtime()
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.pairs = []
        for _ in range(k):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(a)) == 0
            assert self.hip.hipEventCreate(ctypes.byref(b)) == 0
            self.pairs.append((a, b))

    def handles(self, i):
        a, b = self.pairs[i]
        return a.value, b.value

    def times_ms(self):
        out = []
        for a, b in self.pairs:
            ms = ctypes.c_float()
            assert self.hip.hipEventElapsedTime(ctypes.byref(ms), a, b) == 0
            out.append(ms.value)
        return out

    def mean_ms(self):
        v = self.times_ms()
        return float(np.mean(v)), v


def quantiles(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"iters": int(ms.size), "median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)),
            "p90_ms": float(np.percentile(ms, 90)), "mean_ms": float(ms.mean())}


def stats_loop(fn, dev, n_iters, chunk=100):
    """per-step durations of n_iters back-to-back steps (torch events on the current stream: the
    steps are launched on it).  The count is fixed up front -- under torch.distributed every rank
    must issue the same number of collectives."""
    ms = []
    stream = torch.cuda.current_stream(dev)
    while len(ms) < n_iters:
        k = min(chunk, n_iters - len(ms))
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
        evs[0].record(stream)
        for i in range(k):
            fn(-1)
            evs[i + 1].record(stream)
        torch.cuda.synchronize(dev)
        ms.extend(evs[i].elapsed_time(evs[i + 1]) for i in range(k))
    return quantiles(ms)


def measured_traffic(n_draw):
    """HBM bytes per sweep from this round's committed PMC passes (profiles/r02_pmc.json: rocprofv3
    --pmc FETCH_SIZE / WRITE_SIZE in separate runs, FETCH doubled per the gfx950 note), scaled to
    this run's draw count.  A cross-reference, not a live measurement: None if the file is absent
    or was taken on another kernel generation."""
    try:
        import hashlib

        p = json.load(open(os.path.join(ROOT, "profiles", "r02_pmc.json")))
        src = os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_transit.hip")
        if p.get("kernel_source_sha256") != hashlib.sha256(open(src, "rb").read()).hexdigest():
            return None                      # the counters were taken on other kernels: say nothing rather than something stale
        tot = sum(2.0 * k["fetch_kib"] + k["write_kib"] for k in p["kernels"].values() if k.get("dispatches_fetch", 0) > 5)
        return {"bytes": tot * 1024.0 * n_draw / p["draws"], "source": "profiles/r02_pmc.json (same exo_transit.hip)",
                "draws_profiled": p["draws"]}
    except Exception:
        return None


def make_leaves(n_draw, seed, dev):
    """C2 base parameters x (1 + 1e-3 N(0,1)), one row per draw, as autograd leaves."""
    rng = np.random.default_rng(seed)
    base = dict(period=3.5, t0=1.0, b=0.3, ecc=0.3, omega=1.1, r=0.1, u1=0.3, u2=0.2)
    leaves = {}
    for k, v in base.items():
        x = v * (1 + 1e-3 * rng.normal(size=(n_draw, 1)))
        if k == "ecc":
            x = np.clip(x, 0.0, 0.95)
        if k in ("u1", "u2"):
            x = x[:, 0]
        leaves[k] = torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True)
    return leaves


_ONES = {}
# The step goes through torch.autograd (flux_dot + autograd.grad), as in rounds 1-4.  EXO_BENCH_ONE_CALL=1: the one-call
# value-and-gradient form instead (KeplerianOrbit.flux_value_and_grad: no autograd graph) -- the same three launches (packing +
# windows + enumeration, sweep, packing VJP) and the same numbers, bit for bit; timed as the extras leg `c2_one_call`
STEP_THROUGH_AUTOGRAD = os.environ.get("EXO_BENCH_ONE_CALL", "0") != "1"


def step(xo, ops, leaves, t, gbar, events=(None, None), use_in_transit=False, **kw):
    """one pass of the hot path over the batch: returns (flux, L[d], grads of the leaves).  The leaves go to the
    kernels as they are (KeplerianOrbit.flux_dot: column-form packing kernel -> sweep -> packing VJP with the
    cotangent of L folded in); the cotangent of L is a constant vector of ones (d sum(L) / d leaves)."""
    orbit = xo.KeplerianOrbit(period=leaves["period"], t0=leaves["t0"], b=leaves["b"], ecc=leaves["ecc"],
                              omega=leaves["omega"])
    if not STEP_THROUGH_AUTOGRAD:
        # value and gradient in ONE call of the library (round 5: KeplerianOrbit.flux_value_and_grad ->
        # exo_transit_flux_cols_vjp_f64): packing + windows + enumeration in one launch, the sweep, the packing VJP -- the same
        # launches and the same numbers, bit for bit, as the autograd form below (tests/test_gpu_cols.py)
        flux, L, g = orbit.flux_value_and_grad(leaves["r"], (leaves["u1"], leaves["u2"]), t, gbar, use_in_transit=use_in_transit,
                                               events=events, **kw)
        return flux, L, tuple(g[k] for k in leaves)
    flux, L = orbit.flux_dot(leaves["r"], (leaves["u1"], leaves["u2"]), t, gbar, use_in_transit=use_in_transit,
                             events=events, **kw)
    key = (L.shape[0], L.device)
    if key not in _ONES:
        _ONES[key] = torch.ones(L.shape[0], dtype=L.dtype, device=L.device)
    grads = torch.autograd.grad(L, list(leaves.values()), grad_outputs=_ONES[key])
    return flux, L, grads


# ------------------------------------------------------------------------------------------
# The BASELINE configs as steps: what `--config` times, what the `extras` legs report, and what
# tests/test_gpu_timed_config.py checks against the oracle -- one definition each.
# ------------------------------------------------------------------------------------------
class Workload:
    """One BASELINE config on one rank: `fn(*leaves)` is a value + gradient step over `D` draws; its output
    `scalar_index` is the per-draw scalar the ranks exchange (sum(gbar * flux) or the log-likelihood), outputs after
    `grads_from` are the leaf gradients in the order of `names`."""

    def __init__(self, key, label, D, n_cad, names, leaves, fn, scalar_index, grads_from, survey_bytes_per_unit, data, step_text):
        self.key, self.label, self.D, self.n_cad = key, label, D, n_cad
        self.names, self.leaves, self.fn = names, leaves, fn
        self.scalar_index, self.grads_from = scalar_index, grads_from
        self.survey_bytes_per_unit = survey_bytes_per_unit
        self.data = data          # the fixed inputs (t, gbar / yobs, ...), for the parity tests
        self.step_text = step_text


def workload_c2(xo, ops, dev, D, rank=0, events=None):
    """BASELINE configs[1] (module docstring).  `events`: a HipEvents object -> `fn.eager(i)` records pair i around the sweep."""
    t = ops.vouch_sorted(torch.arange(N_CAD, dtype=torch.float64, device=dev) * CADENCE)   # (a fixed series: the caller's word)
    gbar = torch.as_tensor(np.random.default_rng(2 + rank).normal(size=(D, N_CAD)), device=dev)
    leaves = make_leaves(D, 100 + rank, dev)
    names = list(leaves)

    def fn(*vals):
        flux, L, grads = step(xo, ops, dict(zip(names, vals)), t, gbar)
        return (flux, L) + tuple(grads)

    return Workload("c2", "BASELINE configs[1] (C2): single planet e=0.3 Kepler solve + quadratic limb-darkened transit, "
                    "150000 cadences, value+grad, use_in_transit=False: dense flux output", D, N_CAD, names,
                    list(leaves.values()), fn, 1, 2, SURVEY_BYTES_PER_UNIT, dict(t=t, gbar=gbar, leaves=leaves),
                    "leaf params (separate tensors, read in place) -> ONE launch packs the records (orbit algebra + get_cl), works out "
                    "the windows and enumerates the runs -> the sweep (value + VJP; at >= 512 draws its blocks finish their own "
                    "draws, a separate finish kernel below that) -> packing VJP kernel -> leaf gradients: three launches (four below "
                    "512 draws); through torch.autograd (flux_dot + autograd.grad)")


# the light curve that is the mean of a GP travels between the two ops as a [cadence][draw] array (get_light_curve's
# cadence_major: same values, the layout the celerite kernels read with contiguous accesses); EXO_BENCH_ROW_MAJOR=1: A/B
GP_MEAN_CADENCE_MAJOR = os.environ.get("EXO_BENCH_ROW_MAJOR", "0") != "1"
# ... or, round 5, as the sweep's SPARSE output -- the runs of cadences a planet can overlap the disk in + the flux of those
# cadences (get_light_curve's sparse=True): the celerite kernels read the segments, the dense (draw, cadence) array and its
# cotangent never exist.  Offered for one list per draw (C3); C5 (transits + occultations) gets the cadence-major array back.
# EXO_BENCH_DENSE_MEAN=1: A/B
GP_MEAN_SPARSE = os.environ.get("EXO_BENCH_DENSE_MEAN", "0") != "1" and GP_MEAN_CADENCE_MAJOR
C3_HYPER = (1e-3, 5.0, 0.7071)       # SHOTerm(sigma, rho, Q) of SURVEY.md 8d C3


def workload_c3(xo, ops, dev, D, rank=0):
    """BASELINE configs[2] (C3): the C2 light curve + a celerite SHO-term GP log-likelihood on the residual; value +
    gradient w.r.t. the orbit / limb-darkening leaves and the kernel hyper-parameters (sigma, rho, Q) per draw"""
    t = ops.vouch_sorted(torch.arange(N_CAD, dtype=torch.float64, device=dev) * CADENCE)   # (a fixed series: the caller's word)
    yobs = torch.as_tensor(5e-4 * np.random.default_rng(3).normal(size=N_CAD), device=dev)     # (the data: same on every rank)
    leaves = make_leaves(D, 100 + rank, dev)
    for k, v in zip(("sigma", "rho", "Q"), C3_HYPER):
        leaves[k] = torch.full((D,), v, dtype=torch.float64, device=dev, requires_grad=True)
    names = list(leaves)

    def fn(*vals):
        Lv = dict(zip(names, vals))
        orbit = xo.KeplerianOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"])
        lc = xo.LimbDarkLightCurve(Lv["u1"], Lv["u2"]).get_light_curve(orbit=orbit, r=Lv["r"], t=t, total=True,
                                                                      cadence_major=GP_MEAN_CADENCE_MAJOR, sparse=GP_MEAN_SPARSE)
        gp = xo.gp.GaussianProcess(xo.gp.terms.SHOTerm(sigma=Lv["sigma"], rho=Lv["rho"], Q=Lv["Q"]), t=t, yerr=5e-4, mean=lc)
        ll = gp.log_likelihood(yobs)
        return (ll.detach(),) + torch.autograd.grad(ll.sum(), vals)

    J = 2
    return Workload("c3", "BASELINE configs[2] (C3): the C2 system + celerite SHOTerm GP log-likelihood (J = 2) on the residual, "
                    "150000 cadences, value+grad of every leaf incl. (sigma, rho, Q) per draw", D, N_CAD, names,
                    list(leaves.values()), fn, 0, 1, 48 + 16 * (1 + J + J * J), dict(t=t, yobs=yobs, yerr=5e-4, leaves=leaves),
                    "packing -> light-curve sweep into its sparse output (runs + values; no dense flux) -> SHO coefficients -> celerite "
                    "in parallel over time reading the segments (elements, scan trees, chunk recurrences) -> its reverse, the "
                    "cotangent written at the values -> light-curve VJP sweep on the same runs -> packing VJP")


C4_BASE = dict(period=[3.5, 7.9, 13.1, 29.7], t0=[1.0, 2.3, 5.1, 11.7], b=[0.3, 0.1, 0.5, 0.2],
               ecc=[0.05, 0.1, 0.2, 0.3], omega=[1.1, -0.4, 2.0, 0.3], r=[0.1, 0.05, 0.07, 0.03])
C4_NCAD = 200_000


def workload_c4(xo, ops, dev, D, rank=0):
    """BASELINE configs[3] (C4): 4 planets, 200 000 cadences, dense summed flux, value + gradient of all 4 x 6 + 2 leaves
    per draw; D = this rank's share of the 512 draws (64 on each of 8 GPUs)"""
    rng = np.random.default_rng(4 + 1000 * rank)
    n = C4_NCAD
    t = ops.vouch_sorted(torch.arange(n, dtype=torch.float64, device=dev) * CADENCE)
    leaves = {}
    for k, v in C4_BASE.items():
        x = np.asarray(v)[None, :] * (1 + 1e-3 * rng.normal(size=(D, 4)))
        if k == "ecc":
            x = np.clip(x, 0.0, 0.95)
        leaves[k] = torch.tensor(x, dtype=torch.float64, device=dev, requires_grad=True)
    leaves["u1"] = torch.full((D,), 0.3, dtype=torch.float64, device=dev, requires_grad=True)
    leaves["u2"] = torch.full((D,), 0.2, dtype=torch.float64, device=dev, requires_grad=True)
    gbar = torch.as_tensor(rng.normal(size=(D, n)), device=dev)
    names = list(leaves)

    def fn(*vals):
        flux, L, grads = step(xo, ops, dict(zip(names, vals)), t, gbar)
        return (flux, L) + tuple(grads)

    return Workload("c4", "BASELINE configs[3] (C4): 4-planet system, 200000 cadences, value+grad, dense summed flux", D, n, names,
                    list(leaves.values()), fn, 1, 2, SURVEY_BYTES_PER_UNIT, dict(t=t, gbar=gbar, leaves=leaves),
                    "as C2, four planets per draw in one sweep")


C5_BASE = dict(period=2.7, t0=0.4, b=0.2, ecc=0.1, omega=0.7, r=0.08)
C5_NCAD, C5_TEXP = 65_000, 29.4 / 1440.0
C5_TERMS = ((4e-4, 20.0, 2.0), (3e-4, 10.0, 1.0), (2e-4, 2.0, 0.7071))      # (sigma, rho, Q) of the three SHO terms
C5_LD = ((0.3, 0.2), (0.4, 0.1))
C5_YERR = 3e-4


def workload_c5(xo, ops, dev, D, rank=0, bright=0, bright_factor=1e3, kernel="sho3", mean_sparse=False):
    """BASELINE configs[4] (C5): 65 000 long cadences, exposure stencil x 7, secondary eclipse, three SHO terms (J = 6);
    D = this rank's share of the 1024 chains (128 on each of 8 GPUs).  bright (extras only): that many chains with the first
    term's amplitude at 1000 x the error bars -- a conditioning score of 1e6, above the 3e4 of the scan trees: those chains
    take the robust route of the time-parallel path (exo_celerite_core.hpp, chunk_adj_lane); bright_factor: that amplitude in
    error bars (1e3: score 1e6; 10^4.5: score 1e9 -- beyond the robust route, the sequential kernels).
    kernel = "rot2_sho" (extras only): two RotationTerms + one SHO term -- J = 10, the width celerite2 users
    reach with two spotted stars / a harmonic pair: wider than the one-lane time-parallel kernels (J <= 8 here)"""
    rng = np.random.default_rng(5 + 1000 * rank)
    n, texp = C5_NCAD, C5_TEXP
    t = ops.vouch_sorted(torch.arange(n, dtype=torch.float64, device=dev) * texp)
    mk = lambda v: torch.tensor(v * (1 + 1e-3 * rng.normal(size=(D, 1))), dtype=torch.float64, device=dev,  # noqa: E731
                                requires_grad=True)
    leaves = {k: mk(v) for k, v in C5_BASE.items()}
    vec = lambda v: torch.full((D,), v, dtype=torch.float64, device=dev, requires_grad=True)  # noqa: E731
    leaves.update(sbr=vec(0.3), s1=vec(C5_TERMS[0][0]), s2=vec(C5_TERMS[1][0]), s3=vec(C5_TERMS[2][0]))
    if bright:
        s1 = np.full(D, C5_TERMS[0][0])
        s1[:bright] = bright_factor * C5_YERR
        leaves["s1"] = torch.tensor(s1, dtype=torch.float64, device=dev, requires_grad=True)
    yobs = torch.as_tensor(3e-4 * np.random.default_rng(5).normal(size=n), device=dev)       # (the data: same on every rank)
    ones = torch.ones(D, dtype=torch.float64, device=dev)
    fixed = [(rho * ones, Q * ones) for _, rho, Q in C5_TERMS]     # (rho, Q) of the three terms: fixed, per chain
    names = list(leaves)
    T = xo.gp.terms

    def fn(*vals):
        Lv = dict(zip(names, vals))
        orbit = xo.KeplerianOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"])
        # the mean: the dense cadence-major array.  The merged sparse model (round 6: transit + occultation lists merged on
        # the device, ops.MergedSparseLightCurve) is the SLOWER route at this shape -- 2.05 against 1.87 ms, same box: over 1327
        # days the draws' 490 transits and occultations drift apart by half a period, so a wave of 64 chains is inside somebody's
        # segment nearly everywhere and pays the segment cursor for nothing -- `mean_sparse=True` (extras leg) keeps it on record
        lc = xo.SecondaryEclipseLightCurve(C5_LD[0], C5_LD[1], Lv["sbr"]).get_light_curve(
            orbit=orbit, r=Lv["r"], t=t, texp=texp, oversample=7, total=True, cadence_major=GP_MEAN_CADENCE_MAJOR,
            sparse=mean_sparse and GP_MEAN_SPARSE)
        if kernel == "sho4":         # (J = 8: the lane-group time-parallel path, for scale)
            kern = (T.SHOTerm(sigma=Lv["s1"], rho=fixed[0][0], Q=fixed[0][1]) + T.SHOTerm(sigma=Lv["s2"], rho=fixed[1][0], Q=fixed[1][1])
                    + T.SHOTerm(sigma=Lv["s3"], rho=fixed[2][0], Q=fixed[2][1]) + T.SHOTerm(sigma=0.5 * Lv["s3"], rho=0.7 * ones, Q=3.0 * ones))
        elif kernel == "rot2_sho":
            kern = (T.RotationTerm(sigma=Lv["s1"], period=9.0 * ones, Q0=1.5 * ones, dQ=0.4 * ones, f=0.6 * ones)
                    + T.RotationTerm(sigma=Lv["s2"], period=23.0 * ones, Q0=2.5 * ones, dQ=0.7 * ones, f=0.3 * ones)
                    + T.SHOTerm(sigma=Lv["s3"], rho=fixed[2][0], Q=fixed[2][1]))
        elif kernel == "rot3":       # (J = 12; tools only)
            kern = (T.RotationTerm(sigma=Lv["s1"], period=9.0 * ones, Q0=1.5 * ones, dQ=0.4 * ones, f=0.6 * ones)
                    + T.RotationTerm(sigma=Lv["s2"], period=23.0 * ones, Q0=2.5 * ones, dQ=0.7 * ones, f=0.3 * ones)
                    + T.RotationTerm(sigma=Lv["s3"], period=3.1 * ones, Q0=2.0 * ones, dQ=0.5 * ones, f=0.5 * ones))
        else:
            kern = (T.SHOTerm(sigma=Lv["s1"], rho=fixed[0][0], Q=fixed[0][1]) + T.SHOTerm(sigma=Lv["s2"], rho=fixed[1][0], Q=fixed[1][1])
                    + T.SHOTerm(sigma=Lv["s3"], rho=fixed[2][0], Q=fixed[2][1]))
        gp = xo.gp.GaussianProcess(kern, t=t, yerr=C5_YERR, mean=lc)
        ll = gp.log_likelihood(yobs)
        return (ll.detach(),) + torch.autograd.grad(ll.sum(), vals)

    J = 6
    return Workload("c5", "BASELINE configs[4] (C5): 65000 Kepler long cadences, exposure stencil x 7, SecondaryEclipseLightCurve + "
                    "3-term celerite GP (J = 6), value+grad", D, n, names, list(leaves.values()), fn, 0, 1,
                    48 + 16 * (1 + J + J * J), dict(t=t, yobs=yobs, yerr=C5_YERR, texp=texp, leaves=leaves),
                    "packing -> secondary-eclipse light-curve sweep (7 sub-exposures, transit + occultation) -> SHO coefficients "
                    "x 3 -> celerite (J = 6) in parallel over time -> reverse -> light-curve VJP sweep -> packing VJP")


WORKLOADS = {"c2": workload_c2, "c3": workload_c3, "c4": workload_c4, "c5": workload_c5}
DEFAULT_GLOBAL_DRAWS = {"c4": 512, "c5": 1024}       # BASELINE.json states C4 / C5 as totals over 8 GPUs


def exchange_step(exchange, L_local, pipelined=False):
    """the multi-GPU part of a step: one collective, every rank ends up with all per-draw scalars.
    ``pipelined``: the collective is issued asynchronously from a private copy of the rank's scalars and overlaps the
    next step's kernels (LoglikeExchange.start): the return value is then the PREVIOUS step's full vector (None on the
    first call), and the caller ends the loop with ``exchange.finish()``.
    (tests/test_distributed.py drives this function on CPU under gloo, world size 2.)"""
    if pipelined and not _SYNC_EXCHANGE[0]:
        try:
            return exchange.start(L_local)
        except RuntimeError as e:      # (a backend without asynchronous collectives: say so once, go on synchronously)
            print(f"bench.py: asynchronous exchange failed ({e}); using the synchronous collective", file=sys.stderr)
            _SYNC_EXCHANGE[0] = True
    return exchange(L_local)


def make_runner(step_fn, scalar_index, exchange, consume):
    """(run(i), drain()) of the timed loop for ANY config: one step of the rank's shard, then -- with several ranks -- the
    step's ONE collective of per-draw scalars, whose previous result is consumed; `drain` waits for the collective still
    in flight and consumes it (called inside the timed region).  tests/test_distributed.py drives this on CPU (gloo,
    world size 2) with a stand-in step."""
    def run(i):
        out = step_fn()
        if exchange is not None:
            consume(exchange_step(exchange, out[scalar_index], pipelined=True))

    def drain():
        if exchange is not None:
            consume(exchange.finish())

    return run, drain


class ExchangeConsumer:
    """what a sampler does with the exchanged vector, reduced to its cost: every step's full (n_global,) vector is
    folded into a running sum (cross-chain mean log-likelihood for adaptation and logging) on the device -- ONE small
    kernel per step, inside the timed region, so the timed step covers an exchange whose result is USED"""

    def __init__(self, n_global, dev):
        self.acc = torch.zeros(n_global, dtype=torch.float64, device=dev)
        self.steps = 0

    def __call__(self, full):
        if full is None:
            return
        self.acc.add_(full)
        self.steps += 1


_SYNC_EXCHANGE = [os.environ.get("EXO_BENCH_SYNC_EXCHANGE") == "1"]


def time_steps(fn, steps, warmup, dist, dev, drain=None):
    """``drain``: called after the last step, inside the timed region (collectives still in flight are waited for)"""
    for _ in range(warmup):
        fn(-1)
    if drain is not None:
        drain()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(steps):
        fn(i)
    if drain is not None:
        drain()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


# ------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1 only): the oracle's C port -- the thing being CHECKED AGAINST
# elsewhere, timed here beside the GPU number; never part of `value`.
# ------------------------------------------------------------------------------------------
def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def usable_cpus():
    """(threads this process can actually run at once, how that was decided): the affinity mask, capped by the
    cgroup CPU quota -- the GPU boxes show 256 logical cores but grant 16 cores' worth of time (cpu.max), and 256
    OpenMP threads on that only measure the throttling"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    why = f"affinity mask: {n} of {os.cpu_count()} logical cores"
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]          # cgroup v2
        quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        try:                                                                  # cgroup v1
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = q / per if q > 0 else None
        except (OSError, ValueError):
            pass
    if quota is not None and quota < n:
        n = max(1, int(quota))
        why = f"cgroup CPU quota: {quota:g} cores' worth of time on {os.cpu_count()} logical cores"
    return n, why


def cpu_baseline(budget_s=27.0, config="c2"):
    """oracle/c on the host cores of this box, on a bounded sample of the workload.  C2 (the headline):
    (i) 1 core, in-transit cadences only (the reference's default use_in_transit=True, and what the GPU sweep solves:
        the like-for-like leg = `value`);
    (ii) 1 core, every cadence evaluated (what the reference does with use_in_transit=False);
    (iii) / (iv) the same on all usable cores, one draw per thread (PyMC's one process per chain on every core).
    Then one leg each (1 core, all cores) for C3, C4 and C5: light curve value + VJP [+ celerite log-likelihood +
    gradient] per evaluation, the configs the `extras` legs time on the GPU."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import c_port as C
    from oracle import numpy_port as P

    # the library travels prebuilt; rebuild it for THIS host's cores (-march=native) when a compiler is here
    try:
        subprocess.run(["make", "-s", "-B", "-C", os.path.join(ROOT, "oracle", "c")], check=True, timeout=120,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    except Exception:
        pass
    lib = C.lib()
    usable, usable_why = usable_cpus()
    n_threads = int(os.environ.get("EXO_BENCH_CPU_THREADS", usable))
    rng = np.random.default_rng(2)

    def contact_window(orbit, r):
        """first / fourth contact relative to t0 (keplerian.py:744-763)"""
        Ml, Mr, flag = P.contact_points(orbit.a, orbit.ecc, orbit.cos_omega, orbit.sin_omega, orbit.cos_incl,
                                        orbit.sin_incl, orbit.r_star + r)
        assert np.all(flag == 0)
        hp = 0.5 * orbit.period
        ts = np.mod((Ml - orbit.M0) / orbit.n + hp, orbit.period) - hp
        te = np.mod((Mr - orbit.M0) / orbit.n + hp, orbit.period) - hp
        return np.where(ts > 0, ts - orbit.period, ts), np.where(te < 0, te + orbit.period, te)

    def records(orbit, r, n_draw, window, sbr=None):
        Pn = orbit.a.size
        rec = np.zeros((n_draw, Pn, P.NPAR))
        rec[:, :, P.P_N], rec[:, :, P.P_TP], rec[:, :, P.P_ECC] = orbit.n, orbit.t_periastron, orbit.ecc
        rec[:, :, P.P_COSW], rec[:, :, P.P_SINW] = orbit.cos_omega, orbit.sin_omega
        rec[:, :, P.P_COSI], rec[:, :, P.P_SINI] = orbit.cos_incl, orbit.sin_incl
        rec[:, :, P.P_AOR], rec[:, :, P.P_ROR] = orbit.a / orbit.r_star, r / orbit.r_star
        rec[:, :, P.P_T0], rec[:, :, P.P_PERIOD] = orbit.t0, orbit.period
        ts, te = contact_window(orbit, r) if window else (-np.inf, np.inf)
        rec[:, :, P.P_TS], rec[:, :, P.P_TE], rec[:, :, P.P_TS2], rec[:, :, P.P_TE2] = ts, te, -np.inf, np.inf
        if sbr is not None:
            rec[:, :, P.P_FRATIO] = sbr * (r / orbit.r_star) ** 2
        rec[:, :, P.P_ROR] *= 1 + 1e-3 * rng.normal(size=(n_draw, Pn))
        return rec

    def timed(call, n_per_call, seconds):
        call()  # warm
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            call()
            n += n_per_call
        dt = time.perf_counter() - t0
        return {"evals_per_s": n / dt, "evals": n, "seconds": dt}

    def c2_leg(n_draw, threads, window, seconds):
        lib.oracle_set_threads(int(threads))
        t = np.arange(N_CAD) * CADENCE
        orbit = P.KeplerianOrbit(period=3.5, t0=1.0, b=0.3, ecc=0.3, omega=1.1)
        rec = records(orbit, np.array([0.1]), n_draw, window)
        c = np.repeat(P.get_cl(0.3, 0.2)[None], n_draw, 0)
        g = rng.normal(size=(n_draw, N_CAD))
        out = timed(lambda: C.transit(t, rec, c, g, window=window), n_draw, seconds)
        out.update(threads=int(threads), semantics="in-transit cadences only (use_in_transit=True)" if window else
                   "every cadence solved (use_in_transit=False)")
        return out

    def gp_config_leg(which, threads, seconds):
        """C3 / C5: light curve value + VJP, then celerite log-likelihood + gradient of the residual, per draw; `threads`
        draws at once (the C port's light curve is OpenMP over draws; the celerite calls run in a thread pool: ctypes
        releases the GIL)"""
        lib.oracle_set_threads(int(threads))
        n_draw = int(threads)
        if which == "c3":
            n, kw, sec = N_CAD, {}, False
            t = np.arange(n) * CADENCE
            orbit = P.KeplerianOrbit(period=3.5, t0=1.0, b=0.3, ecc=0.3, omega=1.1)
            rec = records(orbit, np.array([0.1]), n_draw, True)
            c = np.repeat(P.get_cl(0.3, 0.2)[None], n_draw, 0)
            parts = [P.sho_coefficients(*P.sho_from_sigma_rho(*C3_HYPER), C3_HYPER[2])]
            yerr = 5e-4
        else:
            n, sec = C5_NCAD, True
            t = np.arange(n) * C5_TEXP
            orbit = P.KeplerianOrbit(**{k: v for k, v in C5_BASE.items() if k != "r"})
            rec = records(orbit, np.array([C5_BASE["r"]]), n_draw, True, sbr=0.3)
            c = np.repeat(np.concatenate([P.get_cl(*C5_LD[0]), P.get_cl(*C5_LD[1])])[None], n_draw, 0)
            sdt, sw = P.exposure_stencil(7, 0)
            kw = dict(texp=C5_TEXP, stencil_dt=sdt, stencil_w=sw, secondary=True)
            parts = [P.sho_coefficients(*P.sho_from_sigma_rho(sg, rho, q), q) for sg, rho, q in C5_TERMS]
            yerr = C5_YERR
        co = tuple(np.concatenate(x) for x in zip(*parts))
        y = yerr * rng.normal(size=n)
        diag = np.full(n, yerr * yerr)
        pool = ThreadPoolExecutor(max_workers=n_draw)

        def call():
            f, gp, gl = C.transit(t, rec, c, None, window=not sec, want_flux=True, **kw)
            res = list(pool.map(lambda d: C.celerite(t, y - f[d], diag, co, grad=True), range(n_draw)))
            gres = np.stack([-r[1]["y"] for r in res])
            C.transit(t, rec, c, gres, window=not sec, want_flux=False, **kw)

        out = timed(call, n_draw, seconds)
        pool.shutdown()
        out.update(threads=int(threads), semantics="light curve (in-transit cadences only) + celerite log-likelihood, value + "
                   "gradient" if not sec else "secondary-eclipse light curve (every cadence, 7 sub-exposures) + 3-term celerite "
                   "log-likelihood, value + gradient")
        return out

    def c4_leg(threads, seconds):
        lib.oracle_set_threads(int(threads))
        n_draw = int(threads)
        t = np.arange(C4_NCAD) * CADENCE
        orbit = P.KeplerianOrbit(**{k: np.array(v) for k, v in C4_BASE.items() if k != "r"})
        rec = records(orbit, np.array(C4_BASE["r"]), n_draw, True)
        c = np.repeat(P.get_cl(0.3, 0.2)[None], n_draw, 0)
        g = rng.normal(size=(n_draw, C4_NCAD))
        out = timed(lambda: C.transit(t, rec, c, g, window=True), n_draw, seconds)
        out.update(threads=int(threads), semantics="4 planets, in-transit cadences only, value + VJP")
        return out

    def guarded(fn, *a):
        try:
            return fn(*a)
        except Exception as exc:      # a leg must not take the record down with it
            return {"error": repr(exc)[:200]}

    share = budget_s / 10.0
    legs = {"one_core_in_transit": guarded(c2_leg, 1, 1, True, share),
            "one_core_every_cadence": guarded(c2_leg, 1, 1, False, share),
            "all_cores_in_transit": guarded(c2_leg, 4 * n_threads, n_threads, True, share),
            "all_cores_every_cadence": guarded(c2_leg, n_threads, n_threads, False, share),
            "c3_one_core": guarded(gp_config_leg, "c3", 1, share), "c3_all_cores": guarded(gp_config_leg, "c3", n_threads, share),
            "c4_one_core": guarded(c4_leg, 1, share), "c4_all_cores": guarded(c4_leg, n_threads, share),
            "c5_one_core": guarded(gp_config_leg, "c5", 1, share), "c5_all_cores": guarded(gp_config_leg, "c5", n_threads, share)}
    lib.oracle_set_threads(1)
    head = {"c2": "one_core_in_transit", "c3": "c3_one_core", "c4": "c4_one_core", "c5": "c5_one_core"}[config]
    one = legs[head]
    return {"value": one.get("evals_per_s"), "unit": "evals/s", "cores": 1, "kind": "port", "leg": head,
            "sample": f"{one.get('evals')} evaluations (value+VJP) of the {config.upper()} workload in {one.get('seconds', 0):.1f} s, oracle/c "
                      f"scalar port on 1 of {os.cpu_count()} host cores; {one.get('semantics')}",
            "sample_note": "the like-for-like leg: the GPU sweep solves only the cadences inside its conjunction windows too.  `legs`: "
                           f"every-cadence semantics, all {n_threads} usable cores ({usable_why}; one draw per thread), and C3 / C4 / C5",
            "cpu_model": cpu_model(), "host_cores": os.cpu_count(), "usable_cores": usable, "usable_cores_from": usable_why,
            "legs": legs,
            "note": "the reference's own Ops (exoplanet_core, celerite2) are not installable here: kind = port"}


# ------------------------------------------------------------------------------------------
# extras (single GPU diagnostics; never `value`)
# ------------------------------------------------------------------------------------------
def time_events(fn, dev, iters, warmup=2):
    """mean / quantiles of `fn` per call, torch events on the current stream"""
    for _ in range(warmup):
        fn()
    stream = torch.cuda.current_stream(dev)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    evs[0].record(stream)
    for i in range(iters):
        fn()
        evs[i + 1].record(stream)
    torch.cuda.synchronize(dev)
    return quantiles([evs[i].elapsed_time(evs[i + 1]) for i in range(iters)])


def extra_ops(ops, dev, n=150_000_000):
    """the reference's standalone Ops at n = 1.5e8 elements: GB/s against
    their algorithmic bytes -- kepler 2 in + 2 out = 32 B/elt; quad_solution_vector 2 in + 3 out =
    40 B/elt (value) or 2 in + 9 out = 88 B/elt (with ds/db, ds/dr)"""
    out = {}
    g = torch.Generator(device=dev).manual_seed(11)
    M = (torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 0.5) * 800.0
    e = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 0.9
    with torch.no_grad():
        q = time_events(lambda: ops.kepler(M, e), dev, 10)
    out["kepler"] = {"n": n, **q, "bytes_per_elt": 32, "GBps": 32.0 * n / (q["median_ms"] * 1e-3) / 1e9,
                     "frac_of_hbm_peak": 32.0 * n / (q["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
    del M, e
    b = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * 1.3
    r = torch.full((n,), 0.1, dtype=torch.float64, device=dev)
    with torch.no_grad():
        q = time_events(lambda: ops.quad_solution_vector(b, r), dev, 6)
        out["quad_solution_vector_value"] = {"n": n, **q, "bytes_per_elt": 40,
                                             "GBps": 40.0 * n / (q["median_ms"] * 1e-3) / 1e9,
                                             "frac_of_hbm_peak": 40.0 * n / (q["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
        q = time_events(lambda: ops.quad_solution_vector_derivs(b, r), dev, 6)
        out["quad_solution_vector_with_derivs"] = {"n": n, **q, "bytes_per_elt": 88,
                                                   "GBps": 88.0 * n / (q["median_ms"] * 1e-3) / 1e9,
                                                   "frac_of_hbm_peak": 88.0 * n / (q["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
    out["note"] = ("b uniform in [0, 1.3], r = 0.1: 85 % of the elements overlap the disk and evaluate the elliptic "
                   "integrals -- the op is fp64-VALU-bound there, not HBM-bound (SURVEY.md 8d caveat)")
    return out


def graphed(xo, fn, inputs, dev, iters):
    """time `fn(*inputs)` replayed as one hipGraph; eager launches if the capture fails"""
    try:
        g = xo.GraphedStep(fn, *inputs)
        q = time_events(lambda: g(), dev, iters)
        return q, "hipGraph replay"
    except Exception as exc:
        torch.cuda.synchronize(dev)
        q = time_events(lambda: fn(*inputs), dev, max(3, iters // 4))
        return q, f"eager launches (capture failed: {repr(exc)[:120]})"


def extra_config(xo, ops, dev, key, D, iters, **kw):
    """one of the BASELINE configs at a per-GPU size, as the very step `--config` times (hipGraph replay)"""
    w = WORKLOADS[key](xo, ops, dev, D, **kw)
    q, how = graphed(xo, w.fn, w.leaves, dev, iters)
    gbps = w.survey_bytes_per_unit * D * w.n_cad / (q["median_ms"] * 1e-3) / 1e9
    out = {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "draws": D, "n_cadences": w.n_cad, "launch": how,
           "survey_8d_bytes_per_unit": w.survey_bytes_per_unit, "survey_8d_GBps": gbps,
           "survey_8d_frac_of_hbm_peak": gbps / HBM_PEAK_GBS, "note": w.label + "; step: " + w.step_text,
           "same_step_as": f"bench.py --config {key} --global-draws {D}"}
    del w
    torch.cuda.empty_cache()
    return out


def sparse_step_fn(xo, ops, names, t, gbar):
    """the C2 step with EXO_FLAG_SPARSE (`extras.c2_sparse_output`): (L, *leaf gradients); no dense flux array"""
    def fn(*vals):
        _, L, grads = step(xo, ops, dict(zip(names, vals)), t, gbar, sparse=True)
        return (L.detach(),) + grads
    return fn


def likelihood_step_fn(xo, names, t, obs, yerr):
    """C2 as a white-noise likelihood (`extras.c2_white_noise_likelihood`): (ll, *leaf gradients)"""
    def fn(*vals):
        Lv = dict(zip(names, vals))
        orbit = xo.KeplerianOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"])
        ll = xo.LimbDarkLightCurve(Lv["u1"], Lv["u2"]).white_noise_log_likelihood(orbit=orbit, r=Lv["r"], t=t, y=obs, yerr=yerr)
        return (ll.detach(),) + torch.autograd.grad(ll.sum(), vals)
    return fn


def extra_gp_conditioning(xo, ops, dev, D):
    """The celerite log-likelihood alone (value + gradient of the hyper-parameters and of the series) at the C3 shape for
    kernels of increasing difficulty for the time-parallel form: the clean SHO term; 1 % of the draws within 1 % of
    critical damping; a Matern-3/2 term (celerite2's eps = 0.01 approximation: b / a = 100); a RotationTerm whose
    second mode sits near Q = 1/2 -- the cases docs/DESIGN_r1_r4.md 3.5 used to send to the sequential kernels."""
    T = xo.gp.terms
    t = ops.vouch_sorted(torch.arange(N_CAD, dtype=torch.float64, device=dev) * CADENCE)   # (a fixed series: the caller's word)
    y = torch.as_tensor(5e-4 * np.random.default_rng(3).normal(size=N_CAD), device=dev)
    # (the mean model draws-innermost, as the C3 step hands it over: get_light_curve(cadence_major=True))
    model = torch.zeros(N_CAD, D, dtype=torch.float64, device=dev).t().requires_grad_(True)
    full = lambda v: torch.full((D,), v, dtype=torch.float64, device=dev, requires_grad=True)  # noqa: E731
    Qmix = np.full(D, 0.7071)
    Qmix[: max(1, D // 100): 2] = 0.505
    Qmix[1: max(2, D // 100): 2] = 0.495
    # bright-star draws: 1 % of the batch with a GP amplitude far above the white noise (conditioning score kappa = (1 + (b/a)^2)
    # sum(a) / min(diag) of 1e6 at J = 2 -- under the J <= 2 threshold of the scan trees -- and of 3e5 at J = 4 -- above the 3e4 of
    # wider states: those draws take the ROBUST route of the time-parallel path (docs/DESIGN_r1_r4.md 3.11; until round 4 the sequential
    # kernels redid them: 27x, the cliff VERDICT r3 item 6 asked to be timed)
    sig_b2 = np.full(D, 1e-3); sig_b2[: max(1, D // 100)] = 0.35
    sig_b4 = np.full(D, 1e-3); sig_b4[: max(1, D // 100)] = 0.25
    vec = lambda a: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=True)  # noqa: E731
    cases = {
        "sho_clean": ([full(1e-3), full(5.0), full(0.7071)], lambda s, r, q: T.SHOTerm(sigma=s, rho=r, Q=q)),
        "sho_1pct_bright_star_kappa_1e6": ([vec(sig_b2), full(5.0), full(0.7071)], lambda s, r, q: T.SHOTerm(sigma=s, rho=r, Q=q)),
        "two_sho_1pct_bright_star_kappa_3e5": ([vec(sig_b4), full(5.0), full(7e-4), full(2.5)],
                                               lambda s1, r1, s2, r2: T.SHOTerm(sigma=s1, rho=r1, Q=1.2) + T.SHOTerm(sigma=s2, rho=r2, Q=1.5)),
        "sho_1pct_near_critical": ([full(1e-3), full(5.0), torch.tensor(Qmix, device=dev, requires_grad=True)],
                                   lambda s, r, q: T.SHOTerm(sigma=s, rho=r, Q=q)),
        "matern32": ([full(1e-3), full(5.0)], lambda s, r: T.Matern32Term(sigma=s, rho=r)),
        "two_sho_clean": ([full(1e-3), full(5.0), full(7e-4), full(2.5)],
                          lambda s1, r1, s2, r2: T.SHOTerm(sigma=s1, rho=r1, Q=1.2) + T.SHOTerm(sigma=s2, rho=r2, Q=1.5)),
        "rotation_term": ([full(1e-3), full(5.0), full(0.02), full(0.5), full(0.5)],
                          lambda s, p, q0, dq, f: T.RotationTerm(sigma=s, period=p, Q0=q0, dQ=dq, f=f)),
    }
    out = {}
    for name, (hyper, build) in cases.items():
        def fn(m, *h):
            gp = xo.gp.GaussianProcess(build(*h), t=t, yerr=5e-4, mean=m)
            ll = gp.log_likelihood(y)
            return (ll.detach(),) + torch.autograd.grad(ll.sum(), (m,) + h)
        try:
            q, how = graphed(xo, fn, [model] + hyper, dev, 8)
            out[name] = {"median_ms": q["median_ms"], "launch": how}
        except Exception as exc:
            out[name] = {"error": repr(exc)[:200]}
        torch.cuda.synchronize(dev)
    for k, ref in (("sho_1pct_near_critical", "sho_clean"), ("matern32", "sho_clean"), ("rotation_term", "two_sho_clean"),
                   ("sho_1pct_bright_star_kappa_1e6", "sho_clean"), ("two_sho_1pct_bright_star_kappa_3e5", "two_sho_clean")):
        if "median_ms" in out.get(k, {}) and "median_ms" in out.get(ref, {}):
            out[k]["over_clean"] = out[k]["median_ms"] / out[ref]["median_ms"]      # against a clean batch of the same J
            out[k]["clean_reference"] = ref
    out["draws"], out["n_cadences"] = D, N_CAD
    out["note"] = ("GP log-likelihood + gradients alone (no light curve); `over_clean` = step time relative to a clean batch of "
                   "the same state width (J = 2: sho_clean; J = 4: two_sho_clean): the cost of over-damped / nearly critically "
                   "damped / Matern-type draws in a batch.  Round 2: 53x (207 ms against 3.9) as soon as ONE draw had Q < 1/2; "
                   "now every such draw stays on the time-parallel path (joint state covariance of the over-damped pair, "
                   "conditioning threshold 1e7 at J <= 2); the lanes of a batch of mixed kinds take the draws kind by kind (a stable partition on the "
                   "device: no wave of mixed kinds, no run-time layout; what is left of the 1.84x of round 3 is one more round of resident "
                   "waves for the second kind's wave).  `*_bright_star_*`: 1 % of the draws at a conditioning score of 1e6 "
                   "(J = 2: under the threshold of the scan trees) / 3e5 (J = 4: above the 3e4 of wider states -- those draws take the "
                   "robust route of the time-parallel path, docs/DESIGN_r1_r4.md section 3.11: Newton iterations on the chunks' entering states, the "
                   "adjoint scan fed from the chunks' own reverse recurrences; the sequential kernels that used to redo them cost 27x)")
    return out


def extra_astrometry(xo, dev, D=1024, n_epoch=64):
    """8f row 3: relative astrometry (separation, position angle) + star velocities of a two-planet system at a few
    dozen epochs, value + gradient of every orbit parameter: the fused position / velocity op against the composed
    torch path it replaces"""
    rng = np.random.default_rng(6)
    t = torch.tensor(np.sort(rng.uniform(0.0, 800.0, n_epoch)), dtype=torch.float64, device=dev)
    base = dict(period=[350.0, 97.0], t0=[10.0, 31.0], incl=[1.1, 1.3], ecc=[0.2, 0.5], omega=[0.3, -1.9], Omega=[0.4, 2.0],
                m_planet=[1e-3, 4e-4])
    leaves = {k: torch.tensor(np.asarray(v)[None, :] * (1 + 1e-3 * rng.normal(size=(D, 2))), dtype=torch.float64, device=dev,
                              requires_grad=True) for k, v in base.items()}
    names = list(leaves)
    w = [torch.randn(D, n_epoch, 2, dtype=torch.float64, device=dev) for _ in range(5)]

    def make(fused):
        def one(*vals):
            orbit = xo.KeplerianOrbit(m_star=1.0, r_star=1.0, **dict(zip(names, vals)))
            if not fused:
                orbit._fused_vector = lambda *a, **k: None
            rho, theta = orbit.get_relative_angles(t, parallax=0.05)
            vx, vy, vz = orbit.get_star_velocity(t)
            L = (rho * w[0] + theta * w[1] + vx * w[2] + vy * w[3] + vz * w[4]).sum((-1, -2))
            return (L.detach(),) + torch.autograd.grad(L.sum(), vals)
        return one

    out = {}
    for tag, fused in (("fused", True), ("composed", False)):
        q, how = graphed(xo, make(fused), list(leaves.values()), dev, 30)
        out[tag] = {"median_ms": q["median_ms"], "launch": how}
    out["draws"], out["n_epoch"], out["n_planet"] = D, n_epoch, 2
    out["note"] = ("astrometry + star velocities of 2 planets at %d epochs, %d draws, value + gradients of 7 x 2 leaves: "
                   "exo_orbit_vector_* (one launch each way per quantity) vs ops.kepler + torch algebra" % (n_epoch, D))
    return out


def extra_hmc(xo, ops, dev, D=1024, n_leapfrog=8, dense=False, nuts=False):
    """8f row 4: one HMC trajectory (n_leapfrog value + gradient evaluations of the C2 likelihood and the position /
    momentum updates between them) for D chains, replayed as one hipGraph"""
    rng = np.random.default_rng(8)
    t = ops.vouch_sorted(torch.arange(N_CAD, dtype=torch.float64, device=dev) * CADENCE)   # (a fixed series: the caller's word)
    lv = make_leaves(D, 11, dev)
    names = [k for k in lv if k not in ("u1", "u2")]
    u1, u2 = lv["u1"].detach(), lv["u2"].detach()
    with torch.no_grad():
        one = lambda v: torch.tensor([v], dtype=torch.float64, device=dev)  # noqa: E731
        orbit = xo.KeplerianOrbit(period=one(3.5), t0=one(1.0), b=one(0.3), ecc=one(0.3), omega=one(1.1))
        truth = xo.LimbDarkLightCurve(0.3, 0.2).get_light_curve(orbit=orbit, r=one(0.1), t=t).sum(-1).reshape(-1)
    obs = truth + 1e-4 * torch.randn(N_CAD, dtype=torch.float64, device=dev)
    ivar = 1e8

    def logp(*vals):
        # Gaussian log-likelihood of the observed light curve (white noise): one call on the sparse light curve
        Lv = dict(zip(names, vals))
        orbit = xo.KeplerianOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"])
        if dense:
            flux = xo.LimbDarkLightCurve(u1, u2).get_light_curve(orbit=orbit, r=Lv["r"], t=t).sum(-1)
            return -0.5 * ivar * ((flux - obs) ** 2).sum(-1)
        return xo.LimbDarkLightCurve(u1, u2).white_noise_log_likelihood(orbit=orbit, r=Lv["r"], t=t, y=obs, yerr=ivar ** -0.5)

    params = [lv[k].detach().clone() for k in names]
    if nuts:
        # (unit masses and a step size far below the posterior's scales: every tree grows to the depth limit, i.e. the
        # leg times 2**4 - 1 = 15 leaves per transition and the tree bookkeeping around them, not a tuned sampler)
        smp = xo.NUTS(logp, params, step_size=1e-11, max_depth=4, generator=torch.Generator(device=dev).manual_seed(12))
        for _ in range(2):
            smp.step()
        torch.cuda.synchronize(dev)
        n0 = smp.n_leapfrog
        q = stats_loop(lambda _: smp.step(), dev, 10)
        leaves = (smp.n_leapfrog - n0) / 10.0
        return {"transitions_per_s": D / (q["median_ms"] * 1e-3), "evals_per_s": D * leaves / (q["median_ms"] * 1e-3), **q,
                "chains": D, "leaves_per_transition": leaves, "ms_per_leaf": q["median_ms"] / leaves,
                "mean_depth": float(smp.mean_depth().mean()),
                "note": "exoplanet_amd.NUTS: %d chains in lockstep, one batched value+gradient evaluation of the C2 white-noise "
                        "likelihood per leaf (leapfrog step replayed as a hipGraph), tree bookkeeping (multinomial sampling, "
                        "checkpointed turning checks, masks) as torch ops on the device, one host synchronisation per doubling" % D}
    hmc = xo.HMC(logp, params, step_size=1e-6, n_leapfrog=n_leapfrog)
    for _ in range(3):
        hmc.step()
    torch.cuda.synchronize(dev)
    q = stats_loop(lambda _: hmc.step(), dev, 30)
    evals = D * (n_leapfrog + 1)
    return {"trajectories_per_s": D / (q["median_ms"] * 1e-3), "evals_per_s": evals / (q["median_ms"] * 1e-3), **q,
            "chains": D, "n_leapfrog": n_leapfrog,
            "note": "exoplanet_amd.HMC: %d chains, %d leapfrog steps per trajectory = %d value+gradient evaluations of the "
                    "C2 white-noise likelihood (LimbDarkLightCurve.white_noise_log_likelihood: exo_transit_chi2_vjp_f64, one "
                    "evaluation per solved cadence; `dense_ms`: the same through get_light_curve and torch passes over (chains, "
                    "cadences) arrays), one hipGraph replay per trajectory + momentum draw and accept / reject on the device"
                    % (D, n_leapfrog, n_leapfrog + 1)}


def extra_ttv(xo, ops, leaves, t, gbar, dev, D):
    n_tr = int((float(t[-1]) - 1.0) / 3.5) + 1
    offs = torch.tensor(0.01 * np.random.default_rng(7).normal(size=(D, n_tr)), dtype=torch.float64, device=dev,
                        requires_grad=True)
    tnames = list(leaves) + ["ttvs"]

    def ttv_step(*vals):
        Lv = dict(zip(tnames, vals))
        orb = xo.orbits.TTVOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"],
                                 ttvs=[Lv["ttvs"]])
        rec_t, ld_t, _, fl = orb.kernel_inputs(Lv["r"], (Lv["u1"], Lv["u2"]))
        ed, sh = orb.kernel_ttv()
        _, dot = ops.transit_flux_dot(t, rec_t, ld_t, gbar, flags=fl, ttv=(ed.contiguous(), sh.contiguous()))
        return (dot.detach(),) + torch.autograd.grad(dot.sum(), vals)

    q, how = graphed(xo, ttv_step, list(leaves.values()) + [offs], dev, 30)
    # the same orbit as a white-noise likelihood (exo_transit_chi2_ttv_vjp_f64): no (draw, cadence) array
    obs = 1e-4 * torch.randn(t.numel(), dtype=torch.float64, device=dev)

    def ttv_like(*vals):
        Lv = dict(zip(tnames, vals))
        orb = xo.orbits.TTVOrbit(period=Lv["period"], t0=Lv["t0"], b=Lv["b"], ecc=Lv["ecc"], omega=Lv["omega"],
                                 ttvs=[Lv["ttvs"]])
        ll = xo.LimbDarkLightCurve(Lv["u1"], Lv["u2"]).white_noise_log_likelihood(orbit=orb, r=Lv["r"], t=t, y=obs, yerr=1e-4)
        return (ll.detach(),) + torch.autograd.grad(ll.sum(), vals)

    ql, _ = graphed(xo, ttv_like, list(leaves.values()) + [offs], dev, 30)
    return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "transits": n_tr, "launch": how,
            "likelihood": {"evals_per_s": D / (ql["median_ms"] * 1e-3), "median_ms": ql["median_ms"]},
            "note": "C2 step with a TTVOrbit (timing tables in the fused kernels, gradients to every per-transit offset); "
                    "`likelihood`: the same orbit through white_noise_log_likelihood (one evaluation per solved cadence)"}


def load_counters():
    """This round's committed counter record (profiles/r06_counters.json: rocprofv3 --pmc passes, tools/profile_r06.sh),
    quoted only when it was taken on the kernel sources this run executes (sha256 of the .hip / .hpp files)."""
    try:
        import hashlib

        p = json.load(open(os.path.join(ROOT, "profiles", "r06_counters.json")))
        h = hashlib.sha256()
        for f in sorted(p["kernel_sources"]):
            h.update(open(os.path.join(ROOT, "exoplanet_amd", "csrc", f), "rb").read())
        return p if h.hexdigest() == p["kernel_sources_sha256"] else None
    except Exception:
        return None


COMPACT_LIMIT = 4096     # bytes of the last stdout line (tests/test_bench_line.py holds compact_line to it)


def _short(x, n=200):
    return x if not isinstance(x, str) or len(x) <= n else x[:n - 3] + "..."


def _num(x, digits=6):
    """numbers to `digits` significant figures (the full precision is in the side file)"""
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        return x
    if isinstance(x, int) or x == 0 or x != x or x in (float("inf"), float("-inf")):
        return x
    return float(f"{x:.{digits}g}")


def compact_line(out):
    """The contract line: the driver's keys + `config` (short strings) + `roofline` + `cpu_baseline` + `configs_ms`, nothing else.
    Built from the full record `out` (which keeps every definition, extras leg and CPU leg: write_full_record)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data")
    line = {k: _num(out.get(k), 8) for k in keep}
    cfg = out.get("config") or {}
    line["config"] = {k: _short(_num(v), 200) for k, v in cfg.items()
                      if k in ("workload", "n_cadences", "draws_per_gpu", "global_draws", "parallelism", "step")}
    line["config"]["parallelism"] = _short(f"draws sharded over {out.get('n_gpus')} GPU(s); one collective of per-draw scalars per step", 120)
    line["config"]["step"] = _short(cfg.get("step"), 160)
    r = out.get("roofline")
    if r:
        rr = {k: _short(_num(r.get(k)), 120) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source",
                                                       "algorithmic_bytes_per_launch", "active_cadences_per_launch", "kernel_ms", "frac_step")
              if k in r}
        pmc = r.get("pmc") or {}
        if pmc:
            rr["pmc_kernel_GBps"] = _num(pmc.get("dominant_kernel_GBps"))
            rr["pmc_kernel_frac"] = _num(pmc.get("dominant_kernel_frac"))
            rr["pmc_kernel_us"] = _num(pmc.get("dominant_kernel_rocprof_avg_us"))
        if r.get("survey_8d_count"):
            rr["survey_8d_GBps"] = _num(r["survey_8d_count"].get("GBps"))
        elif r.get("survey_8d_GBps") is not None:
            rr["survey_8d_GBps"] = _num(r.get("survey_8d_GBps"))
        line["roofline"] = rr
    else:
        line["roofline"] = None
    c = out.get("cpu_baseline")
    if c:
        cc = {k: _short(_num(c.get(k)), 200) for k in ("value", "unit", "cores", "kind", "leg", "sample", "cpu_model", "usable_cores")}
        legs = c.get("legs") or {}
        allc = legs.get((c.get("leg") or "").replace("one_core", "all_cores")) or {}
        cc["all_cores_value"] = _num(allc.get("evals_per_s"))
        cc["all_cores_threads"] = allc.get("threads")
        line["cpu_baseline"] = cc
    else:
        line["cpu_baseline"] = None
    cm = dict(out.get("configs_ms") or {})
    cm.pop("note", None)
    line["configs_ms"] = cm
    line["full_record"] = out.get("full_record")
    n = len(json.dumps(line))
    if n > COMPACT_LIMIT:       # cannot happen with the caps above; never let the line outgrow the driver again
        line["config"] = {"workload": _short(cfg.get("workload"), 100)}
        if line.get("cpu_baseline"):
            line["cpu_baseline"].pop("sample", None)
    return line


def write_full_record(out):
    """the full record (extras, every CPU leg, the definitions) -> gpurun_out/bench_full.json, which gpurun merges back; the
    committed copy of a round is profiles/rNN_bench_full.json.  Not to stderr: the driver's tail may interleave the streams."""
    d = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        name = "bench_full.json" if out.get("n_gpus", 1) == 1 else f"bench_full_{out.get('n_gpus')}gpu.json"
        with open(os.path.join(d, name), "w") as f:
            json.dump(out, f, indent=1)
        out["full_record"] = "gpurun_out/" + name
    except OSError:
        out["full_record"] = None


DUMP_LIMIT = 64 << 20           # bytes of everything --dump-outputs writes
DUMP_ARRAY_LIMIT = 32 << 20     # an output larger than this is written as a seeded sample of its rows
DUMP_SEED = 0
# the outputs of a Workload's step in front of its leaf gradients, by `grads_from`: the dense flux and sum(gbar * flux) per
# draw (C2, C4), or the log-likelihood per draw (C3, C5)
DUMP_HEAD = {2: ("flux", "flux_dot_gbar"), 1: ("loglike",)}


def dump_outputs(d, wl, outputs, suffix=""):
    """what the step computed (`outputs`: the tuple `wl.fn` returns) -> d/<name><suffix>.npy, float64: the outputs of
    DUMP_HEAD, then the gradient of every leaf as `grad_<leaf>`.  An output over DUMP_ARRAY_LIMIT (the dense flux array) is
    written as the whole rows of a fixed, seeded sample of draws, their indices beside it as <name>_rows<suffix>.npy."""
    names = list(DUMP_HEAD[wl.grads_from]) + ["grad_" + n for n in wl.names]
    if len(names) != len(outputs):
        raise RuntimeError(f"--dump-outputs: {len(outputs)} outputs, {len(names)} names")
    os.makedirs(d, exist_ok=True)
    arrays = {}
    for name, x in zip(names, outputs):
        x = x.detach()
        if x.numel() * x.element_size() > DUMP_ARRAY_LIMIT:
            row_bytes = x.numel() // x.shape[0] * x.element_size()
            k = min(x.shape[0], max(1, DUMP_ARRAY_LIMIT // row_bytes))
            rows = np.sort(np.random.default_rng(DUMP_SEED).choice(x.shape[0], size=k, replace=False))
            arrays[name + "_rows"] = rows.astype(np.float64)
            x = x[torch.as_tensor(rows, device=x.device)]
        arrays[name] = x.to(torch.float64).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise RuntimeError(f"--dump-outputs: {total} bytes over the limit of {DUMP_LIMIT}")
    for name, a in arrays.items():
        np.save(os.path.join(d, name + suffix + ".npy"), a)


def launcher_argv(n_gpus, argv):
    """The command `python bench.py --gpus N ...` turns itself into when it was not started by a launcher."""
    import socket

    with socket.socket() as sk:          # a free port now is a free port a moment later, near enough, on a private box
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(argv[0])] + list(argv[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="c2", help="the BASELINE config whose step is timed")
    ap.add_argument("--draws-per-gpu", type=int, default=1024)
    ap.add_argument("--global-draws", type=int, default=0,
                    help="fix the TOTAL number of draws (strong scaling); default for --config c4 / c5: 512 / 1024, "
                         "as BASELINE.json states them over 8 GPUs")
    ap.add_argument("--c5-bright", type=int, default=0, help="profiling aid (--config c5): that many chains at a conditioning score of 1e6 "
                    "(workload_c5); not a BASELINE configuration")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the cold W + K, the >= 2 s timing loop, per-kernel / roofline figures, the extras "
                         "legs, the CPU baseline and the full record (module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-graph", action="store_true", help="launch the step eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip the extras legs")
    ap.add_argument("--no-stats", action="store_true", help="(--full) skip the >= 100 steps / >= 2 s median / p10 / p90 loop")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.gpus > 1:
        # `python bench.py --gpus N` called directly (the form of the driver's recorded command): become the launcher --
        # one rank per GPU of this node under torch.distributed.run, rendezvous on the loopback address (the container's
        # hostname may not resolve), the same argument list
        if "WORLD_SIZE" in os.environ or os.environ.get("EXO_BENCH_NO_REEXEC") == "1":
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE')}: launch with "
                             "torch.distributed.run --nproc-per-node N")
        os.execv(sys.executable, launcher_argv(args.gpus, sys.argv))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}")
    # EXO_BENCH_SHARE_GPU=1 (test aid, tests/test_gpu_bench_ranks.py): every rank on the devices there are (rank % count) and the
    # collective over gloo -- RCCL wants a device per rank -- so that a 1-GPU box runs the whole N-rank control flow (shards,
    # barrier, max over ranks, rank 0's line); the aggregate is then one GPU's, shared
    share_gpu = os.environ.get("EXO_BENCH_SHARE_GPU") == "1"
    dev_index = local_rank % max(torch.cuda.device_count(), 1) if share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or os.environ.get("EXO_BENCH_FORCE_DIST") == "1":   # the env switch lets a 1-GPU box exercise the RCCL path
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if share_gpu:
            dist_mod.init_process_group("gloo")
        else:
            dist_mod.init_process_group("nccl", device_id=dev)
        dist = dist_mod

    import exoplanet_amd as xo
    from exoplanet_amd import ops, _lib
    from exoplanet_amd.distributed import LoglikeExchange, shard_bounds

    _lib.load()  # fail loudly if the HIP library is missing
    cfg = args.config
    global_draws = args.global_draws or DEFAULT_GLOBAL_DRAWS.get(cfg, 0)
    if global_draws:
        lo, hi = shard_bounds(global_draws, rank, world)
        D, n_global, scaling = hi - lo, global_draws, "strong"
    else:
        D, n_global, scaling = args.draws_per_gpu, world * args.draws_per_gpu, "weak"
    events = HipEvents(max(args.steps, 20)) if args.full else None
    wl = WORKLOADS[cfg](xo, ops, dev, D, rank, **({"bright": args.c5_bright} if cfg == "c5" and args.c5_bright else {}))
    leaves = dict(zip(wl.names, wl.leaves))
    N = wl.n_cad
    exchange = LoglikeExchange(n_global, dev, force_collective=os.environ.get("EXO_BENCH_FORCE_DIST") == "1") if dist is not None else None
    consume = ExchangeConsumer(n_global, dev) if exchange is not None else None

    # The step is a handful of short launches: launch-bound when issued eagerly, so the timed region replays it as ONE
    # hipGraph; the collective -- exactly one call, from the graph's static output -- stays outside the graph, and the
    # full vector it hands back (the previous step's) is folded into the running cross-chain sums.
    graph = None
    if not args.no_graph:
        graph = xo.GraphedStep(wl.fn, *wl.leaves)

    # (the graph's static outputs hold the last replay's results; eager steps keep their last outputs only for --dump-outputs)
    last = [None]

    def eager_step():
        out = wl.fn(*wl.leaves)
        if args.dump_outputs:
            last[0] = out
        return out

    run, drain = make_runner(graph if graph is not None else eager_step, wl.scalar_index, exchange, consume)

    # setup, outside the contract's W + K steps: bring clocks, caches and the allocator to the state a sampler runs
    # in (a few hundred steps, ~0.1 s; the same count on every rank)
    SETUP_STEPS = 300 if cfg in ("c2", "c4") else 30
    # (--full: the contract's W + K with NOTHING in front first -- reported beside `value` as
    # `value_after_contract_warmup_only` -- then the setup steps, then the W + K that `value` is)
    wall_cold = None
    if args.full:
        wall_cold = time_steps(run, args.steps, args.warmup, dist, dev, drain=drain if exchange is not None else None)
    for _ in range(SETUP_STEPS):
        run(-1)
    torch.cuda.synchronize(dev)
    wall = time_steps(run, args.steps, args.warmup, dist, dev, drain=drain if exchange is not None else None)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, wl, graph.outputs if graph is not None else last[0],
                     "" if world == 1 else f".rank{rank}")
        last[0] = None
    wall_t = torch.tensor([wall, wall_cold or 0.0], dtype=torch.float64, device=dev)
    if dist is not None:
        dist.all_reduce(wall_t, op=dist.ReduceOp.MAX)
    wall = float(wall_t[0].item())
    wall_cold = float(wall_t[1].item()) if wall_cold is not None else None
    timing = None
    if args.full and not args.no_stats:
        # >= 100 steps and >= 2 s, whatever --steps was; the count follows from the
        # max-over-ranks step time above, so it is the same on every rank
        n_stat = int(min(6000, max(100, np.ceil(2.0 / max(wall / args.steps, 1e-6)))))
        timing = stats_loop(run, dev, n_stat)
        drain()
        if dist is not None:
            dist.barrier()

    light_curve_only = cfg in ("c2", "c4")
    kernel_ms = per_launch = n_active = None
    if args.full and light_curve_only:
        # hipEvents cannot bracket a node inside a replayed graph: time the kernels of the sweep over
        # directly launched steps on the same inputs (events recorded by the C ABI on the launch stream)
        n_ev = len(events.pairs)
        t_dev, gbar = wl.data["t"], wl.data["gbar"]
        for i in range(n_ev):
            step(xo, ops, leaves, t_dev, gbar, events=events.handles(i))
        torch.cuda.synchronize(dev)
        kernel_ms, per_launch = events.mean_ms()
        # cadences the sweep solves = the runs of the conjunction windows (one sparse sweep, outside any timing)
        with torch.no_grad():
            orbit0 = xo.KeplerianOrbit(period=leaves["period"], t0=leaves["t0"], b=leaves["b"], ecc=leaves["ecc"],
                                       omega=leaves["omega"])
            rec0, ld0, _, flags0 = orbit0.kernel_inputs(leaves["r"], (leaves["u1"], leaves["u2"]), use_in_transit=False)
            n_active = ops.transit_flux_sparse(t_dev, rec0.detach(), ld0.detach(), flags=flags0).n_solved()
    elif args.full:
        # GP configs: the step is a chain of ~20 kernels; the whole replayed step is timed with events on the stream it
        # is replayed on (per-kernel averages and counters: profiles/r06_*)
        q = time_events(lambda: run(-1), dev, 20)
        drain()
        kernel_ms = q["median_ms"]

    out = None
    if rank == 0:
        evals = n_global * args.steps
        survey_bytes = wl.survey_bytes_per_unit * D * N
        counters = load_counters() if args.full else None
        out = {
            "metric": "light-curve evals/sec (value+grad) at 150k cadences" if cfg == "c2" else
                      f"evals/sec (value+grad) of BASELINE config {cfg.upper()} ({N} cadences)",
            "value": evals / wall,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "setup_steps_before_warmup": SETUP_STEPS,
            "value_after_contract_warmup_only": evals / wall_cold if wall_cold is not None else None,
            "ms_per_step": 1e3 * wall / args.steps,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": wl.label + (f", every cadence classified on the device, {100.0 * n_active / (D * N):.2f} % solved"
                                        if n_active is not None else ""),
                "n_cadences": N, "draws_per_gpu": D, "global_draws": n_global,
                "setup_steps_before_warmup": SETUP_STEPS,      # (un-timed: clocks, caches, allocator; then the contract's W + K)
                "parallelism": f"draws sharded over {world} GPU(s); one collective of per-draw scalars per step, issued "
                               "asynchronously from a private copy (double-buffered): it overlaps the next step's kernels, "
                               "is waited for inside the timed region, and the previous step's full vector is consumed there "
                               "(running cross-chain sums)",
                "step": wl.step_text + ("; replayed as one hipGraph" if graph is not None else "; eager launches"),
            },
            "timing": timing,
        }
        if not args.full:
            out["roofline"] = None
        elif light_curve_only:
            # bytes this design must move per sweep: the dense flux array once (zeros); for every solved
            # cadence t and gbar in, its flux out to the run-ordered value array, back in and out to its
            # place in the flux array (the binary searches of the windows are a few MB)
            req = {"flux_zero_fill": 8 * D * N, "t_and_gbar_solved": 16 * n_active,
                   "value_and_cadence_arrays_write_read": 24 * n_active, "flux_write_solved": 8 * n_active}
            req_bytes = sum(req.values())
            achieved = req_bytes / (kernel_ms * 1e-3) / 1e9
            roof = {
                "bound": "hbm",
                "kernel": "transit_runs_kernel",
                "kernel_note": "dominant; kernel_ms is the hipEvent time of the whole sweep = transit_enum_kernel + transit_runs_kernel "
                               "[+ transit_finish_kernel below 512 draws]",
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "frac_definition": "achieved / peak; achieved = bytes this design must move per sweep (algorithmic_bytes_breakdown) / "
                                   "mean hipEvent time of the sweep's launches in this run",
                "traffic": None,
                "algorithmic_bytes_per_launch": req_bytes, "algorithmic_bytes_breakdown": req,
                "active_cadences_per_launch": n_active, "kernel_ms": kernel_ms,
                "kernel_ms_quantiles": quantiles(per_launch),
                "survey_8d_count": {"bytes_per_unit": wl.survey_bytes_per_unit, "bytes_per_launch": survey_bytes,
                                    "GBps": survey_bytes / (kernel_ms * 1e-3) / 1e9,
                                    "note": "SURVEY.md 8d charges t + gbar + flux = 24 B to EVERY (draw, cadence); this design "
                                            "finds the cadences to solve by binary search and reads t, gbar only there "
                                            "(8f row 1, compaction, folded into the sweep): bytes NOT moved, so this figure is "
                                            "not a fraction of anything"},
            }
            # ONE definition per field: `achieved` and `frac` are the live figure -- the bytes this design must
            # move per sweep / the hipEvent time of the sweep's launches, measured in this run; what the counters say about the
            # same kernels (committed record, quoted only when it was taken on these kernel sources) sits in `pmc`, and
            # `frac_step` charges the whole step (packing, packing VJP and the gaps of the replayed graph included)
            roof["frac_step"] = req_bytes / (wall / args.steps) / 1e9 / HBM_PEAK_GBS
            roof["frac_step_definition"] = "the same bytes / ms_per_step (the contract's K steps) / 8 TB/s"
            c = (counters or {}).get(cfg) if counters else None
            if c and c.get("draws") == D:
                tr = c["traffic_bytes_per_sweep"]
                dom = c["dominant_kernel"]
                roof["traffic"] = tr
                roof["traffic_source"] = c["source"]
                roof["pmc"] = {
                    "dominant_kernel_traffic_bytes": dom["traffic_bytes"], "dominant_kernel_rocprof_avg_us": dom["rocprof_avg_us"],
                    "dominant_kernel_GBps": dom["traffic_bytes"] / (dom["rocprof_avg_us"] * 1e-6) / 1e9,
                    "dominant_kernel_frac": dom["traffic_bytes"] / (dom["rocprof_avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS,
                    "frac_step": tr / (wall / args.steps) / 1e9 / HBM_PEAK_GBS,
                    "definition": "HBM bytes from the PMC counters (FETCH_SIZE x 2 on gfx950 + WRITE_SIZE, separate passes) of the "
                                  "dominant kernel / its rocprofv3 --kernel-trace average / 8 TB/s; frac_step: the sweep's counter "
                                  "bytes / this run's ms_per_step / 8 TB/s",
                    "traffic_over_required_bytes": tr / req_bytes, "traffic_over_survey_8d_bytes": tr / survey_bytes,
                }
                roof["valu"] = c.get("valu")
            out["roofline"] = roof
        else:
            # GP configs: `frac` is a BANDWIDTH fraction only when it is made of bytes that moved -- the
            # counter record's HBM traffic of one step / this run's step time / 8 TB/s (null when no record matches these
            # kernel sources) -- with the fp64-issue fractions of the kernels that bound the step beside it (`valu`); the
            # SURVEY.md 8d count (state saved and re-read: these kernels checkpoint and recompute instead) is kept as labelled
            # `survey_8d_*` fields, not as `frac`
            c = (counters or {}).get(cfg) if counters else None
            if c and c.get("draws") != D:
                c = None
            traffic = c["traffic_bytes_per_step"] if c else None
            step_s = kernel_ms * 1e-3
            out["roofline"] = {
                "bound": "hbm", "kernel": "whole replayed step (celerite element / scan-tree / chunk kernels + the light-curve "
                                          "sweeps + packing); per-kernel: profiles/r06_*",
                "achieved": traffic / step_s / 1e9 if traffic else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": traffic / step_s / 1e9 / HBM_PEAK_GBS if traffic else None,
                "frac_definition": "HBM bytes of one step from the PMC counters (FETCH_SIZE x 2 on gfx950 + WRITE_SIZE, separate passes: "
                                   "profiles/r06_counters.json, quoted only when taken on these kernel sources) / median event time of "
                                   "one replayed step in THIS run / 8 TB/s.  The step is fp64-issue-bound, not bandwidth-bound: see `valu` "
                                   "(SQ_INSTS_VALU x 4 cycles / (1024 SIMDs x kernel time x 2.4 GHz) per kernel)",
                "traffic": traffic, "traffic_source": c["source"] if c else None, "valu": c.get("valu") if c else None,
                "kernel_ms": kernel_ms,
                "survey_8d_bytes_per_unit": wl.survey_bytes_per_unit, "survey_8d_bytes_per_step": survey_bytes,
                "survey_8d_GBps": survey_bytes / step_s / 1e9,
                "survey_8d_note": "SURVEY.md 8d charges 48 + 16 (1 + J + J^2) B to every (draw, cadence) -- the forward state written "
                                  "and re-read; the J <= 6 kernels keep CHECKPOINTS (10 B per (draw, cadence) at J = 2, 108 B at J = 6) "
                                  "and recompute, and the light curve reaches them as runs + values: bytes NOT moved, so this figure "
                                  "is not a fraction of anything",
            }

    # the extra legs are single-GPU diagnostics: under torch.distributed.run they would only add
    # barriers that every rank has to reach (an exception on one rank would hang the others)
    if args.full and not args.no_extras and world == 1 and dist is None and cfg == "c2":
        extras = {}
        t, gbar = wl.data["t"], wl.data["gbar"]

        def leg(name, fn):
            try:
                extras[name] = fn()
            except Exception as exc:  # an extra leg must not take the headline measurement down with it
                extras[name] = {"error": repr(exc)[:300]}
            torch.cuda.synchronize(dev)

        def in_transit():
            names = list(leaves)
            q, how = graphed(xo, lambda *v: step(xo, ops, dict(zip(names, v)), t, gbar, use_in_transit=True),
                             list(leaves.values()), dev, 50)
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "launch": how,
                    "note": "the reference's default use_in_transit=True: contact-point windows from the packing "
                            "kernel decide what is solved"}

        def op_level():
            orbit = xo.KeplerianOrbit(period=leaves["period"], t0=leaves["t0"], b=leaves["b"], ecc=leaves["ecc"],
                                      omega=leaves["omega"])
            rec, c, _, _ = orbit.kernel_inputs(leaves["r"], (leaves["u1"], leaves["u2"]))
            rec, c = rec.detach(), c.detach()
            q = time_events(lambda: ops.transit_flux_value_and_vjp(t, rec, c, gbar), dev, 50)
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q,
                    "note": "fused kernel call only (4 launches), no orbit algebra / autograd"}

        def small_batch():
            res = {}
            for d in (64, 128, 256):
                lv = make_leaves(d, 300 + d, dev)
                gb = gbar[:d].contiguous()
                nm = list(lv)
                q, how = graphed(xo, lambda *v: step(xo, ops, dict(zip(nm, v)), t, gb), list(lv.values()), dev, 50)
                res[str(d)] = {"evals_per_s": d / (q["median_ms"] * 1e-3), "median_ms": q["median_ms"], "launch": how}
            return res

        def sparse_output():
            q, how = graphed(xo, sparse_step_fn(xo, ops, list(leaves), t, gbar), list(leaves.values()), dev, 50)
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "launch": how,
                    "note": "the same C2 step with EXO_FLAG_SPARSE: the output is the runs of cadences in which the planet "
                            "can overlap the disk plus their flux values (every other cadence is exactly 0) -- no 1.23 GB "
                            "of zeros; what a likelihood needs"}

        def light_delay():
            names = list(leaves)

            def ld_step(*vals):
                _, L, grads = step(xo, ops, dict(zip(names, vals)), t, gbar, light_delay=True)
                return (L.detach(),) + grads

            q, how = graphed(xo, ld_step, list(leaves.values()), dev, 50)
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "launch": how,
                    "note": "the C2 step with light_delay=True (keplerian.py:411-470): every solved sample is evaluated at "
                            "its retarded time -- a second Kepler solve and the reverse sweep through the delay, in the "
                            "same kernel; dense output"}

        def likelihood():
            obs = torch.as_tensor(1e-4 * np.random.default_rng(12).normal(size=N_CAD), device=dev)
            q, how = graphed(xo, likelihood_step_fn(xo, list(leaves), t, obs, 1e-4), list(leaves.values()), dev, 50)
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "launch": how,
                    "note": "C2 as a white-noise likelihood, value + gradient of every leaf (exo_transit_chi2_vjp_f64: one planet, "
                            "one sample per cadence -> ONE evaluation per solved cadence, the cotangent 2 w (F - obs) formed "
                            "inside it; no (draw, cadence) array exists)"}

        def kept_dense():
            # op level (records packed once): the dense sweep, the sparse sweep, and the dense array KEPT across steps
            with torch.no_grad():
                orbit = xo.KeplerianOrbit(**{k: leaves[k].detach() for k in ("period", "t0", "b", "ecc", "omega")})
                params, ld, _, _ = orbit.kernel_inputs(leaves["r"].detach(), (leaves["u1"].detach(), leaves["u2"].detach()))
                params, ld = params.contiguous(), ld.contiguous()
            keeper = ops.KeptDenseFlux(t, D, 1)
            res = {}
            for name, fn in (("dense_sweep", lambda pr: ops.transit_flux_value_and_vjp(t, pr, ld, gbar)[1:]),
                             ("sparse_sweep", lambda pr: ops.transit_flux_sparse(t, pr, ld, gbar)[1:3]),
                             ("kept_dense", lambda pr: keeper.step(pr, ld, gbar)[1:3])):
                q, how = graphed(xo, fn, [params], dev, 50)
                res[name] = {"median_ms": q["median_ms"], "evals_per_s": D / (q["median_ms"] * 1e-3), "launch": how}
            same = bool(torch.equal(keeper.flux, ops.transit_flux_value_and_vjp(t, params, ld, gbar)[0]))
            return {**res, "kept_equals_dense_bit_for_bit": same,
                    "note": "LABELLED EXTRA, not the headline (VERDICT r3 item 5): op level, records packed once.  `kept_dense` = "
                            "ops.KeptDenseFlux: the caller keeps the dense flux array and the sweep's workspace from step to step; a "
                            "step zeroes the cadences the LAST step solved (exo_transit_sparse_scatter_f64), runs the sparse sweep, "
                            "writes the cadences THIS step solved -- the dense sweep's array, bit for bit, without the 1.23 GB "
                            "fill of every cadence.  The headline stays the stateless dense sweep."}

        def one_call():
            global STEP_THROUGH_AUTOGRAD
            names = list(leaves)
            was = STEP_THROUGH_AUTOGRAD
            STEP_THROUGH_AUTOGRAD = False
            try:
                q, how = graphed(xo, lambda *v: step(xo, ops, dict(zip(names, v)), t, gbar), list(leaves.values()), dev, 50)
            finally:
                STEP_THROUGH_AUTOGRAD = was
            return {"evals_per_s": D / (q["median_ms"] * 1e-3), **q, "launch": how,
                    "note": "the headline step as ONE call of the library without an autograd graph (KeplerianOrbit.flux_value_and_grad "
                            "-> exo_transit_flux_cols_vjp_f64): what a sampler's leapfrog step would call; the same three launches and "
                            "numbers as the headline's autograd form"}

        leg("c2_one_call", one_call)
        leg("c2_white_noise_likelihood", likelihood)
        leg("c2_sparse_output", sparse_output)
        leg("c2_dense_kept_across_steps", kept_dense)
        leg("c2_light_delay", light_delay)
        leg("in_transit_only", in_transit)
        leg("op_level_every_cadence", op_level)
        leg("c2_small_batches", small_batch)
        leg("c2_with_transit_timing_variations", lambda: extra_ttv(xo, ops, leaves, t, gbar, dev, D))
        del gbar, wl, graph
        torch.cuda.empty_cache()
        leg("c3_light_curve_plus_sho_gp", lambda: extra_config(xo, ops, dev, "c3", D, 12))
        leg("c3_gp_conditioning", lambda: extra_gp_conditioning(xo, ops, dev, D))
        torch.cuda.empty_cache()
        leg("c4_four_planets_64_draws", lambda: extra_config(xo, ops, dev, "c4", 64, 40))
        leg("c5_secondary_eclipse_3term_gp_128_chains", lambda: extra_config(xo, ops, dev, "c5", 128, 12))

        def c5_bright():
            out = extra_config(xo, ops, dev, "c5", 128, 12, bright=2)
            clean = extras.get("c5_secondary_eclipse_3term_gp_128_chains", {}).get("median_ms")
            out["over_clean"] = out["median_ms"] / clean if clean else None
            out["same_step_as"] = None
            out["note"] = ("the C5 step at 128 chains with 2 of them (1 %) at a conditioning score of 1e6 (first SHO term 1000 x the error "
                           "bars): those chains take the robust route of the time-parallel path -- Newton iterations on the states "
                           "entering the chunks, the adjoint scan's inputs from the chunks' own reverse recurrences -- instead of the sequential "
                           "kernels (VERDICT r3 item 2b: <= 2 x the clean step); " + out["note"])
            return out
        leg("c5_128_chains_1pct_bright_star_kappa_1e6", c5_bright)

        def c5_variant(note, **kw):
            out = extra_config(xo, ops, dev, "c5", 128, 6, **kw)
            clean = extras.get("c5_secondary_eclipse_3term_gp_128_chains", {}).get("median_ms")
            out["over_clean"] = out["median_ms"] / clean if clean else None
            out["same_step_as"] = None
            out["note"] = note + "; " + out["note"]
            return out
        # the cliff remnants as NUMBERS: a state wider than the one-lane time-parallel kernels, and a
        # conditioning score beyond the robust route -- both fall to the sequential kernels (all draws of the call for J = 10;
        # the flagged chains only for kappa = 1e9)
        leg("c5_shape_J8_four_sho_terms", lambda: c5_variant(
            "the C5 step at 128 chains with a J = 8 kernel (four SHO terms): the lane-group time-parallel path (a draw on eight lanes)",
            kernel="sho4"))
        leg("c5_shape_J10_two_rotation_terms_plus_sho", lambda: c5_variant(
            "the C5 step at 128 chains with a J = 10 kernel (two RotationTerms + one SHO term): per unit of J^2 against the clean "
            "J = 6 step = over_clean x 36 / 100", kernel="rot2_sho"))
        leg("c5_128_chains_merged_sparse_mean", lambda: c5_variant(
            "the C5 step at 128 chains with the light curve as a MERGED sparse mean (transit + occultation lists merged on the device, "
            "round 6) instead of the dense cadence-major array", mean_sparse=True))
        leg("c5_128_chains_1pct_kappa_1e9", lambda: c5_variant(
            "the C5 step at 128 chains with 2 of them (1 %) at a conditioning score of 1e9 (first SHO term 31 600 x the error bars): "
            "beyond the robust route's reach -- those chains are redone by the sequential kernels", bright=2, bright_factor=10 ** 4.5))
        torch.cuda.empty_cache()
        leg("astrometry_and_velocities", lambda: extra_astrometry(xo, dev))
        def nuts_leg():
            return extra_hmc(xo, ops, dev, nuts=True)

        def hmc_leg():
            res = extra_hmc(xo, ops, dev)
            res["dense_ms"] = extra_hmc(xo, ops, dev, dense=True)["median_ms"]
            return res

        leg("hmc_trajectory_c2", hmc_leg)
        leg("nuts_transition_c2", nuts_leg)
        torch.cuda.empty_cache()
        leg("ops", lambda: extra_ops(ops, dev))
        if rank == 0:
            out["extras"] = extras

    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(config=cfg)
        else:
            out["cpu_baseline"] = None
    if rank == 0:
        # every config's step time in ONE compact object, the LAST key of the line (the driver keeps the tail of stdout: the
        # C3 / C5 figures used to sit in the middle of `extras` and fall outside it -- VERDICT r4 item 4)
        ex = out.get("extras") or {}
        pick = lambda k, f="median_ms": (round(ex[k][f], 4) if isinstance(ex.get(k), dict) and isinstance(ex[k].get(f), (int, float)) else None)  # noqa: E731
        out["configs_ms"] = {
            cfg: round(out["ms_per_step"], 4),
            "c3": pick("c3_light_curve_plus_sho_gp"), "c4_64": pick("c4_four_planets_64_draws"),
            "c5_128": pick("c5_secondary_eclipse_3term_gp_128_chains"), "c5b": pick("c5_128_chains_1pct_bright_star_kappa_1e6"),
            "sparse": pick("c2_sparse_output"), "chi2": pick("c2_white_noise_likelihood"),
            "c5_j8": pick("c5_shape_J8_four_sho_terms"), "c5_j10": pick("c5_shape_J10_two_rotation_terms_plus_sho"), "c5_kappa1e9": pick("c5_128_chains_1pct_kappa_1e9"),
            "c5_sparse_mean": pick("c5_128_chains_merged_sparse_mean"),
            "hmc": pick("hmc_trajectory_c2"), "nuts_leaf": pick("nuts_transition_c2", "ms_per_leaf"),
            "c2_one_call": pick("c2_one_call"),
            # the reference's standalone Ops at n = 1.5e8 (GB/s of their algorithmic bytes: 32 / 40 / 88 B per element)
            "kepler_GBps": (round(ex["ops"]["kepler"]["GBps"], 1) if isinstance(ex.get("ops"), dict) and "kepler" in ex["ops"] else None),
            "quad_sv_GBps": (round(ex["ops"]["quad_solution_vector_value"]["GBps"], 1)
                             if isinstance(ex.get("ops"), dict) and "quad_solution_vector_value" in ex["ops"] else None),
            "quad_sv_grad_GBps": (round(ex["ops"]["quad_solution_vector_with_derivs"]["GBps"], 1)
                                  if isinstance(ex.get("ops"), dict) and "quad_solution_vector_with_derivs" in ex["ops"] else None),
            "note": "ms per value + gradient step, one MI355X, hipGraph replay; c2 / sparse / chi2 at 1024 draws x 150000 cadences",
        }
        if not args.full:           # (the other configs are extras legs)
            out["configs_ms"] = {cfg: out["configs_ms"][cfg]}
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes its version banner through C stdio (buffered when piped): push it out first so
        # that the JSON line is the last line of stdout
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        # --full: the full record (extras, every CPU leg, definitions) goes to a side file; the LAST line of stdout is the
        # compact contract line only (a 20.8 KB line was not parsed by the driver)
        if args.full:
            write_full_record(out)
        print(json.dumps(compact_line(out)), flush=True)


if __name__ == "__main__":
    main()
