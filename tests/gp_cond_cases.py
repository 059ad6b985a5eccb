"""What tools/make_gp_cond_golden.py, tests/test_gp_cond_host.py and tests/test_gpu_gp_cond.py share: the entries of the
multiprecision fixture tests/golden/gp_cond_mp.npz -- the conditional half of the celerite GP: apply_inverse, dot_tril and
predict (mean, variance, covariance, per-component) -- the float64 yardstick and the tolerance.

Yardstick and tolerance
-----------------------
The yardstick is the published sequential recurrences restated in float64 numpy (oracle.numpy_port.celerite_factor /
celerite_solve / celerite_dot_tril / celerite_predict_mean / celerite_predict_var / celerite_predict_cov).  For every entry
and quantity the fixture stores ``unit_<quantity>``: the yardstick's error on the fixture's float64 inputs against the mpmath
value, in the scale of the quantity:

    alpha: max |alpha|      z: max |z|      mu: max |mu| of that component at the data times      var, cov: k2(0)

and a kernel passes when, in the same scale,

    error <= max(FACTOR * unit, FLOOR),      FACTOR = 16, FLOOR = 1e-13

(the precedent of tests/test_gpu_estimators.py: the kernels differ from the yardstick in summation order, fma contraction
and the device's exp / sincos; the floor covers a unit that happens to be tiny).  The unit is a property of the inputs --
it is what ANY float64 evaluation of the recurrences loses on them -- never of the code under test.  So that a tolerance
cannot hide a failure the generator asserts FACTOR * unit <= CAP = 1e-6 for every entry and quantity; the only exception is
the forward error of alpha for the entries of RESIDUAL_ONLY, whose alpha is held by the backward-error test of
tests/test_gpu_gp_cond.py instead.

Entries (N = 96 data times, M = 31 query times)
-----------------------------------------------
Irregular times: uniform on 30 days with a gap of 4 days and one repeated time stamp (diag0 has no repeated stamp: with a
zero diagonal two equal times make K singular).  Cadence entries: a 2-minute grid.  ``y`` is a draw from the process
(L x' in mpmath, rounded) except for white_y.  Query times: 50 L before the first datum and 500 L after the last (L the
longest time scale of the kernel: the propagators are below 1e-21 there, mu = 0 and var = k2(0)), half a spacing and one
spacing outside either end, exactly on t[0], t[7] (twice), t[-2], t[-1] and the repeated stamp, 1e-6 after and before two
data times each, two in the gap, three mid-way between neighbours and ten random interior times.
"""
import os

import numpy as np

from oracle import numpy_port as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, N_RANDOM = 96, 10
FACTOR, FLOOR, CAP = 16.0, 1e-13, 1e-6
BJD = 2457000.0

ENTRIES = ("benign", "white_y", "snr1e3", "snr1e6", "diag0", "cadence_flagship", "cadence_snr1e6", "q045", "q04999",
           "q05001", "matern", "bjd_highq", "rot2_sho", "rot3", "mixed16", "real_sho_j3", "mix_j5")
WIDE = ("rot2_sho", "rot3", "mixed16")          # coefficient sets of tests/golden/gp_wide.npz (J = 10, 12, 16)

# Entries whose alpha is NOT compared element by element: 16 x the yardstick's own forward error of alpha exceeds CAP there
# (the matrix is that ill-conditioned); their alpha is held by the backward-error test.  Checked by the generator: exactly
# the entries whose alpha breaks the cap, and a subset of the three named here.
RESIDUAL_ONLY_ALLOWED = ("snr1e6", "cadence_snr1e6", "diag0")
RESIDUAL_ONLY = ("snr1e6", "cadence_snr1e6")     # (units of alpha 3.3e-5 and 3.8e-7; diag0, without the repeated stamp, 5.5e-11)

# (entry, quantity prefix) -> a factor above FACTOR for that entry alone, each with its cause
ENTRY_FACTOR = {}

# the SHO terms behind the entries: (sigma, rho, Q) of every pair slot built through SHOTerm, in slot order (None: the slot
# is a ComplexTerm from its stored coefficients).  A Q < 1/2 slot is of kind 1 (two real terms) and exists only so.
SHO = {
    "benign": [(1.0, 3.0, 0.7)], "white_y": [(1.0, 3.0, 0.7)], "snr1e3": [(1.0, 3.0, 0.7)], "snr1e6": [(1.0, 3.0, 0.7)],
    "diag0": [(1.0, 3.0, 0.7)],
    "cadence_flagship": [(1e-3, 5.0, 1 / np.sqrt(2))], "cadence_snr1e6": [(1.0, 5.0, 1 / np.sqrt(2))],
    "q045": [(1.0, 3.0, 0.45)], "q04999": [(1.0, 3.0, 0.4999)], "q05001": [(1.0, 3.0, 0.5001)],
    "bjd_highq": [(1.0, 0.05, 30.0)],
    "real_sho_j3": [(0.7, 2.0, 1.5)], "mix_j5": [(0.6, 4.0, 0.3), (0.5, 1.5, 2.0)],
}
REAL = {"real_sho_j3": [(0.5, 0.2)], "mix_j5": [(0.4, 1.0)]}
DIAG = {"benign": 0.09, "white_y": 0.09, "snr1e3": 1e-6, "snr1e6": 1e-12, "diag0": 0.0, "cadence_flagship": 2.5e-7,
        "cadence_snr1e6": 1e-12, "q045": 1e-4, "q04999": 1e-4, "q05001": 1e-4, "matern": 1e-4, "bjd_highq": 1e-4,
        "rot2_sho": 0.01, "rot3": 0.01, "mixed16": 0.01, "real_sho_j3": 0.01, "mix_j5": 0.01}
# component masks, one flag per slot (real slots first, then pair slots)
MASKS = {"rot2_sho": [[1, 1, 0, 0, 0]], "rot3": [[0, 0, 1, 1, 0, 0]], "mixed16": [[1, 0, 1, 1, 0, 0, 0, 0, 1]],
         "real_sho_j3": [[1, 0], [0, 1]], "mix_j5": [[1, 1, 0], [0, 0, 1]]}
MATERN = (1.0, 3.0, 0.01)        # sigma, rho, eps of Matern32Term


def sho_slot(sigma, rho, Q):
    """(pair slot (4,), kind) of an SHO term as gp.terms.SHOTerm lays it out"""
    S0, w0 = P.sho_from_sigma_rho(sigma, rho, Q)
    ar, cr, ac, bc, cc, dc = P.sho_coefficients(S0, w0, Q)
    if Q < 0.5:
        return np.array([ar[0], cr[0], ar[1], cr[1]]), 1
    return np.array([ac[0], bc[0], cc[0], dc[0]]), 0


def coeffs6(real, pairs, kind, mask=None):
    """(ar, cr, ac, bc, cc, dc) of oracle.numpy_port from slots: real (Jr, 2), pairs (Jc, 4), kind (Jc,); a kind-1 pair slot
    is two real terms; ``mask``: one flag per slot, the slots to keep"""
    real, pairs = np.asarray(real, dtype=np.float64).reshape(-1, 2), np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    kind = np.zeros(len(pairs), np.int32) if kind is None else np.asarray(kind).reshape(-1)
    keep = np.ones(len(real) + len(pairs), bool) if mask is None else np.asarray(mask).astype(bool)
    ar, cr = [a for (a, _), k in zip(real, keep) if k], [c for (_, c), k in zip(real, keep) if k]
    cx = []
    for p, kd, k in zip(pairs, kind, keep[len(real):]):
        if not k:
            continue
        if kd:
            ar += [p[0], p[2]]
            cr += [p[1], p[3]]
        else:
            cx.append(p)
    cx = np.array(cx).reshape(-1, 4)
    return (np.array(ar), np.array(cr)) + tuple(cx[:, i].copy() for i in range(4))


def inputs(name):
    """the float64 inputs of entry ``name`` that do not need mpmath (the generator adds y): a dict of t, diag (N,),
    coef_real (Jr, 2), pairs (Jc, 4), pair_kind (Jc,) int32, tq (M,), x, xy (N,) white noise (for dot_tril; for y),
    masks (n_mask, n_slot) int32"""
    k = ENTRIES.index(name)
    rng = np.random.default_rng(4100 + k)
    real = np.array(REAL.get(name, []), dtype=np.float64).reshape(-1, 2)
    if name in WIDE:
        g = np.load(os.path.join(GOLD, "gp_wide.npz"))
        real = np.stack([g[f"{name}_ar"], g[f"{name}_cr"]], -1).reshape(-1, 2)
        pairs = np.stack([g[f"{name}_{q}"] for q in ("ac", "bc", "cc", "dc")], -1)
        kind = np.zeros(len(pairs), np.int32)
    elif name == "matern":
        sigma, rho, eps = MATERN
        w0 = np.sqrt(3.0) / rho
        S0 = sigma ** 2 / w0
        pairs, kind = np.array([[w0 * S0, w0 * w0 * S0 / eps, w0, eps]]), np.zeros(1, np.int32)
    else:
        slots = [sho_slot(*s) for s in SHO[name]]
        pairs, kind = np.stack([s[0] for s in slots]), np.array([s[1] for s in slots], np.int32)
    co = coeffs6(real, pairs, kind)
    scale = max([1.0 / min(np.concatenate([co[1], co[4]]))] + [s[1] for s in SHO.get(name, [])])
    if name.startswith("cadence"):
        t = np.arange(N) * (2.0 / 1440.0)
        rep, gap = 40, 0.5 * (t[31] + t[32]) + np.array([-2e-4, 2e-4])
    else:
        t = np.sort(rng.uniform(0.0, 30.0, N))
        t[N // 3:] += 4.0                       # a gap
        if name != "diag0":
            t[N // 2 + 1] = t[N // 2]           # a repeated time stamp
        rep, gap = N // 2, t[N // 3 - 1] + np.array([1.3, 2.9])
        if name == "bjd_highq":
            t = t + BJD
            gap = gap + BJD
    h = np.median(np.diff(t))
    tq = np.concatenate([[t[0] - 50 * scale, t[0] - h, t[0] - 0.5 * h, t[0], t[7], t[7], t[rep], t[-2], t[-1],
                          t[-1] + 0.5 * h, t[-1] + h, t[-1] + 500 * scale],
                         t[[20, 60]] + 1e-6, t[[25, 70]] - 1e-6, gap, 0.5 * (t[[10, 44, 80]] + t[[11, 45, 81]]),
                         rng.uniform(t[0], t[-1], N_RANDOM)])
    masks = np.array(MASKS.get(name, []), np.int32).reshape(-1, len(real) + len(pairs))
    return dict(t=t, diag=np.full(N, DIAG[name]), coef_real=real, pairs=pairs, pair_kind=kind, tq=np.sort(tq),
                x=rng.normal(size=N), xy=rng.normal(size=N), masks=masks)


# ------------------------------------------------------------------------------------------------------------------
def load():
    return np.load(os.path.join(GOLD, "gp_cond_mp.npz"))


INPUT_KEYS = ("t", "diag", "coef_real", "pairs", "pair_kind", "tq", "x", "y", "masks")
BASE = ("alpha", "z", "mu_t", "mu_q", "var_t", "var_q", "cov_q")
PER_MASK = ("mu_t", "mu_q", "var_t", "var_q", "cov_q")


def quantities(n_mask):
    return BASE + tuple(f"{q}_m{i}" for i in range(n_mask) for q in PER_MASK)


class Case:
    """entry ``name`` of the fixture: the inputs as attributes, ``want`` / ``unit`` / ``scale`` dicts over quantities()"""

    def __init__(self, g, name):
        self.name = name
        for k in INPUT_KEYS:
            setattr(self, k, g[f"{name}_{k}"])
        self.quantities = quantities(len(self.masks))
        self.want = {q: g[f"{name}_{q}"] for q in self.quantities}
        self.unit = {q: float(g[f"{name}_unit_{q}"]) for q in self.quantities}
        self.scale = {q: float(g[f"{name}_scale_{q}"]) for q in self.quantities}
        self.J = len(self.coef_real) + 2 * len(self.pairs)

    def mask(self, q):
        """the slot mask behind quantity ``q`` (None: the whole kernel)"""
        return self.masks[int(q.rsplit("_m", 1)[1])] if "_m" in q else None

    def coeffs(self, mask=None):
        return coeffs6(self.coef_real, self.pairs, self.pair_kind, mask)

    def far(self):
        """indices of the two far query times"""
        return np.array([0, len(self.tq) - 1])


def yardstick(c, alpha=None):
    """every quantity of ``c`` by the float64 recurrences of oracle.numpy_port (alpha: its own solve unless given)"""
    full = c.coeffs()
    out = {"alpha": P.celerite_solve(c.t, c.diag, full, c.y) if alpha is None else alpha,
           "z": P.celerite_dot_tril(c.t, c.diag, full, c.x)}
    for i in [None] + list(range(len(c.masks))):
        co, sfx = (full, "") if i is None else (c.coeffs(c.masks[i]), f"_m{i}")
        out["mu_t" + sfx] = P.celerite_predict_mean(c.t, co, out["alpha"], c.t)
        out["mu_q" + sfx] = P.celerite_predict_mean(c.t, co, out["alpha"], c.tq)
        out["var_t" + sfx] = P.celerite_predict_var(c.t, c.diag, full, co, c.t)
        out["var_q" + sfx] = P.celerite_predict_var(c.t, c.diag, full, co, c.tq)
        out["cov_q" + sfx] = P.celerite_predict_cov(c.t, c.diag, full, co, c.tq)
    return out


def error(c, q, got):
    """max |got - want| in the scale of quantity ``q``"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == c.want[q].shape, (c.name, q, got.shape, c.want[q].shape)
    if not np.all(np.isfinite(got)):
        return np.inf
    if not got.size:
        return 0.0
    # (the scale may be an array, one per element: tests/gp_like_cases.py; a zero scale admits only an exact zero)
    d, sc = np.abs(got - c.want[q]), np.broadcast_to(np.asarray(c.scale[q], dtype=np.float64), got.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(sc > 0, d / sc, np.where(d == 0, 0.0, np.inf)).max())


def factor(name, q, table=None):
    return (ENTRY_FACTOR if table is None else table).get((name, q.split("_m")[0]), FACTOR)


def tol(c, q):
    """(a case of another fixture carries its own table of factors as ``ENTRY_FACTOR``)"""
    return max(factor(c.name, q, getattr(c, "ENTRY_FACTOR", None)) * c.unit[q], FLOOR)


def check(label, c, got, skip=()):
    """print unit, tolerance and error of every quantity in ``got`` (dict), then assert them against the fixture; a quantity
    in ``skip`` is printed and not asserted"""
    bad = []
    for q, v in got.items():
        err, tl = error(c, q, v), tol(c, q)
        print(f"{label} {c.name} {q}: unit = {c.unit[q]:.3g}, tolerance = {tl:.3g}, error = {err:.3g}" + (" (not asserted)" if q in skip else ""))
        if q not in skip and not err <= tl:
            bad.append((q, err, tl))
    assert not bad, (label, c.name, bad)
