"""What tools/make_gp_like_golden.py, tests/test_gp_like_host.py and tests/test_gpu_gp_like.py share: the entries of the
multiprecision fixture tests/golden/gp_like_mp.npz -- the celerite log-likelihood and its reverse pass at every state width
J = 1 .. 16 and on every route a draw can take -- the float64 yardstick and the tolerance.

Quantities, per entry (A = K + diag, L its Cholesky factor, alpha = A^-1 y, W = 1/2 (alpha alpha^T - A^-1))
-----------------------------------------------------------------------------------------------------------
    loglike        -1/2 y^T alpha - sum_i log L_ii - N/2 log 2 pi
                   scale: 1/2 |y^T alpha| + 1/2 sum_i |log d_i| + N/2 log 2 pi  (d_i = L_ii^2): the terms that cancel
    gy (N,)        -alpha                                       scale: max |alpha|
    gdiag (N,)     1/2 (alpha_i^2 - (A^-1)_ii)                  scale: max |gdiag|
    greal (Jr, 2)  sum_ij W_ij dK_ij / d(a, c) per real slot
    gpairs (Jc, 4) the same per pair slot: d(a, b, c, d) of a complex term, d(a1, c1, a2, c2) of a kind-1 slot (two real terms)
                   scale, per coefficient: 1/2 |alpha^T dK alpha| + 1/2 |tr(A^-1 dK)|: the two halves that cancel

Yardstick and tolerance
-----------------------
The yardstick is oracle.c_port.celerite(..., grad=True): the published recurrences and their reverse pass in float64.  The
fixture stores ``unit_<quantity>``, the yardstick's error on the entry's float64 inputs against the mpmath value in the scale
above, so a machine with neither mpmath nor the C port can apply the rule of tests/gp_cond_cases.py,

    error <= max(FACTOR * unit, FLOOR)        (FACTOR = 16, FLOOR = 1e-13, imported from there)

and the generator asserts FACTOR * unit <= CAP = 1e-6 for every entry and quantity, with no exception: an entry that breaks
the cap gets milder inputs.

Entries (N = 161 unless its name says otherwise: up to five chunks of at least 32 cadences with a ragged last one)
-------------------------------------------------------------------------------------------------------------------
Irregular times: uniform on 30 days with a gap of 4 days and one repeated stamp; diag varies by 30 % from cadence to cadence,
its smallest value set so that the conditioning score of exo_celerite_core.hpp (elem_lane),
(1 + max (b / a)^2) sum |a| / min diag, is what the entry asks for; ``y`` is a draw from the process (L x' in mpmath, rounded).
  j01 .. j16, j04r   one per state width, real and complex slots mixed, seeded coefficients with |b d| <= a c, score < 3e4
  tree_*, robust_*, seq_*   the routes: J = 2 at 1e6 (trees), J = 5 at 1e5 and 3e7 (robust), J = 2 beyond the robust route
                     and at diag = 0 (no repeated stamp), J = 8 and 10 at 1e5 (sequential redo: the lane groups have no robust route)
  q045, q04999, q05001, matern, kinds_j6    pair kinds: SHO either side of critical damping, Matern32Term's slot, two complex
                     slots next to a kind-1 slot
  cadence, cadence_jitter, bjd_grid, stiff, fast_osc   the time axis: a 2-minute grid, the same with the steps' last bits
                     jittered and a gap, stamps on a 2^-20 d grid at 2 457 000 d, c dt = 30 next to c dt = 1e-3, d dt = 10
  n1, n2, n63, n64, n193_j06, n193_j10    sizes: the edges, either side of the shortest series that is cut, six chunks

Routes (ROUTES, further down) include the two ways the benchmark's configurations reach the likelihood: a cadence-major model and
a sparse mean.  For those this file also holds how the fixture's y reaches kernels that see obs - model with one obs per call
(sparse_obs / entry_model), the builder of sparse layouts and descriptors both the host test and the GPU test use (SPARSE_LAYOUTS,
sparse_segments, sparse_model, sparse_entry, sparse_batch), the hand-filled sparse light curve the wrappers take
(sparse_light_curve), the benign draws of a batch (benign, batch) and the sentinel of the untouched-position check (SENTINEL).
"""
import copy
import os

import numpy as np

from gp_cond_cases import CAP, FACTOR, FLOOR, GOLD, check, coeffs6, sho_slot, tol  # noqa: F401

BJD = 2457000.0
N = 161
SCORE_WIDE, SCORE_J2, SCORE_ROBUST = 3e4, 1e7, 1e8     # EXO_GP_COND_MAX, EXO_GP_COND_MAX_J2, EXO_GP_COND_ROBUST_MAX
LANE_MAX_J = 6                                         # one-lane kernels (and tests/gp_host_harness.cpp) up to this width
QUANTITIES = ("loglike", "gy", "gdiag", "greal", "gpairs")

# (entry, quantity) -> a factor above FACTOR for that entry alone; each needs its cause, measured on the yardstick, in DESIGN.md 17
ENTRY_FACTOR = {}

LAYOUT = {1: (1, 0), 2: (0, 1), 3: (1, 1), 4: (0, 2), 5: (1, 2), 6: (2, 2), 7: (1, 3), 8: (2, 3), 9: (1, 4), 10: (2, 4),
          11: (1, 5), 12: (2, 5), 13: (1, 6), 14: (2, 6), 15: (1, 7), 16: (2, 7)}
FLAGSHIP = (1e-3, 5.0, 1 / np.sqrt(2))
MATERN = (1.0, 3.0, 0.01)        # sigma, rho, eps of Matern32Term

# name -> what the entry is made of.  layout (Jr, Jc): seeded coefficients; sho: (sigma, rho, Q) per pair slot; score: the
# conditioning score the smallest diag is set for (else ``diag`` is that smallest value); axis: irr | cad | cadjit | bjd;
# route: what the default plan does with the draw -- tree, robust or seq(uential redo)
SPEC = {f"j{J:02d}": dict(layout=LAYOUT[J]) for J in range(1, 17)}
SPEC["j04r"] = dict(layout=(2, 1))
SPEC.update({
    "tree_j2_1e6": dict(sho=[(1.0, 3.0, 0.7)], score=1e6),
    "robust_j5_1e5": dict(layout=LAYOUT[5], score=1e5, route="robust"),
    "robust_j5_3e7": dict(layout=LAYOUT[5], score=3e7, route="robust"),
    "seq_j2_1e9": dict(sho=[(1.0, 3.0, 0.7)], score=1e9, route="seq"),
    "seq_j2_diag0": dict(sho=[(1.0, 3.0, 0.7)], diag=0.0, rep=False, route="seq"),
    "seq_j8_1e5": dict(layout=LAYOUT[8], score=1e5, route="seq"),
    "seq_j10_1e5": dict(layout=LAYOUT[10], score=1e5, route="seq"),
    "q045": dict(sho=[(1.0, 3.0, 0.45)], score=1e5),
    "q04999": dict(sho=[(1.0, 3.0, 0.4999)], score=1e6),
    "q05001": dict(sho=[(1.0, 3.0, 0.5001)], score=1e6),
    "matern": dict(matern=True, score=1e6),
    "kinds_j6": dict(layout=(0, 2), sho=[None, None, (0.6, 4.0, 0.3)]),
    "cadence": dict(sho=[FLAGSHIP], diag=2.5e-7, axis="cad"),
    "cadence_jitter": dict(sho=[FLAGSHIP], diag=2.5e-7, axis="cadjit"),
    "bjd_grid": dict(layout=LAYOUT[3], axis="bjd"),
    "stiff": dict(real=[(0.5, 160.0), (0.7, 5e-3)]),
    "fast_osc": dict(pairs=[(1.0, 0.005, 0.3, 53.0)]),
    "n1": dict(layout=LAYOUT[3], n=1, route="seq"),
    "n2": dict(layout=LAYOUT[3], n=2, route="seq"),
    "n63": dict(layout=LAYOUT[3], n=63, route="seq"),
    "n64": dict(layout=LAYOUT[3], n=64),
    "n193_j06": dict(layout=LAYOUT[6], n=193),
    "n193_j10": dict(layout=LAYOUT[10], n=193),
})
ENTRIES = tuple(SPEC)
LADDER = tuple(f"j{J:02d}" for J in range(1, 17)) + ("j04r",)


def route(name):
    return SPEC[name].get("route", "tree")


def seeded(jr, jc):
    """the ladder's coefficients of layout (jr, jc): one seed per layout, amplitudes shared out over the slots"""
    rng = np.random.default_rng(5200 + 16 * jr + jc)
    ns = jr + jc
    real = np.stack([rng.uniform(0.3, 1.5, jr) / ns, rng.uniform(0.05, 2.0, jr)], -1)
    a, c, d = rng.uniform(0.3, 1.5, jc) / ns, rng.uniform(0.05, 1.0, jc), rng.uniform(0.3, 4.0, jc)
    b = rng.uniform(-0.9, 0.9, jc) * a * c / d
    return real, np.stack([a, b, c, d], -1)


def score_terms(real, pairs, kind):
    """((1 + max (b / a)^2), sum |a|) of the conditioning score as elem_lane forms it; a kind-1 slot whose amplitudes are not
    both positive counts (|a1| + |a2|) / (a1 + a2) for b / a"""
    asum, ba2 = float(np.abs(real[:, 0]).sum()), 0.0
    for p, kd in zip(pairs, kind):
        if kd:
            asum += abs(p[0]) + abs(p[2])
            if not (p[0] > 0 and p[2] > 0):
                ba2 = max(ba2, ((abs(p[0]) + abs(p[2])) / (p[0] + p[2])) ** 2)
        else:
            asum += abs(p[0])
            ba2 = max(ba2, (p[1] / p[0]) ** 2)
    return 1.0 + ba2, asum


def inputs(name):
    """the float64 inputs of entry ``name`` that do not need mpmath (the generator adds y): t, diag (N,), coef_real (Jr, 2),
    pairs (Jc, 4), pair_kind (Jc,) int32, xy (N,) white noise (for y)"""
    s = SPEC[name]
    k = ENTRIES.index(name)
    rng = np.random.default_rng(6100 + k)
    n = s.get("n", N)
    real, pairs = np.array(s.get("real", []), dtype=np.float64).reshape(-1, 2), np.array(s.get("pairs", []), dtype=np.float64).reshape(-1, 4)
    kind = np.zeros(len(pairs), np.int32)
    if "layout" in s:
        real, pairs = seeded(*s["layout"])
        kind = np.zeros(len(pairs), np.int32)
    if s.get("matern"):
        sigma, rho, eps = MATERN
        w0 = np.sqrt(3.0) / rho
        S0 = sigma ** 2 / w0
        pairs = np.array([[w0 * S0, w0 * w0 * S0 / eps, w0, eps]])
        kind = np.zeros(1, np.int32)
    for q in s.get("sho", []):
        if q is not None:
            p, kd = sho_slot(*q)
            pairs, kind = np.concatenate([pairs, p[None]]), np.concatenate([kind, [kd]]).astype(np.int32)
    axis = s.get("axis", "irr")
    if axis in ("cad", "cadjit"):
        step = np.full(n - 1, 2.0 / 1440.0)
        if axis == "cadjit":
            step = step * (1.0 + rng.integers(-2, 3, n - 1) * 2.0 ** -51)      # the last bits of every step
            step[n // 3] += 0.05                                               # a gap
        t = np.concatenate([[0.0], np.cumsum(step)])
    else:
        t = np.sort(rng.uniform(0.0, 30.0, n))
        if n >= 8:
            t[n // 3:] += 4.0                       # a gap
            if s.get("rep", True):
                t[n // 2 + 1] = t[n // 2]           # a repeated time stamp
        if axis == "bjd":
            t = BJD + np.round(t * 2.0 ** 20) / 2.0 ** 20
    u = rng.uniform(0.0, 1.0, n)
    u[rng.integers(0, n)] = 0.0                     # the smallest diag is the base itself
    f, asum = score_terms(real, pairs, kind)
    base = f * asum / s["score"] if "score" in s else s.get("diag", 0.05)
    return dict(t=t, diag=base * (1.0 + 0.3 * u), coef_real=real, pairs=pairs, pair_kind=kind, xy=rng.normal(size=n))


def sho_of(name):
    """per pair slot the (sigma, rho, Q) it was built from through SHOTerm, or None (a ComplexTerm from its coefficients)"""
    s = SPEC[name]
    sho = list(s.get("sho", []))
    n_plain = len(s.get("pairs", [])) + (s["layout"][1] if "layout" in s else 0) + (1 if s.get("matern") else 0)
    return [None] * n_plain + [q for q in sho if q is not None]


# ------------------------------------------------------------------------------------------------------------------
def load():
    return np.load(os.path.join(GOLD, "gp_like_mp.npz"))


INPUT_KEYS = ("t", "diag", "coef_real", "pairs", "pair_kind", "y")


class Case:
    """entry ``name`` of the fixture: the inputs as attributes, ``want`` / ``unit`` / ``scale`` dicts over QUANTITIES (the
    scale of greal / gpairs is an array: one per coefficient) -- what gp_cond_cases.check reads"""
    ENTRY_FACTOR = ENTRY_FACTOR

    def __init__(self, g, name):
        self.name = name
        for k in INPUT_KEYS:
            setattr(self, k, g[f"{name}_{k}"])
        self.quantities = QUANTITIES
        self.want = {q: g[f"{name}_{q}"] for q in QUANTITIES}
        self.unit = {q: float(g[f"{name}_unit_{q}"]) for q in QUANTITIES}
        self.scale = {q: g[f"{name}_scale_{q}"] for q in QUANTITIES}
        self.J = len(self.coef_real) + 2 * len(self.pairs)
        self.n = self.t.size

    def coeffs(self):
        return coeffs6(self.coef_real, self.pairs, self.pair_kind)

    def score(self):
        f, asum = score_terms(self.coef_real, self.pairs, self.pair_kind)
        return np.inf if self.diag.min() == 0 else f * asum / self.diag.min()

    def weighted(self, w):
        """the case whose gradients are those of w * loglike (the value itself is not weighted)"""
        c = copy.copy(self)
        c.want = {q: v if q == "loglike" else w * v for q, v in self.want.items()}
        c.scale = {q: v if q == "loglike" else abs(w) * v for q, v in self.scale.items()}
        return c


def slot_grads(c, g):
    """(greal (Jr, 2), gpairs (Jc, 4)) from gradients by the six coefficient arrays of coeffs6 (keys ar .. dc): a kind-1 slot's
    two real terms follow the real slots there"""
    jr = len(c.coef_real)
    greal = np.stack([g["ar"][:jr], g["cr"][:jr]], -1).reshape(jr, 2)
    gpairs, kr, kc = np.zeros((len(c.pairs), 4)), jr, 0
    for s, kd in enumerate(c.pair_kind):
        if kd:
            gpairs[s] = [g["ar"][kr], g["cr"][kr], g["ar"][kr + 1], g["cr"][kr + 1]]
            kr += 2
        else:
            gpairs[s] = [g[k][kc] for k in ("ac", "bc", "cc", "dc")]
            kc += 1
    return greal, gpairs


def quantities_of(c, ll, g):
    greal, gpairs = slot_grads(c, g)
    return {"loglike": np.float64(ll), "gy": np.asarray(g["y"]), "gdiag": np.asarray(g["diag"]), "greal": greal, "gpairs": gpairs}


def yardstick(c):
    """every quantity of ``c`` by the float64 recurrences and their reverse pass (oracle/c/exo_oracle.c)"""
    from oracle import c_port as C

    return quantities_of(c, *C.celerite(c.t, c.y, c.diag, c.coeffs(), grad=True))


# ------------------------------------------------------------------------------------------------------------------
# the routes of tests/test_gpu_gp_like.py: every (entry, route) pair runs or sits in EXCLUDED with its reason
ROUTES = ("default", "one_chunk", "forced", "batch", "obs_minus_model", "gaussian_process", "no_grad", "cadence_major", "sparse_mean")
FORCED = (2, 5)                     # the chunk counts of route "forced" (and of the host pipeline)
BATCH, BATCH_RAGGED = 5, 70         # draws of route "batch"; the entries of RAGGED also in a batch whose last wave is ragged
BATCH_WAVES = 130                   # ... and in one of two full waves and a ragged third
RAGGED = ("j03", "j08", "j10")
# (entry, route) -> (the quantities not asserted -- None: the pair does not run --, the reason).  The tree scans amplify rounding
# by up to the conditioning score x 1e-16 where the score comes from b / a (a term next to critical damping) and, on a cadence
# grid with c dt = 1e-3, lose d / d a with every level of the trees; the sequential kernels do neither (DESIGN.md section 17.4,
# which has the cause; the errors below are those measured on the MI355X, as error / tolerance).  The cadence-major and the
# sparse-mean route run the same scans on the same numbers and inherit these entries, nothing else (DESIGN.md section 17.3 has
# their figures: the same); with n_chunks = 1 the quantities are asserted on those two routes all the same
TREES = ("default", "forced", "batch", "obs_minus_model", "cadence_major", "sparse_mean")
EXCLUDED = {(e, "forced"): (None, "N < 64: chunk_plan does not cut a series that short, whatever n_chunks") for e in ("n1", "n2", "n63")}
EXCLUDED.update({("q05001", r): (("gy", "gdiag", "gpairs"), "tree scans at b / a = 50, score 1e6: gy 5.1e-10 / 3.9e-10, gdiag 1.0e-9 / 5.1e-10, "
                                 "gpairs 1.3e-10 / 1.2e-12") for r in TREES})
EXCLUDED.update({("q04999", r): (("gy", "gdiag", "gpairs"), "tree scans at (|a1| + |a2|) / (a1 + a2) = 50, score 1e6: gy 1.0e-11 / 6.4e-12, "
                                 "gdiag 6.7e-12 / 5.1e-12, gpairs 2.8e-12 / 1.1e-13") for r in TREES})
EXCLUDED.update({("cadence", r): (("gpairs",), "tree scans, five chunks of a 2-minute grid: d / d a 2.6e-13 / 1e-13") for r in TREES})
EXCLUDED.update({("cadence_jitter", r): (("gpairs",), "tree scans, five chunks of a 2-minute grid: d / d a 4.0e-13 / 1.5e-13") for r in TREES})
MAX_EXCLUDED = 0.10
# the same on the host-compiled lane pipeline (tests/test_gp_like_host.py), where Matern32Term's slot (b / a = 58) misses too:
# entry -> the quantities not asserted there (measured: q04999 1.2e-12 / 1.1e-13, q05001 4.0e-12 / 1.2e-12, matern 5.4e-11 / 1.2e-11,
# cadence 2.3e-13 / 1e-13, cadence_jitter 4.7e-13 / 1.5e-13)
HOST_EXCLUDED = {e: ("gpairs",) for e in ("q04999", "q05001", "matern", "cadence", "cadence_jitter")}


def benign(c, rng, D):
    """D benign draws of the layout of ``c`` on its time axis: (y, diag, real, pairs), a kind-1 slot two positive real terms"""
    jr, jc, n = len(c.coef_real), len(c.pairs), c.n
    real = np.stack([rng.uniform(0.3, 1.0, (D, jr)), rng.uniform(0.1, 1.0, (D, jr))], -1)
    a, cc, d = rng.uniform(0.3, 1.0, (D, jc)), rng.uniform(0.1, 0.8, (D, jc)), rng.uniform(0.5, 3.0, (D, jc))
    pairs = np.stack([a, 0.3 * a * cc / d, cc, d], -1)
    k1 = np.broadcast_to(c.pair_kind.astype(bool), (D, jc))
    pairs[k1] = np.stack([a, cc, 0.5 * a, d], -1)[k1]
    return rng.normal(size=(D, n)), rng.uniform(0.07, 0.1, (D, n)), real, pairs


def batch(c, D, at, seed=7):
    """(y, diag, real, pairs) of D draws: the entry at the positions ``at`` between benign draws"""
    y, diag, real, pairs = benign(c, np.random.default_rng(seed), D)
    for d in at:
        y[d], diag[d], real[d], pairs[d] = c.y, c.diag, c.coef_real, c.pairs
    return y, diag, real, pairs


def restricted(c, idx):
    """the case whose gy is held at the cadences ``idx`` alone (a sparse model has a cotangent only where it has a value);
    the scale, max |alpha| over the whole series, stays"""
    r = copy.copy(c)
    r.want = dict(c.want, gy=c.want["gy"][idx])
    return r


# ------------------------------------------------------------------------------------------------------------------
# Routes "cadence_major" and "sparse_mean": the fixture's y has to reach the kernels exactly although they see obs - model with
# one obs for all draws of a call.  For a set H of cadences  obs = where(H, y / 2, y);  a draw that carries the entry has the
# model -y / 2 on H and +0.0 -- or no value at all -- elsewhere: y / 2 - (-y / 2) and y - 0 are exact in float64.  Every
# entry-carrying draw of a call covers the same H (cadence-major: H is everything).
#
# Sparse layouts (exo_sparse_model, include/exoplanet_amd.h), by name, for a series of n cadences -- clipped to it:
#   none       no segment: obs = y, and the whole of gvals stays untouched
#   whole      [0, n)
#   edges      [0, 1) and [n - 1, n)                                  (n = 1: the one cadence once)
#   comb       [i, i + 1) for every even i: the most segments a series can have, an edge on either side of every chunk boundary
#   blocks     [7 k, 7 k + 5) for all k: 7 is prime to the block of four cadences and to every chunk length, so the segment
#              edges meet block and chunk boundaries in every phase
#   blocks3    the same shifted by 3                                  (n <= 3: by n - 1)
#   touching   [0, 40), [40, 41), [41, n): hi_k == lo_(k+1)           (n <= 41: cut at n / 2 instead of 40)
#   padded     H as in blocks, every segment widened by two cadences either side that carry +0.0 -- the gaps between the
#              blocks are two cadences wide, so neighbours would overlap: they meet half way, one cadence each (the outer edges
#              of the first and the last segment get their two, clipped to the series).  A padded cadence has a value: its
#              cotangent is -gy there like anywhere else
# Descriptor forms: "sweep" (seg_step = 4, hi_at = 3: rows of r_max runs (lo, a, b, hi), a, b and the unused runs poisoned) and
# "merged" (seg_step = 2, hi_at = 1).  ``off``: "prefix" (exclusive prefix sums) or "gaps" (the values do not start at 0 and
# leave holes between the segments).  Unused entries of seg and off hold SEG_POISON; every position of vals that no segment
# covers holds NaN -- a kernel that reads one shows it.
SPARSE_LAYOUTS = ("none", "whole", "edges", "comb", "blocks", "blocks3", "touching", "padded")
SPARSE_FORMS = {"sweep": (4, 3), "merged": (2, 1)}      # name -> (seg_step, hi_at)
SPARSE_OFFS = ("prefix", "gaps")
SPARSE_VARIANTS = tuple((f, o) for f in SPARSE_FORMS for o in SPARSE_OFFS)
SPARSE_EVERY_ENTRY = ("whole", "comb", "blocks")        # the layouts every entry takes in every variant (the ladder: all of them)
SEG_POISON = np.iinfo(np.int32).min
SENTINEL = -6.0221407612345678e+299                      # what a cotangent array holds before the call, compared bit for bit


def sparse_segments(layout, n):
    """-> (segments [(lo, hi)], ascending and disjoint, H (n,) bool: the cadences at which an entry-carrying draw holds -y / 2)"""
    H = np.zeros(n, bool)
    if layout == "none":
        segs = []
    elif layout == "whole":
        segs = [(0, n)]
    elif layout == "edges":
        segs = [(0, 1)] + ([(n - 1, n)] if n > 1 else [])
    elif layout == "comb":
        segs = [(i, i + 1) for i in range(0, n, 2)]
    elif layout in ("blocks", "blocks3", "padded"):
        s = min(3, n - 1) if layout == "blocks3" else 0
        segs = [(lo, min(lo + 5, n)) for lo in range(s, n, 7)]
    elif layout == "touching":
        a = 40 if n > 41 else n // 2
        segs = [(lo, hi) for lo, hi in ((0, a), (a, a + 1), (a + 1, n)) if hi > lo]
    else:
        raise KeyError(layout)
    for lo, hi in segs:
        H[lo:hi] = True
    if layout == "padded":
        wide = []
        for k, (lo, hi) in enumerate(segs):
            left = 2 if k == 0 else min(2, (lo - segs[k - 1][1]) // 2)
            right = 2 if k + 1 == len(segs) else min(2, (segs[k + 1][0] - hi + 1) // 2)
            wide.append((max(lo - left, 0), min(hi + right, n)))
        segs = wide
        assert all(a[1] <= b[0] for a, b in zip(segs, segs[1:]))
    return segs, H


class SparseModel:
    """the arrays of an exo_sparse_model for D draws (nseg, seg, off, vals; seg_row, off_row, val_row, seg_step, hi_at), ``H``,
    and per draw ``cad[d]`` / ``pos[d]``: the covered cadences and the positions of their values in row d of vals"""

    def dense(self, d):
        m = np.zeros(self.n)
        m[self.cad[d]] = self.vals[d, self.pos[d]]
        return m

    def untouched(self, d):
        mask = np.ones(self.val_row, bool)
        mask[self.pos[d]] = False
        return mask


def sparse_model(n, draws, form="sweep", offs="prefix", seed=3):
    """``draws``: per draw (layout, model (n,)) -- the model's values at the cadences the layout's segments cover"""
    rng = np.random.default_rng(seed)
    m = SparseModel()
    segs = [sparse_segments(layout, n)[0] for layout, _ in draws]
    D, cap = len(draws), max(len(s) for s in segs) + 2
    m.n, m.D, m.form, m.offs = n, D, form, offs
    m.seg_step, m.hi_at = SPARSE_FORMS[form]
    m.seg_row, m.off_row, m.val_row = cap * m.seg_step, cap + 1, n + (3 * cap + 5 if offs == "gaps" else 0)
    m.nseg = np.array([len(s) for s in segs], np.int32)
    m.seg = np.full((D, cap, m.seg_step), SEG_POISON, np.int32)
    m.off = np.full((D, cap + 1), SEG_POISON, np.int32)
    m.vals = np.full((D, m.val_row), np.nan)
    m.cad, m.pos = [], []
    for d, (sg, (_, model)) in enumerate(zip(segs, draws)):
        at = int(rng.integers(1, 5)) if offs == "gaps" else 0
        cad, pos = [], []
        for k, (lo, hi) in enumerate(sg):
            m.seg[d, k, 0], m.seg[d, k, m.hi_at], m.off[d, k] = lo, hi, at
            m.vals[d, at:at + hi - lo] = model[lo:hi]
            cad.append(np.arange(lo, hi))
            pos.append(np.arange(at, at + hi - lo))
            at += hi - lo + (int(rng.integers(0, 3)) if offs == "gaps" else 0)
        assert at <= m.val_row
        m.cad.append(np.concatenate(cad).astype(np.int64) if cad else np.zeros(0, np.int64))
        m.pos.append(np.concatenate(pos).astype(np.int64) if pos else np.zeros(0, np.int64))
    return m


def entry_model(c, H):
    """the model of a draw that carries the entry: -y / 2 on H, +0.0 elsewhere"""
    return np.where(H, -0.5 * c.y, 0.0)


def sparse_obs(c, H):
    return np.where(H, 0.5 * c.y, c.y)


def sparse_entry(c, layout, form="sweep", offs="prefix"):
    """one draw carrying the entry in ``layout`` -> (obs, SparseModel)"""
    _, H = sparse_segments(layout, c.n)
    m = sparse_model(c.n, [(layout, entry_model(c, H))], form, offs)
    m.H = H
    return sparse_obs(c, H), m


def sparse_batch(c, D, at, form="sweep", offs="prefix", seed=9):
    """D draws: the entry at the positions ``at``, alternately as ``blocks`` and ``padded`` (the same H, other segment counts),
    between benign draws of layouts none / edges / whole / comb / touching with arbitrary values -> (obs, SparseModel)"""
    rng = np.random.default_rng(seed)
    _, H = sparse_segments("blocks", c.n)
    other = ("none", "comb", "edges", "touching", "whole")        # (five draws with the entry at 1 and 3: none, edges, whole)
    draws = [(other[d % len(other)], 0.3 * rng.normal(size=c.n)) for d in range(D)]
    for k, d in enumerate(at):
        draws[d] = (("blocks", "padded")[k % 2], entry_model(c, H))
    m = sparse_model(c.n, draws, form, offs)
    m.H = H
    return sparse_obs(c, H), m


def sparse_light_curve(m, dev):
    """a hand-filled sparse light curve the celerite wrappers take (values, n_draw, n_cad, model_struct()): the arrays of
    SparseModel ``m`` on device ``dev``, ``values`` a leaf that requires a gradient"""
    import torch

    from exoplanet_amd import _lib, ops

    class HandMadeSparseLightCurve(ops.SparseLightCurve):
        def __init__(self):
            self.values = torch.as_tensor(m.vals, device=dev).requires_grad_(True)
            self._tables = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (m.nseg, m.seg, m.off)]
            self.n_cad, self.n_draw, self.n_planet, self.flags, self.shape = m.n, m.D, 1, 0, (m.D, m.n)

        def model_struct(self):
            s = _lib.SparseModel()
            s.nseg, s.seg, s.off = (a.data_ptr() for a in self._tables)
            s.vals = self.values.data_ptr()
            s.seg_row, s.off_row, s.val_row, s.seg_step, s.hi_at = m.seg_row, m.off_row, m.val_row, m.seg_step, m.hi_at
            s.row_of_draw = None
            return s

        def merged(self):
            return self

    return HandMadeSparseLightCurve()


def expected_route(c):
    """what the default plan does with a draw of case ``c``, from the thresholds of exo_celerite_core.hpp"""
    if c.n < 64:
        return "seq"
    s = c.score()
    if s <= (SCORE_J2 if c.J <= 2 else SCORE_WIDE):
        return "tree"
    return "robust" if c.J <= LANE_MAX_J and s <= SCORE_ROBUST else "seq"
