"""What the tests of exoplanet_amd.optimize share: the test problems with their conditions (tests/test_optimize.py on the CPU,
tests/test_gpu_optimize.py on the device), and the single-call cases of the two phases behind tests/golden/lbfgs_phase.npz
(written by tests/make_optimize_golden.py; tests/test_optimize_host.py, tests/test_gpu_optimize.py)."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lbfgs_phase.npz")

# ---- the problems ------------------------------------------------------------------------------------------------------------


def quadratic(D, device="cpu", seed=1):
    """f = x'Ax/2 - b'x, n = 8, eigenvalues logspace(0, 3, 8) in a random orthogonal basis; D starts at 3 randn"""
    gen = torch.Generator().manual_seed(seed)
    n = 8
    Q, _ = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=gen))
    A = (Q * torch.logspace(0, 3, n, dtype=torch.float64)) @ Q.T
    A = 0.5 * (A + A.T)
    b = torch.randn(n, dtype=torch.float64, generator=gen)
    x0 = 3.0 * torch.randn(D, n, dtype=torch.float64, generator=gen)
    A, b, x0 = A.to(device), b.to(device), x0.to(device)

    def f(x):          # (elementwise products and sums only: the same kernels eagerly and in a captured tick)
        return 0.5 * ((x.unsqueeze(2) * A).sum(1) * x).sum(1) - (x * b).sum(1)

    return dict(logp=lambda x: -f(x), f=f, x0=x0, A=A, b=b)


def check_quadratic(prob, x, status, n_eval, held=()):
    """every status 1 or 2, (f - f*) / (f0 - f*) <= 1e-8 against the solved optimum, at most 400 evaluations; ``held``: columns
    that were masked -- bit-identical, the others at the optimum of the restricted problem to 1e-5 relative"""
    A, b, x0 = prob["A"].cpu(), prob["b"].cpu(), prob["x0"].cpu()
    x, status, n_eval = x.cpu(), status.cpu(), n_eval.cpu()
    f = lambda v: 0.5 * ((v @ A) * v).sum(1) - v @ b  # noqa: E731
    assert bool(((status == 1) | (status == 2)).all()), status
    assert int(n_eval.max()) <= 400, n_eval
    if not held:
        fstar = f(torch.linalg.solve(A, b)[None])
        gap = (f(x) - fstar) / (f(x0) - fstar)
        print("quadratic: largest (f - f*) / (f0 - f*) = %.3g, evaluations %d-%d" % (gap.max(), n_eval.min(), n_eval.max()))
        assert float(gap.max()) <= 1e-8, gap
        return
    held = list(held)
    move = [i for i in range(A.shape[0]) if i not in held]
    assert torch.equal(x[:, held], x0[:, held])
    # the restricted problem, solved directly per chain: A_mm x_m = b_m - A_mh x_h
    want = torch.linalg.solve(A[move][:, move], (b[move][None] - x0[:, held] @ A[held][:, move]).T).T
    err = (x[:, move] - want).abs().amax(1) / want.abs().amax(1)
    print("quadratic, held columns: largest relative error of the restricted optimum = %.3g, evaluations %d-%d"
          % (err.max(), n_eval.min(), n_eval.max()))
    assert float(err.max()) <= 1e-5, err


def rosenbrock(D, device="cpu", seed=2):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.tensor([-1.2, 1.0], dtype=torch.float64) + 0.5 * torch.randn(D, 2, dtype=torch.float64, generator=gen)

    def f(x):
        return 100.0 * (x[:, 1] - x[:, 0] ** 2) ** 2 + (1.0 - x[:, 0]) ** 2

    return dict(logp=lambda x: -f(x), f=f, x0=x0.to(device))


def check_rosenbrock(x, status, n_eval):
    x, status, n_eval = x.cpu(), status.cpu(), n_eval.cpu()
    print("rosenbrock: largest |x - 1| = %.3g, evaluations %d-%d" % ((x - 1).abs().max(), n_eval.min(), n_eval.max()))
    assert bool(((status == 1) | (status == 2)).all()), status
    assert float((x - 1).abs().max()) <= 1e-4
    assert int(n_eval.max()) <= 250, n_eval


# ---- single calls of the two phases --------------------------------------------------------------------------------------------
# A case is the state of ONE chain before a call (history of 3 pairs) and the scalars of the call; the fixture holds, per
# case, these inputs and the outputs of the long double build of exo_optimize_core.hpp rounded to double.
HIST = 3
FLOATS = ("x", "g", "xt", "gt", "d", "hs", "hy", "hsy", "logp", "alpha", "gamma", "grad_max")      # outputs that are compared
INTS = ("status", "n_iter", "n_eval", "m", "head", "n_rej", "n_small")
SCALARS = ("max_linesearch", "c1", "gtol", "ftol", "phase")
MARGIN = 1e-6                  # no decision of a case hinges on less than this, relative (asserted by the generator)


def _state(rng, n, m=0, head=0, free=None):
    """a chain in mid-run: m pairs of positive curvature from a random positive definite quadratic, a descent direction"""
    B = rng.normal(size=(n, n))
    B = B @ B.T / n + np.eye(n)
    x, g = rng.normal(size=n), rng.normal(size=n)
    free = np.ones(n) if free is None else np.asarray(free, dtype=np.float64)
    g = g * free
    hs, hy, hsy = np.zeros((HIST, n)), np.zeros((HIST, n)), np.zeros(HIST)
    slots = [(head - 1 - j) % HIST for j in range(m)]
    for k in slots:
        hs[k] = 0.3 * rng.normal(size=n) * free
        hy[k] = (B @ hs[k]) * free
        hsy[k] = hs[k] @ hy[k]
    gamma = hsy[slots[0]] / (hy[slots[0]] @ hy[slots[0]]) if m else 1.0
    d = -g * (0.5 + rng.random(n))                         # some descent direction (what it was computed from does not matter)
    alpha = 0.25
    c = dict(n=n, x=x, g=g, xt=x + alpha * d, gt=np.zeros(n), d=d, free=free, hs=hs, hy=hy, hsy=hsy, coef=np.zeros(HIST),
             logp=-3.7, lpt=0.0, alpha=alpha, gamma=gamma, grad_max=np.abs(g).max(), status=0, n_iter=4, n_eval=9, m=m, head=head,
             n_rej=0, n_small=0, max_linesearch=20, c1=1e-4, gtol=1e-5, ftol=2.220446049250313e-09, phase=1)
    c["_B"] = B
    return c


def _trial(c, kind, rng):
    """fill in the evaluation at the trial point: ``gt`` is the gradient of logp as evaluated (unmasked, sign of logp)"""
    n, f, B = c["n"], -c["logp"], c.pop("_B")
    s = c["xt"] - c["x"]
    gd = c["g"] @ c["d"]
    armijo = f + c["c1"] * c["alpha"] * gd
    gt_f = c["g"] + B @ s                                   # gradient of f at xt for the quadratic: positive curvature
    ft = armijo - 0.3 * abs(c["alpha"] * gd)                # accepted with room
    if kind == "reject":
        ft = armijo + 0.2 * abs(c["alpha"] * gd)
    elif kind == "skip":                                     # negative curvature along s: the pair is not stored, the history goes
        gt_f = c["g"] - B @ s
    elif kind == "stop_gtol":
        gt_f = 1e-7 * rng.normal(size=n)
    elif kind == "stop_ftol":
        c["ftol"] = 1e-3
        c["logp"] = -4.0e4
        f = 4.0e4
        ft = f + c["c1"] * c["alpha"] * gd - 1.0             # a decrease of ~1 in 4e4: below ftol = 1e-3, relative
    elif kind == "nan_value":
        ft = np.nan
    elif kind == "inf_grad":
        gt_f = gt_f.copy()
        gt_f[n // 2] = np.inf
    # a masked column's evaluated gradient is whatever the model gives: it must not matter
    c["gt"] = -gt_f + (1.0 - c["free"]) * rng.normal(size=n)
    c["lpt"] = -ft
    return c


def cases():
    rng = np.random.default_rng(20261019)
    mask13 = np.ones(13)
    mask13[[1, 4, 12]] = 0.0
    out = {}

    def start(name, n, lpt=-2.5, gscale=1.0, free=None):
        c = _state(rng, n, free=free)
        c.pop("_B")
        c.update(phase=0, xt=c["x"].copy(), gt=gscale * rng.normal(size=n), lpt=lpt, status=3, n_iter=7, n_eval=5, m=2, head=1,
                 n_rej=6, n_small=2)              # (whatever the counters held: phase 0 sets them)
        out[name] = c

    start("start_n5", 5)
    start("start_small_gradient_n1", 1, gscale=0.3)            # sum |g| < 1: the first step is 1
    start("start_big_gradient_n13", 13, gscale=40.0, free=mask13)
    start("start_converged_n1", 1, gscale=1e-7)
    start("start_value_not_finite_n5", 5, lpt=-np.inf)
    start("start_gradient_not_finite_n5", 5)
    out["start_gradient_not_finite_n5"]["gt"][2] = np.nan

    def decide(name, n, kind, m=0, head=0, free=None, **over):
        c = _state(rng, n, m=m, head=head, free=free)
        c.update(over)
        out[name] = _trial(c, kind, rng)

    decide("accept_first_pair_n5", 5, "accept")
    decide("accept_one_pair_n1", 1, "accept", m=1, head=1)
    decide("accept_two_pairs_n13", 13, "accept", m=2, head=2, free=mask13, n_small=2)     # (a run of small decreases ends)
    decide("accept_full_history_n5", 5, "accept", m=3, head=0)
    decide("accept_wrapped_n13", 13, "accept", m=3, head=1)
    decide("accept_curvature_skip_n5", 5, "skip", m=2, head=2)
    decide("accept_curvature_skip_no_history_n13", 13, "skip")
    # pairs that the store rule would never keep -- negative curvature, and gradient differences so small that their terms
    # outweigh the first scaling: H is not positive definite
    decide("accept_not_descent_n5", 5, "accept", m=2, head=0)
    c = out["accept_not_descent_n5"]
    c.update(hy=-0.01 * c["hy"], hsy=-0.01 * c["hsy"])
    decide("reject_n13", 13, "reject", m=2, head=1, n_rej=3)
    decide("reject_limit_with_history_n5", 5, "reject", m=2, head=2, n_rej=19)
    decide("reject_limit_without_history_n1", 1, "reject", n_rej=4, max_linesearch=5)
    decide("reject_limit_without_history_n5", 5, "reject", n_rej=19)
    decide("stop_gradient_n5", 5, "stop_gtol", m=3, head=2)
    decide("stop_value_n13", 13, "stop_ftol", m=2, head=2, n_small=2)              # the third small decrease in a row (history 3)
    decide("stop_value_waits_n13", 13, "stop_ftol", m=1, head=1, n_small=1)        # the second: the chain goes on
    decide("stop_value_waits_masked_n5", 5, "stop_ftol", m=1, head=1, n_small=1, free=[1.0, 0.0, 0.0, 1.0, 0.0])
    decide("reject_limit_after_small_decrease_n5", 5, "reject", n_rej=19, n_small=1)      # the rounding of f, not an obstacle: status 2
    decide("trial_value_nan_n5", 5, "nan_value", m=2, head=2)
    decide("trial_gradient_inf_n13", 13, "inf_grad", m=3, head=1, free=mask13)
    decide("stopped_chain_n5", 5, "accept", m=2, head=2, status=2)
    return out


def margins(c, out):
    """the relative margins of the decisions that the call on case ``c`` (outputs ``out``) took; all must exceed MARGIN"""
    res = {}
    if c["status"] != 0 and c["phase"] == 1:
        return res
    gtf = np.where(c["free"] != 0, -c["gt"] * c["free"], 0.0)
    gmax = np.abs(gtf).max()
    finite = bool(np.isfinite(gtf).all() and np.isfinite(c["lpt"]))
    if c["phase"] == 0:
        if finite:
            res["gtol"] = abs(gmax - c["gtol"]) / c["gtol"]
            res["first_step"] = abs(np.abs(gtf).sum() - 1.0)
        return res
    if not finite:
        return res
    f, ft = -c["logp"], -c["lpt"]
    bound = f + c["c1"] * c["alpha"] * (c["g"] @ c["d"])
    res["armijo"] = abs(ft - bound) / max(abs(f), abs(ft), 1.0)
    if ft > bound:
        return res
    s, y = c["xt"] - c["x"], gtf - c["g"]
    res["curvature"] = abs(s @ y) / (np.linalg.norm(s) * np.linalg.norm(y))
    res["gtol"] = abs(gmax - c["gtol"]) / c["gtol"]
    if gmax > c["gtol"]:
        scale = c["ftol"] * max(abs(f), abs(ft), 1.0)
        res["ftol"] = abs((f - ft) - scale) / scale
        if out["status"] == 0:
            res["first_step"] = abs(np.abs(gtf).sum() - 1.0)
            if c["m"] > 0 or out["m"] > 0:
                # the two-loop direction's slope (for a reset: of the direction that was refused, recomputed here in numpy)
                res["descent"] = abs(_two_loop_slope(c, out, gtf))
    return res


def _two_loop_slope(c, out, g):
    """d.g / (|d| |g|) of the two-loop direction after the call's history update"""
    hs, hy, hsy = out["hs"], out["hy"], out["hsy"]
    head = int(out["head"])
    m = min(int(c["m"]) + (1 if int(out["head"]) != int(c["head"]) else 0), HIST)
    gamma = out["gamma"]
    q = g.astype(np.longdouble)
    coef = []
    for j in range(m):
        k = (head - 1 - j) % HIST
        a = (hs[k] @ q) / hsy[k]
        coef.append(a)
        q = q - a * hy[k]
    slots = [(head - 1 - j) % HIST for j in range(m)]
    num, den = sum(hs[k] * hy[k] for k in slots), sum(hy[k] * hy[k] for k in slots)
    fits = (num > 0) & (den > 0)
    r = np.where(fits, num / np.where(fits, den, 1.0), gamma) * q
    for j in reversed(range(m)):
        k = (head - 1 - j) % HIST
        r = r + (coef[j] - (hy[k] @ r) / hsy[k]) * hs[k]
    d = -r
    return float((d @ g) / (np.linalg.norm(d.astype(np.float64)) * np.linalg.norm(g)))


# ---- the host build of the core ----------------------------------------------------------------------------------------------
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "optimize_harness.so")
    srcs = [os.path.join(ROOT, "tests", "optimize_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_optimize_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_phase.restype = None
    lib.harness_phase.argtypes = [ctypes.c_int] + [_dp] * 15 + [_ip] * 7 + [ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.c_int]
    return lib


_ORDER = ("x", "g", "xt", "gt", "d", "free", "hs", "hy", "hsy", "coef", "logp", "lpt", "alpha", "gamma", "grad_max")


def run_harness(lib, c, long_double):
    """one call on a copy of the case's state -> dict of the state afterwards"""
    st = {k: np.ascontiguousarray(np.array(c[k], dtype=np.float64, ndmin=1)).copy() for k in _ORDER}
    it = {k: np.array([c[k]], dtype=np.int32) for k in INTS}
    lib.harness_phase(int(long_double), *[st[k].ctypes.data_as(_dp) for k in _ORDER], *[it[k].ctypes.data_as(_ip) for k in INTS],
                      int(c["n"]), HIST, int(c["max_linesearch"]), float(c["c1"]), float(c["gtol"]), float(c["ftol"]), int(c["phase"]))
    res = {k: (v if np.ndim(c[k]) else v[0]) for k, v in st.items()}
    res.update({k: int(v[0]) for k, v in it.items()})
    return res


def load():
    """the fixture as {case: (inputs, expected outputs)} and E_host"""
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files if "/" in k})
    got = {}
    for name in names:
        c = {k.split("/")[2]: z[k] for k in z.files if k.startswith(name + "/in/")}
        w = {k.split("/")[2]: z[k] for k in z.files if k.startswith(name + "/out/")}
        for d in (c, w):
            for k, v in d.items():
                if v.ndim == 0:
                    d[k] = v.item()
        got[name] = (c, w)
    return got, float(z["E_host"])


def float_error(got, want):
    """largest error of the compared float outputs, each relative to the largest magnitude in its array (for the direction:
    max |d|; an array of zeros must be met exactly); an entry that is not finite must match as it is"""
    worst = 0.0
    for k in FLOATS:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        fin = np.isfinite(b)
        assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], b[~fin], equal_nan=True), k
        if fin.any():
            worst = max(worst, float(np.abs(a[fin] - b[fin]).max() / (np.abs(b[fin]).max() or 1.0)))
    return worst
