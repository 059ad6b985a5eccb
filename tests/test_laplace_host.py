"""CPU: the arithmetic of exoplanet_amd/csrc/exo_laplace_core.hpp compiled for the host (tests/laplace_harness.cpp) and the torch
statement that runs for CPU tensors (exoplanet_amd/laplace.py), against the long-double numpy statement of the Laplace
approximation (tests/laplace_oracle.py); the chains that must fail; the public `xo.laplace` on an analytic target whose central
difference has a closed form; `metric`, `draws`, `importance`; the argument checks of the C entry points.  The kernels
themselves: tests/test_gpu_laplace.py.

The yardstick is measured (tests/laplace_oracle.py, `ratio`): one unit is the error of the FLOAT64 numpy statement against long
double, at least one eps of the output's scale, and the allowance is 16 units.  Worst ratios measured: host
core 1.61, torch statement 1.77 (both: logdet)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import laplace_oracle as O  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
ALLOWANCE = 16.0
LD = np.longdouble


def build_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "laplace_harness.so")
    srcs = [os.path.join(ROOT, "tests", "laplace_harness.cpp"), os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_laplace_core.hpp"),
            os.path.join(ROOT, "exoplanet_amd", "csrc", "exo_metric_core.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, srcs[0]], check=True)
    lib = ctypes.CDLL(so)
    lib.harness_points.argtypes = [_dp, _i64, _i32, _ip, _i32, _dp, _i32, _dp, ctypes.c_double, _i32, _dp, _dp]
    lib.harness_factor.argtypes = [_dp, _dp, _dp, _i64, _i32, _ip, _i32, _i32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def harness_factor(lib, grad, dx, logp, free, order):
    grad, dx, logp = (np.ascontiguousarray(a, dtype=np.float64) for a in (grad, dx, logp))
    D, _, n = grad.shape
    m = len(free)
    F = np.asarray(free, dtype=np.int32)
    out = {"hess": np.full((D, m, m), 7.0), "cov": np.full((D, m, m), 7.0), "sd": np.full((D, m), 7.0)}
    out.update({k: np.full(D, 7.0) for k in ("logdet", "log_evidence", "asymmetry", "fd_error")})
    out["status"] = np.full(D, -1, dtype=np.int32)
    assert lib.harness_factor(_p(grad), _p(dx), _p(logp), D, n, F.ctypes.data_as(_ip), m, order,
                              *(_p(out[k]) for k in ("hess", "cov", "sd", "logdet", "log_evidence", "asymmetry", "fd_error")),
                              out["status"].ctypes.data_as(_ip)) == 0
    return out


def harness_points(lib, x, free, scale, hess, delta, order):
    x = np.ascontiguousarray(x, dtype=np.float64)
    D, n = x.shape
    m = len(free)
    F = np.asarray(free, dtype=np.int32)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    hess = None if hess is None else np.ascontiguousarray(hess, dtype=np.float64)
    pts, dx = np.full((D, order * m, n), 7.0), np.full((D, order * m), 7.0)
    assert lib.harness_points(_p(x), D, n, F.ctypes.data_as(_ip), m, _p(scale), int(scale is not None and scale.ndim == 2), _p(hess),
                              delta, order, _p(pts), _p(dx)) == 0
    return pts, dx


def _module():
    """exoplanet_amd/laplace.py (`exoplanet_amd.laplace` is the function, as `exoplanet_amd.optimize` is)"""
    import importlib

    return importlib.import_module("exoplanet_amd.laplace")


def torch_factor(grad, dx, logp, free, order):
    L = _module()
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731
    out = L._factor_torch(T(grad), T(dx), T(logp), torch.as_tensor(list(free), dtype=torch.int64), order)
    return {k: v.numpy() for k, v in out.items()}


def check(got, ld, f64, label):
    """every output of a case within the allowance; the status and the symmetry exactly"""
    assert np.array_equal(got["status"], ld["status"]), label
    assert np.array_equal(got["hess"], np.swapaxes(got["hess"], 1, 2)), label
    assert np.array_equal(got["cov"], np.swapaxes(got["cov"], 1, 2), equal_nan=True), label
    worst = {key: O.ratio(got[key], f64[key], ld[key]) for key in O.FLOATS}
    for key, r in worst.items():
        assert r <= ALLOWANCE, (label, key, r)
    return worst


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def cases():
    """per case: the inputs, the statement in long double and in float64, computed once"""
    return [(c, O.statement(c, LD), O.statement(c, np.float64)) for c in O.cases()]


def test_cases_cover_the_sizes_orders_and_conditions(cases):
    assert {c["n"] for c, _, _ in cases} == set(O.SIZES_N)
    assert {c["D"] for c, _, _ in cases} >= set(O.SIZES_D)
    assert {c["order"] for c, _, _ in cases} == {2, 4} and {c["condition"] for c, _, _ in cases} == set(O.CONDITIONS)
    assert any(c["n"] == 7 and c["free"] == list(O.MASKED) for c, _, _ in cases)
    for n in O.SIZES_N:
        assert {c["order"] for c, _, _ in cases if c["n"] == n} == {2, 4}
    for c, ld, _ in cases:
        assert (ld["status"] == O.OK).all()
        assert (ld["asymmetry"] > 0).all() or c["m"] == 1                        # the antisymmetric part is there
        if c["m"] > 1:
            sd = np.asarray(ld["sd"], dtype=np.float64)
            assert sd.max() / sd.min() >= 1e5                                    # parameter scales spread over 1e-5 .. 1e2
            # the scaled matrix C = S H S has about the condition number asked for
            H = np.asarray(ld["hess"][0], dtype=np.float64)
            s = 1.0 / np.sqrt(np.diagonal(H))
            cond = np.linalg.cond(H * np.outer(s, s))
            assert 0.1 * c["condition"] <= cond <= 10.0 * c["condition"], (c["n"], cond)


@pytest.mark.parametrize("which", ["host core", "torch statement"])
def test_factor_against_long_double(harness, cases, which):
    worst = {}
    for c, ld, f64 in cases:
        run = harness_factor if which == "host core" else (lambda lib, *a: torch_factor(*a))
        got = run(harness, c["grad"], c["dx"], c["logp"], c["free"], c["order"])
        for key, r in check(got, ld, f64, (which, c["n"], c["m"], c["D"], c["order"], c["condition"])).items():
            worst[key] = max(worst.get(key, 0.0), r)
    print(f"{which}: worst error in units of the float64 statement's:", {k: round(v, 2) for k, v in worst.items()})


def test_log_fixed_is_a_logarithm(harness):
    """the written-out logarithm behind logdet: a one-coordinate chain's logdet is log H_00; within 2 eps of the long-double log
    (relative, and absolute near 1) over 40 decades"""
    rng = np.random.RandomState(5)
    Hs = np.concatenate([10.0 ** rng.uniform(-20, 20, 400), 1.0 + rng.uniform(-1e-3, 1e-3, 100), [1.0, 2.0, 0.5, np.sqrt(0.5)]])
    D = Hs.size
    dx = np.tile(np.array([1e-3, -1e-3]), (D, 1))
    grad = (-Hs[:, None] * dx)[:, :, None]
    got = harness_factor(harness, grad, dx, np.zeros(D), [0], 2)
    want = np.log(np.asarray(got["hess"][:, 0, 0], dtype=LD))
    err = np.abs(got["logdet"].astype(LD) - want)
    assert (err <= 2.0 * O.EPS * np.maximum(np.abs(want), 1.0 / 16.0)).all(), float((err / np.maximum(np.abs(want), 1.0 / 16.0)).max())


@pytest.mark.parametrize("order", [2, 4])
def test_points(harness, order):
    """the stencil: the host build gives the float64 statement's bits, the torch statement too; pilot and final pass, the three
    kinds of scale, a masked row; a Hessian entry that is not positive keeps the pilot step"""
    L = _module()
    rng = np.random.RandomState(11)
    D, n, free = 3, 7, list(O.MASKED)
    m = len(free)
    x = rng.standard_normal((D, n)) * 10.0 ** rng.uniform(-5, 2, size=n)
    x[0, 2] = 0.0
    hess = np.stack([np.diag(10.0 ** rng.uniform(-4, 10, size=m)) for _ in range(D)])
    hess[1, 2, 2], hess[2, 0, 0] = -1.0, np.nan
    T = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)  # noqa: E731
    for scale in (None, 10.0 ** rng.uniform(-5, 2, size=n), 10.0 ** rng.uniform(-5, 2, size=(D, n))):
        for H in (None, hess):
            want_p, want_dx = O.points(x, free, scale, H, 1e-3, order, np.float64)
            got_p, got_dx = harness_points(harness, x, free, scale, H, 1e-3, order)
            assert np.array_equal(got_p, want_p) and np.array_equal(got_dx, want_dx)
            tp, tdx = L._points_torch(T(x), torch.as_tensor(free), T(scale), T(H), 1e-3, order)
            assert np.array_equal(tp.numpy(), want_p) and np.array_equal(tdx.numpy(), want_dx)
            # one coordinate per row moves, by the realised offset; the others are x's bits
            moved = want_p != x[:, None, :]
            assert (moved.sum(2) == 1).all() and np.array_equal(want_p[moved].reshape(D, -1) - np.tile(x[:, free], order), want_dx)
            if H is not None:
                h = O.steps(x, free, scale, H, 1e-3, np.float64)
                pilot = O.steps(x, free, scale, None, 1e-3, np.float64)
                assert h[1, 2] == pilot[1, 2] and h[2, 0] == pilot[2, 0] and h[0, 0] == 1e-3 / np.sqrt(hess[0, 0, 0])


def _batch_with(failing):
    """three chains of n = 2, order 2: a good one, the failing one, another good one"""
    good = O.case(2, None, 2, 2, 1e2, 77)
    _, _, g, dx = failing
    grad = np.stack([good["grad"][0], g, good["grad"][1]])
    return grad, np.stack([good["dx"][0], dx, good["dx"][1]]), np.array([-3.0, -4.0, -5.0]), good


@pytest.mark.parametrize("failing", O.failing_chains(), ids=lambda f: f[0])
@pytest.mark.parametrize("which", ["host core", "torch statement"])
def test_a_failing_chain_fails_alone(harness, failing, which):
    run = (lambda *a: harness_factor(harness, *a)) if which == "host core" else torch_factor
    grad, dx, logp, good = _batch_with(failing)
    got = run(grad, dx, logp, [0, 1], 2)
    alone = run(good["grad"], good["dx"], logp[[0, 2]], [0, 1], 2)
    assert list(got["status"]) == [O.OK, failing[1], O.OK]
    assert O.factor_chain(failing[2], failing[3], -4.0, [0, 1], 2, LD)["status"] == failing[1]
    for key in ("cov", "sd", "logdet", "log_evidence"):
        assert np.isnan(got[key][1]).all(), key
    assert np.isnan(got["fd_error"][1])                                            # (order 2)
    if failing[0] in ("indefinite", "negative diagonal"):                          # hess and asymmetry are still written
        want = O.factor_chain(failing[2], failing[3], -4.0, [0, 1], 2, np.float64)
        assert np.allclose(got["hess"][1], want["hess"], rtol=1e-14) and np.isfinite(got["asymmetry"][1])
    for key in O.FLOATS + ("status",):                                            # the neighbours: bit for bit what they are without it
        assert np.array_equal(got[key][[0, 2]], alone[key], equal_nan=True), key


# ---- the public interface on the CPU ---------------------------------------------------------------------------------------------
class Target:
    """f(z) = sum_k w_k exp(a_k . (z - c)) - b . (z - c), logp = -f, with b such that the mode is at a chosen z*; parameter scales
    sigma spread over 1e-5 .. 1e2 (a_kj is of the order 1 / sigma_j)"""

    def __init__(self, n=8, K=12, seed=3):
        rng = np.random.RandomState(seed)
        self.n, self.K = n, K
        self.sigma = 10.0 ** np.linspace(-5.0, 2.0, n)
        rng.shuffle(self.sigma)
        self.a = rng.standard_normal((K, n)) / self.sigma
        self.w = rng.uniform(0.5, 2.0, size=K)
        self.c = self.sigma * rng.standard_normal(n)
        self.zstar = self.c + 0.3 * self.sigma * rng.standard_normal(n)
        e = np.exp(self.a.astype(LD) @ (self.zstar - self.c).astype(LD))
        self.b = np.asarray((self.w * e) @ self.a.astype(LD), dtype=np.float64)

    def logp_torch(self, z):
        a, w, c, b = (torch.as_tensor(v, dtype=z.dtype, device=z.device) for v in (self.a, self.w, self.c, self.b))
        u = z - c
        return -((w * torch.exp(u @ a.T)).sum(1) - u @ b)

    def value_and_grad(self, z, dtype):
        """(logp (S,), its gradient (S, n)) at the rows z, in numpy at `dtype`"""
        a, w, c, b = (np.asarray(v, dtype=dtype) for v in (self.a, self.w, self.c, self.b))
        u = np.asarray(z, dtype=dtype) - c
        e = w * np.exp(u @ a.T)
        return -(e.sum(1) - u @ b), -(e @ a - b)

    def hessian(self, z):
        """the true Hessian of f at one point, long double"""
        a = self.a.astype(LD)
        e = self.w * np.exp(a @ (np.asarray(z, dtype=LD) - self.c))
        return (a * e[:, None]).T @ a

    def stencil(self, z, dx, order):
        """what the central difference of the EXACT gradient returns at the realised offsets dx (order m,), long double: every
        term of the Hessian carries (exp(a_kj dx+) - exp(a_kj dx-)) / (dx+ - dx-), i.e. sinh(a_kj h) / (a_kj h) at dx = +-h"""
        a, n = self.a.astype(LD), self.n
        dx = np.asarray(dx, dtype=LD)
        e = self.w * np.exp(a @ (np.asarray(z, dtype=LD) - self.c))

        def raw(s):
            plus, minus = dx[s * n:(s + 1) * n], dx[(s + 1) * n:(s + 2) * n]
            factor = (np.expm1(a * plus) - np.expm1(a * minus)) / (plus - minus)              # [k][j]
            return (a * e[:, None]).T @ factor                                                # [i][j]

        A = raw(0) if order == 2 else (4 * raw(0) - raw(2)) / 3
        return 0.5 * (A + A.T)


def numpy_laplace(target, x, order, delta, passes, dtype):
    """the numpy statement of `xo.laplace` on the target: (the factor's outputs, the last pass's dx)"""
    free = list(range(target.n))
    logp, _ = target.value_and_grad(x, dtype)
    hess = None
    for _ in range(passes):
        pts, dx = O.points(x, free, None, hess, delta, order, dtype)
        D, rows, n = pts.shape
        grad = target.value_and_grad(pts.reshape(D * rows, n), dtype)[1].reshape(D, rows, n)
        out = O.factor(grad, dx, logp, free, order, dtype)
        hess = out["hess"]
    return out, dx


@pytest.fixture(scope="module")
def target():
    return Target()


def _scaled(H, Htrue):
    s = 1.0 / np.sqrt(np.diagonal(np.asarray(Htrue, dtype=LD)))
    return np.asarray(H, dtype=LD) * np.outer(s, s)


@pytest.mark.parametrize("order", [2, 4])
def test_public_laplace_against_the_closed_form(target, order):
    """hess against the closed form of the stencil, in units of the float64 numpy statement's error against it, the matrices
    scaled to a unit diagonal (the parameter scales span seven decades); log_evidence and cov against numpy on the closed form"""
    import exoplanet_amd as xo

    D = 3
    x = np.tile(target.zstar, (D, 1))
    x[1] += 1e-3 * target.sigma                                    # (near the mode is enough for a Hessian)
    x[2] -= 2e-3 * target.sigma
    lap = xo.laplace(target.logp_torch, [torch.as_tensor(x)], order=order, delta=1e-3)
    f64, dx = numpy_laplace(target, x, order, 1e-3, 2, np.float64)
    assert lap.status.tolist() == [0] * D and tuple(lap.hess.shape) == (D, target.n, target.n)
    assert lap.n_eval.tolist() == [1 + 2 * order * target.n] * D and lap.free_index.tolist() == list(range(target.n))
    worst = 0.0
    for d in range(D):
        Htrue = target.hessian(x[d])
        want = target.stencil(x[d], dx[d], order)
        r = O.ratio(_scaled(lap.hess[d].numpy(), Htrue), _scaled(f64["hess"][d], Htrue), _scaled(want, Htrue))
        worst = max(worst, r)
        assert r <= ALLOWANCE, (order, d, r)
        # the stencil's own truncation at delta = 1e-3: 1e-7 at order 2, 1e-12 at order 4, of the scaled matrix
        assert np.abs(_scaled(want, Htrue) - _scaled(Htrue, Htrue)).max() < (3e-7 if order == 2 else 1e-11)
        # cov and log_evidence: numpy on the closed-form Hessian (float64 inversion of a matrix of condition ~1e3 after scaling)
        Hs = np.asarray(_scaled(want, Htrue), dtype=np.float64)
        s = 1.0 / np.sqrt(np.asarray(np.diagonal(Htrue), dtype=np.float64))
        cov = np.linalg.inv(Hs) * np.outer(s, s)
        bound = 64 * O.EPS * np.linalg.cond(Hs)
        assert np.abs(lap.cov[d].numpy() / np.sqrt(np.outer(np.diagonal(cov), np.diagonal(cov))) -
                      cov / np.sqrt(np.outer(np.diagonal(cov), np.diagonal(cov)))).max() <= bound + 1e-9
        logdet = np.linalg.slogdet(Hs)[1] - 2.0 * np.log(s).sum()
        want_ev = float(lap.logp[d]) + 0.5 * target.n * math.log(2 * math.pi) - 0.5 * logdet
        assert abs(float(lap.log_evidence[d]) - want_ev) <= 1e-9 * max(abs(want_ev), 1.0) + bound
        assert np.allclose(lap.sd[d].numpy(), np.sqrt(np.diagonal(lap.cov[d].numpy())), rtol=4 * O.EPS, atol=0)
    print(f"xo.laplace (torch statement), order {order}: worst error of the scaled hess in units of the float64 statement's: {worst:.2f}")


@pytest.mark.parametrize("order", [2, 4])
def test_truncation_error_falls_as_the_closed_form_says(target, order):
    """the error against the TRUE Hessian at delta = 0.1 and 0.05: in the ratio the closed form gives, near 4 (order 2), near 16
    (order 4)"""
    import exoplanet_amd as xo

    x = target.zstar[None, :]
    Htrue = target.hessian(x[0])
    errs, want = [], []
    for delta in (0.1, 0.05):
        lap = xo.laplace(target.logp_torch, [torch.as_tensor(x)], order=order, delta=delta)
        _, dx = numpy_laplace(target, x, order, delta, 2, np.float64)
        errs.append(np.abs(_scaled(lap.hess[0].numpy(), Htrue) - _scaled(Htrue, Htrue)).max())
        want.append(np.abs(_scaled(target.stencil(x[0], dx[0], order), Htrue) - _scaled(Htrue, Htrue)).max())
    got, closed = float(errs[0] / errs[1]), float(want[0] / want[1])
    print(f"order {order}: error ratio delta 0.1 / 0.05 = {got:.4f}, closed form {closed:.4f}")
    assert abs(got - closed) <= 1e-3 * closed
    assert abs(closed - 2.0 ** order) <= 0.05 * 2.0 ** order


def test_passes_scale_and_masks(target):
    import exoplanet_amd as xo

    z = torch.as_tensor(np.tile(target.zstar, (2, 1)))
    one = xo.laplace(target.logp_torch, [z], passes=1, scale=torch.as_tensor(target.sigma))
    assert one.status.tolist() == [0, 0] and one.n_eval.tolist() == [1 + 2 * target.n] * 2
    Htrue = target.hessian(target.zstar)
    assert np.abs(_scaled(one.hess[0].numpy(), Htrue) - _scaled(Htrue, Htrue)).max() < 1e-9        # h = 6e-6 sigma: 1e-11 + rounding
    # two parameter blocks, one element of the second held: the Hessian of the free ones is the sub-matrix
    a, b = z[:, :3].clone(), z[:, 3:].clone()
    mask = torch.ones(5, dtype=torch.float64)
    mask[1] = 0
    fn = lambda a, b: target.logp_torch(torch.cat([a, b], 1))  # noqa: E731
    part = xo.laplace(fn, [a, b], free=[None, mask], delta=1e-3)
    keep = [0, 1, 2, 3, 5, 6, 7]
    assert part.free_index.tolist() == keep and tuple(part.cov.shape) == (2, 7, 7)
    full = xo.laplace(target.logp_torch, [z], delta=1e-3)
    assert np.allclose(_scaled(part.hess[0].numpy(), Htrue[np.ix_(keep, keep)]),
                       _scaled(full.hess[0].numpy()[np.ix_(keep, keep)], Htrue[np.ix_(keep, keep)]), rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="held coordinate has no variance"):
        part.metric()
    rows = part.draws(16, generator=torch.Generator().manual_seed(1))
    assert tuple(rows.shape) == (16, 8) and bool((rows[:, 4] == z[0, 4]).all()) and bool((rows[:, 0] != z[0, 0]).all())
    per_chain = torch.ones(2, 5, dtype=torch.float64)
    per_chain[0, 1] = 0
    with pytest.raises(ValueError, match="same for every chain"):
        xo.laplace(fn, [a, b], free=[None, per_chain])
    with pytest.raises(ValueError):
        xo.laplace(target.logp_torch, [z], order=3)
    with pytest.raises(ValueError, match="MAX_N"):
        xo.laplace(lambda q: -(q * q).sum(1), [torch.zeros(2, 65, dtype=torch.float64)])


def test_a_saddle_fails_alone_and_metric_refuses_it():
    """chain 1 sits at a saddle: status 2, NaN outputs, `best` and `metric` pass it over"""
    import exoplanet_amd as xo

    fn = lambda q: -(0.5 * q[:, 0] ** 2 - torch.cos(q[:, 1]))  # noqa: E731  (minima at q1 = 0, 2 pi; a saddle at q1 = pi)
    start = torch.tensor([[0.0, 0.0], [0.0, math.pi], [0.0, 2.0 * math.pi]], dtype=torch.float64)
    lap = xo.laplace(fn, [start])
    assert lap.status.tolist() == [0, 2, 0] and lap.best() == 0
    assert bool(torch.isnan(lap.cov[1]).all()) and bool(torch.isnan(lap.log_evidence[1])) and bool(torch.isfinite(lap.hess[1]).all())
    with pytest.raises(ValueError, match="no variance to give"):
        lap.metric(1)
    cov, center = lap.metric()
    assert torch.allclose(cov, torch.eye(2, dtype=torch.float64), rtol=1e-8) and tuple(center.shape) == (2,)
    assert abs(float(lap.log_evidence[0]) - (1.0 + math.log(2 * math.pi))) < 1e-8


def test_nuts_accepts_the_metric_of_a_dense_gaussian():
    """n = 8, condition 1e4: `NUTS(cov=, center=)` takes `lap.metric()`, and its chol is the Cholesky factor of the true
    covariance within the allowance -- the unit: float64 numpy inversion + factorisation of the exact Hessian, against long
    double, at least one eps of the factor's scale; the Gaussian's gradient is linear, so the stencil adds rounding only"""
    import exoplanet_amd as xo
    import metric_oracle as M

    rng = np.random.RandomState(21)
    n = 8
    Sigma = M.covariance(n, 1e4, rng)
    P = np.linalg.inv(Sigma)
    P = 0.5 * (P + P.T)                                              # the Hessian IS this float64 matrix
    mu = rng.standard_normal(n)
    Pt, mut = torch.as_tensor(P), torch.as_tensor(mu)
    fn = lambda q: -0.5 * (((q - mut) @ Pt) * (q - mut)).sum(1)  # noqa: E731
    z = torch.as_tensor(np.tile(mu, (2, 1)))
    lap = xo.laplace(fn, [z])
    assert lap.status.tolist() == [0, 0]
    cov, center = lap.metric()
    nuts = xo.NUTS(fn, [z.clone()], step_size=0.5, cov=cov, center=center, graph=False)
    assert torch.equal(nuts.center, torch.as_tensor(mu))

    def chol_of_inverse(dtype):
        inv = np.linalg.inv(P) if dtype is np.float64 else _inverse_ld(P)
        Lf = np.zeros((n, n), dtype=dtype)
        for i in range(n):
            for j in range(i + 1):
                acc = inv[i, j] - (Lf[i, :j] * Lf[j, :j]).sum()
                Lf[i, j] = np.sqrt(acc) if i == j else acc / Lf[j, j]
        return Lf

    ld, f64 = chol_of_inverse(LD), chol_of_inverse(np.float64)
    r = M.ratio(nuts.chol.numpy(), f64, ld)
    print(f"NUTS chol from lap.metric(): {r:.2f} units")
    assert r <= ALLOWANCE


def _inverse_ld(P):
    """the inverse of a small symmetric positive definite matrix in long double (Gauss-Jordan; numpy.linalg has no long double)"""
    n = P.shape[0]
    A = np.concatenate([P.astype(LD), np.eye(n, dtype=LD)], axis=1)
    for i in range(n):
        A[i] = A[i] / A[i, i]
        for j in range(n):
            if j != i:
                A[j] = A[j] - A[j, i] * A[i]
    return A[:, n:]


def test_importance_on_a_quartic_product():
    """a product of three densities exp(-z^2 / 2 - z^4 / 4): pareto_k is `comparison.loo`'s of the same column, bit for bit;
    log_evidence_is at S = 65536 within 6 standard errors of the normaliser (both from quadrature here; fixed seed)"""
    import exoplanet_amd as xo
    from exoplanet_amd import comparison

    fn = lambda q: -(0.5 * q * q + 0.25 * q ** 4).sum(1)  # noqa: E731
    lap = xo.laplace(fn, [torch.zeros(1, 3, dtype=torch.float64)])
    assert lap.status.tolist() == [0] and torch.allclose(lap.cov[0], torch.eye(3, dtype=torch.float64), rtol=1e-7)
    S = 65536
    res = lap.importance(S, generator=torch.Generator().manual_seed(1234))
    rho = res["log_ratio"]
    assert tuple(rho.shape) == (S,)
    k = comparison.loo((-rho)[:, None].contiguous())["pareto_k"][0]
    assert torch.equal(res["pareto_k"], k) and float(k) < 0.7
    # quadrature (trapezoid on a fine grid; the integrands are entire and decay like exp(-z^4 / 4)): Z1 = int exp(-z^2/2 - z^4/4),
    # and under q = N(0, 1) the ratio r = p / q of one factor has E r = Z1, E r^2 = int exp(-z^2/2 - z^4/2) sqrt(2 pi)
    z = np.linspace(-12.0, 12.0, 240001)
    dz = z[1] - z[0]
    Z1 = np.exp(-0.5 * z * z - 0.25 * z ** 4).sum() * dz
    Er2 = np.exp(-0.5 * z * z - 0.5 * z ** 4).sum() * dz * math.sqrt(2 * math.pi)
    # three independent factors: E R = Z1^3, E R^2 = Er2^3; the standard error of log(mean R) by the delta method
    rel_var = Er2 ** 3 / Z1 ** 6 - 1.0
    se = math.sqrt(rel_var / S)
    got = float(res["log_evidence_is"])
    print(f"log_evidence_is = {got:.6f}, normaliser {3 * math.log(Z1):.6f}, se {se:.2e}, k = {float(k):.3f}")
    assert abs(got - 3.0 * math.log(Z1)) <= 6.0 * se
    # the Laplace evidence itself is off by the quartic term, by far more than that
    assert abs(float(lap.log_evidence[0]) - 3.0 * math.log(Z1)) > 100 * se


def test_entry_points_reject_bad_arguments():
    """on the host, before any launch (no GPU needed: the pointers are never followed)"""
    import re

    import __graft_entry__ as g

    g.build()
    from exoplanet_amd import _lib

    L = _module()
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_[A-Z0-9_]+)\s+(\d+)u?\b", text))
    assert int(consts["EXO_LAPLACE_MAX_N"]) == L.MAX_N == 64
    assert [int(consts[f"EXO_LAPLACE_STATUS_{k}"]) for k in ("OK", "NOT_FINITE", "NOT_POSITIVE")] == \
        [L.STATUS_OK, L.STATUS_NOT_FINITE, L.STATUS_NOT_POSITIVE] == [O.OK, O.NOT_FINITE, O.NOT_POSITIVE]
    INVALID, p = 1, 0x1000
    points = lambda D=4, n=8, m=8, order=2, x=p, F=p, hess=None, delta=1e-3, out=p, dx=p: lib.exo_laplace_points_f64(  # noqa: E731
        x, D, n, F, m, None, 0, hess, delta, order, out, dx, None)
    factor = lambda D=4, n=8, m=8, order=2, grad=p, status=p: lib.exo_laplace_factor_f64(  # noqa: E731
        grad, p, p, D, n, p, m, order, p, p, p, p, p, p, p, status, None)
    for call in (points, factor):
        assert call(m=0) == INVALID and call(m=9) == INVALID and call(n=65, m=65) == INVALID and call(n=65, m=8) == INVALID
        assert call(order=3) == INVALID and call(order=0) == INVALID and call(D=-1) == INVALID
        assert call(D=0) == 0                                                     # no chains: nothing to do
    assert points(x=None) == INVALID and points(F=None) == INVALID and points(out=None) == INVALID and points(dx=None) == INVALID
    assert points(hess=p, delta=0.0) == INVALID and points(hess=p, delta=float("nan")) == INVALID
    assert factor(grad=None) == INVALID and factor(status=None) == INVALID
    assert lib.exo_laplace_points_f64(None, 0, 8, None, 8, None, 0, None, 0.0, 2, None, None, None) == 0
