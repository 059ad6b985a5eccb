"""GPU: exoplanet_amd.optimize on the device -- the two kernels of exo_lbfgs_f64 against the long double fixture
tests/golden/lbfgs_phase.npz (batched to 97 chains, a tail wave, chains that have stopped mixed in), the native optimiser
eager and as a replayed hipGraph and the torch statement on the problems of tests/test_optimize.py, and the MAP of an
injected transit through a ParameterSpace in the two stages of the reference's tutorials."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optimize_cases as K

pytestmark = pytest.mark.gpu

ULP = 2.220446049250313e-16
D_BATCH = 97


def _batches(cases):
    """the cases grouped by what a launch shares (n, phase and the scalars), each group dealt over D_BATCH chains; in
    phase 1 every fifth chain is a copy that has stopped: its row must come back bit for bit"""
    groups = {}
    for name, (c, want) in sorted(cases.items()):
        groups.setdefault((c["n"],) + tuple(c[k] for k in K.SCALARS), []).append((c, want))
    for key, members in sorted(groups.items()):
        chains = []
        for d in range(D_BATCH):
            c, want = members[d % len(members)]
            if c["phase"] == 1 and d % 5 == 3:
                c = dict(c, status=1 + d % 3)
                want = {k: c[k] for k in K.FLOATS + K.INTS}
            chains.append((c, want))
        yield key, chains


def test_phase_kernels_against_the_fixture(dev):
    from exoplanet_amd import _lib

    lib = _lib.load()
    cases, e_host = K.load()
    tol = max(4 * e_host, 16 * ULP)
    worst, n_frozen = 0.0, 0
    order = ("x", "g", "xt", "gt", "d", "free", "hs", "hy", "hsy", "coef", "logp", "lpt", "alpha", "gamma", "grad_max") + K.INTS
    for key, chains in _batches(cases):
        n, phase = key[0], chains[0][0]["phase"]
        host = {}
        for k in order:
            a = np.stack([np.asarray(c[k]) for c, _ in chains])                  # (D, ...) chain-major
            if k in ("hs", "hy"):
                a = a.transpose(1, 2, 0)                                          # [hist][n][D]
            elif k in ("hsy", "coef"):
                a = a.T                                                           # [hist][D]
            host[k] = np.ascontiguousarray(a, dtype=np.int32 if k in K.INTS else np.float64)
        st = {k: torch.as_tensor(v).to(dev) for k, v in host.items()}
        ptrs = (ctypes.c_void_p * len(order))(*[st[k].data_ptr() for k in order])
        c0 = chains[0][0]
        _lib.check(lib.exo_lbfgs_f64(ptrs, D_BATCH, n, K.HIST, int(c0["max_linesearch"]), float(c0["c1"]), float(c0["gtol"]),
                                     float(c0["ftol"]), int(phase), torch.cuda.current_stream(dev).cuda_stream), "exo_lbfgs_f64")
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in st.items()}
        for d, (c, want) in enumerate(chains):
            got = {k: (out[k][:, :, d] if k in ("hs", "hy") else out[k][:, d] if k == "hsy" else out[k][d]) for k in K.FLOATS + K.INTS}
            assert {k: int(got[k]) for k in K.INTS} == {k: int(want[k]) for k in K.INTS}, (key, d)
            if phase == 1 and c["status"] != 0:
                n_frozen += 1
                for k in K.FLOATS:
                    assert np.array_equal(got[k], np.asarray(c[k])), (key, d, k)
            worst = max(worst, K.float_error(got, want))
    print(f"phase kernels: largest error {worst:.2e} against the long double values (E_host {e_host:.2e}, bound {tol:.2e}); "
          f"{n_frozen} stopped chains")
    assert n_frozen > 50 and worst <= tol


def _three_ways(prob, dev):
    """(x, status, n_eval, logp) of the native optimiser replayed as a graph, launched eagerly, and of the torch statement"""
    from exoplanet_amd.optimize import LBFGS

    out = {}
    for mode, kw in (("graph", {}), ("eager", dict(graph=False)), ("torch", dict(native=False))):
        opt = LBFGS(prob["logp"], [prob["x0"].clone()], **kw)
        assert (opt._graph is not None) == (mode == "graph") and (opt._native is not None) == (mode != "torch")
        opt.run()
        out[mode] = (opt.params[0].clone(), opt.status.clone(), opt.n_eval.clone(), opt.logp.clone(), opt.n_iter.clone())
    for a, b in zip(out["graph"], out["eager"]):
        assert torch.equal(a, b)
    return out


def test_quadratic_native_graphed_eager_and_torch(dev):
    prob = K.quadratic(D_BATCH, device=dev)
    for mode, (x, status, n_eval, _, _) in _three_ways(prob, dev).items():
        print(mode, end=" ")
        K.check_quadratic(prob, x, status, n_eval)


def test_rosenbrock_native_graphed_eager_and_torch(dev):
    prob = K.rosenbrock(D_BATCH, device=dev)
    for mode, (x, status, n_eval, _, _) in _three_ways(prob, dev).items():
        print(mode, end=" ")
        K.check_rosenbrock(x, status, n_eval)


def test_held_columns_and_max_evals_on_the_device(dev):
    from exoplanet_amd.optimize import LBFGS

    prob = K.quadratic(D_BATCH, device=dev)
    free = torch.ones(8, dtype=torch.float64)
    free[[1, 4]] = 0.0
    opt = LBFGS(prob["logp"], [prob["x0"].clone()], free=[free]).run()
    K.check_quadratic(prob, opt.params[0], opt.status, opt.n_eval, held=(1, 4))
    short = LBFGS(prob["logp"], [prob["x0"].clone()]).run(max_evals=7, check_every=4)
    assert short.n_ticks == 6 and short.n_eval.tolist() == [7] * D_BATCH


# ---- an injected transit ------------------------------------------------------------------------------------------------------
TRUTH = dict(t0=1.0, r=0.1, b=0.3, mean=0.0, log_jitter=math.log(4e-4))
N_CAD, D_MAP = 8000, 16


@pytest.fixture(scope="module")
def transit(dev):
    return transit_model(dev)


def transit_model(dev):
    import exoplanet_amd as xo
    from exoplanet_amd import distributions as xd

    rng = np.random.default_rng(71)
    t = torch.arange(N_CAD, dtype=torch.float64, device=dev) * (2.0 / 1440.0)
    T = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)   # noqa: E731
    lc = xo.LimbDarkLightCurve(0.3, 0.2)
    with torch.no_grad():
        f0 = lc.get_light_curve(orbit=xo.KeplerianOrbit(period=T(3.5), t0=T(TRUTH["t0"]), b=T(TRUTH["b"])), r=T(TRUTH["r"]), t=t)[:, 0]
    yerr = 3e-4                                                       # (with the jitter of 4e-4: a scatter of 5e-4)
    y = f0 + 5e-4 * torch.as_tensor(rng.normal(size=N_CAD), device=dev)
    space = xd.ParameterSpace(t0=xd.normal(1.0, 0.1), r=xd.uniform(0.01, 0.3), b=xd.impact_parameter(ror="r"),
                              mean=xd.normal(0.0, 1e-2), log_jitter=xd.normal(math.log(4e-4), 2.0), device=dev)

    def loglike(t0, r, b, mean, log_jitter):
        return lc.white_noise_log_likelihood(orbit=xo.KeplerianOrbit(period=3.5, t0=t0, b=b), r=r, t=t, y=y, yerr=yerr, mean=mean,
                                             jitter=torch.exp(log_jitter))

    g = np.random.default_rng(72)
    col = lambda v: torch.tensor(v).reshape(D_MAP, 1)  # noqa: E731
    # a few posterior standard deviations off (t0: ~2e-4, r: ~5e-4, b: ~0.05, mean: ~6e-6, log_jitter: ~0.01)
    z0 = space.unconstrain(D_MAP, t0=col(1.0 + 6e-4 * g.normal(size=D_MAP)), r=col(0.1 * (1 + 0.015 * g.normal(size=D_MAP))),
                           b=col(np.clip(0.3 + 0.1 * g.normal(size=D_MAP), 0.05, 0.6)), mean=col(2e-5 * g.normal(size=D_MAP)),
                           log_jitter=col(math.log(4e-4) + 0.05 * g.normal(size=D_MAP)))
    return dict(space=space, logp=space.wrap(loglike), z0=z0, z_truth=space.unconstrain(1, **TRUTH))


def test_map_of_an_injected_transit_in_two_stages(dev, transit):
    """Stage one frees t0 and r, stage two everything; statuses 1 or 2, every chain ends above the log-posterior of the truth, the
    held columns are bit-identical after stage one, and the chains agree to 1e-3.  Measured on the MI355X: 17-83 evaluations in
    stage one, 40-98 in stage two; the truth at 49579.977, all 16 chains at 49585.000751 with a spread of 1.1e-9.  In the
    unconstrained coordinates the curvatures run from ~1e2 (b) to ~3e6 (mean): what gets every chain there is the per-column
    first scaling of the two-loop recursion (with one scalar the chains ended up to 1.5 apart)."""
    import exoplanet_amd as xo

    space, logp, z0 = transit["space"], transit["logp"], transit["z0"]
    mask = space.free_mask(["t0", "r"])
    assert mask.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    z1, info1 = xo.optimize(logp, [z0], free=[mask], return_info=True)
    assert torch.equal(z1[0][:, 2:], z0[:, 2:]) and not torch.equal(z1[0][:, :2], z0[:, :2])
    z2, info = xo.optimize(logp, z1, return_info=True)
    with torch.no_grad():
        lp_truth = float(logp(transit["z_truth"])[0])
        lp_start = logp(z0)
    lp = info["logp"]
    print("transit MAP: evaluations stage one %d-%d, stage two %d-%d; logp at the starts %.1f .. %.1f, at the truth %.3f, final "
          "%.6f .. %.6f (spread %.2e)" % (info1["n_eval"].min(), info1["n_eval"].max(), info["n_eval"].min(), info["n_eval"].max(),
                                          lp_start.min(), lp_start.max(), lp_truth, lp.min(), lp.max(), lp.max() - lp.min()))
    for i in (info1, info):
        assert bool(((i["status"] == 1) | (i["status"] == 2)).all()), i["status"]
    assert bool((info1["logp"] >= lp_start).all())
    assert bool((lp >= lp_truth).all())
    assert float(lp.max() - lp.min()) <= 1e-3
    theta, _ = space.constrain(z2[0])
    assert float((theta["t0"] - TRUTH["t0"]).abs().max()) < 1e-3 and float((theta["r"] - TRUTH["r"]).abs().max()) < 5e-3


def test_a_chain_outside_the_support_is_never_moved_and_disturbs_nobody(dev, transit):
    """a wall as in tests/test_gpu_inject_recover.py: log-density -inf where t0 lies beyond it; the chain that starts there gets
    status 4 and keeps its row, the rows of the others are what they are without it"""
    import exoplanet_amd as xo

    logp, z0 = transit["logp"], transit["z0"]
    wall = float(z0[:, 0].max()) + 1.0

    def walled(z):
        lp = logp(z)
        return torch.where(z[:, 0] > wall, torch.full_like(lp, -float("inf")), lp)

    mask = transit["space"].free_mask(["t0", "r"])
    za = z0.clone()
    za[5, 0] = wall + 0.5
    (a,), ia = xo.optimize(walled, [za], free=[mask], return_info=True)
    (b,), ib = xo.optimize(walled, [z0], free=[mask], return_info=True)
    assert int(ia["status"][5]) == 4 and int(ia["n_eval"][5]) == 1 and torch.equal(a[5], za[5])
    others = [i for i in range(D_MAP) if i != 5]
    assert bool(((ia["status"][others] == 1) | (ia["status"][others] == 2)).all())
    assert torch.equal(a[others], b[others]) and torch.equal(ia["n_eval"][others], ib["n_eval"][others])
    assert torch.equal(ia["logp"][others], ib["logp"][others])
