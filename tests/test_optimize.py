"""CPU: exoplanet_amd.optimize -- the torch statement of the batched L-BFGS, which is its definition and
what runs off the device -- on problems with known optima, and `ParameterSpace.free_mask`.  The problems and their conditions:
tests/optimize_cases.py (shared with tests/test_gpu_optimize.py, where the native kernels meet the same conditions)."""
import pytest
import torch

import optimize_cases as K

import exoplanet_amd as xo
from exoplanet_amd import distributions as dist
from exoplanet_amd.optimize import LBFGS


def test_quadratic_reaches_the_solved_optimum():
    prob = K.quadratic(33)
    x = prob["x0"].clone()
    opt = LBFGS(prob["logp"], [x]).run()
    assert opt.params[0] is not prob["x0"] and torch.equal(opt.params[0], x)       # (updated in place)
    K.check_quadratic(prob, x, opt.status, opt.n_eval)
    assert torch.allclose(opt.logp, prob["logp"](x), rtol=1e-13, atol=0) and bool((opt.n_iter < opt.n_eval).all())
    assert bool((opt.grad_max <= 1e-5)[opt.status == 1].all())
    i, lp = opt.best()
    assert lp == float(opt.logp.max()) and float(opt.logp[i]) == lp


def test_rosenbrock():
    prob = K.rosenbrock(33)
    (x,), info = xo.optimize(prob["logp"], [prob["x0"]], return_info=True)
    K.check_rosenbrock(x, info["status"], info["n_eval"])
    assert x is not prob["x0"] and sorted(info) == ["grad_max", "logp", "n_eval", "n_iter", "status"]


def test_a_wall_is_a_rejected_trial_and_a_start_outside_is_never_moved():
    class Wall(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            inside = x[:, 0] >= -3.0
            ctx.save_for_backward(x, inside)
            return torch.where(inside, -0.5 * (x[:, 0] ** 2 + 100.0 * x[:, 1] ** 2), torch.full_like(x[:, 0], float("-inf")))

        @staticmethod
        def backward(ctx, gout):
            x, inside = ctx.saved_tensors
            g = -torch.stack([x[:, 0], 100.0 * x[:, 1]], 1)
            return gout.unsqueeze(1) * torch.where(inside.unsqueeze(1), g, torch.full_like(g, float("nan")))

    x0 = torch.tensor([[2.9, 1.0], [-2.9, -1.0], [0.5, 0.5], [-4.0, 0.0]], dtype=torch.float64)
    (x,), info = xo.optimize(Wall.apply, [x0], return_info=True)
    assert bool(((info["status"][:3] == 1) | (info["status"][:3] == 2)).all()) and int(info["status"][3]) == 4, info["status"]
    print("wall: largest |x| of the chains inside = %.3g, evaluations %s" % (x[:3].abs().max(), info["n_eval"].tolist()))
    assert float(x[:3].abs().max()) <= 1e-6
    assert torch.equal(x[3], x0[3]) and int(info["n_eval"][3]) == 1 and int(info["n_iter"][3]) == 0


def test_free_mask_holds_columns():
    prob = K.quadratic(33)
    free = torch.ones(8, dtype=torch.float64)
    free[[1, 4]] = 0.0
    (x,), info = xo.optimize(prob["logp"], [prob["x0"]], free=[free], return_info=True)
    K.check_quadratic(prob, x, info["status"], info["n_eval"], held=(1, 4))


def test_several_parameter_tensors_and_tick():
    """two tensors (one of them with trailing dimensions), a mask for one of them; tick() by hand equals run()"""
    prob = K.quadratic(5)
    a0, b0 = prob["x0"][:, :2].clone(), prob["x0"][:, 2:].reshape(5, 3, 2).clone()
    logp = lambda a, b: prob["logp"](torch.cat([a, b.reshape(5, 6)], 1))  # noqa: E731
    opt = LBFGS(logp, [a0.clone(), b0.clone()], free=[torch.tensor([1.0, 0.0], dtype=torch.float64), None])
    ref = LBFGS(logp, [a0.clone(), b0.clone()], free=[torch.tensor([1.0, 0.0], dtype=torch.float64), None]).run(check_every=3)
    while bool((opt.tick() == 0).any()):
        pass
    for p, q in zip(opt.params, ref.params):
        assert torch.equal(p, q)
    assert torch.equal(opt.params[0][:, 1], a0[:, 1]) and opt.params[1].shape == (5, 3, 2)
    assert torch.equal(opt.n_eval, ref.n_eval) and int(opt.n_eval.max()) == opt.n_ticks + 1
    # max_evals bounds the evaluations of every chain, the one at the start included
    short = LBFGS(logp, [a0.clone(), b0.clone()]).run(max_evals=7)
    assert int(short.n_eval.max()) == 7 and bool((short.status == 0).all())


def test_argument_checks():
    x = torch.zeros(4, 3, dtype=torch.float64)
    logp = lambda v: -(v * v).sum(1)  # noqa: E731
    for bad in (dict(history=0), dict(history=33), dict(max_linesearch=0), dict(c1=0.0), dict(c1=1.0), dict(ftol=-1.0),
                dict(gtol=float("nan")), dict(free=[None, None]), dict(free=[torch.full((3,), 0.5, dtype=torch.float64)])):
        with pytest.raises(ValueError):
            LBFGS(logp, [x.clone()], **bad)
    with pytest.raises(ValueError):
        LBFGS(logp, [])
    with pytest.raises(ValueError):
        LBFGS(logp, [x.clone(), torch.zeros(5, 2, dtype=torch.float64)])
    with pytest.raises(ValueError):
        LBFGS(logp, [x.float()])
    opt = LBFGS(logp, [x.clone()])                      # at the optimum already: converged at the start
    assert opt.status.tolist() == [1] * 4 and opt.run().n_ticks == 0 and opt.n_eval.tolist() == [1] * 4


def test_best_ignores_chains_without_a_density():
    x = torch.tensor([[1.0], [float("inf")], [0.25]], dtype=torch.float64)
    opt = LBFGS(lambda v: -(v * v).sum(1), [x], gtol=10.0)
    assert opt.status.tolist() == [1, 4, 1]
    assert opt.best() == (2, -0.0625)


def test_free_mask_names_blocks():
    space = xo.ParameterSpace(t0=dist.normal(0.0, 1.0), r=dist.uniform(0.01, 0.3), u=dist.quad_limb_dark(),
                              ecc=dist.kipping13(fixed=False, shape=(2,)), b=dist.impact_parameter("r"))
    n_hyper = len(space.blocks[3][1].hyper)
    assert n_hyper > 0 and space.n_free == 1 + 1 + 2 + n_hyper + 2 + 1
    m = space.free_mask(["r", "b"])
    assert m.dtype == torch.float64 and m.shape == (space.n_free,)
    assert m.tolist() == [0.0, 1.0, 0.0, 0.0] + [0.0] * (n_hyper + 2) + [1.0]
    assert space.free_mask(["ecc"]).tolist() == [0.0] * 4 + [1.0] * (n_hyper + 2) + [0.0]      # hyperparameter columns included
    assert space.free_mask("u").tolist() == [0.0, 0.0, 1.0, 1.0] + [0.0] * (n_hyper + 3)       # a multi-value block, by its name
    assert space.free_mask(list(n for n, *_ in space.blocks)).tolist() == [1.0] * space.n_free
    with pytest.raises(ValueError, match="block 'u'"):
        space.free_mask(["u1"])
    with pytest.raises(ValueError, match="block 'ecc'"):
        space.free_mask(["ecc::alpha"])
    with pytest.raises(ValueError, match="no block named 'period'"):
        space.free_mask(["t0", "period"])


def test_two_stage_call_on_a_parameter_space():
    """the tutorial's shape: some blocks first, then all, through space.wrap; the held columns are bit-identical after stage one"""
    space = xo.ParameterSpace(mu=dist.normal(1.0, 2.0), s=dist.uniform(0.1, 5.0))
    gen = torch.Generator().manual_seed(5)
    y = 1.7 + 0.8 * torch.randn(200, dtype=torch.float64, generator=gen)

    def loglike(mu, s):
        return (-0.5 * ((y[None, :] - mu) / s) ** 2 - torch.log(s)).sum(1)

    z0 = space.unconstrain(6, mu=torch.linspace(-1.0, 3.0, 6).reshape(6, 1), s=2.0)
    z1 = xo.optimize(space.wrap(loglike), [z0], free=[space.free_mask(["mu"])])
    assert torch.equal(z1[0][:, 1], z0[:, 1]) and not torch.equal(z1[0][:, 0], z0[:, 0])
    z2, info = xo.optimize(space.wrap(loglike), z1, return_info=True)
    assert bool(((info["status"] == 1) | (info["status"] == 2)).all())
    assert float(info["logp"].max() - info["logp"].min()) <= 1e-6
    theta, _ = space.constrain(z2[0])
    assert abs(float(theta["mu"][0]) - float(y.mean())) < 0.05 and abs(float(theta["s"][0]) - float(y.std())) < 0.05


def test_at_the_rounding_floor_a_failed_line_search_is_as_close_as_the_rest():
    """tolerances tighter than the arithmetic: chains may end with status 3 at the rounding floor; they must be as close to the
    optimum as the chains that met a tolerance (not: there are none)"""
    prob = K.quadratic(97, seed=3)
    x = prob["x0"].clone()
    opt = LBFGS(prob["logp"], [x], ftol=1e-14, gtol=1e-7).run()
    assert bool((opt.status != 0).all() and (opt.status != 4).all())
    fstar = prob["f"](torch.linalg.solve(prob["A"], prob["b"])[None])
    gap = (prob["f"](x) - fstar) / (prob["f"](prob["x0"]) - fstar)
    failed = opt.status == 3
    print("tight tolerances: %d of 97 chains with status 3; largest gap %.3g (status 3: %.3g)"
          % (int(failed.sum()), gap.max(), gap[failed].max() if bool(failed.any()) else 0.0))
    assert float(gap.max()) <= 1e-8
    if bool(failed.any()) and bool((~failed).any()):
        # (as close as the others, or within the rounding of f itself: 64 ulp of max(|f*|, 1) on the scale of the gap)
        floor = 64 * 2.220446049250313e-16 * max(float(fstar.abs()), 1.0) / float((prob["f"](prob["x0"]) - fstar).min())
        assert float(gap[failed].max()) <= max(float(gap[~failed].max()), floor)
