"""Batched maximum a posteriori by L-BFGS, on the device, before the samplers.

The reference's models climb to the posterior mode with ``pmx.optimize(vars=[...])`` and ``pmx.optimize(soln)`` (scipy's
L-BFGS-B on one point; the reference's docs/tutorials/data-and-models.md:287-296) and sample from there.  Here the D chains
of a batch are the draw dimension of the kernels, as they are for `sampling.NUTS`: every chain minimises ``f = -logp`` on
its own, all chains in lockstep.  One TICK is one batched value + gradient evaluation at every chain's trial point and one
decision per chain (Armijo test, history, two-loop direction, convergence, the next trial point): on a ROCm device the
decision is one native kernel (``exo_lbfgs_f64``), the whole tick is captured once as a hipGraph and replayed, and the
host looks at the device once every few ticks ("is any chain still running?").

The rules are DESIGN.md section 15; their definition is the torch statement below (`LBFGS._start_torch`,
`LBFGS._decide_torch`), which is what runs on the CPU.
"""
import torch

from .graph import GraphedStep
from .sampling import _ChainSampler

__all__ = ["LBFGS", "optimize"]

RUNNING, GRADIENT, VALUE, LINE_SEARCH, BAD_START = range(5)   # the values of ``status``
MAX_HISTORY = 32                                               # EXO_LBFGS_MAX_HISTORY
_EPS = 2.220446049250313e-16


class LBFGS:
    """``logp_fn(*params) -> (D,)`` log-density of every chain; ``params``: tensors with a common leading chain dimension D
    (the starting points; updated in place).  L-BFGS with ``history`` correction pairs and a backtracking Armijo line search
    (``c1``, at most ``max_linesearch`` halvings in a row), stopped per chain by ``gtol`` (largest gradient component) or
    ``ftol`` (relative decrease of a step, for ``history`` accepted steps in a row) -- scipy's L-BFGS-B defaults.  ``free``: one 0 / 1 mask per parameter
    (broadcastable to it); a masked element never moves.  The tolerances are constructor arguments: a captured tick bakes
    the kernel's scalars in.

    Device tensors, one entry per chain: ``logp``, ``grad_max``, ``status`` (0 running, 1 gradient below ``gtol``, 2 decrease
    below ``ftol``, 3 line search failed, 4 the starting value or gradient is not finite: never moved), ``n_iter``, ``n_eval``.

    On a ROCm device the decision is the native kernel and the tick a hipGraph replay (``graph=False``: launched eagerly);
    on the CPU the torch statement runs -- the module is device-agnostic, which is how tests/test_optimize.py checks it
    without a GPU.  ``native=False`` runs the torch statement on the device too (tests and measurements).
    """

    _flat, _parts, _value_and_grad_flat = _ChainSampler._flat, _ChainSampler._parts, _ChainSampler._value_and_grad_flat

    def __init__(self, logp_fn, params, *, history=8, max_linesearch=20, c1=1e-4, ftol=2.220446049250313e-09, gtol=1e-5,
                 free=None, graph=True, native=True):
        self.params = [p.detach() for p in params]
        if not self.params or any(p.dim() < 1 or p.shape[0] != self.params[0].shape[0] for p in self.params):
            raise ValueError("params must be tensors with a common leading chain dimension")
        if any(p.dtype != torch.float64 or p.device != self.params[0].device for p in self.params):
            raise ValueError("params must be float64 tensors on one device")
        self.history, self.max_linesearch = int(history), int(max_linesearch)
        if not 1 <= self.history <= MAX_HISTORY:
            raise ValueError(f"need 1 <= history <= {MAX_HISTORY}")
        if self.max_linesearch < 1:
            raise ValueError("need max_linesearch >= 1")
        self.c1, self.ftol, self.gtol = float(c1), float(ftol), float(gtol)
        if not 0 < self.c1 < 1 or not self.ftol >= 0 or not self.gtol >= 0:
            raise ValueError("need 0 < c1 < 1, ftol >= 0 and gtol >= 0")
        if free is not None and len(free) != len(self.params):
            raise ValueError("free must hold one mask per parameter")
        self.logp_fn = logp_fn
        self.D = D = self.params[0].shape[0]
        self._shapes = [tuple(p.shape) for p in self.params]
        self._sizes = [int(p[0].numel()) for p in self.params]
        dev = self.params[0].device
        masks = [torch.ones_like(p) if m is None else torch.as_tensor(m, dtype=p.dtype, device=p.device).expand_as(p).clone()
                 for p, m in zip(self.params, free or [None] * len(self.params))]
        if any(bool(((m != 0) & (m != 1)).any()) for m in masks):
            raise ValueError("free must be masks of 0 and 1")
        x = self._flat(self.params)
        n, H = int(x.shape[1]), self.history
        if n < 1:
            raise ValueError("params hold no element")
        zq = lambda: torch.zeros_like(x)  # noqa: E731
        zd = lambda: torch.zeros(D, dtype=x.dtype, device=dev)  # noqa: E731
        zi = lambda: torch.zeros(D, dtype=torch.int32, device=dev)  # noqa: E731
        # static buffers, in the order of exo_lbfgs_f64's pointer table: the trajectory arrays are (D, n) as logp_fn sees them;
        # the history is chain-innermost
        self._st = dict(x=x, g=zq(), xt=zq(), gt=zq(), d=zq(), free=self._flat(masks),
                        hs=torch.zeros((H, n, D), dtype=x.dtype, device=dev), hy=torch.zeros((H, n, D), dtype=x.dtype, device=dev),
                        hsy=torch.zeros((H, D), dtype=x.dtype, device=dev), coef=torch.zeros((H, D), dtype=x.dtype, device=dev),
                        logp=zd(), lpt=zd(), alpha=zd(), gamma=zd(), grad_max=zd(),
                        status=zi(), n_iter=zi(), n_eval=zi(), m=zi(), head=zi(), n_rej=zi(), n_small=zi())
        st = self._st
        self.logp, self.grad_max, self.status, self.n_iter, self.n_eval = (st[k] for k in ("logp", "grad_max", "status", "n_iter",
                                                                                              "n_eval"))
        self.n_ticks = 0
        self._native = None
        if native and x.is_cuda:
            import ctypes

            ptrs = [v.data_ptr() for v in st.values()]
            self._native = ((ctypes.c_void_p * len(ptrs))(*ptrs), n)
        self._graph = None
        self._start()
        if graph and self._native is not None:
            # (capturing runs a few ticks: the optimisation starts over afterwards, from the params)
            self._graph = GraphedStep(lambda *a: self._tick(), *st.values())
            self._start()

    # ---- the two decisions: native kernels on the device, the torch statement otherwise ----------------------------------------
    def _phase(self, phase):
        if self._native is None:
            return (self._start_torch, self._decide_torch)[phase]()
        from . import _lib

        ptrs, n = self._native
        dev = self._st["x"].device
        with torch.cuda.device(dev):
            _lib.check(_lib.load().exo_lbfgs_f64(ptrs, self.D, n, self.history, self.max_linesearch, self.c1, self.gtol, self.ftol,
                                                 phase, torch.cuda.current_stream(dev).cuda_stream), "exo_lbfgs_f64")

    def _masked(self):
        """gt <- -(gradient of logp) * free; (all finite, largest |.|, sum of |.|) per chain"""
        st = self._st
        gt = torch.where(st["free"] != 0, -st["gt"] * st["free"], torch.zeros_like(st["gt"]))
        st["gt"].copy_(gt)
        ok = torch.isfinite(gt).all(1) & torch.isfinite(st["lpt"])
        return gt, ok, gt.abs().amax(1), gt.abs().sum(1)

    def _start_torch(self):
        st = self._st
        gt, ok, gmax, gsum = self._masked()
        done = ok & (gmax <= self.gtol)
        go = (ok & ~done).unsqueeze(1)
        alpha = torch.where(gsum > 1, 1 / gsum, torch.ones_like(gsum))
        one, zero = torch.ones_like(st["status"]), torch.zeros_like(st["status"])
        for k, v in (("g", gt), ("d", torch.where(go, -gt, torch.zeros_like(gt))), ("logp", st["lpt"]), ("grad_max", gmax),
                     ("alpha", torch.where(go[:, 0], alpha, torch.zeros_like(alpha))), ("gamma", torch.ones_like(alpha)),
                     ("status", torch.where(ok, torch.where(done, GRADIENT * one, zero), BAD_START * one)),
                     ("n_iter", zero), ("n_eval", one), ("m", zero), ("head", zero), ("n_rej", zero), ("n_small", zero)):
            st[k].copy_(v)
        st["xt"].copy_(torch.where(go, st["x"] + st["alpha"].unsqueeze(1) * st["d"], st["x"]))

    def _two_loop(self, g, m, head):
        """-H g of every chain over its m newest pairs (newest first), first scaling per column"""
        st, H = self._st, self.history
        ar = torch.arange(self.D, device=g.device)
        q, coef, pairs = g, [], []
        for j in range(H):
            k = ((head - 1 - j) % H).long()
            S, Y, sy, valid = st["hs"][k, :, ar], st["hy"][k, :, ar], st["hsy"][k, ar], (j < m).unsqueeze(1)
            a = ((S * q).sum(1) / sy).unsqueeze(1)
            q = torch.where(valid, q - a * Y, q)
            coef.append(a)
            pairs.append((S, Y, sy, valid))
        # the first scaling, per column: the diagonal that fits the stored pairs, sum_k s_i y_i / sum_k y_i^2 (exact for a
        # separable quadratic); gamma of the newest pair where that is not positive
        num = sum(torch.where(valid, S * Y, torch.zeros_like(S)) for S, Y, _, valid in pairs)
        den = sum(torch.where(valid, Y * Y, torch.zeros_like(Y)) for S, Y, _, valid in pairs)
        fits = (num > 0) & (den > 0)
        r = torch.where(fits, num / torch.where(fits, den, torch.ones_like(den)), st["gamma"].unsqueeze(1).expand_as(q)) * q
        for a, (S, Y, sy, valid) in zip(reversed(coef), reversed(pairs)):
            b = ((Y * r).sum(1) / sy).unsqueeze(1)
            r = torch.where(valid, r + (a - b) * S, r)
        return -r

    def _decide_torch(self):
        st, H = self._st, self.history
        run = st["status"] == RUNNING
        gt, ok, gmax, gsum = self._masked()
        x, g, xt, d, alpha, m, head = st["x"], st["g"], st["xt"], st["d"], st["alpha"], st["m"], st["head"]
        f, ft = -st["logp"], -st["lpt"]
        accept = run & ok & (ft <= f + self.c1 * alpha * (g * d).sum(1))
        reject = run & ~accept
        # accept: the pair joins the history -- if its curvature is not positive it does not, and the history goes; the chain moves
        s, y = xt - x, gt - g
        sy, yy = (s * y).sum(1), (y * y).sum(1)
        store = accept & (sy > _EPS * yy)
        ar = torch.arange(self.D, device=x.device)[store]
        k = head[store].long()
        st["hs"][k, :, ar] = s[store]
        st["hy"][k, :, ar] = y[store]
        st["hsy"][k, ar] = sy[store]
        gamma = torch.where(store, sy / yy, st["gamma"])
        st["gamma"].copy_(gamma)
        head = torch.where(store, (head + 1) % H, head)
        m = torch.where(store, torch.clamp(m + 1, max=H), torch.where(accept, torch.zeros_like(m), m))
        stop_g = accept & (gmax <= self.gtol)
        # (one small decrease says little: a step that settles the stiff directions of a badly scaled f decreases it by next to
        # nothing while the gradient along the soft ones is as large as ever.  Status 2 takes a history's worth of small decreases
        # in a row: then every pair the model is built from comes from a step that achieved nothing)
        small = f - ft <= self.ftol * torch.clamp(torch.maximum(f.abs(), ft.abs()), min=1.0)
        n_small = torch.where(accept, torch.where(small, st["n_small"] + 1, torch.zeros_like(m)), st["n_small"])
        stop_f = accept & ~stop_g & (n_small >= H)
        move = accept & ~stop_g & ~stop_f
        g_new = torch.where(accept.unsqueeze(1), gt, g)
        d_new = self._two_loop(g_new, m, head)
        m = torch.where(move & ~((d_new * g_new).sum(1) < 0), torch.zeros_like(m), m)      # not a descent direction
        # reject: half the step; at the limit a chain with history drops it, one without gives up
        n_rej = torch.where(accept, torch.zeros_like(m), st["n_rej"] + reject.to(m.dtype))
        limit = reject & (n_rej >= self.max_linesearch)
        fail = limit & (m == 0)
        restart = limit & (m > 0)
        m = torch.where(restart, torch.zeros_like(m), m)
        n_rej = torch.where(restart, torch.zeros_like(m), n_rej)
        steep = (move & (m == 0)) | restart
        first = torch.where(g_new.abs().sum(1) > 1, 1 / g_new.abs().sum(1), torch.ones_like(alpha))
        d = torch.where(steep.unsqueeze(1), -g_new, torch.where(move.unsqueeze(1), d_new, d))
        alpha = torch.where(steep, first, torch.where(move, torch.ones_like(alpha), torch.where(reject, 0.5 * alpha, alpha)))
        x_new = torch.where(accept.unsqueeze(1), xt, x)
        going = (move | (reject & ~fail)).unsqueeze(1)
        one = torch.ones_like(st["status"])
        # (a line search that fails right after small decreases has met the rounding of f, not an obstacle: status 2)
        fail_code = torch.where(n_small > 0, VALUE * one, LINE_SEARCH * one)
        status = torch.where(stop_g, GRADIENT * one, torch.where(stop_f, VALUE * one, torch.where(fail, fail_code,
                                                                                                  st["status"])))
        for key, v in (("xt", torch.where(going, x_new + alpha.unsqueeze(1) * d, x_new)), ("x", x_new), ("g", g_new), ("d", d),
                       ("alpha", alpha), ("logp", torch.where(accept, st["lpt"], st["logp"])),
                       ("grad_max", torch.where(accept, gmax, st["grad_max"])), ("status", status),
                       ("n_iter", st["n_iter"] + accept.to(m.dtype)), ("n_eval", st["n_eval"] + run.to(m.dtype)),
                       ("m", m), ("head", head), ("n_rej", n_rej), ("n_small", n_small)):
            st[key].copy_(v)

    # ---- evaluation + decision ------------------------------------------------------------------------------------------------
    def _evaluate(self):
        st = self._st
        lp, _ = self._value_and_grad_flat(st["xt"], grad_out=st["gt"])       # (the gradient lands in the trial point's buffer)
        st["lpt"].copy_(lp)

    def _start(self):
        """the evaluation at the starting points (the params as they are now) and phase 0"""
        st = self._st
        with torch.no_grad():
            self._flat(self.params, out=st["x"])
            st["xt"].copy_(st["x"])
        self._evaluate()
        with torch.no_grad():
            self._phase(0)
        self.n_ticks = 0

    def _tick(self):
        self._evaluate()
        with torch.no_grad():
            self._phase(1)
        return self._st["status"]

    def _to_params(self):
        with torch.no_grad():
            for p, v in zip(self.params, self._parts(self._st["x"])):
                p.copy_(v)

    def tick(self):
        """one evaluation + decision of every chain (a chain that has stopped rides along unchanged); returns ``status``"""
        if self._graph is not None:
            self._graph()
        else:
            self._tick()
        self.n_ticks += 1
        self._to_params()
        return self.status

    def run(self, max_evals=1000, check_every=8):
        """ticks until no chain is running or every chain has been evaluated ``max_evals`` times (the one at the start
        counts); the host reads ``(status == 0).any()`` once per ``check_every`` ticks.  Returns ``self``."""
        step = self._graph if self._graph is not None else self._tick
        check_every = max(int(check_every), 1)
        while self.n_ticks + 1 < max_evals:
            if self.n_ticks % check_every == 0 and not bool((self.status == RUNNING).any()):
                break
            step()
            self.n_ticks += 1
        self._to_params()
        return self

    def best(self):
        """(index of the chain with the largest log-density among those with a finite one, that log-density)"""
        lp = torch.where(torch.isfinite(self.logp), self.logp, torch.full_like(self.logp, float("-inf")))
        i = int(torch.argmax(lp))
        return i, float(self.logp[i])


def optimize(logp_fn, params, *, free=None, return_info=False, max_evals=1000, **kw):
    """``params`` (tensors with a leading chain dimension; not modified) climbed to a mode of ``logp_fn`` by `LBFGS`:
    the list of optimised tensors, and with ``return_info`` a dict of the per-chain tensors ``logp``, ``grad_max``,
    ``status``, ``n_iter``, ``n_eval``.  ``free``: as `LBFGS` (``ParameterSpace.free_mask`` names blocks) -- the two stages of
    the reference's tutorials are ``z = optimize(logp, [z0], free=[space.free_mask(["r", "b"])])`` then ``optimize(logp, z)``."""
    check_every = kw.pop("check_every", 8)
    opt = LBFGS(logp_fn, [p.detach().clone() for p in params], free=free, **kw).run(max_evals=max_evals, check_every=check_every)
    if return_info:
        return opt.params, {k: getattr(opt, k).clone() for k in ("logp", "grad_max", "status", "n_iter", "n_eval")}
    return opt.params
