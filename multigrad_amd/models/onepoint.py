"""One-point models: differentiable summary statistics summed over data shards.

Reference: ``multigrad/multigrad.py:186-607`` (``OnePointModel``, ``OnePointGroup``).

The distributed chain rule (reference ``_vjp``, ``:508-538``)::

    S(theta) = sum_r s_r(theta)                   # partial sumstats, all-reduced
    L(theta) = l(S(theta))                        # loss on the total, every rank
    dL/dtheta = sum_r J_{s_r}(theta)^T dl/dS      # local VJP with the global cotangent,
                                                  # then all-reduced

is evaluated here with PyTorch-ROCm autograd on the rank's GPU.  Both reductions are
device collectives (RCCL over xGMI, stream ordered; gloo on CPU) -- there is no
host round trip per step as in the reference's numpy-staged MPI calls.  Models whose
sumstats are produced by hand-written HIP kernels plug in through custom autograd
functions (see :mod:`multigrad_amd.models.smf`) or the fused-engine protocol
(:mod:`multigrad_amd.engine`).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Tuple, Union

import numpy as np
import torch

from ..optim import adam as _adam
from ..optim import bfgs as _bfgs
from ..parallel.comm import get_world_comm
from ..utils import util
from ..utils.random import init_randkey
from ..utils.tensors import as_param_tensor, detach_tree, infer_device

__all__ = ["OnePointModel", "OnePointGroup"]


def _rk(randkey):
    return {} if randkey is None else {"randkey": randkey}


class _OptimizerFrontEnds:
    """``run_simple_grad_descent`` / ``run_adam`` / ``run_bfgs`` shared by models and groups
    (reference ``multigrad/multigrad.py:226-352``, ``:583-599``)."""

    def _opt_comm(self):
        raise NotImplementedError

    def param_device(self) -> torch.device:
        raise NotImplementedError

    def _engine_members(self):
        return tuple(self.models) if isinstance(self, OnePointGroup) else (self,)

    def _generic_engine_ok(self, x0, loss_aux_ok: bool = True) -> bool:
        """Whether this model's (or group's) optimizer steps can go through the captured
        generic engine (engine/generic.py): torch OnePointModels on a GPU, an fp32 guess
        (the engine's Adam state is fp32; an fp64 fit keeps the eager loop), no fused-engine
        protocol (a single model that has one uses the fused engine), not disabled."""
        members = self._engine_members()
        single_fused = (not isinstance(self, OnePointGroup)
                        and getattr(self, "fused_engine", None) is not None)
        return (x0.is_cuda and x0.dtype == torch.float32 and not single_fused
                and all(isinstance(m, OnePointModel) for m in members)
                and (loss_aux_ok or not any(m.loss_func_has_aux for m in members))
                and os.environ.get("MULTIGRAD_GENERIC_ENGINE", "1") != "0")

    def _step_engine(self, x0, comm=None):
        """The model's cached fused step engine (``fused_step_engine``: the shared-parameter
        SMF models, engine/smf2.py) for an fp32 device guess, or None."""
        fn = getattr(self, "fused_step_engine", None)
        if fn is None or not (x0.is_cuda and x0.dtype == torch.float32) or \
                os.environ.get("MULTIGRAD_GENERIC_ENGINE", "1") == "0":
            return None
        return fn(comm=self._opt_comm() if comm is None else comm)

    def run_simple_grad_descent(self, guess, nsteps: int = 100, learning_rate: float = 0.01):
        """Fixed-learning-rate gradient descent.

        Returns ``GradDescentResult(loss, params, aux)`` where ``params[i]`` is the point at
        which ``loss[i]`` was evaluated.
        """
        has_aux = bool(getattr(self, "loss_func_has_aux", False))
        x0 = as_param_tensor(guess, device=self.param_device())
        eng = self._step_engine(x0)
        if eng is not None and not has_aux:
            # fused device step (engine/smf2.py): one pass + one exchange per step
            return eng.run_simple_grad_descent(x0, nsteps=nsteps, learning_rate=learning_rate)
        if self._generic_engine_ok(x0, loss_aux_ok=False):
            # one captured step replayed per iteration (engine/generic.py)
            from ..engine.generic import GraphAdamEngine
            return GraphAdamEngine(self, comm=self._opt_comm()).run_simple_grad_descent(
                x0, nsteps=nsteps, learning_rate=learning_rate)
        return util.simple_grad_descent(
            None, guess=as_param_tensor(guess, device=self.param_device()), nsteps=nsteps,
            learning_rate=learning_rate,
            loss_and_grad_func=self.calc_loss_and_grad_from_params, has_aux=has_aux,
            comm=self._opt_comm())

    def run_adam(self, guess, nsteps: int = 100, param_bounds=None, learning_rate: float = 0.01,
                 randkey=None, const_randkey: bool = False, comm=None, **kw):
        """Adam from ``guess``; returns the parameter trajectory ``(nsteps+1, ndim)``.

        ``randkey`` (int or :class:`~multigrad_amd.utils.random.PRNGKey`) gives a fresh key
        per step, or the same key every step with ``const_randkey=True``.  Extra keywords
        (``history``, ``checkpoint_path``, ``checkpoint_every``, ``resume_from``,
        ``legacy_bounds_jacobian``, ``b1``, ``b2``, ``eps``, ``callback``) go to
        :func:`multigrad_amd.optim.adam.run_adam`.  Every rank returns the trajectory.
        """
        comm = self._opt_comm() if comm is None else comm
        guess = as_param_tensor(guess, device=self.param_device())
        if const_randkey:
            assert randkey is not None, "Must pass randkey if const_randkey"
            const_key = init_randkey(randkey) if not hasattr(randkey, "split") else randkey
            randkey = None

            def loss_and_grad_fn(x, _, **k):
                return self.calc_loss_and_grad_from_params(x, randkey=const_key, **k)
        else:
            def loss_and_grad_fn(x, _, **k):
                return self.calc_loss_and_grad_from_params(x, **k)
        fused = getattr(self, "fused_engine", None)
        use_engine = kw.pop("use_engine", True)
        keyed = randkey is not None or const_randkey
        step_kw = ("history", "legacy_bounds_jacobian", "b1", "b2", "eps", "callback")
        if use_engine and all(k in step_kw for k in kw) and (
                not keyed or getattr(self, "engine_randkey_invariant", False)):
            eng = self._step_engine(guess, comm)
            if eng is not None:
                return eng.run_adam(guess, nsteps=nsteps, param_bounds=param_bounds,
                                    learning_rate=learning_rate, **kw)
        if fused is not None and use_engine and (
                not keyed or getattr(self, "engine_randkey_invariant", False)):
            # a fused-protocol model whose hooks ignore randkey gives the same trajectory
            # with or without keys (engine_randkey_invariant)
            eng = fused()
            if eng is not None:
                try:
                    return eng.run_adam(guess, nsteps=nsteps, param_bounds=param_bounds,
                                        learning_rate=learning_rate, **kw)
                finally:
                    if not getattr(eng, "cached", False):  # a model's cached engine stays up
                        eng.close()
        # any other model or group on a GPU: one captured step replayed per iteration
        # (engine/generic.py), per-step or constant keys included
        graph_kw = {k: kw[k] for k in kw if k in ("history", "legacy_bounds_jacobian", "b1",
                                                   "b2", "eps", "callback")}
        if use_engine and len(graph_kw) == len(kw) and self._generic_engine_ok(guess):
            from ..engine.generic import GraphAdamEngine
            return GraphAdamEngine(self, comm=comm).run_adam(
                guess, nsteps=nsteps, param_bounds=param_bounds, learning_rate=learning_rate,
                randkey=const_key if const_randkey else randkey, const_randkey=const_randkey,
                **graph_kw)
        return _adam.run_adam(loss_and_grad_fn, params=guess, data=None, nsteps=nsteps,
                              param_bounds=param_bounds, learning_rate=learning_rate,
                              randkey=randkey, comm=comm, **kw)

    def run_bfgs(self, guess, maxsteps: int = 100, param_bounds=None, randkey=None,
                 comm=None, method: str = "auto", hess_inv: bool = True, prior=None,
                 prior_weight: float = 1.0, **kw):
        """L-BFGS(-B); returns a ``scipy.optimize.OptimizeResult`` on every rank.

        ``method="scipy"``: scipy's L-BFGS-B on the root rank, other ranks serve its
        evaluations (the reference's protocol).
        ``method="device"``: SPMD device L-BFGS with all-reduced dot products; with
        ``param_bounds`` it is L-BFGS-B (generalized Cauchy point, subspace minimisation,
        projected line search: :mod:`multigrad_amd.optim.lbfgsb`), so bounded fits keep
        scipy's semantics (``bounds_mode="transform"`` uses the Adam reparameterisation
        instead).  Models with the fused-engine protocol run it over the engine's (ZeRO-
        or owner-) sharded vectors.  ``"auto"`` picks ``device`` above 1e5 parameters.

        ``hess_inv`` (``method="device"``): return the inverse-Hessian approximation as
        ``res.hess_inv``, a :class:`~multigrad_amd.optim.invhess.DeviceLbfgsInvHessProduct`
        (products, diagonal, ``todense()``, ``pairs()``; user parameter order, collective on
        sharded runs).  It holds the optimizer's history ring on the device without a copy
        (``2 (history + 1)`` fp32 vectors: 0.9 GB at 1e7 parameters); ``hess_inv=False`` frees
        the ring on return.  ``method="scipy"`` always returns scipy's own operator.

        ``prior`` (a :class:`~multigrad_amd.optim.prior.GaussianPrior` on the parameters
        themselves, in every bounds mode) minimises ``loss + prior_weight * prior.penalty(x)``;
        ``prior_weight = 1 / loss_scale`` gives the MAP of the posterior that
        ``run_hmc(prior=prior, loss_scale=loss_scale)`` samples.  ``res.fun`` is the minimised
        objective, ``res.prior_penalty`` the unweighted penalty at ``res.x``, and
        ``res.hess_inv`` approximates the inverse Hessian of likelihood plus prior.
        """
        from ..optim.prior import PriorObjective, check_prior, penalised_function, with_penalty
        comm = self._opt_comm() if comm is None else comm
        x0 = as_param_tensor(guess, device=self.param_device())
        check_prior(prior, x0.numel())  # before any collective
        pkw = {} if prior is None else {"prior": prior, "prior_weight": prior_weight}
        if method == "auto":
            method = "device" if x0.numel() > 100_000 else "scipy"
        if method == "scipy":
            fn = self.calc_loss_and_grad_from_params
            eng = None
            step_eng = self._step_engine(x0, comm) if (
                getattr(self, "engine_randkey_invariant", False) or randkey is None) else None
            if step_eng is not None:
                # each scipy evaluation is one fused device evaluation (engine/smf2.py)
                fn = step_eng.evaluator()
            elif self._generic_engine_ok(x0):
                # each scipy evaluation replays one captured evaluation (engine/generic.py)
                from ..engine.generic import GraphAdamEngine
                eng = GraphAdamEngine(self, comm=comm)
                fn = eng.evaluator(x0, randkey=None if randkey is None else init_randkey(randkey)
                                   if not hasattr(randkey, "split") else randkey)
            if prior is not None:  # on every rank: the workers serve the same function
                fn = penalised_function(fn, prior, prior_weight)
            try:
                return with_penalty(_bfgs.run_bfgs(
                    fn, x0, maxsteps=maxsteps, param_bounds=param_bounds, randkey=randkey,
                    comm=comm, device=self.param_device(), **kw), prior)
            finally:
                if eng is not None:
                    eng.close()
        from ..optim import lbfgs as _lbfgs
        from ..optim import lbfgsb as _lbfgsb
        hist = kw.pop("history", 10)
        kw["hess_inv"] = bool(hess_inv)
        mode = kw.pop("bounds_mode", "project")
        if mode not in ("project", "transform"):
            raise ValueError("bounds_mode must be 'project' or 'transform'")
        fused = getattr(self, "fused_engine", None)
        if fused is not None and randkey is None and (param_bounds is None or mode == "project"):
            eng = fused(comm=comm, **{k: kw.pop(k) for k in ("zero", "chunks") if k in kw})
            if eng is not None:
                try:
                    obj = eng.lbfgs_objective(x0)
                    if prior is not None:
                        obj = PriorObjective(obj, prior, prior_weight)
                    if param_bounds is None:
                        return with_penalty(
                            _lbfgs.lbfgs_minimize(obj, maxiter=maxsteps, m=hist, **kw), prior)
                    lo, hi = obj.local_box(param_bounds)
                    return with_penalty(_lbfgsb.lbfgsb_minimize(
                        obj, lo, hi, maxiter=maxsteps, m=hist, **kw), prior)
                finally:
                    if not getattr(eng, "cached", False):
                        eng.close()
        if param_bounds is not None and mode == "project":
            return _lbfgsb.run_lbfgsb_device(self.calc_loss_and_grad_from_params, x0,
                                             maxsteps=maxsteps, param_bounds=param_bounds,
                                             randkey=randkey, comm=comm, history=hist, **pkw,
                                             **kw)
        return _lbfgs.run_lbfgs_device(self.calc_loss_and_grad_from_params, x0, maxsteps=maxsteps,
                                       param_bounds=param_bounds, randkey=randkey, comm=comm,
                                       history=hist, **pkw, **kw)

    def run_hmc(self, guess, nsamples: int = 1000, warmup: int = 500, nleapfrog: int = 10,
                step_size: float = 0.1, param_bounds=None, randkey=0, loss_scale: float = 1.0,
                history: str = "full", track=None, comm=None, prior=None, **kw):
        """Draw from the posterior ``exp(-loss_scale * loss)`` -- with ``prior``, a
        :class:`~multigrad_amd.optim.prior.GaussianPrior`,
        ``exp(-(loss_scale * loss + prior.penalty(x)))`` -- by Hamiltonian Monte Carlo
        (:mod:`multigrad_amd.optim.hmc`); returns an
        :class:`~multigrad_amd.optim.hmc.HMCResult` on every rank.

        ``loss_scale = 0.5`` makes a chi^2 loss a Gaussian log-likelihood.  ``warmup``
        iterations adapt the step size (dual averaging) and the diagonal mass (Stan's windows)
        from ``step_size``; ``randkey`` (int or key) seeds the sampler.  ``history="full"``
        returns ``samples [nsamples, P]``; ``history="moments"`` only ``mean`` and ``var``
        (with ``track=indices`` for the chains of a few parameters: the intended use at 1e7
        parameters).  With ``param_bounds`` the chain runs in the unbounded coordinates of
        :mod:`~multigrad_amd.optim.transforms` with a flat prior on the bounded parameters
        unless ``prior`` is given.  The prior is on the bounded parameters and is a density: it
        is not scaled by ``loss_scale``, so the MAP of the sampled posterior is
        ``run_bfgs(prior=prior, prior_weight=1 / loss_scale)``.  On the engine path its force
        and its energy come out of the fused leapfrog pass (``csrc/prior.hip``).
        Models with the fused-engine protocol (and no bounds) sample over the engine's
        (ZeRO- or owner-) sharded vectors, the evaluations of a trajectory staying on the
        device; everything else goes through ``calc_loss_and_grad_from_params``.  Extra
        keywords (``jitter``, ``noise``, ``target_accept``, ``adapt_step_size``,
        ``adapt_mass``, ``inv_mass``) go to :func:`multigrad_amd.optim.hmc.hmc_sample`."""
        from ..optim import hmc as _hmc
        from ..optim.lbfgs import GenericObjective
        from ..optim.prior import check_prior
        from ..optim.transforms import Bounds
        comm = self._opt_comm() if comm is None else comm
        x0 = as_param_tensor(guess, device=self.param_device())
        check_prior(prior, x0.numel())  # before any collective
        skw = dict(nsamples=nsamples, warmup=warmup, nleapfrog=nleapfrog, step_size=step_size,
                   loss_scale=loss_scale, seed=randkey, history=history, track=track)
        if prior is not None:
            skw["prior"] = prior
        fused = getattr(self, "fused_engine", None)
        if fused is not None and param_bounds is None:
            eng = fused(comm=comm, **{k: kw.pop(k) for k in ("zero", "chunks") if k in kw})
            if eng is not None:
                try:
                    return _hmc.hmc_sample(eng.lbfgs_objective(x0), **skw, **kw)
                finally:
                    if not getattr(eng, "cached", False):
                        eng.close()
        bounds = Bounds.from_spec(param_bounds, x0.numel(), device=x0.device, dtype=torch.float32)
        obj = GenericObjective(self.calc_loss_and_grad_from_params, x0, comm=comm, bounds=bounds)
        return _hmc.hmc_sample(obj, **skw, **kw)


@dataclass
class OnePointModel(_OptimizerFrontEnds):
    """Differentiable one-point model whose summary statistics add across ranks.

    Subclasses implement two torch-differentiable hooks:

    * ``calc_partial_sumstats_from_params(params[, randkey])`` -> this rank's partial
      sumstats (or ``(sumstats, aux)`` if ``sumstats_func_has_aux``);
    * ``calc_loss_from_sumstats(sumstats[, sumstats_aux][, randkey])`` -> loss (or
      ``(loss, aux)`` if ``loss_func_has_aux``).

    ``randkey`` is forwarded only when not ``None``.  (The reference docstring swaps the
    two ``*_has_aux`` descriptions; the behaviour above follows its code.)

    Parameters
    ----------
    aux_data : any auxiliary data for the hooks (typically this rank's data shard)
    comm : communicator (default: world)
    loss_func_has_aux, sumstats_func_has_aux : aux flags as above
    device : device of the parameters (default: inferred from ``aux_data`` tensors)
    dtype : parameter dtype for non-tensor guesses (default float32)
    """

    aux_data: Any = None
    comm: Any = None
    loss_func_has_aux: bool = False
    sumstats_func_has_aux: bool = False
    device: Any = None
    dtype: Any = None

    # ------------------------------------------------------------------ user hooks
    def calc_partial_sumstats_from_params(self, params, randkey=None):
        """Custom method to map parameters to (partial) summary statistics."""
        raise NotImplementedError(
            "Subclass must implement `calc_partial_sumstats_func_from_params`")

    def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
        """Custom method to map summary statistics to loss."""
        raise NotImplementedError("Subclass must implement `calc_loss_func_from_sumstats`")

    # ------------------------------------------------------------------ plumbing
    def __post_init__(self):
        if self.comm is None:
            self.comm = get_world_comm()

    def _opt_comm(self):
        return self.comm

    def param_device(self) -> torch.device:
        if self.device is not None:
            return torch.device(self.device)
        return infer_device(self.aux_data)

    def _params(self, params) -> torch.Tensor:
        return as_param_tensor(params, device=self.param_device(), dtype=self.dtype)

    def _allreduce(self, x: torch.Tensor) -> torch.Tensor:
        x = x.detach().contiguous()
        if self.comm is not None and self.comm.size > 1:
            x = x.clone()
            self.comm.all_reduce(x)
        return x

    def run_lhs_param_scan(self, xmins, xmaxs, n_dim, num_evaluations, seed=None,
                           randkey=None):
        """Sumstats and loss over a Latin-hypercube sample of parameters.

        The sample is drawn on rank 0 and broadcast, so every rank evaluates the same
        points even with ``seed=None`` (reference Q8); with ``sumstats_func_has_aux`` the
        aux is passed to the loss properly (Q9).

        Returns ``(params[num_eval, n_dim], sumstats[num_eval, ...], losses[num_eval])``.
        """
        params = None
        if self.comm is None or self.comm.rank == 0:
            params = util.latin_hypercube_sampler(xmins, xmaxs, n_dim, num_evaluations, seed=seed)
        if self.comm is not None and self.comm.size > 1:
            params = self.comm.bcast(params, root=0)
        rk = _rk(randkey)
        # all partial sumstats first, then ONE all-reduce of the stacked [num_eval, ...]
        # tensor instead of one small collective per evaluation (reference
        # multigrad/multigrad.py:354-388 reduces inside the loop)
        partials, auxes = [], []
        with torch.no_grad():
            for x in params:
                r = self.calc_partial_sumstats_from_params(self._params(x), **rk)
                a = None
                if self.sumstats_func_has_aux:
                    r, a = r
                partials.append(torch.as_tensor(r))
                auxes.append(a)
        if not partials:
            return params, np.array([]), np.array([])
        totals = self._allreduce(torch.stack(partials))
        sumstats, losses = [], []
        for s, a in zip(totals, auxes):
            args = (s, a) if self.sumstats_func_has_aux else (s,)
            loss = self.calc_loss_from_sumstats(*args, **rk)
            if self.loss_func_has_aux:
                loss = loss[0]
            sumstats.append(np.asarray(s.cpu()))
            losses.append(float(loss))
        return params, np.array(sumstats), np.array(losses)

    # ------------------------------------------------------------------ sumstats
    def calc_sumstats_from_params(self, params, total: bool = True, randkey=None):
        """Summary statistics at ``params``, summed over ``comm`` when ``total``."""
        with torch.no_grad():
            result = self.calc_partial_sumstats_from_params(self._params(params), **_rk(randkey))
            aux = None
            if self.sumstats_func_has_aux:
                result, aux = result
            if total:
                result = self._allreduce(torch.as_tensor(result))
        return (result, aux) if self.sumstats_func_has_aux else result

    def calc_dloss_dsumstats(self, sumstats, sumstats_aux=None, randkey=None):
        """Gradient of the loss w.r.t. the (total) sumstats (``(grad, aux)`` with loss aux)."""
        s = torch.as_tensor(sumstats).detach().clone().requires_grad_(True)
        args = (s, sumstats_aux) if self.sumstats_func_has_aux else (s,)
        with torch.enable_grad():
            out = self.calc_loss_from_sumstats(*args, **_rk(randkey))
            loss = out[0] if self.loss_func_has_aux else out
            (g,) = torch.autograd.grad(loss, s, allow_unused=True)
        if g is None:
            g = torch.zeros_like(s)
        return (g, detach_tree(out[1])) if self.loss_func_has_aux else g

    def calc_loss_from_params(self, params, randkey=None):
        """Loss at ``params`` (sumstats summed over all ranks first)."""
        rk = _rk(randkey)
        with torch.no_grad():
            s = self.calc_sumstats_from_params(params, **rk)
            args = s if self.sumstats_func_has_aux else (s,)
            return detach_tree(self.calc_loss_from_sumstats(*args, **rk))

    def calc_dloss_dparams(self, params, randkey=None):
        """Gradient of the loss w.r.t. ``params`` (distributed chain rule)."""
        return self._vjp(params, randkey=randkey, include_loss=False)

    def calc_loss_and_grad_from_params(self, params, randkey=None):
        """``(loss, grad)`` -- cheaper than computing them separately."""
        return self._vjp(params, randkey=randkey, include_loss=True)

    def _vjp(self, params, randkey=None, include_loss=True):
        rk = _rk(randkey)
        p = self._params(params).detach().requires_grad_(True)
        with torch.enable_grad():
            out = self.calc_partial_sumstats_from_params(p, **rk)
            if self.sumstats_func_has_aux:
                partial, saux = out
            else:
                partial, saux = out, None
            partial = torch.as_tensor(partial)
            # (1) all-reduce the partial sumstats
            total = self._allreduce(partial).requires_grad_(True)
            args = (total, saux) if self.sumstats_func_has_aux else (total,)
            # (2) loss and its cotangent on the total sumstats (redundant on every rank)
            loss_out = self.calc_loss_from_sumstats(*args, **rk)
            loss = loss_out[0] if self.loss_func_has_aux else loss_out
            (cot,) = torch.autograd.grad(loss, total, allow_unused=True)
            if cot is None:
                cot = torch.zeros_like(total)
            # (3) local pullback with the global cotangent
            if partial.requires_grad:
                (g,) = torch.autograd.grad(partial, p, cot, allow_unused=True)
            else:
                g = None
        if g is None:
            g = torch.zeros_like(p)
        # (4) all-reduce the parameter gradient
        grad = self._allreduce(g)
        if include_loss:
            return detach_tree(loss_out), grad
        return grad

    # ------------------------------------------------------------------ second order
    def calc_hvp_from_params(self, params, vector, randkey=None):
        """Hessian of the all-rank loss at ``params`` times ``vector``; identical on every rank.

        The distributed chain rule at second order: with ``S = sum_r s_r(theta)``, ``J_r`` the
        Jacobian of this rank's partial sumstats and ``c = dl/dS``,

            H v = sum_r [ d/dtheta (J_r^T c) v  +  J_r^T (d2l/dS2) (sum_r' J_r' v) ]

        from one run of the hooks: ``J_r v`` by the double-VJP trick, then exact second
        derivatives of the hooks by autograd (every op the hooks use must be twice
        differentiable; ``gaussian_binned_sum`` and the group ops are).  Collectives per
        product: two of the sumstats' size, one of the parameters'.
        """
        return self._hvp_graph(params, randkey)(vector)

    def calc_hessian_from_params(self, params, randkey=None):
        """Dense ``[ndim, ndim]`` Hessian of the all-rank loss at ``params``, identical on every
        rank: ``ndim`` Hessian-vector products (:meth:`calc_hvp_from_params`, one per unit
        vector; the hooks run once and the loss cotangent is shared), symmetrised as
        ``(H + H^T)/2``.  The cost is ``ndim`` second-order backward passes and ``ndim^2``
        memory, so this is meant for tens to thousands of parameters (covariances and error
        bars at an optimum); larger problems use the products directly."""
        hvp = self._hvp_graph(params, randkey)
        p = hvp.params
        cols = []
        for i in range(p.numel()):
            v = torch.zeros_like(p).reshape(-1)
            v[i] = 1.0
            cols.append(hvp(v.reshape(p.shape)).reshape(-1))
        if not cols:
            return p.new_zeros(0, 0)
        H = torch.stack(cols, dim=1)
        return 0.5 * (H + H.T)

    def _hvp_graph(self, params, randkey=None):
        """Run the hooks once (aux and ``randkey`` as in ``_vjp``) and return ``hvp(vector)``,
        which can be called for several vectors; ``hvp.params`` is the parameter tensor."""
        rk = _rk(randkey)
        p = self._params(params).detach().requires_grad_(True)
        with torch.enable_grad():
            out = self.calc_partial_sumstats_from_params(p, **rk)
            partial, saux = out if self.sumstats_func_has_aux else (out, None)
            partial = torch.as_tensor(partial)
            # (1) total sumstats and the loss cotangent on them, kept differentiable
            total = self._allreduce(partial).requires_grad_(True)
            args = (total, saux) if self.sumstats_func_has_aux else (total,)
            loss_out = self.calc_loss_from_sumstats(*args, **rk)
            loss = loss_out[0] if self.loss_func_has_aux else loss_out
            cot = None
            if torch.is_tensor(loss) and loss.requires_grad:
                (cot,) = torch.autograd.grad(loss, total, create_graph=True, allow_unused=True)
            cot_is_const = cot is None or not cot.requires_grad  # the loss is linear in S
            cot_val = torch.zeros_like(total) if cot is None else cot.detach()
            # the local pullbacks u -> J^T u (for J v) and J^T cot, kept differentiable
            jt_u = jt_c = None
            if partial.requires_grad:
                u = torch.zeros_like(partial).requires_grad_(True)
                (jt_u,) = torch.autograd.grad(partial, p, u, create_graph=True, allow_unused=True)
                (jt_c,) = torch.autograd.grad(partial, p, cot_val, create_graph=True,
                                              allow_unused=True)

        def hvp(vector):
            v = torch.as_tensor(vector).to(p).reshape(p.shape)
            hv = torch.zeros_like(p)
            if jt_u is not None and jt_u.requires_grad:
                with torch.enable_grad():
                    # (2) J v = d/du <J^T u, v>, summed over the ranks
                    (jv,) = torch.autograd.grad(jt_u, u, v, retain_graph=True, allow_unused=True)
                    jv = self._allreduce(torch.zeros_like(partial) if jv is None else jv)
                    # (3) q = (d2l/dS2) J v: zero when the loss is linear in the sumstats
                    q = None
                    if not cot_is_const:
                        (q,) = torch.autograd.grad(cot, total, jv, retain_graph=True,
                                                   allow_unused=True)
                    # (4) d/dtheta <J^T cot, v> (zero when the sumstats are linear in the
                    # parameters) + J^T q
                    if jt_c is not None and jt_c.requires_grad:
                        (t1,) = torch.autograd.grad(jt_c, p, v, retain_graph=True,
                                                    allow_unused=True)
                        if t1 is not None:
                            hv = hv + t1
                    if q is not None:
                        (t2,) = torch.autograd.grad(partial, p, q, retain_graph=True,
                                                    allow_unused=True)
                        if t2 is not None:
                            hv = hv + t2
            else:
                # no local dependence on the parameters: this rank still joins the collectives
                self._allreduce(torch.zeros_like(partial))
            return self._allreduce(hv)

        hvp.params = p.detach()
        return hvp

    # ------------------------------------------------------------------ sumstat Jacobian
    def calc_sumstats_jacobian_from_params(self, params, randkey=None, mode: str = "auto"):
        """``(sumstats, jac)``: the all-rank total sumstats and their Jacobian with respect to
        the parameters, ``jac.shape == sumstats.shape + (ndim,)``; identical on every rank.
        The Jacobian adds across ranks like the sumstats, so both travel in one all-reduce
        of the packed block.

        ``mode="forward"``: ``ndim`` runs of the sumstats hook under
        ``torch.autograd.forward_ad`` with unit tangents (every op the hook applies to the
        parameters needs a forward rule: torch's own ops, ``gaussian_binned_sum`` and the
        group ops have one; ``gaussian_binned_sum_2d``, ``gaussian_binned_sum_multi``,
        ``gaussian_binned_sum_by_group`` and the SMF ops raise ``NotImplementedError``).
        ``mode="reverse"``: one run of the hook and one backward pass per sumstat, which works
        with every first-order op.
        ``mode="auto"`` (default): forward, and reverse if the hook meets an op without a
        forward rule.  Forward costs ``ndim`` runs of the hook and keeps no graph (peak
        memory of a ``no_grad`` evaluation); reverse costs one run and ``K`` backward passes.
        Measured on the grouped population model (profiles/binned_jvp/README.md, 4e6 halos,
        ``K = 10``), reverse is faster even at ``ndim = 8`` (1.4 ms against 2.7 ms) and far
        faster at ``ndim = 64``, because every forward column reruns the hook's own torch
        ops: pass ``mode="reverse"`` where speed matters and the graph fits.
        ``mode="native"``: the model's own
        ``calc_partial_sumstats_and_jacobian_from_params(params, randkey=None) -> (partial,
        jac)`` hook (optionally ``(partial, jac, sumstats_aux)``), for models that can write
        every row of their Jacobian in one pass
        (:class:`~multigrad_amd.models.population.PopulationSMFModel`); the base class does
        not define it, and ``mode="native"`` on a model without it raises ``ValueError``.
        ``mode="auto"`` uses the hook first when the model defines one.

        Aux and ``randkey`` are handled as in the gradient; the sumstats aux is not returned.
        """
        total, jac, _, _ = self._sumstats_jacobian(params, randkey, mode)
        return total, jac

    def _sumstats_jacobian(self, params, randkey=None, mode="auto"):
        """``(total, jac, sumstats_aux, mode_used)``; one all-reduce."""
        if mode not in ("auto", "forward", "reverse", "native"):
            raise ValueError("mode must be 'auto', 'forward', 'reverse' or 'native', "
                             f"got {mode!r}")
        p = self._params(params).detach()
        hook = getattr(self, "calc_partial_sumstats_and_jacobian_from_params", None)
        if mode == "native" and hook is None:
            raise ValueError("mode='native' needs the model to define "
                             "calc_partial_sumstats_and_jacobian_from_params")
        used = "reverse" if mode == "reverse" else "forward"
        if hook is not None and mode in ("auto", "native"):
            used = "native"
            with torch.no_grad():
                out = hook(p, **_rk(randkey))
            partial, jac = torch.as_tensor(out[0]).detach(), torch.as_tensor(out[1]).detach()
            saux = detach_tree(out[2]) if len(out) > 2 else None
        if used == "forward":
            try:
                partial, jac, saux = self._local_jacobian_forward(p, randkey)
            except NotImplementedError:
                # an op without a forward rule; every rank runs the same hook and lands here
                # before any collective, so the ranks stay in step
                if mode == "forward":
                    raise
                used = "reverse"
        if used == "reverse":
            partial, jac, saux = self._local_jacobian_reverse(p, randkey)
        k = partial.numel()
        if self.comm is None or self.comm.size == 1:
            # nothing to reduce: no packed copy of the K * ndim Jacobian
            jac = jac.detach().to(partial.dtype).reshape(partial.shape + (p.numel(),))
            return partial.detach(), jac, saux, used
        packed = self._allreduce(torch.cat([partial.reshape(-1),
                                            jac.reshape(-1).to(partial.dtype)]))
        total = packed[:k].reshape(partial.shape)
        jac = packed[k:].reshape(partial.shape + (p.numel(),))
        return total, jac, saux, used

    def _sumstats_hook(self, p, randkey):
        out = self.calc_partial_sumstats_from_params(p, **_rk(randkey))
        partial, saux = out if self.sumstats_func_has_aux else (out, None)
        return torch.as_tensor(partial), saux

    def _local_jacobian_forward(self, p, randkey):
        import torch.autograd.forward_ad as fwad
        primal, saux, cols = None, None, []
        with torch.no_grad():
            for i in range(p.numel()):
                unit = torch.zeros_like(p).reshape(-1)
                unit[i] = 1.0
                with fwad.dual_level():
                    partial, aux_i = self._sumstats_hook(fwad.make_dual(p, unit.reshape(p.shape)),
                                                         randkey)
                    value, tangent = fwad.unpack_dual(partial)
                    if primal is None:
                        primal, saux = value.detach(), detach_tree(aux_i)
                    cols.append(torch.zeros_like(value) if tangent is None else tangent)
            if primal is None:  # no parameters
                primal, saux = self._sumstats_hook(p, randkey)
        jac = torch.stack(cols, dim=-1) if cols else primal.new_zeros(primal.shape + (0,))
        return primal, jac, saux

    def _local_jacobian_reverse(self, p, randkey):
        p = p.requires_grad_(True)
        with torch.enable_grad():
            partial, saux = self._sumstats_hook(p, randkey)
            flat = partial.reshape(-1)
            rows = []
            for k in range(flat.numel()):
                g = None
                if partial.requires_grad:
                    unit = torch.zeros_like(flat)
                    unit[k] = 1.0
                    (g,) = torch.autograd.grad(flat, p, unit, retain_graph=True, allow_unused=True)
                rows.append(torch.zeros_like(p).reshape(-1) if g is None else g.reshape(-1))
        jac = torch.stack(rows) if rows else p.new_zeros(0, p.numel())
        return partial.detach(), jac.reshape(partial.shape + (p.numel(),)), saux

    def _loss_derivatives(self, total, saux, randkey):
        """The loss hook's output, gradient ``[K]`` and symmetrised Hessian ``[K, K]`` at
        the total sumstats, by autograd (a loss linear in the sumstats has a zero Hessian)."""
        s = total.detach().clone().requires_grad_(True)
        k = s.numel()
        args = (s, saux) if self.sumstats_func_has_aux else (s,)
        with torch.enable_grad():
            loss_out = self.calc_loss_from_sumstats(*args, **_rk(randkey))
            loss = loss_out[0] if self.loss_func_has_aux else loss_out
            cot = None
            if torch.is_tensor(loss) and loss.requires_grad:
                (cot,) = torch.autograd.grad(loss, s, create_graph=True, allow_unused=True)
            hess = s.new_zeros(k, k)
            if cot is not None and cot.requires_grad:
                flat = cot.reshape(-1)
                for i in range(k):
                    unit = torch.zeros_like(flat)
                    unit[i] = 1.0
                    (row,) = torch.autograd.grad(flat, s, unit, retain_graph=True,
                                                 allow_unused=True)
                    if row is not None:
                        hess[i] = row.reshape(-1)
        grad = torch.zeros_like(s) if cot is None else cot.detach()
        return detach_tree(loss_out), grad.reshape(-1), 0.5 * (hess + hess.T).detach()

    def calc_gauss_newton_from_params(self, params, randkey=None, mode: str = "auto",
                                      psd: bool = True):
        """``(loss, grad, G)`` at ``params``: the loss, its gradient ``J^T dl/dS`` and the
        Gauss-Newton matrix ``G = J^T H J``, where ``J`` is the sumstat Jacobian
        (:meth:`calc_sumstats_jacobian_from_params`, ``mode`` as there) and ``H`` the
        symmetrised ``[K, K]`` Hessian of the loss hook at the total sumstats (zero for a
        loss linear in the sumstats).  With ``psd=True`` the negative eigenvalues of ``H``
        are set to zero, so ``G`` is positive semi-definite whatever the loss.  ``grad``
        (the parameters' shape) and ``G`` (``[ndim, ndim]``) are float64 and identical on
        every rank; no collective beyond the Jacobian's."""
        return self._gauss_newton(params, randkey, mode, psd)[:3]

    def calc_gauss_newton_factors_from_params(self, params, randkey=None, mode: str = "auto",
                                              psd: bool = True):
        """``(loss, grad, J, H)`` at ``params``: the factors of the Gauss-Newton matrix
        ``J^T H J`` instead of the matrix.  ``J`` is the ``[K, ndim]`` sumstat Jacobian
        (flattened sumstats; the parameters' dtype and device, ``mode`` as in
        :meth:`calc_sumstats_jacobian_from_params`), ``H`` the symmetrised float64 ``[K, K]``
        Hessian of the loss hook on the host (negative eigenvalues set to zero with
        ``psd=True``) and ``grad = J^T dl/dS`` in the parameters' shape and dtype.  Nothing
        of size ``ndim x ndim`` is formed, so this works at any parameter count; ``J`` is
        ``K * ndim`` values (400 MB at ``K = 10`` and 1e7 float32 parameters).  Identical on
        every rank; no collective beyond the Jacobian's."""
        loss_out, c, J, H, _ = self._gauss_newton_factors(params, randkey, mode, psd)
        p = self._params(params)
        grad = (c.to(J.dtype) @ J).reshape(p.shape) if J.numel() else torch.zeros_like(p)
        return loss_out, grad, J, H

    def _gauss_newton_factors(self, params, randkey=None, mode="auto", psd=True):
        """``(loss, c, J, H, mode_used)``: ``c = dl/dS`` ``[K]`` on the parameters' device,
        ``J`` ``[K, ndim]`` in the parameters' dtype, ``H`` ``[K, K]`` float64 on the host."""
        total, jac, saux, used = self._sumstats_jacobian(params, randkey, mode)
        loss_out, gs, hess = self._loss_derivatives(total, saux, randkey)
        p = self._params(params)
        J = jac.reshape(total.numel(), -1).to(p.dtype)
        hess = hess.double().cpu()   # K is small: the eigendecomposition runs on the host
        if psd and hess.numel() and bool(torch.isfinite(hess).all()):
            lam, vec = torch.linalg.eigh(hess)
            hess = (vec * lam.clamp_min(0.0)) @ vec.T
        return loss_out, gs, J, hess, used

    def _gauss_newton(self, params, randkey=None, mode="auto", psd=True):
        total, jac, saux, used = self._sumstats_jacobian(params, randkey, mode)
        loss_out, gs, hess = self._loss_derivatives(total, saux, randkey)
        J = jac.reshape(total.numel(), -1).double()
        hess = hess.double()
        if psd and hess.numel():
            # K is small: the eigendecomposition runs on the host
            lam, vec = torch.linalg.eigh(hess.cpu())
            hess = ((vec * lam.clamp_min(0.0)) @ vec.T).to(J.device)
        grad = (J.T @ gs.double()).reshape(jac.shape[total.dim():])
        return loss_out, grad, J.T @ hess @ J, used

    def calc_fisher_from_params(self, params, sumstats_cov, randkey=None, mode: str = "auto"):
        """The Fisher matrix ``J^T C^-1 J`` (float64, ``[ndim, ndim]``, identical on every
        rank) of the sumstats at ``params`` for Gaussian errors: ``sumstats_cov`` holds the
        ``K`` variances or the ``[K, K]`` covariance of the (flattened) total sumstats."""
        total, jac, _, _ = self._sumstats_jacobian(params, randkey, mode)
        k = total.numel()
        J = jac.reshape(k, -1).double()
        cov = torch.as_tensor(sumstats_cov).detach().to(device=J.device, dtype=torch.float64)
        if cov.shape == (k,):
            return J.T @ (J / cov[:, None])
        if cov.shape == (k, k):
            # K is small: the solve runs on the host
            return J.T @ torch.linalg.solve(cov.cpu(), J.cpu()).to(J.device)
        raise ValueError(f"sumstats_cov must have shape ({k},) or ({k}, {k}), "
                         f"got {tuple(cov.shape)}")

    def run_gauss_newton(self, guess, maxsteps: int = 50, randkey=None, damping: float = 1e-3,
                         ftol: float = 2.2e-9, gtol: float = 1e-8, mode: str = "auto",
                         param_bounds=None, solver: str = "auto"):
        """Damped Gauss-Newton (Levenberg-Marquardt) fit from ``guess``; returns a
        ``scipy.optimize.OptimizeResult`` on every rank
        (:func:`multigrad_amd.optim.gauss_newton.run_gauss_newton`).  Each iteration takes one
        sumstat Jacobian (``mode`` as in :meth:`calc_sumstats_jacobian_from_params`) and one
        loss evaluation per trial step; ``randkey`` is held constant.  Parameter bounds are
        not offered here: :meth:`run_gauss_newton_box` takes them.

        ``solver="dense"`` forms the ``[ndim, ndim]`` Gauss-Newton matrix and solves on the
        host (thousands of parameters at most).  ``solver="dual"`` solves the same damped
        system through its ``K x K`` dual
        (:func:`multigrad_amd.optim.gauss_newton.run_gauss_newton_dual`): every
        ``ndim``-sized vector stays on the parameters' device, ``res.x`` and ``res.jac`` are
        tensors there, ``res.hess_inv`` is an operator and ``res.solver == "dual"``; it holds
        the ``K * ndim`` Jacobian (400 MB at ``K = 10`` and 1e7 float32 parameters) and works
        at any parameter count.  ``solver="auto"`` (default) picks the dual form only for
        ``ndim > 8192``, where the dense float64 matrix passes 0.5 GB."""
        from ..optim import gauss_newton as _gn
        if param_bounds is not None:
            raise ValueError("run_gauss_newton does not offer parameter bounds; use "
                             "run_gauss_newton_box (or run_bfgs, run_adam) for a bounded fit")
        if solver not in ("auto", "dense", "dual"):
            raise ValueError(f"solver must be 'auto', 'dense' or 'dual', got {solver!r}")
        key = None if randkey is None else (
            randkey if hasattr(randkey, "split") else init_randkey(randkey))
        x0 = as_param_tensor(guess, device=self.param_device(), dtype=self.dtype)
        if solver == "dual" or (solver == "auto" and x0.numel() > 8192):
            return _gn.run_gauss_newton_dual(
                lambda x: self._gauss_newton_factors(x, key, mode, True),
                lambda x: self.calc_loss_from_params(x, randkey=key),
                x0, maxsteps=maxsteps, damping=damping, ftol=ftol, gtol=gtol, comm=self.comm)
        return _gn.run_gauss_newton(
            lambda x: self._gauss_newton(x, key, mode, True),
            lambda x: self.calc_loss_from_params(x, randkey=key),
            x0, maxsteps=maxsteps, damping=damping, ftol=ftol, gtol=gtol, comm=self.comm)

    def run_gauss_newton_box(self, guess, param_bounds=None, max_step=None, maxsteps: int = 50,
                             randkey=None, damping: float = 1e-3, min_damping: float = 1e-4,
                             ftol: float = 2.2e-9, gtol: float = 1e-8, inner_passes: int = 40,
                             mode: str = "auto"):
        """Damped Gauss-Newton fit from ``guess`` inside ``param_bounds`` (a reference-style
        ``(ndim, 2)`` spec, ``None`` for an open side) and with no parameter moving by more
        than ``max_step`` (a scalar or ``[ndim]``, in parameter units) in one step
        (:func:`multigrad_amd.optim.gauss_newton_box.run_gauss_newton_box`).  Every trial step
        is the exact minimiser of the damped model inside that box, found through its
        ``K x K`` dual, so every point the loss sees lies inside the bounds.  It always runs
        the dual form: ``res.x``, ``res.jac`` and ``res.active`` are tensors on the
        parameters' device, ``res.hess_inv`` is an operator and ``res.solver == "dual-box"``.
        ``mode`` and ``randkey`` as in :meth:`run_gauss_newton`."""
        from ..optim import gauss_newton_box as _gnb
        key = None if randkey is None else (
            randkey if hasattr(randkey, "split") else init_randkey(randkey))
        x0 = as_param_tensor(guess, device=self.param_device(), dtype=self.dtype)
        return _gnb.run_gauss_newton_box(
            lambda x: self._gauss_newton_factors(x, key, mode, True),
            lambda x: self.calc_loss_from_params(x, randkey=key),
            x0, param_bounds=param_bounds, max_step=max_step, maxsteps=maxsteps,
            damping=damping, min_damping=min_damping, ftol=ftol, gtol=gtol,
            inner_passes=inner_passes, comm=self.comm)

    # ------------------------------------------------------------------ identity
    def __hash__(self):
        name = getattr(self.comm, "name", None)
        return hash((name, type(self).calc_loss_from_sumstats))

    def __eq__(self, other):
        # identity equality (the reference compares against OnePointGroup)
        return self is other


@dataclass
class OnePointGroup(_OptimizerFrontEnds):
    """Sum of several models' losses, each model on its own sub-communicator.

    Only each sub-communicator's rank 0 contributes its model's ``(loss, grad)``; the
    contributions are summed with ONE all-reduce of a packed ``[loss, grad...]`` vector
    over ``main_comm`` (reference: two pickled allgathers, ``multigrad/multigrad.py:578-580``).
    Ranks may hold different numbers of models.
    """

    models: Union[Tuple[OnePointModel, ...], OnePointModel] = ()
    main_comm: Any = None

    def __post_init__(self):
        if self.main_comm is None:
            self.main_comm = get_world_comm()
        if isinstance(self.models, OnePointModel):
            self.models = (self.models,)
        self.models = tuple(self.models)
        assert len(self.models) and isinstance(self.models[0], OnePointModel)

    def _opt_comm(self):
        return self.main_comm

    @property
    def comm(self):
        return self.main_comm

    def param_device(self) -> torch.device:
        return self.models[0].param_device()

    def calc_loss_and_grad_from_params(self, params, randkey=None):
        rk = _rk(randkey)
        packed, gshape = None, None
        for model in self.models:
            loss, grad = model.calc_loss_and_grad_from_params(params, **rk)
            if isinstance(loss, (tuple, list)):
                loss = loss[0]
            gshape = grad.shape
            vec = torch.cat([torch.as_tensor(loss).reshape(1).to(grad), grad.reshape(-1)])
            if model.comm is not None and model.comm.rank:
                vec = torch.zeros_like(vec)
            packed = vec if packed is None else packed + vec
        if self.main_comm is not None and self.main_comm.size > 1:
            packed = packed.contiguous()
            self.main_comm.all_reduce(packed)
        return packed[0], packed[1:].reshape(gshape)

    def calc_loss_from_params(self, params, randkey=None):
        return self.calc_loss_and_grad_from_params(params, randkey=randkey)[0]

    def calc_dloss_dparams(self, params, randkey=None):
        return self.calc_loss_and_grad_from_params(params, randkey=randkey)[1]

    def __hash__(self):
        return hash((getattr(self.main_comm, "name", None), self.models[0]))

    def __eq__(self, other):
        return self is other
