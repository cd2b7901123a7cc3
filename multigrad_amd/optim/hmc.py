"""Hamiltonian Monte Carlo on the device, SPMD like the device L-BFGS.

The optimizers give Gaussian error bars at the optimum (``hess_inv``, the Hessian, the Fisher
matrix); this module draws from the posterior itself.  The potential is
``U = loss_scale * loss`` (``loss_scale = 0.5`` for a chi^2 loss), the kinetic energy
``K = 1/2 sum p^2 inv_mass`` with a diagonal mass.  The reference has no sampler.

* **Vectors** (position, momentum, gradient, ``inv_mass``, the Welford moments) are fp32
  device tensors -- replicated, or sharded 1/W per rank over an engine objective -- and all
  vector work is three fused kernels (``csrc/hmc.hip``): a trajectory of ``L`` leapfrog steps
  is ``L + 1`` launches of ``hmc_leapfrog_`` around the ``L`` evaluations, the momentum draw
  is ``hmc_momentum_``, and ``hmc_commit_`` folds the kept position into the moments, the
  tracked chains and the sample row in one pass.  Energies are fp64.
* **One iteration** ``t`` (0-based, warm-up and sampling counted together): draw the noise,
  ``hmc_momentum_``, ``L`` steps of size ``eps_t = eps (1 + jitter (2 u_jitter - 1))``,
  ``dH = (U' + K') - (U + K)``, accept if ``u_accept < exp(min(0, -dH))``.  A non-finite
  ``dH`` or ``dH > 1000`` rejects and counts as divergent.  Rejection is a pointer swap on the
  host; the gradient at the kept position is cached, so an iteration costs ``L`` evaluations.
* **Device-resident evaluation**: with ``obj.device_call`` the ``L`` evaluations stay on the
  device and ``[K, K', U']`` reach the host in one copy per trajectory.  On a sharded
  objective ``K`` is summed over the ranks in that same reduction
  (:class:`~multigrad_amd.optim._reduce.DeviceReducer`), so every decision is taken on values
  identical on all ranks: no broadcasts.
* **Noise** comes from a ``noise`` object: ``normal(t, n, device) -> float32[n]`` and
  ``uniforms(t) -> (u_accept, u_jitter)``.  The default :class:`KeyNoise` is a documented
  recipe, the same on every rank of a replicated run.
* **Warm-up** adapts the step size by dual averaging (Hoffman & Gelman 2014: ``gamma = 0.05``,
  ``t0 = 10``, ``kappa = 0.75``, ``mu = log(10 eps)``) and the diagonal mass in Stan's windows
  (:func:`warmup_windows`).  At the end of a window over ``c`` draws
  ``inv_mass = (c / (c + 5)) var + 1e-3 * 5 / (c + 5)``, the moments are reset and dual
  averaging restarts from the averaged step; sampling uses the averaged step.
* **Bounds** (``GenericObjective(bounds=...)``) sample the unbounded coordinate ``u`` of
  :mod:`~multigrad_amd.optim.transforms` with a flat prior on the bounded parameter:
  ``U(u) = loss_scale * loss(x(u)) - sum log dp/du``.  Samples, ``mean`` and ``var`` are in the
  bounded parameters.
* **Prior** (``prior=``, a :class:`~multigrad_amd.optim.prior.GaussianPrior`): the chain draws
  from ``exp(-(loss_scale * loss + pen))`` -- the prior is a density and is not scaled by
  ``loss_scale``, so the MAP of this posterior is
  ``run_bfgs(prior=..., prior_weight=1 / loss_scale)``.  ``g`` stays the gradient of the loss
  (the cached one included): every leapfrog launch is ``hmc_leapfrog_prior_``
  (``csrc/prior.hip``), which takes the prior's force from the position it reads, and the
  launch that ends a trajectory also sums the penalty there, so ``[K, K', pen']`` travel in
  the one reduction and ``U' = loss_scale * loss' + pen'`` comes out of the same single copy.
  With bounds the prior is folded into the wrapped function in ``x`` before the chain rule:
  ``U(u) = loss_scale * loss(x(u)) + pen(x(u)) - sum log dp/du``.  ``prior=None`` runs the
  code without any of this.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import numpy as np
import scipy.optimize
import torch

from ..ops.hmc import hmc_commit_, hmc_leapfrog_, hmc_momentum_, hmc_workspace
from ..ops.prior import gaussian_prior_grad_, hmc_leapfrog_prior_, prior_workspace
from ..utils.random import PRNGKey, init_randkey
from ._quasi_newton import driver, finish
from ._reduce import DeviceReducer

__all__ = ["hmc_sample", "run_hmc", "KeyNoise", "HMCResult", "warmup_windows", "DualAveraging"]

_MAX_DH = 1000.0


class HMCResult(scipy.optimize.OptimizeResult):
    """Result of :func:`hmc_sample` (attribute access as ``OptimizeResult``), on every rank,
    in the user's parameter order:

    ``samples`` ``[nsamples, P]`` (``history="full"``, else ``None``), ``tracked``
    ``[nsamples, len(track)]`` (or ``None``), ``mean`` / ``var`` ``[P]`` of the draws (``var``
    with ``ddof = 1``), ``x`` the last position, ``potential`` ``[nsamples]`` (numpy, ``U`` of
    every draw), ``accept_rate`` (of the sampling iterations; of the warm-up when
    ``nsamples = 0``; with a prior ``U`` includes the penalty), ``step_size``, ``inv_mass`` (one element while no mass was adapted or
    given per parameter), ``n_divergent`` (of the sampling iterations; the warm-up's, which
    dual averaging provokes while it explores steps up to ten times the initial one, are
    ``n_divergent_warmup``), ``nfev``, ``warmup_windows``."""


class KeyNoise:
    """The default random numbers of :func:`hmc_sample`, for iteration ``t``::

        k = key.fold_in(t)
        z = torch.randn(n, generator=k.generator(device), device=device)   # float32
        u_accept, u_jitter = k.numpy_rng().random(2)

    On a sharded objective (``rank`` given) the normals use ``k.fold_in(rank + 1)`` instead
    of ``k``, so every rank draws its own slice; the uniforms are the same on all ranks."""

    def __init__(self, key, rank: Optional[int] = None):
        self.key: PRNGKey = init_randkey(key)
        self.rank = rank

    def normal(self, t: int, n: int, device) -> torch.Tensor:
        k = self.key.fold_in(t)
        if self.rank is not None:
            k = k.fold_in(self.rank + 1)
        return torch.randn(n, generator=k.generator(device), device=device, dtype=torch.float32)

    def uniforms(self, t: int) -> Tuple[float, float]:
        u = self.key.fold_in(t).numpy_rng().random(2)
        return float(u[0]), float(u[1])


def warmup_windows(warmup: int) -> List[Tuple[int, int]]:
    """Stan's slow (mass-adaptation) windows ``[(start, end), ...]`` of a warm-up of
    ``warmup`` iterations: initial buffer 75, final buffer 50, windows of 25, 50, 100, ...
    where the last one extends to the final buffer when the next doubled window would not
    fit -- ``warmup = 1000``: ``(75,100) (100,150) (150,250) (250,450) (450,950)``.  Below 150
    iterations the split is 15 % / 75 % / 10 % with one window; below 20 there is none (step
    size only)."""
    warmup = int(warmup)
    if warmup < 20:
        return []
    if warmup < 150:
        first, last = int(0.15 * warmup), int(0.1 * warmup)
        return [(first, warmup - last)]
    end_slow = warmup - 50
    out, start, size = [], 75, 25
    while start < end_slow:
        end = start + size
        if end + 2 * size > end_slow:
            end = end_slow
        out.append((start, end))
        start, size = end, 2 * size
    return out


class DualAveraging:
    """Step-size adaptation of Hoffman & Gelman (2014), Algorithm 5."""

    def __init__(self, eps: float, target: float = 0.8, gamma: float = 0.05, t0: float = 10.0,
                 kappa: float = 0.75):
        self.target, self.gamma, self.t0, self.kappa = target, gamma, t0, kappa
        self.restart(eps)

    def restart(self, eps: float) -> None:
        self.mu = math.log(10.0 * eps)
        self.m = 0
        self.hbar = 0.0
        self.log_eps = math.log(eps)
        self.log_avg = 0.0

    def update(self, accept_prob: float) -> float:
        """Fold one acceptance probability in; returns the next step size."""
        self.m += 1
        m = self.m
        w = 1.0 / (m + self.t0)
        self.hbar = (1.0 - w) * self.hbar + w * (self.target - accept_prob)
        self.log_eps = self.mu - math.sqrt(m) / self.gamma * self.hbar
        eta = m ** -self.kappa
        self.log_avg = eta * self.log_eps + (1.0 - eta) * self.log_avg
        return math.exp(self.log_eps)

    @property
    def averaged(self) -> float:
        return math.exp(self.log_avg if self.m else self.log_eps)


def _local_track(layout, track: torch.Tensor, P: int, device) -> torch.Tensor:
    """Positions of the user indices ``track`` in the objective's local vector (-1 where this
    rank does not hold one)."""
    ids = layout.to_local(torch.arange(1, P + 1, dtype=torch.int64, device=device))
    pos = torch.full((P + 1,), -1, dtype=torch.int64, device=device)
    pos[ids] = torch.arange(ids.numel(), dtype=torch.int64, device=device)
    pos[0] = -1  # padding
    return pos[track + 1].contiguous()


@driver(single_thread_blas=False)
def hmc_sample(obj, nsamples: int = 1000, warmup: int = 500, nleapfrog: int = 10,
               step_size: float = 0.1, loss_scale: float = 1.0, jitter: float = 0.0,
               seed=0, noise=None, target_accept: float = 0.8, adapt_step_size: bool = True,
               adapt_mass: bool = True, inv_mass=None, history: str = "full",
               track=None, prior=None) -> HMCResult:
    """Sample ``exp(-loss_scale * loss)`` -- with ``prior``,
    ``exp(-(loss_scale * loss + prior.penalty(x)))`` -- over ``obj`` (the objective interface of the device
    L-BFGS: :class:`~multigrad_amd.optim.lbfgs.GenericObjective`, the engine objective) by
    HMC; see the module docstring for the algorithm.

    Parameters
    ----------
    nsamples, warmup : sampling and warm-up iterations (``warmup = 0``: no adaptation)
    nleapfrog : leapfrog steps ``L`` per trajectory
    step_size : the (initial) step ``eps``
    loss_scale : ``U = loss_scale * loss``
    jitter : relative step jitter, ``eps_t = eps (1 + jitter (2 u - 1))``
    seed : int or :class:`~multigrad_amd.utils.random.PRNGKey` of the default
        :class:`KeyNoise`; ``noise`` replaces it (``normal(t, n, device)``, ``uniforms(t)``)
    target_accept, adapt_step_size : dual averaging during the warm-up
    adapt_mass : adapt the diagonal mass in the warm-up windows
    inv_mass : initial inverse mass, a scalar or a vector in the user's parameter order (with
        bounds: of the unbounded coordinate); default 1
    history : ``"full"`` returns ``samples [nsamples, P]``, ``"moments"`` only ``mean``, ``var``
    track : indices (user order) whose chains are always returned, ``[nsamples, len(track)]``;
        at 1e7 parameters ``history="moments"`` with ``track`` is the intended use
    prior : a :class:`~multigrad_amd.optim.prior.GaussianPrior` on the (bounded) parameters,
        not scaled by ``loss_scale``; the MAP of the sampled posterior is
        ``run_bfgs(prior=prior, prior_weight=1 / loss_scale)``

    Returns
    -------
    :class:`HMCResult`, the same on every rank."""
    if history not in ("full", "moments"):
        raise ValueError("history must be 'full' or 'moments'")
    nsamples, warmup, L = int(nsamples), int(warmup), int(nleapfrog)
    if nsamples < 0 or warmup < 0 or L < 1:
        raise ValueError("nsamples >= 0, warmup >= 0 and nleapfrog >= 1")
    if not step_size > 0:
        raise ValueError("step_size must be positive")
    comm, sharded = obj.comm, obj.sharded
    n, dev = obj.n_local, obj.device
    layout = obj.vector_layout()
    identity = bool(getattr(layout, "identity", False))
    P = int(layout.P)
    bounds = getattr(obj, "bounds", None)
    scale = float(loss_scale)
    pm = pw = None
    if prior is not None:
        from .prior import check_prior, penalised_function
        check_prior(prior, P)  # before any collective
        if bounds is not None:
            # the prior is on x: into the wrapped function, before the chain rule to u; the
            # evaluation below multiplies the whole of it by loss_scale
            import copy
            obj = copy.copy(obj)
            obj.fn = penalised_function(obj.fn, prior, 1.0 / scale)
        else:
            pm, pw = prior.local(layout, dev)
    red = DeviceReducer(comm, sharded, dev)  # collective (may connect peer memory)
    if noise is None:
        rank = comm.rank if (sharded and comm is not None and comm.size > 1) else None
        noise = KeyNoise(seed, rank=rank)
    # with bounds the evaluation below returns U and its gradient themselves; otherwise the
    # loss and its gradient, and loss_scale rides in the kernel's step factor
    gscale = 1.0 if bounds is not None else scale
    dev_call = getattr(obj, "device_call", None) if (dev.type == "cuda" and bounds is None) else None
    nfev = 0

    def evaluate(x):
        """Host evaluation: (U, gradient to be scaled by gscale)."""
        nonlocal nfev
        nfev += 1
        f, gr = obj(x)
        if bounds is None:
            return scale * f, gr
        jac = float(bounds.log_dpdu(x).double().sum())
        return scale * f - jac, scale * gr - bounds.dlog_dpdu(x)

    # ---------------------------------------------------------------- state
    q = obj.x0().contiguous()
    U, g0 = evaluate(q)
    g = g0.clone()  # the objective may return a view of a buffer the next evaluation reuses
    if not math.isfinite(U):
        raise ValueError(f"HMC: the potential at the initial position is {U}")
    q_new, g_new, p = torch.empty_like(q), torch.empty_like(g), torch.empty_like(q)
    # [K, K'] and, with a prior, pen' behind them: one block for the one reduction
    ke = torch.zeros(2 if pm is None else 3, dtype=torch.float64, device=dev)
    ke0, ke1 = ke[0:1], ke[1:2]
    ws = hmc_workspace(dev)
    if pm is not None:
        pen1, pws = ke[2:3], prior_workspace(dev)
        # the penalty at the start (g_new is scratch here: out = g + 0), summed over the ranks
        gaussian_prior_grad_(q, g, pm, pw, 0.0, g_new, pen1, pws)
        U += float(red.reduce(sums=[pen1])[0])
        if not math.isfinite(U):
            raise ValueError(f"HMC: the potential at the initial position is {U}")
    # the padding of an engine vector stays where it is: no momentum there
    real = None
    if not identity and n:
        mask = layout.to_local(torch.ones(P, dtype=torch.float32, device=dev))
        if bool((mask == 0).any()):
            real = mask
    if inv_mass is None:
        im = torch.ones(1, dtype=torch.float32, device=dev)
    else:
        im = torch.as_tensor(inv_mass, dtype=torch.float32, device=dev).reshape(-1)
        if im.numel() != 1:
            if im.numel() != P:
                raise ValueError(f"inv_mass must be a scalar or have {P} elements")
            im = layout.to_local(im)
            if real is not None:
                im = torch.where(real > 0, im, torch.ones_like(im))
        im = im.contiguous().clone()
        if not bool((im > 0).all()) or not bool(torch.isfinite(im).all()):
            raise ValueError("inv_mass must be positive and finite")
    windows = warmup_windows(warmup) if adapt_mass else []
    mean = torch.zeros(n, dtype=torch.float32, device=dev)
    m2 = torch.zeros(n, dtype=torch.float32, device=dev)
    keep_full = history == "full"
    samples = torch.zeros((nsamples, n), dtype=torch.float32, device=dev) if keep_full else None
    track_idx = tracked = None
    if track is not None:
        tr = torch.as_tensor(track, dtype=torch.int64, device=dev).reshape(-1)
        if tr.numel() and (int(tr.min()) < 0 or int(tr.max()) >= P):
            raise ValueError(f"track indices must lie in [0, {P})")
        track_idx = tr.contiguous() if identity else _local_track(layout, tr, P, dev)
        tracked = torch.zeros((nsamples, tr.numel()), dtype=torch.float32, device=dev)
    potential = np.zeros(nsamples)
    eps = float(step_size)
    da = DualAveraging(eps, target=target_accept) if (adapt_step_size and warmup > 0) else None
    win = 0
    n_acc = n_acc_warm = n_div = n_div_warm = 0

    from ..utils.hooks import StepHooks
    from ..utils.progress import trange
    hooks = StepHooks(comm, what="HMC position")  # MULTIGRAD_CHECK_EVERY / _METRICS
    total = warmup + nsamples
    bar = trange(total, desc="HMC Sampling Progress")
    for t in bar:
        # ------------------------------------------------------------ trajectory
        u_acc, u_jit = noise.uniforms(t)
        e = eps * (1.0 + jitter * (2.0 * u_jit - 1.0))
        z = noise.normal(t, n, dev)
        if real is not None:
            z = z * real
        hmc_momentum_(z.contiguous(), im, p, ke0, ws)
        q_new.copy_(q)
        if pm is None:
            hmc_leapfrog_(q_new, p, g, im, 0.5 * e * gscale, e)
        else:
            hmc_leapfrog_prior_(q_new, p, g, im, 0.5 * e * gscale, e, pm, pw, 0.5 * e)
        for i in range(L):
            last = i == L - 1
            if dev_call is not None:
                nfev += 1
                lt, gt = dev_call(q_new)
            else:
                U_new, gt = evaluate(q_new)
            if last:
                g_new.copy_(gt)
                if pm is None:
                    hmc_leapfrog_(q_new, p, g_new, im, 0.5 * e * gscale, 0.0, ke1, ws)
                else:  # b = 0: the penalty it sums is the one at the final position
                    hmc_leapfrog_prior_(q_new, p, g_new, im, 0.5 * e * gscale, 0.0, pm, pw,
                                        0.5 * e, ke1, pen1, pws)
            elif pm is None:
                hmc_leapfrog_(q_new, p, gt, im, e * gscale, e)
            else:
                hmc_leapfrog_prior_(q_new, p, gt, im, e * gscale, e, pm, pw, e)
        # K, K' (summed over the ranks of a sharded objective) and U' in one copy
        if dev_call is not None:
            h = red.reduce(sums=[ke], local=[lt.reshape(-1)[:1]])
            U_new = scale * float(h[-1])
        else:
            h = red.reduce(sums=[ke])
        if pm is not None:
            U_new += float(h[2])
        dH = (U_new + float(h[1])) - (U + float(h[0]))
        divergent = not math.isfinite(dH) or dH > _MAX_DH
        prob = 0.0 if divergent else math.exp(min(0.0, -dH))
        accept = (not divergent) and u_acc < prob
        if accept:
            q, q_new = q_new, q
            g, g_new = g_new, g
            U = U_new
        if t < warmup:
            n_div_warm += int(divergent)
        else:
            n_div += int(divergent)
        # ------------------------------------------------------------ warm-up / commit
        if t < warmup:
            n_acc_warm += int(accept)
            if da is not None:
                eps = da.update(prob)
            if win < len(windows) and windows[win][0] <= t < windows[win][1]:
                s0, s1 = windows[win]
                c = t - s0 + 1
                hmc_commit_(q, c, mean, m2)
                if t == s1 - 1:
                    var = m2 / max(c - 1, 1)
                    im = ((c / (c + 5.0)) * var + 1e-3 * 5.0 / (c + 5.0)).contiguous()
                    if real is not None:
                        im = torch.where(real > 0, im, torch.ones_like(im))
                    mean.zero_()
                    m2.zero_()
                    win += 1
                    if da is not None:
                        eps = da.averaged
                        da.restart(eps)
            if t == warmup - 1:
                if da is not None:
                    eps = da.averaged
                mean.zero_()
                m2.zero_()
        else:
            i = t - warmup
            n_acc += int(accept)
            potential[i] = U
            x = obj.full(q) if identity else q
            hmc_commit_(x.contiguous(), i + 1, mean, m2, track_idx,
                        tracked[i] if tracked is not None else None,
                        samples[i] if keep_full else None)
        if hooks.active:
            hooks(t, U, None, (lambda: q) if not sharded else None)
    if hasattr(bar, "close"):
        bar.close()
    xf = finish(obj, red, q, "HMC")
    # ---------------------------------------------------------------- results, user order
    var = m2 / max(nsamples - 1, 1)
    if tracked is not None and not identity and sharded and comm is not None and comm.size > 1:
        comm.all_reduce(tracked)  # the owner's values; zeros elsewhere
    rate = n_acc / nsamples if nsamples else (n_acc_warm / warmup if warmup else 0.0)
    return HMCResult(
        samples=layout.from_local(samples) if keep_full else None, tracked=tracked,
        mean=layout.from_local(mean), var=layout.from_local(var), x=xf, potential=potential,
        accept_rate=rate, step_size=eps,
        inv_mass=im if im.numel() == 1 else layout.from_local(im), n_divergent=n_div, n_divergent_warmup=n_div_warm, nfev=nfev,
        warmup_windows=windows, reduction=red.describe())


def run_hmc(loss_and_grad_fn: Callable, params, nsamples: int = 1000, warmup: int = 500,
            nleapfrog: int = 10, step_size: float = 0.1, param_bounds=None, randkey=0, comm=None,
            loss_scale: float = 1.0, history: str = "full", track=None, prior=None,
            **kw) -> HMCResult:
    """HMC for a generic ``loss_and_grad_fn(params) -> (loss, grad)`` (replicated: the
    gradient is the same on every rank).  ``randkey`` (int or key) seeds the sampler's noise;
    with ``param_bounds`` the chain runs in the unbounded coordinates with a flat prior on the
    bounded parameters unless ``prior`` (a :class:`~multigrad_amd.optim.prior.GaussianPrior`,
    on the bounded parameters, not scaled by ``loss_scale``) says otherwise: the chain draws
    from ``exp(-(loss_scale * loss + prior.penalty(x)))``, whose MAP is
    ``run_bfgs(prior=prior, prior_weight=1 / loss_scale)``.  Other keywords go to
    :func:`hmc_sample`."""
    from ..utils.tensors import as_param_tensor
    from .lbfgs import GenericObjective
    from .transforms import Bounds
    from .prior import check_prior
    x0 = as_param_tensor(params)
    check_prior(prior, x0.numel())
    bounds = Bounds.from_spec(param_bounds, x0.numel(), device=x0.device, dtype=torch.float32)
    obj = GenericObjective(loss_and_grad_fn, x0, comm=comm, bounds=bounds)
    return hmc_sample(obj, nsamples=nsamples, warmup=warmup, nleapfrog=nleapfrog,
                      step_size=step_size, loss_scale=loss_scale, seed=randkey, history=history,
                      track=track, prior=prior, **kw)
