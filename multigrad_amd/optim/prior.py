"""Gaussian parameter priors for the device L-BFGS(-B), scipy's BFGS and the HMC sampler.

A model's loss sees only the sumstats, so a prior or a regulariser on the parameters is
added here, outside the model: :class:`GaussianPrior` holds a mean and a width per parameter
(a width of ``inf`` leaves a parameter flat) and the penalty is::

    pen(x) = 1/2 sum_i ((x_i - m_i) / sigma_i)^2

* The optimizers minimise ``loss + prior_weight * pen(x)`` (``prior_weight = 1`` by default).
* The sampler draws from ``exp(-(loss_scale * loss + pen))``: the prior is a density and is
  not scaled by ``loss_scale``.  The MAP of that posterior is therefore
  ``run_bfgs(prior=..., prior_weight=1 / loss_scale)``.
* The prior is always on the bounded parameter ``x``, never on the unbounded coordinate ``u``
  of :mod:`~multigrad_amd.optim.transforms`.

On the ``P``-sized device vectors the prior is applied by the kernels of ``csrc/prior.hip``
(:mod:`multigrad_amd.ops.prior`): :class:`PriorObjective` wraps an objective of the device
L-BFGS(-B) and adds the prior's gradient in one pass that also sums the penalty, and the
sampler's leapfrog takes the prior's force inside its own pass.

Out of scope: Adam and plain gradient descent (their fused and captured engines apply the
update inside model kernels), the Gauss-Newton drivers (a prior's gradient is not in the
range of ``J^T``, so the ``K x K`` dual changes shape) and non-Gaussian priors.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from ..ops.prior import gaussian_prior_grad_, prior_workspace

__all__ = ["GaussianPrior", "PriorObjective", "penalised_function", "check_prior",
           "with_penalty"]


def _as_array(v, what: str) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().double().numpy()
    elif isinstance(v, (list, tuple)):
        v = [np.inf if e is None else e for e in v] if what == "sigma" else v
        v = [float(e.detach().cpu()) if isinstance(e, torch.Tensor) else e for e in v]
    a = np.asarray(v, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError(f"GaussianPrior: {what} must be a scalar or a vector")
    return a.reshape(-1) if a.ndim == 1 else a


class GaussianPrior:
    """Independent Gaussian prior ``x_i ~ N(mean_i, sigma_i^2)`` on the parameters.

    ``mean`` and ``sigma`` are each a scalar or a length-``P`` array in the user's parameter
    order.  A ``sigma`` entry of ``inf`` (or ``None`` in a list) makes that parameter flat: its
    inverse variance is 0 and its mean is not read.  ``sigma <= 0``, a NaN, a non-finite
    ``mean`` of a parameter that is not flat, or two vectors of different lengths raise
    ``ValueError``.

    The optimizers minimise ``loss + prior_weight * penalty(x)``; the sampler draws from
    ``exp(-(loss_scale * loss + penalty(x)))``, whose MAP is
    ``run_bfgs(prior=..., prior_weight=1 / loss_scale)``."""

    def __init__(self, mean, sigma):
        m, s = _as_array(mean, "mean"), _as_array(sigma, "sigma")
        if np.isnan(s).any() or np.isnan(m).any():
            raise ValueError("GaussianPrior: NaN in mean or sigma")
        if not (s > 0).all():
            raise ValueError("GaussianPrior: sigma must be positive (inf or None: flat)")
        if m.ndim == 1 and s.ndim == 1 and m.size != s.size:
            raise ValueError(f"GaussianPrior: mean has {m.size} elements, sigma has {s.size}")
        w = np.where(np.isinf(s), 0.0, 1.0 / np.square(np.where(np.isinf(s), 1.0, s)))
        if not np.isfinite(np.where(np.broadcast_to(w, np.broadcast(m, w).shape) > 0, m, 0.0)).all():
            raise ValueError("GaussianPrior: the mean of a parameter with a finite sigma must be "
                             "finite")
        self._mean, self._w = m, w
        # what local() sends to a device, formed once: fp32, the mean 0 where the parameter
        # is flat (so no 0 * inf meets a kernel), a vector only where one was given
        flat = np.broadcast_to(w, np.broadcast(m, w).shape) <= 0
        self._mean32 = torch.as_tensor(np.where(flat, 0.0, m) if flat.any() else m,
                                       dtype=torch.float32).reshape(-1)
        self._w32 = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        #: length of the vector arguments (None: both scalars, any parameter count)
        self.size: Optional[int] = next((a.size for a in (m, w) if a.ndim == 1), None)

    # ------------------------------------------------------------------ host side, float64
    def check(self, P: int) -> None:
        """``ValueError`` unless the prior fits ``P`` parameters."""
        if self.size is not None and self.size != int(P):
            raise ValueError(f"GaussianPrior has {self.size} elements, the model has {int(P)} "
                             "parameters")

    @property
    def inv_var(self) -> np.ndarray:
        """``1 / sigma^2`` (0 where flat), float64, a scalar array or ``[P]``."""
        return self._w

    @property
    def mean(self) -> np.ndarray:
        return self._mean

    def _terms(self, x):
        """(d, w) in float64 on x's device, d = 0 where the parameter is flat."""
        if isinstance(x, torch.Tensor):
            xd = x.detach().double().reshape(-1)
            w = torch.as_tensor(self._w, device=xd.device)
            m = torch.as_tensor(self._mean, device=xd.device)
            self.check(xd.numel())
            return torch.where(w > 0, xd - m, torch.zeros_like(xd)), w
        xd = np.asarray(x, dtype=np.float64).reshape(-1)
        self.check(xd.size)
        return np.where(self._w > 0, xd - self._mean, 0.0), self._w

    def penalty(self, x) -> float:
        """``1/2 sum ((x - mean) / sigma)^2`` in float64 (``x``: tensor or array, user order)."""
        d, w = self._terms(x)
        return float((w * d * d).sum()) * 0.5

    def grad(self, x):
        """The penalty's gradient ``(x - mean) / sigma^2`` in float64, a tensor on ``x``'s
        device for a tensor, else an array."""
        d, w = self._terms(x)
        return w * d

    # ------------------------------------------------------------------ device side, float32
    def local(self, layout, device):
        """fp32 ``(mean, inv_var)`` in the vector order of an objective with this
        ``vector_layout()`` (``layout.to_local``).  The inverse variance is 0 on the padding of
        an engine vector, and the mean is 0 wherever the inverse variance is.  Each stays one
        element when it was given as a scalar and the layout has no padding."""
        P = int(layout.P)
        self.check(P)
        padded = not (bool(getattr(layout, "identity", False))
                      or int(getattr(layout, "P_pad", -1)) == P)
        out = []
        for a in (self._mean32, self._w32):
            t = a.to(device)
            if t.numel() != 1 or padded:
                t = layout.to_local(t.expand(P)).contiguous()
            out.append(t)
        return out[0], out[1]


def check_prior(prior, P: int) -> None:
    """The front ends' first look at ``prior=``: its type and its length, before any
    collective."""
    if prior is None:
        return
    if not isinstance(prior, GaussianPrior):
        raise TypeError("prior must be a GaussianPrior (or None)")
    prior.check(P)


def with_penalty(res, prior):
    """``res`` with ``prior_penalty``, the unweighted float64 penalty at ``res.x`` (``None``
    prior: ``res`` as it is)."""
    if prior is not None:
        res["prior_penalty"] = prior.penalty(res.x)
    return res


def penalised_function(fn: Callable, prior: GaussianPrior, weight: float = 1.0) -> Callable:
    """``fn(x, **kw) -> (loss, grad)`` with ``weight * penalty(x)`` added to the loss and its
    gradient to the gradient -- the prior in the parameters themselves, for a function that an
    optimizer or the sampler calls through a transform, and for scipy.  fp32 vectors go
    through ``gaussian_prior_grad_``; any other dtype is computed in that dtype."""
    weight = float(weight)
    cache = {}

    def local(device):
        if device not in cache:
            size = prior.size if prior.size is not None else 1
            from .invhess import IdentityLayout
            cache[device] = prior.local(IdentityLayout(size), device) + (
                torch.zeros(1, dtype=torch.float64, device=device), prior_workspace(device))
        return cache[device]

    def wrapped(x, **kw):
        loss, grad = fn(x, **kw)
        aux = None
        if isinstance(loss, (tuple, list)):
            loss, aux = loss[0], loss[1:]
        xt = torch.as_tensor(x).detach()
        g = torch.as_tensor(grad).detach()
        prior.check(xt.numel())
        if xt.dtype == torch.float32 and g.dtype == torch.float32 and g.device == xt.device:
            mean, inv_var, pen, ws = local(xt.device)
            xf, gf = xt.reshape(-1).contiguous(), g.reshape(-1).contiguous()
            out = gaussian_prior_grad_(xf, gf, mean, inv_var, weight, torch.empty_like(gf), pen, ws)
            pen = pen.clone().reshape(())
        else:
            w = torch.as_tensor(prior.inv_var, device=xt.device)
            m = torch.as_tensor(np.where(np.broadcast_to(prior.inv_var, np.broadcast(
                prior.mean, prior.inv_var).shape) > 0, prior.mean, 0.0), device=xt.device)
            d = xt.double().reshape(-1) - m
            pen = 0.5 * (w * d * d).sum()
            out = (g.double().reshape(-1) + weight * w * d).to(g.dtype)
        lt = torch.as_tensor(loss).detach()
        total = lt.double() + weight * pen.to(lt.device)
        total = total if aux is None else (total,) + tuple(aux)
        return total, out.reshape(g.shape)

    return wrapped


class PriorObjective:
    """``obj`` with ``weight * penalty(x)`` added: the objective protocol of the device
    L-BFGS(-B) drivers and the sampler (``comm``, ``sharded``, ``device``, ``n_local``,
    ``x0``, ``__call__``, ``device_call`` when ``obj`` has one, ``full``, ``vector_layout``,
    and ``check``, ``local_box``, ``finalize`` where ``obj`` has them).

    The prior's gradient is added by ``gaussian_prior_grad_`` into a buffer of this object
    (never into ``obj``'s own gradient view: the engine reuses that buffer), in the pass that
    also sums the penalty.  On a sharded objective that penalty is this rank's partial sum.
    :meth:`partial_call` hands it to the driver, whose
    :class:`~multigrad_amd.optim._quasi_newton.TrialPoints` puts it among the ``sums`` of the
    one reduction it makes for that evaluation anyway: no extra collective and no extra
    device->host copy.  ``__call__`` and ``device_call`` return the complete value; on several
    ranks of a sharded objective they pay an all-reduce of their own for it.

    ``obj`` must work in the parameters themselves: with a transform (``obj.bounds``) the
    prior belongs inside the wrapped function (:func:`penalised_function`)."""

    bounds = None

    def __init__(self, obj, prior: GaussianPrior, weight: float = 1.0):
        if getattr(obj, "bounds", None) is not None:
            raise ValueError("PriorObjective: the objective works in transformed coordinates; "
                             "put the prior inside its function (penalised_function)")
        self.inner, self.prior, self.weight = obj, prior, float(weight)
        self.comm, self.sharded = obj.comm, obj.sharded
        self.device, self.n_local = obj.device, obj.n_local
        self.mean, self.inv_var = prior.local(obj.vector_layout(), self.device)
        self._g = torch.empty(self.n_local, dtype=torch.float32, device=self.device)
        self._pen = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._ws = prior_workspace(self.device)
        self._multi = bool(self.sharded) and self.comm is not None and self.comm.size > 1

    def __getattr__(self, name):
        # the optional members, present exactly where the inner objective has them (looked up
        # on demand: a bound method kept on the instance would be a reference cycle)
        if name in ("check", "local_box", "finalize", "device_call"):
            member = getattr(self.__dict__["inner"], name, None)
            if member is not None:
                return self._device_call if name == "device_call" else member
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def x0(self) -> torch.Tensor:
        return self.inner.x0()

    def full(self, x: torch.Tensor) -> torch.Tensor:
        return self.inner.full(x)

    def vector_layout(self):
        return self.inner.vector_layout()

    def partial_call(self, x: torch.Tensor, device: bool = False):
        """``(loss, grad, partial)``: the inner objective's (global) loss -- a float, or with
        ``device`` its 1-element device tensor -- the gradient of loss plus weighted penalty
        (a buffer the next evaluation reuses) and this rank's weighted partial penalty, a
        1-element fp64 device tensor whose sum over the ranks of a sharded objective (the
        value itself otherwise) completes the loss."""
        f, g = (self.inner.device_call if device else self.inner)(x)
        gaussian_prior_grad_(x, g, self.mean, self.inv_var, self.weight, self._g, self._pen,
                             self._ws)
        return f, self._g, self._pen * self.weight

    def __call__(self, x: torch.Tensor):
        f, g, part = self.partial_call(x)
        if self._multi:
            part = part.cpu()
            self.comm.all_reduce(part)
        return f + float(part), g

    def _device_call(self, x: torch.Tensor):
        lt, g, part = self.partial_call(x, device=True)
        if self._multi:
            self.comm.all_reduce(part)
        return lt.reshape(-1)[:1].double() + part, g
