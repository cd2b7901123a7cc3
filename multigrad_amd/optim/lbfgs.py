"""Device L-BFGS with globally consistent (all-reduced) dot products.

The reference's ``run_bfgs`` (``multigrad/bfgs.py:32-113``) runs scipy's compiled
L-BFGS-B on the root rank and broadcasts every trial point.  For 1e6-1e8 parameters the
optimizer itself must live on the GPUs, so this is an SPMD L-BFGS:

* vectors (x, g, the m (s, y) history pairs) are device tensors -- replicated, or
  **sharded 1/W per rank** when driven by the ZeRO engine (each rank owns a slice of
  every vector, BASELINE config 4);
* the inverse-Hessian product uses the compact representation (Byrd, Nocedal & Schnabel
  1994), so one iteration needs the 2m x 3 inner products [S; Y] . [s_new, y_new, g_new]:
  one fused pass (``csrc/lbfgs.hip: multi_dot``, fp64 deterministic reduction) and ONE
  small all-reduce of 6m doubles -- instead of the two-loop recursion's 2m *sequential*
  reductions;
* the search direction ``d = -(gamma g + S a + gamma Y b)`` is one fused pass
  (``lincomb``);
* the strong-Wolfe line search (Nocedal & Wright Alg. 3.5/3.6, cubic interpolation)
  decides on loss values and directional derivatives that are bitwise identical on all
  ranks (all-reduced), so every rank takes the same decisions without broadcasts.

The history ring, the line search and the frame of the driver are shared with L-BFGS-B
(:mod:`multigrad_amd.optim._quasi_newton`); this module keeps the compact inverse-Hessian
product and the phases of one iteration: direction, search, update.

Termination follows scipy's L-BFGS-B: ``(f_k - f_{k+1}) / max(|f_k|, |f_{k+1}|, 1) <= ftol``
or ``max|g| <= gtol`` or ``maxiter``.  Box bounds are supported through the same
bijective transforms as Adam (:mod:`multigrad_amd.optim.transforms`); the exact scipy
L-BFGS-B projection semantics remain available through :func:`multigrad_amd.optim.bfgs.run_bfgs`.
"""
from __future__ import annotations

import math
from typing import Callable

import numpy as np
import scipy.linalg
import scipy.optimize
import torch

from ..ops.lbfgs import MultiDot
from ._quasi_newton import HostCollectives, PairRing, Run, best_decrease, driver, strong_wolfe
from ._reduce import DeviceReducer

__all__ = ["lbfgs_minimize", "GenericObjective", "run_lbfgs_device"]

_EPS = np.finfo(np.float64).eps


class GenericObjective:
    """Replicated objective around ``loss_and_grad_fn(x_full) -> (loss, grad)`` (the
    gradient is already all-reduced by the model, so every rank holds the same vector)."""

    def __init__(self, loss_and_grad_fn: Callable, x0: torch.Tensor, comm=None, bounds=None,
                 **fn_kwargs):
        self.fn = loss_and_grad_fn
        self.kw = fn_kwargs
        self.comm = comm
        self.sharded = False
        self.bounds = bounds
        x0 = x0.detach().reshape(-1).to(torch.float32)
        self.device = x0.device
        self.shape = x0.shape
        self.u0 = bounds.forward(x0) if bounds is not None else x0.clone()
        self.n_local = self.u0.numel()

    def x0(self) -> torch.Tensor:
        return self.u0.clone()

    def full(self, u: torch.Tensor) -> torch.Tensor:
        return self.bounds.inverse(u) if self.bounds is not None else u

    def vector_layout(self):
        """The optimizer's vector is the user's (transformed) parameter vector."""
        from .invhess import IdentityLayout
        return IdentityLayout(self.n_local)

    def __call__(self, u: torch.Tensor):
        x = self.full(u)
        loss, grad = self.fn(x, **self.kw)
        if isinstance(loss, (tuple, list)):
            loss = loss[0]
        g = torch.as_tensor(grad).detach().reshape(-1).to(device=u.device, dtype=torch.float32)
        if self.bounds is not None:
            g = g * self.bounds.dpdu(u)
        return float(torch.as_tensor(loss).detach().double()), g.contiguous()


def _absmax(gv: torch.Tensor) -> torch.Tensor:
    return gv.abs().max().double() if gv.numel() else torch.zeros((), dtype=torch.float64,
                                                                 device=gv.device)


class _Run(Run):
    """A run of the unbounded driver.  The current gradient lives in the row behind the ring
    (``HX[2R]``): one multi-dot of all rows against (s_new, y_new, g) gives every scalar an
    iteration needs (s.y, y.y, the new Gram rows, S^T g, Y^T g, g.g), and max|g| rides along in
    the same reduction and device->host copy: with the line search's one copy per
    evaluation, a typical iteration makes two."""

    def __init__(self, obj, red, m: int):
        n, dev = obj.n_local, obj.device
        super().__init__(obj, red, PairRing(m, n, dev, extra_rows=1), "L-BFGS")
        R = self.ring.R
        self.g_row = self.ring.HX[2 * R]
        self.dot = MultiDot(2 * R + 1, n, dev)
        self.dot1 = MultiDot(1, n, dev)
        self.Sg = np.zeros(R)
        self.Yg = np.zeros(R)
        self.x = obj.x0().contiguous()
        self.f, self.g = self.trial.initial(self.x)
        self.d = torch.empty_like(self.x)
        # (global g.g, global max|g|) in one copy
        h = red.reduce(sums=[self.dot1(self.g.view(1, -1), 1, [self.g])], maxes=[_absmax(self.g)])
        self.gg, self.gmax = float(h[0]), float(h[1])


def _direction(st: _Run):
    """Write the search direction ``st.d`` (compact inverse-Hessian product); returns
    ``(g.d, first trial step)``.  g.d follows from the host copies of S^T g, Y^T g and g.g (no
    device round trip)."""
    ring = st.ring
    R, order = ring.R, ring.order
    gd = -st.gg
    if order:
        idx = np.array(order)
        gamma, a, b = compact_coefficients(ring.SY, ring.YY, st.Sg, st.Yg, order)
        cvec = np.zeros(2 * R)
        cvec[idx] = -a
        cvec[R + idx] = -gamma * b
        ring.lincomb(cvec, -gamma, st.g, st.d)
        gd = -gamma * st.gg - float(a @ st.Sg[idx]) - gamma * float(b @ st.Yg[idx])
    else:
        st.d.copy_(-st.g)
    if not np.isfinite(gd) or gd >= 0:  # not a descent direction: reset memory
        order.clear()
        st.d.copy_(-st.g)
        gd = -st.gg
    return gd, (1.0 if order else min(1.0, 1.0 / math.sqrt(max(-gd, 1e-300))))


def _search(st: _Run, gd: float, a1: float, c1: float, c2: float, maxls: int):
    """Strong-Wolfe step along ``st.d``, else the best decrease seen, else None.  The local
    d.g of a trial point goes into the one reduction of its evaluation."""
    dot1, d = st.dot1, st.d
    st.trial.start(st.x, d, lambda ga, first: [dot1(ga.view(1, -1), 1, [d])])
    best = strong_wolfe(st.trial, st.f, gd, a1, c1, c2, maxls)
    return best_decrease(best, st.trial.cache, st.f)


def _update(st: _Run, best: float) -> None:
    """Move to the accepted trial point; the new pair goes into the spare slot and is
    measured there (the one dot block of the iteration)."""
    ring = st.ring
    R = ring.R
    f_new, g_new, _ = st.trial.cache[best]
    q = ring.spare()
    s_vec, y_vec = ring.s(q), ring.y(q)
    torch.mul(st.d, best, out=s_vec)
    st.x.add_(s_vec)
    torch.sub(g_new, st.g, out=y_vec)
    st.g_row.copy_(g_new)
    dv = st.dot(ring.HX, 2 * R + 1, [s_vec, y_vec, st.g_row])  # (2R+1, 3)
    host = st.red.reduce(sums=[dv], maxes=[_absmax(g_new)])
    dots = host[:-1].reshape(2 * R + 1, 3)
    st.gmax = float(host[-1])
    st.gg = float(dots[2 * R, 2])
    ring.accept(q, dots)
    st.Sg[:] = dots[:R, 2]
    st.Yg[:] = dots[R:2 * R, 2]
    st.f, st.g = f_new, g_new


@driver(single_thread_blas=True)
def lbfgs_minimize(obj, maxiter: int = 100, m: int = 10, ftol: float = 1e7 * _EPS,
                   gtol: float = 1e-5, maxls: int = 20, c1: float = 1e-4, c2: float = 0.9,
                   callback=None, hess_inv: bool = True) -> scipy.optimize.OptimizeResult:
    """Minimise ``obj`` (see :class:`GenericObjective`) with L-BFGS; SPMD-consistent.

    ``hess_inv=True`` adds ``hess_inv``, a
    :class:`~multigrad_amd.optim.invhess.DeviceLbfgsInvHessProduct` over the accepted pairs, to
    the result.  It keeps the history ring alive (a reference, no copy: ``2 (m + 1)`` fp32
    vectors, 0.9 GB at 1e7 parameters and ``m = 10``); ``hess_inv=False`` frees it on return.

    Every cross-rank reduction of the loop runs on the devices (:class:`DeviceReducer`:
    the wide one-shot peer-memory kernel, else RCCL) and comes back in one device->host copy:
    one per iteration (the dot block with max|g|) and one per line-search evaluation (the
    loss with the directional derivative).  The result records the host collectives the
    iterations made (``host_collectives``; 0 on GPUs)."""
    if hess_inv:
        from .invhess import check_hess_inv_objective
        check_hess_inv_objective(obj)
    if not 1 <= int(m) <= 120:
        # 2 (m + 1) history rows go through one lincomb launch (csrc/lbfgs.hip: <= 256 rows)
        raise ValueError(f"L-BFGS history m must be in 1..120, got {m}")
    red = DeviceReducer(obj.comm, obj.sharded, obj.device)  # collective (may connect peer memory)
    st = _Run(obj, red, m)
    host = HostCollectives(obj.comm)
    if st.gmax <= gtol:
        st.converged_gradient()
    else:
        for k in range(maxiter):
            gd, a1 = _direction(st)
            best = _search(st, gd, a1, c1, c2, maxls)
            if best is None:
                st.no_step()
                break
            f_old = st.f
            _update(st, best)
            st.nit = k + 1
            if callback is not None:
                host.callback(callback, obj, st.x)
            if st.hooks.active:
                st.hooks(k, st.f, None, (lambda: st.x) if not obj.sharded else None)
            if st.gmax <= gtol:
                st.converged_gradient()
                break
            if st.converged_decrease(f_old, ftol):
                break
    return st.result(host.count, hess_inv, st.dot)


def compact_coefficients(SY, YY, Sg, Yg, order):
    """Coefficients of the compact L-BFGS product ``H g = gamma g + S a + gamma Y b``
    (Byrd, Nocedal & Schnabel 1994) from the inner products of the pairs listed in
    ``order`` (oldest first): returns ``(gamma, a, b)``."""
    idx = np.asarray(order)
    sy = SY[np.ix_(idx, idx)]
    yy = YY[np.ix_(idx, idx)]
    last = order[-1]
    gamma = SY[last, last] / YY[last, last]
    R = np.triu(sy)
    D = np.diag(np.diag(sy))
    t = scipy.linalg.solve_triangular(R, Sg[idx], lower=False)
    a = scipy.linalg.solve_triangular(R, (D + gamma * yy) @ t - gamma * Yg[idx], lower=False,
                                      trans="T")
    return gamma, a, -t


def run_lbfgs_device(loss_and_grad_fn: Callable, params, maxsteps: int = 100, param_bounds=None,
                     randkey=None, comm=None, history: int = 10, prior=None,
                     prior_weight: float = 1.0, **kw):
    """Device L-BFGS for a generic ``loss_and_grad_fn(params[, randkey])`` (replicated).

    ``prior`` (a :class:`~multigrad_amd.optim.prior.GaussianPrior`) minimises
    ``loss + prior_weight * prior.penalty(x)`` -- with ``prior_weight = 1 / loss_scale`` the
    MAP of the posterior that ``run_hmc(prior=..., loss_scale=...)`` samples.  The prior is on
    the parameters themselves, also with ``param_bounds``.  ``res.fun`` is the minimised
    objective, ``res.prior_penalty`` the unweighted penalty at ``res.x``, and ``res.hess_inv``
    approximates the inverse Hessian of likelihood plus prior.

    ``hess_inv=True`` (default) returns the inverse-Hessian operator as ``res.hess_inv``
    (it holds the history ring, see :func:`lbfgs_minimize`).  With ``param_bounds`` the
    iteration runs in the transformed variables ``u`` and the operator is ``J H_u J`` with
    ``J = diag(dx/du)`` at the final iterate (:mod:`multigrad_amd.optim.invhess`)."""
    from ..utils.random import init_randkey
    from .transforms import Bounds
    from ..utils.tensors import as_param_tensor
    from .prior import PriorObjective, check_prior, penalised_function, with_penalty
    x0 = as_param_tensor(params)
    check_prior(prior, x0.numel())
    bounds = Bounds.from_spec(param_bounds, x0.numel(), device=x0.device, dtype=torch.float32)
    fkw = {} if randkey is None else {"randkey": init_randkey(randkey)}
    if prior is not None and bounds is not None:
        # the iteration runs in u: the prior goes into the function of x, before the chain rule
        loss_and_grad_fn = penalised_function(loss_and_grad_fn, prior, prior_weight)
    obj = GenericObjective(loss_and_grad_fn, x0, comm=comm, bounds=bounds, **fkw)
    if prior is not None and bounds is None:
        obj = PriorObjective(obj, prior, prior_weight)
    return with_penalty(lbfgs_minimize(obj, maxiter=maxsteps, m=history, **kw), prior)
