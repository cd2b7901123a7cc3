"""Damped Gauss-Newton (Levenberg-Marquardt) driver for one-point models.

Every model here has the shape ``loss(S)`` with ``S = sum_r s_r(theta)`` a short sumstat
vector, so the natural second-order model of the loss is the Gauss-Newton matrix
``G = J^T H J`` built from the sumstat Jacobian ``J`` and the (positive semi-definite part of
the) ``K x K`` Hessian ``H`` of the loss hook
(:meth:`~multigrad_amd.models.onepoint.OnePointModel.calc_gauss_newton_from_params`).  A fit
then needs tens of Jacobians where Adam needs hundreds of gradients.

The driver is SPMD like Adam: every rank receives the same all-reduced ``(loss, grad, G)``
and does the same small float64 host algebra, so the iterates are identical on every rank
without a broadcast.  Per iteration it solves

    (G + lambda diag(d)) delta = -grad,      d = max(diag G, 1e-12 max diag G),

evaluates the loss at ``x + delta``, and accepts the step if the loss is lower and finite
(``lambda <- max(lambda / 10, 1e-12)``); otherwise ``lambda <- 10 lambda`` and the solve is
repeated with the same Jacobian.  It stops as scipy's L-BFGS-B does, on
``(L - L_new) / max(|L|, |L_new|, 1) <= ftol`` or ``max |grad| <= gtol``, after ``maxsteps``
iterations, or without success once ``lambda`` exceeds ``1e12``.
"""
from __future__ import annotations

from typing import Callable

import numpy as np
import scipy.optimize
import torch

from ..utils.hooks import driver_guard
from ..utils.progress import trange

__all__ = ["run_gauss_newton"]

_LAMBDA_MIN, _LAMBDA_MAX = 1e-12, 1e12


def _scalar(loss) -> float:
    if isinstance(loss, (tuple, list)):
        loss = loss[0]
    return float(torch.as_tensor(loss).detach().cpu().double())


def _host(t) -> np.ndarray:
    return torch.as_tensor(t).detach().cpu().double().numpy()


def _solve(G: np.ndarray, lam: float, g: np.ndarray) -> np.ndarray:
    diag = np.diag(G)
    top = float(diag.max()) if diag.size else 0.0
    d = np.maximum(diag, 1e-12 * top)
    A = G + lam * np.diag(d)
    try:
        return np.linalg.solve(A, -g)
    except np.linalg.LinAlgError:
        return np.linalg.lstsq(A, -g, rcond=None)[0]


def run_gauss_newton(gauss_newton_fn: Callable, loss_fn: Callable, params, maxsteps: int = 50,
                     damping: float = 1e-3, ftol: float = 2.2e-9, gtol: float = 1e-8, comm=None):
    """Minimise by damped Gauss-Newton steps.

    Parameters
    ----------
    gauss_newton_fn : ``params -> (loss, grad, G, jac_mode)``, identical on every rank
    loss_fn : ``params -> loss``, identical on every rank
    params : initial guess (a tensor; its shape, dtype and device are kept)
    maxsteps : maximum number of iterations (accepted steps)
    damping : initial ``lambda``
    ftol, gtol : stopping tolerances (module docstring)
    comm : communicator whose ranks all take part (for the fail-fast guard only: the
        driver itself issues no collective)

    Returns
    -------
    scipy.optimize.OptimizeResult, identical on every rank: ``x``, ``fun``, ``jac``, ``nit``,
    ``nfev``, ``njev``, ``success``, ``message``, ``jac_mode`` (``"forward"`` or
    ``"reverse"``, the Jacobian mode actually used) and ``hess_inv``, the float64
    pseudo-inverse of the final Gauss-Newton matrix.
    """
    x_t = torch.as_tensor(params).detach()
    shape, dtype, device = x_t.shape, x_t.dtype, x_t.device
    x = _host(x_t).reshape(-1)

    def tensor(v):
        return torch.as_tensor(v, dtype=dtype, device=device).reshape(shape)

    lam = float(damping)
    nit = nfev = njev = 0
    success, message, jac_mode = False, "maximum number of iterations reached", None
    with driver_guard(comm):
        bar = trange(maxsteps, desc="Gauss-Newton Progress")
        steps = iter(bar)
        loss = g = G = None
        while True:
            out = gauss_newton_fn(tensor(x))
            njev += 1
            jac_mode = out[3]
            loss, g, G = _scalar(out[0]), _host(out[1]).reshape(-1), _host(out[2])
            if not g.size or np.max(np.abs(g)) <= gtol:
                success, message = True, "converged: max |grad| <= gtol"
                break
            if next(steps, None) is None:
                break
            accepted = None
            while lam <= _LAMBDA_MAX:
                trial = x + _solve(G, lam, g)
                new = _scalar(loss_fn(tensor(trial)))
                nfev += 1
                if np.isfinite(new) and new < loss:
                    accepted = new
                    break
                lam *= 10.0
            if accepted is None:
                message = "no step reduced the loss (damping above 1e12)"
                break
            x = trial
            lam = max(lam / 10.0, _LAMBDA_MIN)
            nit += 1
            if (loss - accepted) / max(abs(loss), abs(accepted), 1.0) <= ftol:
                # the state below belongs to the accepted point
                out = gauss_newton_fn(tensor(x))
                njev += 1
                loss, g, G = _scalar(out[0]), _host(out[1]).reshape(-1), _host(out[2])
                success, message = True, "converged: relative loss decrease <= ftol"
                break
        if hasattr(bar, "close"):
            bar.close()
    return scipy.optimize.OptimizeResult(
        x=x.reshape(shape), fun=loss, jac=g.reshape(shape), nit=nit, nfev=nfev, njev=njev,
        success=success, message=message, jac_mode=jac_mode,
        hess_inv=np.linalg.pinv(G) if G.size else G)
