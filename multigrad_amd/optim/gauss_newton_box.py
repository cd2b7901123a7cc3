"""Box-constrained damped Gauss-Newton: parameter bounds and a per-parameter step cap through
the ``K x K`` dual of :mod:`multigrad_amd.optim.gauss_newton`.

The scaled step of the dual driver, ``delta_p ~ 1 / J_p``, carries parameters the sumstats
barely depend on far outside the data; a bound ``l <= x <= u`` and a cap ``|delta| <= Delta``
(a trust region in parameter units) are both a box on the step,

    lo = max(l - x, -Delta) <= 0 <= hi = min(u - x, Delta),

and the box-constrained damped problem (``g = J^T c``, ``H+ = L L^T``, ``d`` and ``lambda`` as
in ``_DualFactors``)

    min_delta  g^T delta + 1/2 delta^T J^T H+ J delta + 1/2 lambda delta^T diag(d) delta
    subject to lo <= delta <= hi

has an exact dual of the size of ``L``'s columns.  With ``s = L^T J delta`` and a multiplier
``z`` in ``R^r`` the inner minimisation separates per parameter:

    a = c + L z,   t = J^T a,   sigma_p = -t_p / (lambda d_p),   delta_p(z) = clip(sigma_p, lo_p, hi_p),
    q(z) = sum_p (t_p delta_p + 1/2 lambda d_p delta_p^2) - 1/2 z^T z.

``q`` is concave, C1 and piecewise quadratic, with ``grad q = L^T J delta(z) - z`` and the
generalised Hessian ``-(I + L^T W_F L)``, ``W_F = J diag(free_p / (lambda d_p)) J^T``,
``free_p = lo_p < sigma_p < hi_p``.  It is maximised by a semismooth Newton iteration,
``dz = (I + L^T W_F L)^-1 grad q`` with Armijo backtracking on ``q`` (a full step that lowers
``|grad q|`` and keeps ``q`` to ``1e-10`` relative is accepted too: close to the solution its
gain in ``q`` is below the rounding of the sum), from the unconstrained solution of the dual driver.  With no active side and
float64 parameters the first pass already has ``grad q = 0`` and ``delta`` is
:func:`~multigrad_amd.optim.gauss_newton.dual_step`; with float32 parameters ``W1`` was built
from the float32-rounded ``1 / d``, the start is off by about ``6e-8`` relative, and one
Newton step (a second pass) removes that.  Every ``delta(z)``
lies inside the box, converged or not.  One iteration is one pass over ``J``
(:func:`multigrad_amd.ops.box_dual.box_dual_pass`: ``J delta``, ``W_F``, the sum in ``q`` and
the number of free parameters, one float64 block of ``K + K*K + 2`` values copied to the
host) and ``r x r`` host algebra.  It stops on ``|grad q| <= 1e-9 (|L^T J delta| + |z|)``.

When a parameter leaves its bound the curvature of ``q`` jumps by about ``1 / lambda``, and
at small ``lambda`` Newton frees roughly one parameter per iteration.  The driver therefore
does not fight for convergence: a solve that needs more than ``inner_passes`` passes counts
as a rejected trial, costs no loss evaluation, raises ``lambda`` tenfold and makes that the
floor below which ``lambda`` does not fall again in this run; ``min_damping`` is the general
floor (``1e-12`` in the unconstrained drivers).

Every pass writes ``delta``: which pass proves convergence is not known when it is launched,
and repeating it for the write would cost ``(K + 3) * 4 P`` bytes against ``4 P`` per pass.
"""
from __future__ import annotations

from typing import Callable

import numpy as np
import scipy.linalg
import scipy.optimize
import torch

from ..ops.box_dual import box_dual_pass
from ._damped import damped_loop
from .gauss_newton import GaussNewtonInvProduct, _DualFactors, _factors, _scalar
from .transforms import Bounds

__all__ = ["run_gauss_newton_box", "box_step", "BoxSolve"]

_INNER_RTOL = 1e-9
_ARMIJO = 1e-4
_MIN_ALPHA = 1e-8
_Q_NOISE = 1e-10   # of |sum| + |z|^2 / 2: far above the rounding of q, far below a real loss


def _spd_solve(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    try:
        return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A), b)
    except (np.linalg.LinAlgError, ValueError):
        return np.linalg.lstsq(A, b, rcond=None)[0]


class BoxSolve:
    """The outcome of one inner solve: ``converged``, the number of ``passes`` it took, the
    multiplier ``z`` and the last pass's ``free`` count and dual gradient norm ``residual``
    (relative to ``|L^T J delta| + |z|``).  ``delta`` itself is in the buffer the caller
    gave."""

    def __init__(self, converged, passes, z, free, residual):
        self.converged, self.passes, self.z = converged, passes, z
        self.free, self.residual = free, residual


def _scaling(fac: _DualFactors) -> torch.Tensor:
    """``d`` from the ``1 / d`` that ``_DualFactors`` keeps (``d > 0`` whenever it is used)."""
    return 1.0 / fac.inv_d


def _solve_box(fac: _DualFactors, d, lo, hi, lam: float, delta: torch.Tensor,
               max_passes: int, copies: list) -> BoxSolve:
    """Maximise ``q`` (module docstring) for one ``lambda``; ``delta`` ``[P]`` receives
    ``delta(z)`` of the last pass."""
    J, L, c, K = fac.J, fac.L, fac.c, fac.K
    r = L.shape[1]
    eye = np.eye(r)
    npass = 0

    def evaluate(z):
        nonlocal npass
        a = torch.as_tensor(np.ascontiguousarray(c + L @ z), dtype=torch.float64).to(J.device)
        blk = box_dual_pass(J, a, d, lam, lo, hi, delta).cpu().numpy()
        copies.append(blk.size)
        npass += 1
        v, W = blk[:K], blk[K:K + K * K].reshape(K, K)
        ltv = L.T @ v
        grad = ltv - z
        scale = float(np.linalg.norm(ltv) + np.linalg.norm(z))
        return dict(z=z, q=float(blk[-2] - 0.5 * z @ z), grad=grad, W=W, free=int(blk[-1]),
                    gnorm=float(np.linalg.norm(grad)), scale=scale,
                    qscale=float(abs(blk[-2]) + 0.5 * z @ z),
                    finite=bool(np.isfinite(blk).all()))

    def done(cur, ok):
        rel = cur["gnorm"] / cur["scale"] if cur["scale"] > 0.0 else cur["gnorm"]
        return BoxSolve(ok, npass, cur["z"], cur["free"], rel)

    z = np.zeros(r)
    if r:   # the unconstrained solution: L z0 = -y of _DualFactors.coefficients
        LtW = L.T @ (fac.W1 / lam)
        z = -_spd_solve(eye + LtW @ L, LtW @ c)
    cur = evaluate(z)
    while True:
        if not cur["finite"]:
            return done(cur, False)
        if cur["gnorm"] <= _INNER_RTOL * cur["scale"]:
            return done(cur, True)
        if npass >= max_passes:
            return done(cur, False)
        dz = _spd_solve(eye + L.T @ cur["W"] @ L, cur["grad"])
        slope = float(cur["grad"] @ dz)
        alpha = 1.0
        while True:
            new = evaluate(cur["z"] + alpha * dz)
            if new["finite"] and new["q"] >= cur["q"] + _ARMIJO * alpha * slope:
                break
            # near the solution the gain of a Newton step (about |grad q|^2) is below the
            # rounding of q, a sum over P terms: a full step that lowers |grad q|, the
            # merit function of a semismooth Newton iteration, and leaves q where it was to
            # that rounding is taken as well
            if (new["finite"] and alpha == 1.0 and new["gnorm"] < cur["gnorm"]
                    and new["q"] >= cur["q"] - _Q_NOISE * cur["qscale"]):
                break
            if alpha < _MIN_ALPHA or npass >= max_passes:
                return done(new, False)
            alpha *= 0.5
        cur = new


def box_step(J, c, H, lam: float, lo, hi, inner_passes: int = 40):
    """One box-constrained damped Gauss-Newton step: ``(delta, info)`` with ``delta`` ``[P]``
    on ``J``'s device the minimiser of the problem in the module docstring for the step box
    ``lo <= 0 <= hi`` (tensors ``[P]``, ``+-inf`` allowed) and ``info`` a :class:`BoxSolve`.
    ``delta`` lies inside the box whether or not the solve converged."""
    fac = _DualFactors(torch.as_tensor(J), c, H, [])
    J = fac.J
    lo = torch.as_tensor(lo).to(device=J.device, dtype=J.dtype).contiguous()
    hi = torch.as_tensor(hi).to(device=J.device, dtype=J.dtype).contiguous()
    delta = torch.zeros(fac.P, dtype=J.dtype, device=J.device)
    if not fac.P or not fac.dmax > 0.0:
        return delta, BoxSolve(True, 0, np.zeros(fac.L.shape[1]), 0, 0.0)
    return delta, _solve_box(fac, _scaling(fac), lo, hi, float(lam), delta, int(inner_passes), [])


def _box_tensor(value, like: torch.Tensor, name: str):
    """A scalar or ``[ndim]`` ``max_step`` as a tensor broadcastable against ``like``."""
    t = torch.as_tensor(value, dtype=like.dtype).to(like.device).reshape(-1)
    if t.numel() not in (1, like.numel()):
        raise ValueError(f"{name} must be a scalar or have {like.numel()} entries, got {t.numel()}")
    if bool((t <= 0).any()) or bool(torch.isnan(t).any()):
        raise ValueError(f"{name} must be positive")
    return t


def run_gauss_newton_box(factors_fn: Callable, loss_fn: Callable, params, param_bounds=None,
                         max_step=None, maxsteps: int = 50, damping: float = 1e-3,
                         min_damping: float = 1e-4, ftol: float = 2.2e-9, gtol: float = 1e-8,
                         inner_passes: int = 40, comm=None):
    """:func:`~multigrad_amd.optim.gauss_newton.run_gauss_newton_dual` with parameter bounds
    and a cap on the step per parameter (module docstring): the same iteration, acceptance
    rule, damping schedule and messages, with every trial step the minimiser of the damped
    model inside the box and every trial point inside the bounds.

    Parameters
    ----------
    factors_fn, loss_fn, params, maxsteps, damping, ftol, comm : as in
        :func:`~multigrad_amd.optim.gauss_newton.run_gauss_newton_dual`
    param_bounds : ``None`` or a reference-style ``(ndim, 2)`` spec (``None`` or a non-finite
        value for an open side); the start point is clamped into the bounds
    max_step : ``None`` (no cap), a scalar or ``[ndim]`` positive values in parameter units:
        no trial step changes a parameter by more
    min_damping : the floor of ``lambda``
    gtol : stop when L-BFGS-B's projected gradient ``max |clip(x - g, l, u) - x| <= gtol``
    inner_passes : passes over ``J`` allowed per trial step; a solve that needs more is a
        rejected trial without a loss evaluation

    Returns
    -------
    scipy.optimize.OptimizeResult with the dual driver's fields and ``solver="dual-box"``,
    plus ``inner_passes`` (passes over ``J`` in all inner solves), ``inner_unconverged``
    (trials rejected because their solve did not converge), ``active`` (int8 ``[ndim]`` on
    the parameters' device: -1 on the lower bound, +1 on the upper, 0 free; a parameter on a
    bound counts as active when the gradient pushes it outward), ``hess_inv`` (a
    :class:`~multigrad_amd.optim.gauss_newton.GaussNewtonInvProduct` over ``J`` with the
    active columns zeroed), ``damping`` and ``damping_floor`` (the final ``lambda`` and its
    floor) and ``trials`` (one ``(lambda, passes, converged, accepted)`` per trial step).
    ``host_copy_sizes`` lists the packed block per Jacobian, one scalar per projected
    gradient and one ``K + K*K + 2`` block per inner pass.
    """
    x_t = torch.as_tensor(params).detach()
    shape = x_t.shape
    x = x_t.reshape(-1).clone()
    P, dev, dt = x.numel(), x.device, x.dtype
    bounds = Bounds.from_spec(param_bounds, P, device=dev, dtype=dt)
    if bounds is None:
        l = torch.full((P,), -float("inf"), dtype=dt, device=dev)
        u = torch.full((P,), float("inf"), dtype=dt, device=dev)
    else:
        l, u = bounds.lo.contiguous(), bounds.hi.contiguous()
        if bool((l > u).any()):
            raise ValueError("param_bounds has a lower bound above its upper bound")
    cap = None if max_step is None else _box_tensor(max_step, x, "max_step")
    x = torch.clamp(x, min=l, max=u)
    copies: list = []
    trials: list = []

    def projected_gradient(g, x):
        if not P:
            return 0.0
        copies.append(1)
        # clip(x - g, l, u) - x, formed as clip(-g, l - x, u - x): in float32 a gradient entry
        # below half a unit in the last place of x would otherwise vanish in x - g
        return float(torch.clamp(-g, min=l - x, max=u - x).abs().max())

    delta = torch.zeros(P, dtype=dt, device=dev)

    def trials_from(state, x):
        fac = state[0]
        lo = l - x if cap is None else torch.maximum(l - x, -cap)
        hi = u - x if cap is None else torch.minimum(u - x, cap)
        lo, hi = lo.clamp_(max=0.0), hi.clamp_(min=0.0)
        d = _scaling(fac) if fac.dmax > 0.0 else None

        def propose(lam):
            if d is None:   # J^T H+ J = 0: no step, as in the dual driver
                delta.zero_()
                trials.append((lam, 0, True, False))
            else:
                sol = _solve_box(fac, d, lo, hi, lam, delta, int(inner_passes), copies)
                trials.append((lam, sol.passes, sol.converged, False))
                if not sol.converged:
                    return None
            trial = torch.clamp(x + delta, min=l, max=u)
            # a step that the bound itself limits ends on the bound, not an ulp inside
            return torch.where(delta <= l - x, l, torch.where(delta >= u - x, u, trial))
        return propose

    def accept():
        trials[-1] = trials[-1][:3] + (True,)

    run = damped_loop(
        x, lambda xv: _factors(factors_fn, xv, shape, copies),
        finite=lambda state: state[0].finite,
        converged=lambda state, xv: not P or projected_gradient(state[0].g, xv) <= gtol,
        measure="max |projected grad|", trials=trials_from,
        loss_at=lambda trial: _scalar(loss_fn(trial.reshape(shape))),
        maxsteps=maxsteps, damping=max(float(damping), float(min_damping)), floor=min_damping,
        ftol=ftol, comm=comm, on_accept=accept)
    (fac, jac_mode), x = run.state, run.x
    g = fac.g
    fixed = l == u
    lower = (x <= l) & ((g > 0) | fixed)
    upper = (x >= u) & ((g < 0) | fixed) & ~lower
    active = upper.to(torch.int8) - lower.to(torch.int8)
    Jm = fac.J      # masked in place: fac is dropped here, and no second K x P array is made
    if P and bool(active.any()):
        Jm.mul_((active == 0).to(Jm.dtype))
    return scipy.optimize.OptimizeResult(
        x=x.reshape(shape), fun=run.loss, jac=g.reshape(shape), nit=run.nit, nfev=run.nfev,
        njev=run.njev, success=run.success, message=run.message, jac_mode=jac_mode,
        solver="dual-box", hess_inv=GaussNewtonInvProduct(Jm, fac.L), host_copy_sizes=copies,
        inner_passes=sum(t[1] for t in trials), inner_unconverged=sum(not t[2] for t in trials),
        active=active.reshape(shape), damping=run.damping, damping_floor=run.floor, trials=trials)
