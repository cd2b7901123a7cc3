"""The outer loop the three Gauss-Newton drivers share (Levenberg-Marquardt damping).

A driver supplies how a point is evaluated into a state, whether a state is finite and
converged, and how a trial point is proposed for a ``lambda``; the iteration, the ``lambda``
schedule, the acceptance and stopping rules, the counters and the messages are here once.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable

from ..utils.hooks import driver_guard
from ..utils.progress import trange

LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12
NOT_FINITE = "the Jacobian or the loss derivatives are not finite at the current point"


def damped_loop(x, evaluate: Callable, finite: Callable, converged: Callable, measure: str,
                trials: Callable, loss_at: Callable, *, maxsteps: int, damping: float,
                floor: float, ftol: float, comm=None, on_accept: Callable = lambda: None):
    """Run the damped iteration from ``x``.

    evaluate : ``x -> (loss, state)``: one Jacobian.  The previous state is dropped before the
        call, so a state that holds the Jacobian keeps at most one alive.
    finite : ``state -> bool``; a state that is not ends the run without success
    converged : ``(state, x) -> bool``, the gtol test; ``measure`` names it in the message
    trials : ``(state, x) -> propose`` once per iteration, with ``propose(lam)`` the trial
        point for that ``lambda``, or ``None`` for "no trial": that costs no loss evaluation,
        raises ``lambda`` tenfold and makes it the floor for the rest of the run
    loss_at : ``trial -> float``
    on_accept : called when the last proposed trial is accepted

    Returns a namespace of ``x``, ``loss``, ``state`` (of the final ``x``), ``nit``, ``nfev``,
    ``njev``, ``success``, ``message`` and the final ``damping`` and ``floor``.
    """
    lam, floor = float(damping), float(floor)
    nit = nfev = njev = 0
    success, message = False, "maximum number of iterations reached"
    with driver_guard(comm):
        bar = trange(maxsteps, desc="Gauss-Newton Progress")
        steps = iter(bar)
        while True:
            state = None
            loss, state = evaluate(x)
            njev += 1
            if not finite(state):
                message = NOT_FINITE
                break
            if converged(state, x):
                success, message = True, f"converged: {measure} <= gtol"
                break
            if next(steps, None) is None:
                break
            propose = trials(state, x)
            accepted = trial = None
            while lam <= LAMBDA_MAX:
                trial = propose(lam)
                if trial is None:
                    lam *= 10.0
                    floor = max(floor, lam)
                    continue
                new = loss_at(trial)
                nfev += 1
                if math.isfinite(new) and new < loss:
                    accepted = new
                    on_accept()
                    break
                lam *= 10.0
            propose = None
            if accepted is None:
                message = "no step reduced the loss (damping above 1e12)"
                break
            x = trial
            lam = max(lam / 10.0, floor)
            nit += 1
            if (loss - accepted) / max(abs(loss), abs(accepted), 1.0) <= ftol:
                # the state returned belongs to the accepted point
                state = None
                loss, state = evaluate(x)
                njev += 1
                success, message = True, "converged: relative loss decrease <= ftol"
                if not finite(state):
                    success, message = False, NOT_FINITE
                break
        if hasattr(bar, "close"):
            bar.close()
    return SimpleNamespace(x=x, loss=loss, state=state, nit=nit, nfev=nfev, njev=njev,
                           success=success, message=message, damping=lam, floor=floor)
