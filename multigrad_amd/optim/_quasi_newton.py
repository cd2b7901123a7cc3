"""What the device L-BFGS (:mod:`.lbfgs`), L-BFGS-B (:mod:`.lbfgsb`) and, for the frame, the
HMC sampler (:mod:`.hmc`) share:

* :class:`PairRing` -- the ring of (s, y) history pairs on the device with their inner
  products on the host, the one acceptance rule and the upload of combination coefficients;
* :func:`strong_wolfe` -- the bracketing / zoom line search (Nocedal & Wright Alg. 3.5/3.6,
  cubic interpolation) and :func:`best_decrease`, its fallback;
* :class:`TrialPoints` -- the evaluation of ``x + alpha d`` with one reduction and one
  device->host copy per point;
* the driver frame: :func:`driver` (fail-fast guard, single-threaded BLAS),
  :class:`HostCollectives`, :func:`finish` and :class:`Run` (status, hooks, the result).
"""
from __future__ import annotations

import contextlib
import functools
import math

import numpy as np
import scipy.optimize
import torch

from ..ops.lbfgs import lincomb_

__all__ = ["PairRing", "strong_wolfe", "best_decrease", "TrialPoints", "driver",
           "HostCollectives", "finish", "Run"]

_EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------- the pair ring
class PairRing:
    """m accepted (s, y) pairs in a ring of R = m + 1 device slots, with their inner products.

    Rows 0..R-1 of ``HX`` hold s, rows R..2R-1 hold y (``HS`` is that block), and
    ``extra_rows`` more rows follow for the driver's own vectors, so that one multi-dot over
    ``HX`` covers them too.  A new pair is written straight into the spare slot -- the one no
    accepted pair uses, so the dot block never reads a row that is being overwritten, and
    accepting the pair is no copy -- and measured there before :meth:`accept` decides.
    ``SY[i, j] = s_i . y_j``, ``SS`` and ``YY`` are global inner products by slot."""

    def __init__(self, m: int, n: int, device, extra_rows: int = 0):
        self.m = int(m)
        self.R = self.m + 1
        self.HX = torch.zeros((2 * self.R + extra_rows, n), dtype=torch.float32, device=device)
        self.HS = self.HX[:2 * self.R]
        self.SY = np.zeros((self.R, self.R))
        self.SS = np.zeros((self.R, self.R))
        self.YY = np.zeros((self.R, self.R))
        self.order: list = []   # accepted slots, oldest first (at most m)
        self.gamma = self.theta = 1.0  # s.y / y.y of the newest accepted pair, and y.y / s.y
        self._coef = torch.zeros(2 * self.R, dtype=torch.float32, device=device)

    def spare(self) -> int:
        return min(set(range(self.R)) - set(self.order))

    def s(self, q: int) -> torch.Tensor:
        return self.HS[q]

    def y(self, q: int) -> torch.Tensor:
        return self.HS[self.R + q]

    def accept(self, q: int, dots: np.ndarray) -> bool:
        """``dots[r, :2] = (HS_r . s_q, HS_r . y_q)`` for every ring row r; decide and record."""
        R = self.R
        sy, yy = float(dots[q, 1]), float(dots[R + q, 1])
        if not (sy > _EPS * yy and yy > 0):
            return False
        # The oldest pair leaves before the Gram rows are written.  Leaving after would only
        # write entries of the evicted slot as well, and those are never read again: only the
        # order x order blocks are read, and a slot that comes back is rewritten against
        # every pair of `order` here.
        if len(self.order) == self.m:
            self.order.pop(0)
        self.order.append(q)
        for o in self.order:
            self.SY[q, o] = dots[R + o, 0]     # s_new . y_o
            self.SY[o, q] = dots[o, 1]         # s_o . y_new (o = q: the s.y tested above)
            self.SS[o, q] = self.SS[q, o] = dots[o, 0]
            self.YY[o, q] = self.YY[q, o] = dots[R + o, 1]
        self.gamma, self.theta = sy / yy, yy / sy
        return True

    def lincomb(self, cvec: np.ndarray, alpha: float, v, out: torch.Tensor) -> torch.Tensor:
        """``out = alpha v + sum_r cvec[r] HS_r`` in one fused pass; the 2R coefficients go
        up through one persistent device buffer (no allocation per call)."""
        self._coef.copy_(torch.from_numpy(cvec.astype(np.float32)))
        return lincomb_(self.HS, 2 * self.R, self._coef, alpha, v, out)


# ---------------------------------------------------------------------------- the line search
def _cubic_min(a, fa, da, b, fb, db):
    """Minimiser of the cubic interpolating (a, fa, da), (b, fb, db) (None if degenerate)."""
    d1 = da + db - 3 * (fa - fb) / (a - b)
    disc = d1 * d1 - da * db
    if disc < 0 or not np.isfinite(disc):
        return None
    d2 = math.copysign(math.sqrt(disc), b - a)
    den = db - da + 2 * d2
    if den == 0:
        return None
    return b - (b - a) * (db + d2 - d1) / den


def _zoom(phi, lo, hi, flo, fhi, dlo, dhi, f0, d0, c1, c2, maxiter):
    for _ in range(maxiter):
        a = _cubic_min(lo, flo, dlo, hi, fhi, dhi)
        span = hi - lo
        lo_b, hi_b = min(lo, hi) + 0.1 * abs(span), max(lo, hi) - 0.1 * abs(span)
        if a is None or not (lo_b <= a <= hi_b):
            a = 0.5 * (lo + hi)
        fa, da = phi(a)
        if not np.isfinite(fa) or fa > f0 + c1 * a * d0 or fa >= flo:
            hi, fhi, dhi = a, fa, da
        else:
            if abs(da) <= -c2 * d0:
                return a
            if da * (hi - lo) >= 0:
                hi, fhi, dhi = lo, flo, dlo
            lo, flo, dlo = a, fa, da
        if abs(hi - lo) < 1e-12 * max(1.0, abs(lo)):
            break
    return lo if lo != 0.0 else None


def strong_wolfe(phi, f0, d0, a1, c1, c2, maxls, amax=math.inf):
    """Strong-Wolfe step on ``(0, amax]`` by bracketing from ``a1`` (doubling) and zoom, or
    None.  ``phi(alpha) -> (value, slope)``; ``d0`` is the slope at 0: a float, or a
    zero-argument callable read after the first evaluation (a slope that travels with that
    evaluation's reduction) -- then a slope that is not negative returns None at once."""
    alpha = a1
    fa, da = phi(alpha)
    if callable(d0):
        d0 = d0()
        if d0 >= 0:
            return None
    a_prev, f_prev, dphi_prev = 0.0, f0, d0
    for i in range(maxls):
        if i > 0:
            fa, da = phi(alpha)
        if not np.isfinite(fa) or fa > f0 + c1 * alpha * d0 or (i > 0 and fa >= f_prev):
            return _zoom(phi, a_prev, alpha, f_prev, fa, dphi_prev, da, f0, d0, c1, c2, maxls)
        if abs(da) <= -c2 * d0:
            return alpha
        if da >= 0:
            return _zoom(phi, alpha, a_prev, fa, f_prev, da, dphi_prev, f0, d0, c1, c2, maxls)
        if alpha >= amax:
            return alpha  # the cap, with sufficient decrease and a still negative slope: accept
        a_prev, f_prev, dphi_prev = alpha, fa, da
        alpha = min(amax, alpha * 2.0)
    return None


def best_decrease(best, cache, f0):
    """``best`` if the search returned an evaluated step; else the evaluated step of the
    largest decrease below ``f0``; None when there is none."""
    if best is not None and best in cache:
        return best
    cands = [(v[0], a) for a, v in cache.items() if v[0] < f0]
    return min(cands)[1] if cands else None


class TrialPoints:
    """``phi(alpha)`` along ``x + alpha d`` for :func:`strong_wolfe`, and the count of every
    evaluation of the run.

    One point is one evaluation (``obj.device_call`` on the GPU where the objective has it,
    else the host call), a clone of the gradient (the objective may return a view of a buffer
    the next evaluation reuses) and ONE reduction with one device->host copy: the partial
    sums that ``sums(gradient, first)`` returns -- the first of them is the directional
    derivative; ``first`` says that this is the first point since :meth:`start` -- summed over
    the ranks, together with the (already global) loss of a device call.  ``cache`` maps every
    step tried since :meth:`start` to ``(loss, gradient, slope)``; ``last`` is the reduced
    block of the latest point.

    ``sums`` must not refer to the run or to this object: a reference cycle would keep the
    run's device vectors (the ring among them) alive until the next garbage collection
    instead of freeing them when the driver returns.

    Optional protocol: an objective whose loss has a term that is a per-rank partial sum (the
    penalty of :class:`~multigrad_amd.optim.prior.PriorObjective` on sharded vectors) offers
    ``partial_call(x, device=False) -> (loss, grad, partial)`` with ``partial`` a 1-element
    fp64 device tensor.  It then rides behind the partial sums above in the same reduction and
    copy, and its sum over the ranks completes the loss.  An objective without
    ``partial_call`` takes the path described first."""

    def __init__(self, obj, red, device):
        self.obj, self.red = obj, red
        self.dev_call = getattr(obj, "device_call", None) if device.type == "cuda" else None
        self.partial = getattr(obj, "partial_call", None)
        self.nfev = 0
        self.xt = None
        self.cache: dict = {}

    def initial(self, x: torch.Tensor):
        """``(f, g)`` at the start point."""
        self.nfev += 1
        self.xt = torch.empty_like(x)
        if self.partial is not None:
            f, g, part = self.partial(x)
            g = g.clone()
            return f + float(self.red.reduce(sums=[part])[0]), g
        f, g = self.obj(x)
        return f, g.clone()

    def start(self, x, d, sums) -> None:
        self.x, self.d, self.sums = x, d, sums
        self.cache = {}

    def __call__(self, alpha):
        torch.add(self.x, self.d, alpha=float(alpha), out=self.xt)
        first = not self.cache
        if self.partial is not None:
            dev = self.dev_call is not None
            lt, ga, part = self.partial(self.xt, device=dev)
            ga = ga.clone()
            sums = list(self.sums(ga, first)) + [part]
            if dev:
                h = self.red.reduce(sums=sums, local=[lt.reshape(1)])
                fa, h = float(h[-1]) + float(h[-2]), h[:-2]
            else:
                h = self.red.reduce(sums=sums)
                fa, h = lt + float(h[-1]), h[:-1]
        elif self.dev_call is not None:
            lt, ga = self.dev_call(self.xt)
            ga = ga.clone()
            h = self.red.reduce(sums=self.sums(ga, first), local=[lt.reshape(1)])
            fa = float(h[-1])
        else:
            fa, ga = self.obj(self.xt)
            ga = ga.clone()
            h = self.red.reduce(sums=self.sums(ga, first))
        self.nfev += 1
        self.last = h
        self.cache[alpha] = (fa, ga, float(h[0]))
        return fa, float(h[0])


# ---------------------------------------------------------------------------- the driver frame
def driver(single_thread_blas: bool):
    """Decorator of a driver ``f(obj, ...)``: runs it inside the fail-fast guard of
    ``obj.comm`` and, for the optimizers, with the BLAS pools limited to one thread (the
    host-side compact-form solves are tiny; a spinning BLAS pool would slow the CPU
    evaluations)."""
    def wrap(impl):
        @functools.wraps(impl)
        def run(obj, *args, **kwargs):
            from ..utils.hooks import driver_guard
            from ..utils.tensors import blas_single_thread
            blas = blas_single_thread() if single_thread_blas else contextlib.nullcontext()
            with driver_guard(getattr(obj, "comm", None)), blas:
                return impl(obj, *args, **kwargs)
        return run
    return wrap


class HostCollectives:
    """The host collectives a loop made since construction (``count``), without those of the
    user's callback when it is called through :meth:`callback`."""

    def __init__(self, comm):
        self.comm = comm
        self.start = self._now()

    def _now(self) -> int:
        return getattr(self.comm, "host_collectives", 0) if self.comm is not None else 0

    def callback(self, fn, obj, x) -> None:
        """``fn(obj.full(x))``; neither its collectives nor those of assembling the full
        vector are the loop's."""
        h0 = self._now()
        fn(obj.full(x))
        self.start += self._now() - h0

    @property
    def count(self) -> int:
        return self._now() - self.start


def finish(obj, red, x, where: str):
    """The end of every driver: raise if a reduction of the loop or one of the objective's own
    exchanges (engine: ZeRO two-shot, one-shot) timed out, then return the final vector in the
    user's parameter order."""
    red.check(where)
    if getattr(obj, "check", None) is not None:
        obj.check(where)
    xf = obj.full(x)
    if getattr(obj, "finalize", None) is not None:
        xf = obj.finalize(x)
    return xf


class Run:
    """The state of one optimizer run that crosses its phases: the iterate ``x``, ``f``, ``g``,
    the ring, the trial points, the hooks, where it stands and why it stopped.  The drivers
    add their own fields."""

    def __init__(self, obj, red, ring: PairRing, where: str):
        from ..utils.hooks import StepHooks
        self.obj, self.red, self.ring, self.where = obj, red, ring, where
        self.trial = TrialPoints(obj, red, obj.device)
        self.hooks = StepHooks(obj.comm, what=f"{where} iterate")  # MULTIGRAD_CHECK_EVERY / _METRICS
        self.nit = 0
        self.status, self.message = 1, "STOP: TOTAL NO. of ITERATIONS REACHED LIMIT"

    def stop(self, status: int, message: str) -> None:
        self.status, self.message = status, message

    def converged_gradient(self) -> None:
        self.stop(0, "CONVERGENCE: NORM_OF_PROJECTED_GRADIENT_<=_PGTOL")

    def converged_decrease(self, f_old: float, ftol: float) -> bool:
        """scipy's test ``(f_k - f_{k+1}) / max(|f_k|, |f_{k+1}|, 1) <= ftol``."""
        if (f_old - self.f) <= ftol * max(abs(f_old), abs(self.f), 1.0):
            self.stop(0, "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH")
            return True
        return False

    def no_step(self) -> None:
        self.stop(2, "ABNORMAL_TERMINATION_IN_LNSRCH")

    def result(self, host_calls: int, hess_inv: bool, dot) -> scipy.optimize.OptimizeResult:
        xf = finish(self.obj, self.red, self.x, self.where)
        nfev = self.trial.nfev
        res = scipy.optimize.OptimizeResult(
            x=xf, fun=self.f, jac=self.g, nit=self.nit, nfev=nfev, njev=nfev,
            status=self.status, success=self.status == 0, message=self.message,
            host_collectives=host_calls, reduction=self.red.describe())
        if hess_inv:
            from .invhess import build_hess_inv
            res["hess_inv"] = build_hess_inv(self.obj, self.ring, self.red, self.x, dot=dot)
        return res
