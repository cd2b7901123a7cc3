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

Termination follows scipy's L-BFGS-B: ``(f_k - f_{k+1}) / max(|f_k|, |f_{k+1}|, 1) <= ftol``
or ``max|g| <= gtol`` or ``maxiter``.  Box bounds are supported through the same
bijective transforms as Adam (:mod:`multigrad_amd.optim.transforms`); the exact scipy
L-BFGS-B projection semantics remain available through :func:`multigrad_amd.optim.bfgs.run_bfgs`.
"""
from __future__ import annotations

import math
import os
from typing import Callable

import numpy as np
import scipy.linalg
import scipy.optimize
import torch

from ..ops.lbfgs import MultiDot, lincomb_
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


def _lbfgs_minimize_impl(obj, maxiter: int = 100, m: int = 10, ftol: float = 1e7 * _EPS,
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
    comm, sharded = obj.comm, obj.sharded
    n = obj.n_local
    dev = obj.device
    if not 1 <= int(m) <= 120:
        # 2 (m + 1) history rows go through one lincomb launch (csrc/lbfgs.hip: <= 256 rows)
        raise ValueError(f"L-BFGS history m must be in 1..120, got {m}")
    red = DeviceReducer(comm, sharded, dev)  # collective (may connect peer memory)
    x = obj.x0().contiguous()
    f, g = obj(x)
    g = g.clone()  # the objective may return a view of a buffer the next evaluation reuses
    nfev = 1
    # A ring of R = m + 1 pair slots: rows 0..R-1 hold s, rows R..2R-1 hold y, row 2R the
    # current gradient.  The new pair is written straight into the spare slot (no copy when
    # it is accepted); one multi-dot of all rows against (s_new, y_new, g) gives every scalar
    # an iteration needs (s.y, y.y, the new Gram rows, S^T g, Y^T g, g.g), and max|g| rides
    # along in the same reduction and device->host copy: with the line search's one copy per
    # evaluation, a typical iteration makes two.
    R = m + 1
    HX = torch.zeros((2 * R + 1, n), dtype=torch.float32, device=dev)
    HS = HX[:2 * R]
    g_row = HX[2 * R]
    dot = MultiDot(2 * R + 1, n, dev)
    dot1 = MultiDot(1, n, dev)
    SY = np.zeros((R, R))
    YY = np.zeros((R, R))
    Sg = np.zeros(R)
    Yg = np.zeros(R)
    order: list = []  # accepted slots, oldest -> newest (at most m)
    d = torch.empty_like(x)
    xt = torch.empty_like(x)
    dev_call = getattr(obj, "device_call", None) if dev.type == "cuda" else None
    coef = torch.zeros(2 * R, dtype=torch.float32, device=dev)

    def absmax(gv: torch.Tensor) -> torch.Tensor:
        return gv.abs().max().double() if gv.numel() else torch.zeros((), dtype=torch.float64,
                                                                     device=gv.device)

    def gstats(gv: torch.Tensor):
        """(global g.g, global max|g|) in one copy."""
        h = red.reduce(sums=[dot1(gv.view(1, -1), 1, [gv])], maxes=[absmax(gv)])
        return float(h[0]), float(h[1])

    status, message = 1, "STOP: TOTAL NO. of ITERATIONS REACHED LIMIT"
    nit = 0
    from ..utils.hooks import StepHooks
    hooks = StepHooks(comm, what="L-BFGS iterate")  # MULTIGRAD_CHECK_EVERY / _METRICS
    gg, gmax = gstats(g)
    host0 = getattr(comm, "host_collectives", 0) if comm is not None else 0
    if gmax <= gtol:
        status, message = 0, "CONVERGENCE: NORM_OF_PROJECTED_GRADIENT_<=_PGTOL"
    else:
        for k in range(maxiter):
            # ---------------- search direction (compact inverse-Hessian product); g.d
            # follows from the host copies of S^T g, Y^T g and g.g (no device round trip)
            gd = -gg
            if order:
                idx = np.array(order)
                gamma, a, b = compact_coefficients(SY, YY, Sg, Yg, order)
                cvec = np.zeros(2 * R)
                cvec[idx] = -a
                cvec[R + idx] = -gamma * b
                coef.copy_(torch.from_numpy(cvec.astype(np.float32)))
                lincomb_(HS, 2 * R, coef, -gamma, g, d)
                gd = -gamma * gg - float(a @ Sg[idx]) - gamma * float(b @ Yg[idx])
            else:
                d.copy_(-g)
            if not np.isfinite(gd) or gd >= 0:  # not a descent direction: reset memory
                order.clear()
                d.copy_(-g)
                gd = -gg
            a1 = 1.0 if order else min(1.0, 1.0 / math.sqrt(max(-gd, 1e-300)))
            # ---------------- strong-Wolfe line search
            cache = {}

            def phi(alpha):
                nonlocal nfev
                torch.add(x, d, alpha=float(alpha), out=xt)
                if dev_call is not None:
                    # the loss (already global) and the local d.g: one reduction, one copy
                    lt, ga = dev_call(xt)
                    ga = ga.clone()
                    h = red.reduce(sums=[dot1(ga.view(1, -1), 1, [d])], local=[lt.reshape(1)])
                    da, fa = float(h[0]), float(h[1])
                else:
                    fa, ga = obj(xt)
                    ga = ga.clone()
                    da = float(red.reduce(sums=[dot1(ga.view(1, -1), 1, [d])])[0])
                nfev += 1
                cache[alpha] = (fa, ga, da)
                return fa, da

            f0, d0 = f, gd
            a_prev, f_prev, dphi_prev = 0.0, f0, d0
            alpha, best = a1, None
            for i in range(maxls):
                fa, da = phi(alpha)
                if not np.isfinite(fa) or fa > f0 + c1 * alpha * d0 or (i > 0 and fa >= f_prev):
                    best = _zoom(phi, a_prev, alpha, f_prev, fa, dphi_prev, da, f0, d0, c1, c2, maxls)
                    break
                if abs(da) <= -c2 * d0:
                    best = alpha
                    break
                if da >= 0:
                    best = _zoom(phi, alpha, a_prev, fa, f_prev, da, dphi_prev, f0, d0, c1, c2, maxls)
                    break
                a_prev, f_prev, dphi_prev = alpha, fa, da
                alpha = alpha * 2.0
            if best is None or best not in cache:
                # no acceptable step: keep the best decrease seen, else stop
                cands = [(v[0], a) for a, v in cache.items() if v[0] < f0]
                if not cands:
                    status, message = 2, "ABNORMAL_TERMINATION_IN_LNSRCH"
                    break
                best = min(cands)[1]
            f_new, g_new, _ = cache[best]
            # ---------------- update iterate and history (new pair in the spare slot q)
            q = min(set(range(R)) - set(order))
            s_vec, y_vec = HS[q], HS[R + q]
            torch.mul(d, best, out=s_vec)
            x.add_(s_vec)
            torch.sub(g_new, g, out=y_vec)
            g_row.copy_(g_new)
            nit = k + 1
            dv = dot(HX, 2 * R + 1, [s_vec, y_vec, g_row])  # (2R+1, 3)
            host = red.reduce(sums=[dv], maxes=[absmax(g_new)])
            dots = host[:-1].reshape(2 * R + 1, 3)
            gmax = float(host[-1])
            sy_new, yy_new = float(dots[q, 1]), float(dots[R + q, 1])
            gg = float(dots[2 * R, 2])
            if sy_new > _EPS * yy_new and yy_new > 0:  # accept: q joins, the oldest leaves
                if len(order) == m:
                    order.pop(0)
                order.append(q)
                for o in order:
                    if o == q:
                        SY[q, q] = sy_new
                        YY[q, q] = yy_new
                    else:
                        SY[o, q] = dots[o, 1]          # s_o . y_new
                        SY[q, o] = dots[R + o, 0]      # s_new . y_o
                        YY[o, q] = YY[q, o] = dots[R + o, 1]
            Sg[:] = dots[:R, 2]
            Yg[:] = dots[R:2 * R, 2]
            f_old, f, g = f, f_new, g_new
            if callback is not None:
                h0 = getattr(comm, "host_collectives", 0) if comm is not None else 0
                callback(obj.full(x))
                if comm is not None:  # the callback's own collectives are not the loop's
                    host0 += getattr(comm, "host_collectives", 0) - h0
            if hooks.active:
                hooks(k, f, None, (lambda: x) if not sharded else None)
            if gmax <= gtol:
                status, message = 0, "CONVERGENCE: NORM_OF_PROJECTED_GRADIENT_<=_PGTOL"
                break
            if (f_old - f) <= ftol * max(abs(f_old), abs(f), 1.0):
                status, message = 0, "CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH"
                break
    host_calls = (getattr(comm, "host_collectives", 0) - host0) if comm is not None else 0
    red.check("L-BFGS")
    if getattr(obj, "check", None) is not None:
        obj.check("L-BFGS")  # the objective's own exchanges (engine: ZeRO two-shot, one-shot)
    xf = obj.full(x)
    if getattr(obj, "finalize", None) is not None:
        xf = obj.finalize(x)
    res = scipy.optimize.OptimizeResult(
        x=xf, fun=f, jac=g, nit=nit, nfev=nfev, njev=nfev, status=status,
        success=status == 0, message=message, host_collectives=host_calls,
        reduction=red.describe())
    if hess_inv:
        from .invhess import build_hess_inv
        res["hess_inv"] = build_hess_inv(obj, HS, R, order, SY, YY, red, x, dot=dot)
    return res


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


def run_lbfgs_device(loss_and_grad_fn: Callable, params, maxsteps: int = 100, param_bounds=None,
                     randkey=None, comm=None, history: int = 10, **kw):
    """Device L-BFGS for a generic ``loss_and_grad_fn(params[, randkey])`` (replicated).

    ``hess_inv=True`` (default) returns the inverse-Hessian operator as ``res.hess_inv``
    (it holds the history ring, see :func:`lbfgs_minimize`).  With ``param_bounds`` the
    iteration runs in the transformed variables ``u`` and the operator is ``J H_u J`` with
    ``J = diag(dx/du)`` at the final iterate (:mod:`multigrad_amd.optim.invhess`)."""
    from ..utils.random import init_randkey
    from .transforms import Bounds
    from ..utils.tensors import as_param_tensor
    x0 = as_param_tensor(params)
    bounds = Bounds.from_spec(param_bounds, x0.numel(), device=x0.device, dtype=torch.float32)
    fkw = {} if randkey is None else {"randkey": init_randkey(randkey)}
    obj = GenericObjective(loss_and_grad_fn, x0, comm=comm, bounds=bounds, **fkw)
    return lbfgs_minimize(obj, maxiter=maxsteps, m=history, **kw)


def lbfgs_minimize(*args, **kwargs):
    """See ``_lbfgs_minimize_impl``; runs with the BLAS pools limited to one thread (the host-side
    compact-form solves are tiny; a spinning BLAS pool would slow the CPU evaluations)."""
    from ..utils.hooks import driver_guard
    from ..utils.tensors import blas_single_thread
    obj = args[0] if args else kwargs.get("obj")
    with driver_guard(getattr(obj, "comm", None)), blas_single_thread():
        return _lbfgs_minimize_impl(*args, **kwargs)


lbfgs_minimize.__doc__ = _lbfgs_minimize_impl.__doc__
