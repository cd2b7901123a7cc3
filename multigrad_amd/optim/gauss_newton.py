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

The scaling ``diag(d)`` makes the step invariant to the units of the parameters, and with it a
parameter the sumstats barely depend on takes a large step (``delta_p ~ 1 / J_p``).  With far
more parameters than sumstats that is the common case: at 1e7 parameters of the population
model the first accepted ``lambda`` is near 1e8 (every rejected trial costs one loss
evaluation), and single parameters are carried far outside the data's range within a few
iterations (profiles/smf_gauss_newton/README.md).  The dual driver ends without success when
the Jacobian stops being finite there.

**Dual form** (:func:`run_gauss_newton_dual`).  ``G`` has rank at most ``K``, so the same step
needs only ``K x K`` algebra and nothing of size ``ndim x ndim`` (Woodbury).  With
``c = dl/dS``, ``g = J^T c``, ``H = L L^T`` (``L = V_+ sqrt(Lambda_+)``, ``[K, r]``, from the
eigendecomposition that clips the negative eigenvalues) and ``M = lambda diag(d)``:

    W1 = J diag(1/d) J^T   (float64, once per Jacobian: ops.gram.weighted_gram),
    W = W1 / lambda,   u = W c,   y = L (I_r + L^T W L)^-1 L^T u   (Cholesky, host),
    delta = -(g - J^T y) / (lambda d) = -J^T ((c - y) / lambda) / d.

The last form is the one evaluated: ``c - y`` is formed in float64 on the host, so the device
pass has no cancellation.  ``J``, ``g``, ``d``, ``x``, ``delta`` and the trial point stay on
the parameters' device in the parameters' dtype; a Jacobian costs one device->host copy of
the packed ``[W1, c, H, max|g|, max d]`` block, a trial one host->device copy of ``K`` floats,
one pass over ``J`` for ``delta`` and one vector add for the trial point.  ``J`` itself is
``K * ndim`` values (400 MB at ``K = 10`` and 1e7 float32 parameters, 4 GB at 1e8): there is
no streaming variant.
"""
from __future__ import annotations

from typing import Callable

import numpy as np
import scipy.optimize
import torch

from scipy.sparse.linalg import LinearOperator

from ..ops.gram import weighted_gram
from ..ops.lbfgs import MultiDot, compact_diag_, lincomb_, lincomb_cols_
from ._damped import LAMBDA_MIN, damped_loop

__all__ = ["run_gauss_newton", "run_gauss_newton_dual", "dual_step", "GaussNewtonInvProduct"]

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
    ``"reverse"``, the Jacobian mode of the last evaluation) and ``hess_inv``, the float64
    pseudo-inverse of the final Gauss-Newton matrix.
    """
    x_t = torch.as_tensor(params).detach()
    shape, dtype, device = x_t.shape, x_t.dtype, x_t.device
    x = _host(x_t).reshape(-1)

    def tensor(v):
        return torch.as_tensor(v, dtype=dtype, device=device).reshape(shape)

    def evaluate(xv):
        out = gauss_newton_fn(tensor(xv))
        return _scalar(out[0]), (_host(out[1]).reshape(-1), _host(out[2]), out[3])

    run = damped_loop(
        x, evaluate, finite=lambda state: True,
        converged=lambda state, xv: not state[0].size or np.max(np.abs(state[0])) <= gtol,
        measure="max |grad|",
        trials=lambda state, xv: lambda lam: xv + _solve(state[1], lam, state[0]),
        loss_at=lambda trial: _scalar(loss_fn(tensor(trial))),
        maxsteps=maxsteps, damping=damping, floor=LAMBDA_MIN, ftol=ftol, comm=comm)
    g, G, jac_mode = run.state
    return scipy.optimize.OptimizeResult(
        x=run.x.reshape(shape), fun=run.loss, jac=g.reshape(shape), nit=run.nit, nfev=run.nfev,
        njev=run.njev, success=run.success, message=run.message, jac_mode=jac_mode,
        hess_inv=np.linalg.pinv(G) if G.size else G)


# ---------------------------------------------------------------------------- dual form
_MAX_SUMSTATS = 240   # compact_diag_ takes up to 240 rows
_MAX_DENSE = 4096
_COLS = 4             # columns per pass (lincomb_cols_, MultiDot)


def _native(J: torch.Tensor) -> bool:
    """Whether the fused vector ops take ``J``: float32 on the GPU (the HIP kernels) or any
    CPU tensor (their PyTorch forms).  Other device dtypes use torch's own ops."""
    return J.device.type != "cuda" or J.dtype == torch.float32


def _coef(v: np.ndarray, J: torch.Tensor) -> torch.Tensor:
    """A small host float64 array as the coefficient tensor the vector ops take."""
    if J.device.type != "cuda":
        dt = torch.float64        # the CPU forms of the vector ops work in float64
    else:
        dt = torch.float32 if _native(J) else J.dtype
    return torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64).to(device=J.device, dtype=dt)


def _psd_factor(H: np.ndarray) -> np.ndarray:
    """``L`` ``[K, r]`` with ``L L^T`` the positive part of the symmetric ``H``."""
    lam, vec = np.linalg.eigh(0.5 * (H + H.T))
    keep = lam > 0.0
    return vec[:, keep] * np.sqrt(lam[keep])


def _jt_combine(J, coef: np.ndarray, post=None):
    """``post * (J^T coef)`` as a ``[P]`` tensor in ``J``'s dtype: one pass over ``J``."""
    K, P = J.shape
    if not _native(J):
        out = _coef(coef, J) @ J
        return out if post is None else out * post
    out = torch.empty(1, P, dtype=J.dtype, device=J.device)
    lincomb_cols_(J, K, _coef(coef, J).reshape(K, 1), 0.0, None, out, post=post)
    return out[0]


def _diag_jhj(J, Q: np.ndarray):
    """``diag(J^T Q J)`` ``[P]`` in ``J``'s dtype for a symmetric host ``Q``: one pass."""
    K, P = J.shape
    if not _native(J):
        return ((_coef(Q, J) @ J) * J).sum(0)
    out = torch.empty(P, dtype=J.dtype, device=J.device)
    rows = torch.arange(K, dtype=torch.int32, device=J.device)
    fac = torch.ones(K, dtype=torch.float32, device=J.device)
    compact_diag_(J, rows, fac, _coef(Q, J), 0.0, out)
    return out


class _DualFactors:
    """Everything one Jacobian gives the dual solve: ``g``, ``d``, ``1/d`` on the device and
    the packed host block (module docstring).  ``copies`` records the sizes of the
    device->host copies made here."""

    def __init__(self, J: torch.Tensor, c, H, copies: list):
        J = J.detach()
        if J.dim() != 2:
            raise ValueError("J must be [K, P]")
        if not J.is_contiguous():
            J = J.contiguous()
        K, P = J.shape
        if not 1 <= K <= _MAX_SUMSTATS:
            raise ValueError(f"the dual solve takes 1..{_MAX_SUMSTATS} sumstats, got {K}")
        self.J, self.K, self.P = J, K, P
        dev = J.device
        c_dev = torch.as_tensor(c).detach().reshape(-1).to(dev, torch.float64)
        if not P:
            self.g = J.new_zeros(0)
        elif _native(J):
            self.g = torch.empty(P, dtype=J.dtype, device=dev)
            cdt = torch.float32 if dev.type == "cuda" else J.dtype
            lincomb_(J, K, c_dev.to(cdt), 0.0, None, self.g)
        else:
            self.g = c_dev.to(J.dtype) @ J
        # H+ is needed before the diagonal pass; the models hand H over on the host (its
        # eigendecomposition runs there), so this is a device copy only for a device H
        H_t = torch.as_tensor(H).detach().reshape(K, K)
        if H_t.device.type != "cpu":
            copies.append(K * K)
        Hh = H_t.cpu().double().numpy()
        h_finite = bool(np.isfinite(Hh).all())
        self.L = _psd_factor(Hh) if h_finite else np.zeros((K, 0))
        Hp = self.L @ self.L.T
        if P:
            d = _diag_jhj(J, Hp)
            dmax = d.max()
            d = torch.maximum(d, 1e-12 * dmax)
            self.inv_d = torch.where(d > 0, 1.0 / d, torch.zeros_like(d))
            W1 = weighted_gram(J, self.inv_d) if _native(J) or J.dtype == torch.float64 else \
                weighted_gram(J.double(), self.inv_d.double())
            gmax = self.g.abs().max()
        else:
            self.inv_d = J.new_zeros(0)
            W1 = torch.zeros(K, K, dtype=torch.float64, device=dev)
            dmax = gmax = torch.zeros((), dtype=J.dtype, device=dev)
        packed = torch.cat([W1.reshape(-1), c_dev, gmax.reshape(1).double(),
                            dmax.reshape(1).double()]).cpu().numpy()
        copies.append(packed.size)
        self.W1 = packed[:K * K].reshape(K, K)
        self.W1 = 0.5 * (self.W1 + self.W1.T)
        self.c = packed[K * K:K * K + K]
        self.gmax, self.dmax = float(packed[-2]), float(packed[-1])
        # a non-finite Jacobian entry reaches max|g|, max d or W1
        self.finite = bool(np.isfinite(packed).all() and h_finite)

    def coefficients(self, lam: float) -> np.ndarray:
        """``(c - y) / lambda`` (host float64): ``delta = -J^T coefficients / d``."""
        L, c = self.L, self.c
        W = self.W1 / lam
        y = np.zeros_like(c)
        if L.shape[1]:
            A = np.eye(L.shape[1]) + L.T @ W @ L
            rhs = L.T @ (W @ c)
            try:
                y = L @ scipy.linalg.cho_solve(scipy.linalg.cho_factor(A), rhs)
            except (np.linalg.LinAlgError, ValueError):
                y = L @ np.linalg.lstsq(A, rhs, rcond=None)[0]
        return (c - y) / lam

    def step(self, lam: float) -> torch.Tensor:
        """The damped step ``delta`` ``[P]`` on the device (one pass over ``J``)."""
        if not self.dmax > 0.0:   # J^T H+ J = 0: the dense system is singular, no step
            return torch.zeros(self.P, dtype=self.J.dtype, device=self.J.device)
        return _jt_combine(self.J, -self.coefficients(lam), post=self.inv_d)


def dual_step(J, c, H, lam: float) -> torch.Tensor:
    """One damped Gauss-Newton step by the dual solve: the solution of
    ``(J^T H+ J + lam diag(d)) delta = -J^T c`` (module docstring) as a ``[P]`` tensor on
    ``J``'s device, without forming anything ``P x P``."""
    return _DualFactors(torch.as_tensor(J), c, H, []).step(float(lam))


class GaussNewtonInvProduct(LinearOperator):
    """``hess_inv`` of the dual Gauss-Newton driver: the pseudo-inverse of the final
    Gauss-Newton matrix ``J^T H+ J`` as an operator that holds ``J`` (``[K, P]``) on its
    device.  With ``B = L^T J`` and ``B B^T = U Sigma^2 U^T`` it is

        pinv(J^T H+ J) = B^T U Sigma^-4 U^T B = J^T C J,   C = L U Sigma^-4 U^T L^T,

    dropping the eigenvalues ``Sigma^2`` below numpy ``pinv``'s default relative cutoff
    (``1e-15`` of the largest).  ``C`` is ``K x K`` float64 on the host; a product is two
    passes over ``J``, the diagonal one.  The operator keeps ``J`` alive (``K * P`` values)
    until it is dropped.  A ``J`` with non-finite entries gives an operator of NaNs."""

    def __init__(self, J: torch.Tensor, L: np.ndarray):
        self.J = J.detach().contiguous()
        K, P = self.J.shape
        self.device = self.J.device
        L = np.asarray(L, dtype=np.float64).reshape(K, -1)
        C = np.zeros((K, K))
        if L.shape[1] and P:
            Jd = self.J if _native(self.J) or self.J.dtype == torch.float64 else self.J.double()
            JJ = weighted_gram(Jd).cpu().numpy()
            S = L.T @ (0.5 * (JJ + JJ.T)) @ L
            if not np.isfinite(S).all():
                C[:] = np.nan    # a non-finite J has no pseudo-inverse: every product is NaN
            else:
                sig2, U = np.linalg.eigh(0.5 * (S + S.T))
                keep = sig2 > 1e-15 * max(float(sig2.max()), 0.0)
                if keep.any():
                    LU = L @ U[:, keep]
                    C = (LU / sig2[keep] ** 2) @ LU.T
        self.C = 0.5 * (C + C.T)
        self._dot = MultiDot(K, P, self.device) if _native(self.J) and P else None
        super().__init__(dtype=np.dtype(np.float64), shape=(P, P))

    def apply(self, V: torch.Tensor) -> torch.Tensor:
        """``pinv @ V`` for a tensor ``[P]`` or ``[P, c]``; returns ``J``'s dtype on ``J``'s
        device, same shape."""
        V = torch.as_tensor(V)
        P = self.shape[0]
        one = V.dim() == 1
        if V.dim() not in (1, 2) or V.shape[0] != P:
            raise ValueError(f"expected [{P}] or [{P}, c], got {tuple(V.shape)}")
        J, K = self.J, self.J.shape[0]
        Vt = V.detach().to(device=self.device, dtype=J.dtype).reshape(P, -1).T
        out = torch.empty((Vt.shape[0], P), dtype=J.dtype, device=self.device)
        for c0 in range(0, Vt.shape[0], _COLS):
            cols = Vt[c0:c0 + _COLS].contiguous()
            nc = cols.shape[0]
            if self._dot is None:
                if P:
                    out[c0:c0 + nc] = (_coef(self.C, J) @ (J @ cols.T)).T @ J
                continue
            t = self._dot(J, K, list(cols)).cpu().numpy()          # J v: [K, nc]
            lincomb_cols_(J, K, _coef(self.C @ t, J), 0.0, None, out[c0:c0 + nc])
        return out.reshape(-1) if one else out.T

    def _matmat(self, X):
        X = np.asarray(X, dtype=np.float64)
        return self.apply(torch.from_numpy(np.ascontiguousarray(X))).double().cpu().numpy()

    def _matvec(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        return self.apply(torch.from_numpy(np.ascontiguousarray(x))).double().cpu().numpy()

    _rmatvec = _matvec  # symmetric
    _rmatmat = _matmat

    def _adjoint(self):
        return self

    def diagonal(self) -> torch.Tensor:
        """``diag(pinv)`` ``[P]`` in ``J``'s dtype on ``J``'s device: one pass over ``J``.
        Evaluated as ``sum_ab J_a C_ab J_b``: with a float32 ``J`` on the GPU the error is
        float32 relative to ``|J|^T |C| |J|``, so entries far below the largest can come out
        with the wrong sign when ``C`` is ill-conditioned."""
        if not self.shape[0]:
            return self.J.new_zeros(0)
        return _diag_jhj(self.J, self.C)

    def todense(self) -> np.ndarray:
        """The dense matrix (float64 numpy), for ``P <= 4096``."""
        P = self.shape[0]
        if P > _MAX_DENSE:
            raise ValueError(f"todense() is limited to P <= {_MAX_DENSE} (P = {P}); use "
                             "apply(), matvec() or diagonal()")
        Jh = self.J.double().cpu().numpy()
        return Jh.T @ self.C @ Jh


def _factors(factors_fn: Callable, x: torch.Tensor, shape, copies: list):
    """One call of a dual driver's ``factors_fn`` at the flat ``x`` as the frame's
    ``(loss, state)``, the state being ``(_DualFactors, jac_mode)``."""
    out = factors_fn(x.reshape(shape))
    K = torch.as_tensor(out[1]).numel()
    J = torch.as_tensor(out[2]).detach().reshape(K, x.numel())
    J = J.to(device=x.device, dtype=x.dtype)
    return _scalar(out[0]), (_DualFactors(J, out[1], out[3], copies), out[4])


def run_gauss_newton_dual(factors_fn: Callable, loss_fn: Callable, params, maxsteps: int = 50,
                          damping: float = 1e-3, ftol: float = 2.2e-9, gtol: float = 1e-8,
                          comm=None):
    """:func:`run_gauss_newton` in the dual form (module docstring): the same iteration,
    damping schedule, stopping rules and messages, with ``K x K`` host algebra and every
    ``ndim``-sized vector on the parameters' device.

    Parameters
    ----------
    factors_fn : ``params -> (loss, c, J, H, jac_mode)``, identical on every rank: the loss,
        ``c = dl/dS`` ``[K]``, the sumstat Jacobian ``J`` ``[K, ndim]`` on the parameters'
        device (``K <= 240``), and the symmetric ``[K, K]`` loss Hessian (its negative
        eigenvalues are clipped here)
    loss_fn, params, maxsteps, damping, ftol, gtol, comm : as in :func:`run_gauss_newton`

    Returns
    -------
    scipy.optimize.OptimizeResult with the dense driver's fields and ``solver="dual"``.
    ``x`` and ``jac`` are tensors of the parameters' shape, dtype and device (nothing
    ``ndim``-sized is copied to the host); ``hess_inv`` is a
    :class:`GaussNewtonInvProduct`; ``host_copy_sizes`` lists the element counts of the
    device->host copies of arrays the driver itself made (one packed block per Jacobian; the
    loss scalars and whatever the model's hooks copy are not counted).
    """
    x_t = torch.as_tensor(params).detach()
    shape = x_t.shape
    x = x_t.reshape(-1).clone()
    copies: list = []

    run = damped_loop(
        x, lambda xv: _factors(factors_fn, xv, shape, copies),
        finite=lambda state: state[0].finite,
        converged=lambda state, xv: not state[0].P or state[0].gmax <= gtol,
        measure="max |grad|",
        trials=lambda state, xv: lambda lam: xv + state[0].step(lam),
        loss_at=lambda trial: _scalar(loss_fn(trial.reshape(shape))),
        maxsteps=maxsteps, damping=damping, floor=LAMBDA_MIN, ftol=ftol, comm=comm)
    fac, jac_mode = run.state
    return scipy.optimize.OptimizeResult(
        x=run.x.reshape(shape), fun=run.loss, jac=fac.g.reshape(shape), nit=run.nit,
        nfev=run.nfev, njev=run.njev, success=run.success, message=run.message,
        jac_mode=jac_mode, solver="dual", hess_inv=GaussNewtonInvProduct(fac.J, fac.L),
        host_copy_sizes=copies)
