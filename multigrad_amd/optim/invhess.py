"""The inverse-Hessian approximation of a device L-BFGS / L-BFGS-B run as a device operator.

scipy's L-BFGS-B result carries ``hess_inv``, a ``LinearOperator`` over host copies of the
(s, y) pairs.  At 1e6-1e9 parameters the pairs live on the GPUs -- sharded 1/W per rank under
the ZeRO or owner engine, in the optimizer's internal (permuted, padded) order -- so
:class:`DeviceLbfgsInvHessProduct` keeps a *reference* to the optimizer's history ring and
evaluates products and the diagonal there, in the compact form (Byrd, Nocedal & Schnabel
1994)::

    H = h0 I + W' Q W,   W = [S ; h0 Y]  (2k x n),
    Q = [[R^-T (D + h0 Y'Y) R^-1, -R^-T], [-R^-1, 0]],   R = triu(S'Y), D = diag(S'Y)

built from the k accepted pairs (oldest first).  One product of up to 4 columns is one pass
over the history for the inner products (``MultiDot``), one small cross-rank reduction with
ONE device->host copy (2k x c doubles), the 2k x 2k host algebra, and one pass for the
combination (``lincomb_cols``); the diagonal is one pass (``compact_diag``).

**Scaling.**  The default ``h0`` is the optimizers' own, ``gamma = s.y / y.y`` of the newest
accepted pair (``1 / theta`` for L-BFGS-B), so ``-(op.apply(g))`` is the direction the
unbounded iteration would take next.  ``scipy.optimize.LbfgsInvHessProduct`` starts from
``H0 = I`` instead; :meth:`DeviceLbfgsInvHessProduct.with_h0` with ``1.0`` gives that operator
on the same storage.  Without an accepted pair ``H = I``.  Bounds of L-BFGS-B do not enter.

**Bound transforms.**  When the optimizer ran in transformed variables ``u`` (``x = T(u)``,
:func:`multigrad_amd.optim.lbfgs.run_lbfgs_device` with ``param_bounds``) the pairs are
``u``-space pairs and the operator is ``J H_u J`` with ``J = diag(dx/du)`` at the final
iterate: the inverse Hessian in ``x`` at a stationary point.  :meth:`pairs` then returns the
``u``-space pairs.

**Memory.**  The operator holds the optimizer's ring of ``2 (m + 1)`` fp32 vectors (no copy):
0.9 GB at 1e7 parameters and ``m = 10`` on one rank, until the result is dropped.  Pass
``hess_inv=False`` to the optimizers to free the ring on return.

On several ranks with sharded vectors every method is collective: the same call with the same
input on every rank.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import scipy.linalg
import torch
from scipy.sparse.linalg import LinearOperator

from ..ops.lbfgs import MultiDot, compact_diag_, lincomb_cols_

__all__ = ["DeviceLbfgsInvHessProduct", "IdentityLayout"]

_MAX_DENSE = 8192
_MAX_PAIRS = 1 << 27
_COLS = 4  # columns per pass (csrc/lbfgs.hip: lincomb_cols, multi_dot)


class IdentityLayout:
    """Layout of an optimizer vector that *is* the user's parameter vector (replicated
    objectives): ``to_local`` / ``from_local`` map ``[..., P]`` user order to and from the
    optimizer's local ``[..., n_local]`` vector."""

    identity = True  # from_local returns its argument: results can be written in place

    def __init__(self, P: int):
        self.P = int(P)
        self.n_local = int(P)

    def to_local(self, v: torch.Tensor) -> torch.Tensor:
        return v.contiguous()

    def from_local(self, t: torch.Tensor) -> torch.Tensor:
        return t


class DeviceLbfgsInvHessProduct(LinearOperator):
    """``hess_inv`` of the device optimizers (see the module docstring).

    ``HS`` is the history ring ``[>= 2 R, n_local]`` (rows ``0..R-1`` the ``s`` slots, rows
    ``R..2R-1`` the ``y`` slots), ``order`` the accepted slots oldest first, ``SY`` / ``YY``
    the ``R x R`` global inner products by slot (``SS``, which both optimizers hand over with
    their :class:`~multigrad_amd.optim._quasi_newton.PairRing`, is only held: no method reads
    it yet; it is what the direct form ``B = H^-1`` would need), ``red``
    the optimizer's :class:`~multigrad_amd.optim._reduce.DeviceReducer`, ``layout`` the
    objective's ``vector_layout()`` and ``jac`` the local ``dx/du`` (transform mode)."""

    def __init__(self, HS: torch.Tensor, R: int, order, SY, YY, red, layout, SS=None,
                 jac: Optional[torch.Tensor] = None, h0: Optional[float] = None,
                 dot: Optional[MultiDot] = None):
        self.HS, self.R = HS, int(R)
        self.order = [int(o) for o in order]
        self.SY, self.YY = np.array(SY, dtype=np.float64), np.array(YY, dtype=np.float64)
        self.SS = None if SS is None else np.array(SS, dtype=np.float64)
        self.red, self.layout, self.jac = red, layout, jac
        self.n_local = int(HS.shape[1])
        self.device = HS.device
        if h0 is None:
            h0 = 1.0
            if self.order:
                last = self.order[-1]
                h0 = float(self.SY[last, last] / self.YY[last, last])
        self._h0 = float(h0)
        self._Qc = self._Mc = self._Dc = None
        self._dot = dot if dot is not None else MultiDot(2 * self.R, self.n_local, self.device)
        super().__init__(dtype=np.dtype(np.float64), shape=(layout.P, layout.P))

    # ------------------------------------------------------------------ properties
    @property
    def n_corrs(self) -> int:
        """Number of accepted (s, y) pairs the operator is built from."""
        return len(self.order)

    @property
    def h0(self) -> float:
        """The scaling of ``H0 = h0 I``."""
        return self._h0

    def with_h0(self, h0: float) -> "DeviceLbfgsInvHessProduct":
        """The operator with another initial scaling on the same device storage
        (``with_h0(1.0)`` is ``scipy.optimize.LbfgsInvHessProduct`` over :meth:`pairs`)."""
        return DeviceLbfgsInvHessProduct(self.HS, self.R, self.order, self.SY, self.YY, self.red,
                                         self.layout, SS=self.SS, jac=self.jac, h0=float(h0),
                                         dot=self._dot)

    # ------------------------------------------------------------------ compact form
    def _Q(self) -> np.ndarray:
        """The 2k x 2k middle matrix for ``W = [S ; h0 Y]`` (fp64, host; made once: the
        operator never changes)."""
        if self._Qc is None:
            idx = np.asarray(self.order, dtype=np.int64)
            k = idx.size
            sy = self.SY[np.ix_(idx, idx)]
            yy = self.YY[np.ix_(idx, idx)]
            Rinv = scipy.linalg.solve_triangular(np.triu(sy), np.eye(k), lower=False)
            A = Rinv.T @ (np.diag(np.diag(sy)) + self._h0 * yy) @ Rinv
            Q = np.block([[A, -Rinv.T], [-Rinv, np.zeros((k, k))]])
            self._Qc = 0.5 * (Q + Q.T)  # exactly symmetric (compact_diag reads the upper triangle)
        return self._Qc

    def _coef_map(self) -> np.ndarray:
        """``M`` (2R x 2R) with ``coef = M @ dots``: from the ring rows' inner products with a
        vector to the ring rows' coefficients in ``H v = h0 v + sum_r coef_r HS_r`` (E picks
        the accepted rows as ``W = E HS``, so ``M = E' Q E``; other rows get zero)."""
        if self._Mc is None:
            k, R = len(self.order), self.R
            E = np.zeros((2 * k, 2 * R))
            E[np.arange(k), self.order] = 1.0
            E[k + np.arange(k), R + np.asarray(self.order, dtype=np.int64)] = self._h0
            self._Mc = E.T @ self._Q() @ E
        return self._Mc

    def _diag_args(self):
        """``(rows, fac, Q)`` of ``compact_diag`` on the device (made once)."""
        if self._Dc is None:
            k, R = len(self.order), self.R
            idx = np.asarray(self.order, dtype=np.int64)
            rows = torch.from_numpy(np.concatenate([idx, R + idx]).astype(np.int32))
            fac = torch.from_numpy(np.concatenate([np.ones(k), np.full(k, self._h0)]).astype(np.float32))
            Q = torch.from_numpy(self._Q().astype(np.float32))
            self._Dc = tuple(t.to(self.device) for t in (rows, fac, Q))
        return self._Dc

    def _check(self) -> None:
        self.red.check("hess_inv")

    # ------------------------------------------------------------------ products
    def apply(self, V: torch.Tensor) -> torch.Tensor:
        """``H @ V`` for a device tensor ``[P]`` or ``[P, c]`` in the user's parameter order;
        returns fp32 of the same shape.  Collective on sharded runs.

        The kernels take columns as contiguous vectors: a column-major ``V`` (``A.T`` of a
        contiguous ``[c, P]`` tensor) is used as it is, a row-major one is transposed first;
        the ``[P, c]`` result is column-major (the transposed view of the ``[c, P]`` buffer
        the kernels wrote)."""
        V = torch.as_tensor(V)
        one = V.dim() == 1
        if V.dim() not in (1, 2) or V.shape[0] != self.shape[0]:
            raise ValueError(f"expected [{self.shape[0]}] or [{self.shape[0]}, c], got {tuple(V.shape)}")
        Vt = V.detach().to(device=self.device, dtype=torch.float32).reshape(self.shape[0], -1).T
        out = torch.empty((Vt.shape[0], self.shape[0]), dtype=torch.float32, device=self.device)
        R, k, h0 = self.R, len(self.order), self._h0
        M = self._coef_map() if k else None
        inplace = getattr(self.layout, "identity", False)
        for c0 in range(0, Vt.shape[0], _COLS):
            loc = self.layout.to_local(Vt[c0:c0 + _COLS].contiguous())
            nc = loc.shape[0]
            y = out[c0:c0 + nc] if inplace else torch.empty_like(loc)
            coef = torch.empty((0, nc), dtype=torch.float32, device=self.device)
            if k:
                vj = loc * self.jac if self.jac is not None else loc
                dots = self.red.reduce(sums=[self._dot(self.HS, 2 * R, list(vj))])
                cm = (M @ dots.reshape(2 * R, nc)).astype(np.float32)
                coef = torch.from_numpy(cm).to(self.device)
            lincomb_cols_(self.HS, 2 * R if k else 0, coef, h0, loc, y, pre=self.jac,
                          post=self.jac)
            if not inplace:
                out[c0:c0 + nc] = self.layout.from_local(y)
        self._check()
        return out.reshape(-1) if one else out.T

    def _matmat(self, X):
        X = np.asarray(X, dtype=np.float64)
        return self.apply(torch.from_numpy(np.ascontiguousarray(X))).double().cpu().numpy()

    def _matvec(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        return self.apply(torch.from_numpy(np.ascontiguousarray(x))).double().cpu().numpy()

    _rmatvec = _matvec  # H is symmetric
    _rmatmat = _matmat

    def _adjoint(self):
        return self

    def diagonal(self) -> torch.Tensor:
        """``diag(H)`` as an fp32 device tensor ``[P]`` in the user's order: one pass over the
        history, no product.  Collective on sharded runs."""
        k, R, h0 = len(self.order), self.R, self._h0
        out = torch.empty(self.n_local, dtype=torch.float32, device=self.device)
        if k:
            rows, fac, Q = self._diag_args()
            compact_diag_(self.HS, rows, fac, Q, h0, out, scale=self.jac)
        else:
            out.fill_(h0)
            if self.jac is not None:
                out.mul_(self.jac * self.jac)
        res = self.layout.from_local(out.reshape(1, -1))[0]
        self._check()
        return res

    def todense(self) -> np.ndarray:
        """The dense matrix (fp64 numpy), for ``P <= 8192``."""
        P = self.shape[0]
        if P > _MAX_DENSE:
            raise ValueError(f"todense() is limited to P <= {_MAX_DENSE} (P = {P}); use "
                             "apply() or diagonal()")
        return self.apply(torch.eye(P, dtype=torch.float32, device=self.device)).double().cpu().numpy()

    def pairs(self):
        """``(sk, yk)``: the accepted pairs as fp64 numpy ``[k, P]`` in the user's order, oldest
        first (the arguments of ``scipy.optimize.LbfgsInvHessProduct``).  Collective."""
        k, P = len(self.order), self.shape[0]
        if k * P > _MAX_PAIRS:
            raise ValueError(f"pairs() would gather {k} x {P} values (limit 2**27)")
        if k == 0:
            return np.zeros((0, P)), np.zeros((0, P))
        idx = torch.as_tensor(self.order, dtype=torch.int64, device=self.device)
        sk = self.layout.from_local(self.HS[idx]).double().cpu().numpy()
        yk = self.layout.from_local(self.HS[self.R + idx]).double().cpu().numpy()
        self._check()
        return sk, yk


def _layout_of(obj):
    """``obj.vector_layout()``; an objective without one whose vector is not sharded is taken
    to optimise the user's vector itself (the documented objective protocol has no layout)."""
    fn = getattr(obj, "vector_layout", None)
    if fn is not None:
        return fn()
    if getattr(obj, "sharded", False) and getattr(obj, "comm", None) is not None \
            and obj.comm.size > 1:
        raise TypeError("hess_inv=True needs vector_layout() on an objective with sharded "
                        "vectors (or pass hess_inv=False)")
    return IdentityLayout(obj.n_local)


def check_hess_inv_objective(obj) -> None:
    """Raise before the run, not after it, if no operator can be built for ``obj``."""
    if getattr(obj, "vector_layout", None) is None:
        _layout_of(obj)


def build_hess_inv(obj, ring, red, x, dot=None):
    """The operator for an optimizer's final state (``ring``: its
    :class:`~multigrad_amd.optim._quasi_newton.PairRing`, ``x``: its final local vector)."""
    HS, R, order = ring.HS, ring.R, ring.order
    layout = _layout_of(obj)
    bounds = getattr(obj, "bounds", None)
    jac = bounds.dpdu(x).to(torch.float32).contiguous() if bounds is not None else None
    # slots outside `order` hold a rejected or stale pair: they get zero coefficients, and a
    # non-finite entry there must not reach a product (0 * inf)
    for q in set(range(R)) - set(order):
        HS[q].zero_()
        HS[R + q].zero_()
    return DeviceLbfgsInvHessProduct(HS, R, order, ring.SY, ring.YY, red, layout, SS=ring.SS,
                                     jac=jac, dot=dot)
