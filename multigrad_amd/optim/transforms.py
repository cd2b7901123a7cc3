"""Box-constraint reparameterisation for Adam (reference ``multigrad/adam.py:192-239``).

Each bounded parameter ``p`` is optimised in an unbounded coordinate ``u = T(p)``:

=================  ===========================  ==============================  =====================
bounds             u = T(p)                     p = T^-1(u)                     dp/du
=================  ===========================  ==============================  =====================
both finite        s tan((p - mid)/s)           mid + s atan(u/s)               1/(1 + (u/s)^2)
low only           p - lo + 1/(lo - p)          lo + h(u)                       h(u)/sqrt(u^2+4)
high only          p - hi + 1/(hi - p)          hi - h(-u)                      h(-u)/sqrt(u^2+4)
none               p                            u                               1
=================  ===========================  ==============================  =====================

with ``mid = (lo+hi)/2``, ``s = (hi-lo)/pi`` and the distance to a one-sided bound
``h(u) = (u + sqrt(u^2+4))/2``.  Towards the bound (``u < 0``) that difference cancels in
floating point -- in float32 it is exactly 0 from ``|u| ~ 1e4``, which would put the
parameter on its bound with ``dp/du = 0`` for good -- so there ``h`` is evaluated as
``2/(sqrt(u^2+4) + |u|)``; away from the bound the expressions are
``(2 lo + u + sqrt(u^2+4))/2`` and ``(1 + u/sqrt(u^2+4))/2`` (mirrored for a high bound).
The two-sided result is clamped into ``[lo, hi]``: for ``|u/s|`` large, rounding would
otherwise carry ``mid +- s pi/2`` past the box.  The reference builds a dense
``P x P`` ``jax.jacobian`` of the inverse transform and evaluates it at the *bounded*
parameters; the Jacobian is diagonal, so here it is the elementwise
``dp/du`` evaluated at ``u`` (``legacy=True`` evaluates it at ``p`` for bit-parity).
The device path fuses these formulas into the Adam kernel (``csrc/adam.hip``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

__all__ = ["Bounds", "transform", "inverse_transform", "apply_transforms",
           "apply_inverse_transforms", "dparams_duparams"]

# per-parameter bound kinds (shared with the HIP kernel)
KIND_NONE, KIND_BOTH, KIND_LOW, KIND_HIGH = 0, 1, 2, 3


def _finite(x) -> bool:
    return x is not None and np.isfinite(x)


def _bound_pair(b):
    if b is None:
        return (None, None)
    lo, hi = b
    return (float(lo) if _finite(lo) else None, float(hi) if _finite(hi) else None)


@dataclass
class Bounds:
    """Vectorised per-parameter bounds: ``lo``/``hi`` tensors (+-inf where absent)."""

    lo: torch.Tensor
    hi: torch.Tensor
    kind: torch.Tensor  # int8 KIND_* per parameter

    @staticmethod
    def from_spec(param_bounds, ndim: int, device=None, dtype=torch.float32) -> Optional["Bounds"]:
        if param_bounds is None:
            return None
        if isinstance(param_bounds, (np.ndarray, torch.Tensor)) and \
                param_bounds.dtype not in (object, np.object_) and tuple(param_bounds.shape) == (ndim, 2):
            # numeric (ndim, 2) array: vectorised (a 1e7-row Python loop takes seconds);
            # non-finite entries mark an absent side, as in the list form
            arr = torch.as_tensor(param_bounds).to(device=device, dtype=torch.float64)
            lo_t, hi_t = arr[:, 0], arr[:, 1]
            fl, fh = torch.isfinite(lo_t), torch.isfinite(hi_t)
            kind = torch.where(fl & fh, KIND_BOTH, torch.where(fl, KIND_LOW, torch.where(
                fh, KIND_HIGH, KIND_NONE))).to(torch.int8)
            return Bounds(torch.where(fl, lo_t, -math.inf).to(dtype),
                          torch.where(fh, hi_t, math.inf).to(dtype), kind)
        if hasattr(param_bounds, "tolist"):
            param_bounds = param_bounds.tolist()
        pb = list(param_bounds)
        assert len(pb) == ndim, "param_bounds must have shape (ndim, 2)"
        lo = np.full(ndim, -np.inf)
        hi = np.full(ndim, np.inf)
        kind = np.zeros(ndim, dtype=np.int8)
        for i, b in enumerate(pb):
            l, h = _bound_pair(b)
            if l is not None:
                lo[i] = l
            if h is not None:
                hi[i] = h
            kind[i] = (KIND_BOTH if (l is not None and h is not None) else
                       KIND_LOW if l is not None else KIND_HIGH if h is not None else KIND_NONE)
        return Bounds(torch.as_tensor(lo, dtype=dtype, device=device),
                      torch.as_tensor(hi, dtype=dtype, device=device),
                      torch.as_tensor(kind, device=device))

    def to(self, device=None, dtype=None) -> "Bounds":
        return Bounds(self.lo.to(device=device, dtype=dtype), self.hi.to(device=device, dtype=dtype),
                      self.kind.to(device=device))

    # ------------------------------------------------------------- vectorised maps
    def _safe(self, like: torch.Tensor):
        """Bounds with absent sides replaced by finite dummies, so the branches that
        ``torch.where`` discards never produce inf/NaN (which would poison gradients)."""
        k = self.kind.to(like.device)
        lo = torch.where(torch.isfinite(self.lo), self.lo, torch.zeros_like(self.lo)).to(like)
        hi = torch.where(torch.isfinite(self.hi), self.hi, torch.ones_like(self.hi)).to(like)
        both = k == KIND_BOTH
        mid = torch.where(both, (hi + lo) / 2, torch.zeros_like(lo))
        s = torch.where(both, (hi - lo) / math.pi, torch.ones_like(lo))
        return k, lo, hi, mid, s

    def forward(self, p: torch.Tensor) -> torch.Tensor:
        k, lo, hi, mid, s = self._safe(p)
        both = torch.where(k == KIND_BOTH, s * torch.tan((p - mid) / s), p)
        dl = torch.where(k == KIND_LOW, lo - p, torch.ones_like(p))
        low = torch.where(k == KIND_LOW, p - lo + 1.0 / dl, both)
        dh = torch.where(k == KIND_HIGH, hi - p, torch.ones_like(p))
        return torch.where(k == KIND_HIGH, p - hi + 1.0 / dh, low)

    def inverse(self, u: torch.Tensor) -> torch.Tensor:
        k, lo, hi, mid, s = self._safe(u)
        r = torch.sqrt(u * u + 4)
        h = 2.0 / (r + u.abs())  # distance to a one-sided bound on the side towards it
        box = torch.minimum(torch.maximum(mid + s * torch.atan(u / s), lo), hi)
        both = torch.where(k == KIND_BOTH, box, u)
        low = torch.where(k == KIND_LOW, torch.where(u < 0, lo + h, 0.5 * (2 * lo + u + r)), both)
        return torch.where(k == KIND_HIGH, torch.where(u > 0, hi - h, 0.5 * (2 * hi + u - r)), low)

    def dpdu(self, u: torch.Tensor) -> torch.Tensor:
        k, lo, hi, mid, s = self._safe(u)
        r = torch.sqrt(u * u + 4)
        one = torch.ones_like(u)
        hr = 2.0 / (r + u.abs()) / r  # h/r: dp/du on the side towards a one-sided bound
        both = torch.where(k == KIND_BOTH, 1.0 / (1.0 + (u / s) ** 2), one)
        low = torch.where(k == KIND_LOW, torch.where(u < 0, hr, 0.5 * (1 + u / r)), both)
        return torch.where(k == KIND_HIGH, torch.where(u > 0, hr, 0.5 * (1 - u / r)), low)

    def log_dpdu(self, u: torch.Tensor) -> torch.Tensor:
        """``log dp/du``, the log-Jacobian a sampler in ``u`` adds for a flat prior on ``p``.
        Two-sided: ``-log1p((u/s)^2)``.  One-sided, with ``v = u`` for a low and ``v = -u``
        for a high bound: towards the bound (``v < 0``) ``log(h/r)`` with the cancellation-free
        ``h`` of :meth:`dpdu`; away from it ``dp/du = 1 - 2/((r + v) r)`` (the same value as
        ``(1 + v/r)/2``, written so that the logarithm keeps its digits as ``dp/du -> 1``)."""
        k, lo, hi, mid, s = self._safe(u)
        r = torch.sqrt(u * u + 4)
        a = u.abs()
        toward = math.log(2.0) - torch.log(r + a) - torch.log(r)
        away = torch.log1p(-2.0 / ((r + a) * r))
        both = torch.where(k == KIND_BOTH, -torch.log1p((u / s) ** 2), torch.zeros_like(u))
        low = torch.where(k == KIND_LOW, torch.where(u < 0, toward, away), both)
        return torch.where(k == KIND_HIGH, torch.where(u > 0, toward, away), low)

    def dlog_dpdu(self, u: torch.Tensor) -> torch.Tensor:
        """``d/du log dp/du``.  Two-sided: ``-2u/(s^2 + u^2)``.  One-sided (``v`` as in
        :meth:`log_dpdu`): ``d/dv log(h/r) = (r - v)/r^2``, evaluated as ``(r + |v|)/r^2``
        towards the bound and ``4/((r + v) r^2)`` away from it; a high bound flips the sign."""
        k, lo, hi, mid, s = self._safe(u)
        r = torch.sqrt(u * u + 4)
        a = u.abs()
        toward = (r + a) / (r * r)
        away = 4.0 / ((r + a) * r * r)
        both = torch.where(k == KIND_BOTH, -2.0 * u / (s * s + u * u), torch.zeros_like(u))
        low = torch.where(k == KIND_LOW, torch.where(u < 0, toward, away), both)
        return torch.where(k == KIND_HIGH, -torch.where(u > 0, toward, away), low)


def transform(param, bounds):
    """Transform one bounded parameter into its unbounded coordinate."""
    lo, hi = _bound_pair(bounds)
    p = torch.as_tensor(param, dtype=torch.float32) if not isinstance(param, torch.Tensor) else param
    if lo is not None and hi is not None:
        mid, s = (hi + lo) / 2.0, (hi - lo) / math.pi
        return s * torch.tan((p - mid) / s)
    if lo is not None:
        return p - lo + 1.0 / (lo - p)
    if hi is not None:
        return p - hi + 1.0 / (hi - p)
    return p


def inverse_transform(uparam, bounds):
    """Map one unbounded coordinate back into its bounded parameter."""
    lo, hi = _bound_pair(bounds)
    u = torch.as_tensor(uparam, dtype=torch.float32) if not isinstance(uparam, torch.Tensor) else uparam
    if lo is not None and hi is not None:
        mid, s = (hi + lo) / 2.0, (hi - lo) / math.pi
        return torch.clamp(mid + s * torch.atan(u / s), lo, hi)
    # one-sided: towards the bound the distance to it is 2/(sqrt(u^2+4) + |u|) (no cancellation)
    r = torch.sqrt(u ** 2 + 4)
    if lo is not None:
        return torch.where(u < 0, lo + 2.0 / (r - u), 0.5 * (2.0 * lo + u + r))
    if hi is not None:
        return torch.where(u > 0, hi - 2.0 / (r + u), 0.5 * (2.0 * hi + u - r))
    return u


def apply_transforms(params, bounds: Sequence):
    return torch.stack([torch.as_tensor(transform(p, b)) for p, b in zip(params, bounds)])


def apply_inverse_transforms(uparams, bounds: Sequence):
    return torch.stack([torch.as_tensor(inverse_transform(u, b)) for u, b in zip(uparams, bounds)])


def dparams_duparams(uparams: torch.Tensor, bounds: Bounds) -> torch.Tensor:
    """Diagonal of the Jacobian dp/du (the reference's dense ``jax.jacobian``)."""
    return bounds.dpdu(uparams)
