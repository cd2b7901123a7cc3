"""One pass of the box-constrained dual Gauss-Newton solve (``csrc/box_dual.hip``) with a
float64 torch path and a composition of the existing vector ops for what the kernel does not
take.

For ``J`` ``[K, P]``, coefficients ``a`` ``[K]``, the scaling ``d`` ``[P]`` and the step box
``lo <= 0 <= hi`` ``[P]``, with ``t = J^T a``, ``sigma = -t / (lam d)``,
``delta = clip(sigma, lo, hi)`` and ``free = lo < sigma < hi``, a pass returns

    v = J delta,   W = J diag(free / (lam d)) J^T,   s = sum(t delta + lam d delta^2 / 2),
    nfree = sum(free)

as one float64 block ``[v, W, s, nfree]`` of ``K + K*K + 2`` values: what one iteration of the
semismooth Newton solve in :mod:`multigrad_amd.optim.gauss_newton_box` needs from the device.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._ext import ext
from .gram import weighted_gram
from .lbfgs import MultiDot, lincomb_cols_

__all__ = ["box_dual_pass", "box_dual_pass_composed", "vector_loads", "MAX_FUSED_ROWS", "MAX_ROWS"]

MAX_FUSED_ROWS = 10   # largest K the kernel keeps in registers (K = 16 spills to scratch)
MAX_ROWS = 256        # lincomb_cols_ and weighted_gram take up to 256 rows


def _check(J, a, d, lo, hi, delta_out):
    if not torch.is_tensor(J) or J.dim() != 2:
        raise ValueError("J must be a 2-d tensor [K, P]")
    K, P = J.shape
    if not 1 <= K <= MAX_ROWS:
        raise ValueError(f"box_dual_pass takes 1..{MAX_ROWS} rows of J, got {K}")
    if P > 1 and J.stride(1) != 1:
        raise ValueError("J must be row-major (unit column stride)")
    if not torch.is_tensor(a) or a.shape != (K,) or a.dtype != torch.float64:
        raise ValueError(f"a must be a float64 [K] = [{K}] tensor")
    vecs = [("d", d), ("lo", lo), ("hi", hi)]
    if delta_out is not None:
        vecs.append(("delta_out", delta_out))
    for name, t in vecs:
        if not torch.is_tensor(t) or t.shape != (P,) or not t.is_floating_point():
            raise ValueError(f"{name} must be a floating [P] = [{P}] tensor")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    for name, t in [("a", a)] + vecs:
        if t.device != J.device:
            raise ValueError(f"{name} must be on J's device")
    return K, P


def box_dual_pass(J: torch.Tensor, a: torch.Tensor, d: torch.Tensor, lam: float,
                  lo: torch.Tensor, hi: torch.Tensor,
                  delta_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The block ``[v (K), W (K*K), s, nfree]`` (module docstring) as a float64
    ``[K + K*K + 2]`` tensor on ``J``'s device; ``delta`` is written to ``delta_out`` when
    one is given.

    ``J`` is ``[K, P]`` with unit column stride, ``a`` ``[K]`` float64, ``d > 0``, ``lo <= 0``
    and ``hi >= 0`` contiguous ``[P]`` (``+-inf`` sides allowed), ``delta_out`` contiguous
    ``[P]``; everything on one device.  Anything else raises ``ValueError``.

    float32 ``J``, ``d``, ``lo``, ``hi`` (and ``delta_out``) on the GPU with
    ``K <= MAX_FUSED_ROWS`` run the HIP kernel: one pass over ``J``, every per-column
    operation and every sum in float64 (operands converted before the first multiply, the
    sums taken with the unrounded ``delta``), a fixed-order reduction without atomics (bitwise
    reproducible for a fixed ``P`` and device), the current stream and no host
    synchronisation.  Without ``delta_out`` nothing of size ``P`` is allocated or written.
    Every other GPU input (``K > MAX_FUSED_ROWS``, another dtype) is computed by torch in
    float64, a chunk of columns at a time, so that the solve that calls this meets the same
    stop rule on every path; CPU tensors run :func:`box_dual_pass_composed`, float64 there.
    """
    K, _ = _check(J, a, d, lo, hi, delta_out)
    if _fused(J, d, lo, hi, delta_out):
        return ext().box_dual_pass(J, a, d, float(lam), lo, hi, delta_out)
    if J.device.type == "cuda":
        return _float64_pass(J, a, d, float(lam), lo, hi, delta_out)
    return _composed(J, a, d, float(lam), lo, hi, delta_out)


def _fused(J, d, lo, hi, delta_out) -> bool:
    f32 = torch.float32
    return (J.device.type == "cuda" and J.shape[0] <= MAX_FUSED_ROWS and J.dtype == f32
            and d.dtype == f32 and lo.dtype == f32 and hi.dtype == f32
            and (delta_out is None or delta_out.dtype == f32))


def vector_loads(J, d, lo, hi, delta_out=None) -> bool:
    """Whether :func:`box_dual_pass` runs the kernel with 16-byte loads for these tensors
    (``False`` also when it does not run the kernel at all)."""
    return bool(_fused(J, d, lo, hi, delta_out) and J.shape[1]
                and ext().box_dual_vector_loads(J, d, lo, hi, delta_out))


def box_dual_pass_composed(J, a, d, lam, lo, hi, delta_out=None) -> torch.Tensor:
    """:func:`box_dual_pass` from the existing ops: ``lincomb_cols_`` for ``t`` (one pass over
    ``J``), torch ``clamp`` and compares, ``MultiDot`` for ``v`` (a second pass) and
    ``weighted_gram`` with ``w = free / (lam d)`` (a third).  On the CPU every step is
    float64.  On the GPU (float32 ``J``) ``t``, ``sigma`` and ``delta`` are float32 vectors
    and ``MultiDot`` sums float32 lane chains, so the block is accurate to about ``1e-7``
    relative: enough for one step, not for the ``1e-9`` stop rule of the inner solve, which
    is why :func:`box_dual_pass` does not dispatch to it there.  It is the baseline the fused
    pass is measured against.  A device dtype other than float32 takes the float64 path."""
    _check(J, a, d, lo, hi, delta_out)
    if J.device.type == "cuda" and J.dtype != torch.float32:
        return _float64_pass(J, a, d, float(lam), lo, hi, delta_out)
    return _composed(J, a, d, float(lam), lo, hi, delta_out)


_CHUNK = 1 << 20   # columns per step of the float64 path: K * 8 MiB of float64 J alive


def _float64_pass(J, a, d, lam, lo, hi, delta_out):
    K, P = J.shape
    f64 = torch.float64
    v = torch.zeros(K, dtype=f64, device=J.device)
    W = torch.zeros(K, K, dtype=f64, device=J.device)
    s = torch.zeros((), dtype=f64, device=J.device)
    nfree = torch.zeros((), dtype=f64, device=J.device)
    for c0 in range(0, P, _CHUNK):
        c1 = min(P, c0 + _CHUNK)
        Jc = J[:, c0:c1].to(f64)
        ld = lam * d[c0:c1].to(f64)
        lc, hc = lo[c0:c1].to(f64), hi[c0:c1].to(f64)
        t = a @ Jc
        sigma = -t / ld
        delta = torch.minimum(torch.maximum(sigma, lc), hc)
        free = (sigma > lc) & (sigma < hc)
        v += Jc @ delta
        W += (Jc * (free.to(f64) / ld)) @ Jc.T
        s += (delta * (t + 0.5 * ld * delta)).sum()
        nfree += free.sum()
        if delta_out is not None:
            delta_out[c0:c1] = delta
    W = 0.5 * (W + W.T)
    return torch.cat([v, W.reshape(-1), s.reshape(1), nfree.reshape(1)])


_dots: dict = {}


def _multi_dot(K: int, P: int, device) -> MultiDot:
    key = (K, P, str(device))
    if key not in _dots:
        _dots.clear()          # one workspace alive
        _dots[key] = MultiDot(K, P, device)
    return _dots[key]


def _composed(J, a, d, lam, lo, hi, delta_out):
    K, P = J.shape
    dev = J.device
    f64 = torch.float64
    if not P:
        return torch.zeros(K + K * K + 2, dtype=f64, device=dev)
    if not J.is_contiguous():
        J = J.contiguous()
    work = f64 if dev.type != "cuda" else torch.float32
    d, lo, hi = d.to(work), lo.to(work), hi.to(work)
    ld = lam * d
    t = torch.empty(1, P, dtype=work, device=dev)
    lincomb_cols_(J, K, a.to(work).reshape(K, 1), 0.0, None, t)
    t = t[0]
    sigma = -t / ld
    delta = torch.clamp(sigma, min=lo, max=hi)
    free = (sigma > lo) & (sigma < hi)
    w = free.to(work) / ld
    v = _multi_dot(K, P, dev)(J, K, [delta]).reshape(-1).clone()
    W = weighted_gram(J, w)
    td, dd = t.double(), delta.double()
    s = (td * dd + 0.5 * ld.double() * dd * dd).sum()
    if delta_out is not None:
        delta_out.copy_(delta)
    return torch.cat([v.to(f64), W.reshape(-1).to(f64), s.reshape(1),
                      free.sum().reshape(1).to(f64)])
