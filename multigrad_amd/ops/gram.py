"""Weighted Gram matrix of a short, wide matrix (``csrc/gram.hip``) with a PyTorch fallback.

``weighted_gram(J, w)`` is ``J diag(w) J^T`` in float64: the ``K x K`` matrix the dual
Gauss-Newton solve (:mod:`multigrad_amd.optim.gauss_newton`) factorises, from one pass over
the ``[K, n]`` Jacobian.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._ext import ext

__all__ = ["weighted_gram", "MAX_ROWS"]

MAX_ROWS = 256


def weighted_gram(J: torch.Tensor, w: Optional[torch.Tensor] = None,
                  nrows: Optional[int] = None) -> torch.Tensor:
    """``out[k, l] = sum_p J[k, p] * w[p] * J[l, p]`` over the first ``nrows`` rows of ``J``
    (default all), as a float64 ``[K, K]`` tensor on ``J``'s device.

    ``J`` is ``[K, n]`` and contiguous with ``1 <= K <= 256``; ``w`` is ``[n]`` or ``None``
    (all ones).  Anything else raises ``ValueError``.

    float32 device tensors run the HIP kernel: operands are converted to float64 before any
    multiply (the product of two float32 is exact), sums are reduced in a fixed order without
    atomics (bitwise reproducible for a fixed ``n`` and device), on the current stream with
    no host synchronisation.  For ``K <= 16`` the kernel streams ``J`` once; larger ``K`` is
    tiled over pairs of 8-row blocks, which re-reads ``J`` once per row block
    (``(ceil(K / 8) + 1) / 2`` passes per row).  Every other dtype or device runs
    ``(J.double() * w.double()) @ J.double().T``.
    """
    if not torch.is_tensor(J) or J.dim() != 2:
        raise ValueError("J must be a 2-d tensor [K, n]")
    if not J.is_contiguous():
        raise ValueError("J must be contiguous")
    K = J.shape[0] if nrows is None else int(nrows)
    if not 1 <= K <= MAX_ROWS or K > J.shape[0]:
        raise ValueError(f"weighted_gram takes 1..{MAX_ROWS} rows of J, got {K} of {J.shape[0]}")
    n = J.shape[1]
    if w is not None:
        if not torch.is_tensor(w) or w.dim() != 1 or w.numel() != n:
            raise ValueError(f"w must be [n] = [{n}], got {tuple(getattr(w, 'shape', ()))}")
        if w.device != J.device:
            raise ValueError("w must be on J's device")
    if J.device.type == "cuda" and J.dtype == torch.float32 and (w is None or w.dtype == torch.float32):
        return ext().weighted_gram(J, None if w is None else w.contiguous(), K)
    Jd = J[:K].double()
    return (Jd if w is None else Jd * w.double()) @ Jd.T
