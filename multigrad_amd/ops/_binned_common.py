"""Helpers shared by the Gaussian-binned-sum ops (``binned.py``, ``binned2d.py``,
``binned_multi.py``, ``binned_group.py``, ``binned_fine.py``): constants, host-edge validation,
operand checks and the pieces of the chunked torch paths."""
from __future__ import annotations

import math
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_BINS = 32  # kMaxBins in csrc/smf_device.h
_CHUNK = 1 << 16  # objects per chunk of the torch path
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def _host_edges(edges) -> Tuple[float, ...]:
    if isinstance(edges, torch.Tensor):
        if edges.device.type != "cpu":
            raise TypeError(
                "gaussian_binned_sum: `edges` must live on the host (a sequence, a numpy array "
                "or a CPU tensor); convert a device tensor once at setup (tuple(edges.tolist())) "
                "-- reading it back on every call would be a host sync inside a captured step")
        edges = edges.detach().double().numpy()
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    nb = e.size - 1
    if nb < 1 or nb > MAX_BINS:
        raise ValueError(f"gaussian_binned_sum: need 1 <= nb <= {MAX_BINS} bins, got {nb}")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("gaussian_binned_sum: `edges` must be finite and strictly increasing")
    return tuple(float(v) for v in e)


def _bcast(t: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    return t if t.numel() == 1 else t[lo:hi]


def _native(mu: torch.Tensor) -> bool:
    return mu.is_cuda and mu.dtype == torch.float32


def _check_operands(op_name: str, ref_name: str, ref: torch.Tensor,
                    named: Iterable[Tuple[str, Optional[torch.Tensor]]]) -> None:
    """Every tensor of ``named`` (``None`` entries are skipped) has ``ref.numel()`` elements or
    one, and ``ref``'s dtype and device.  All element counts are checked before any dtype; a
    caller that wants one operand checked in full before the next calls once per operand."""
    named = [(label, t) for label, t in named if t is not None]
    n = ref.numel()
    for label, t in named:
        if t.numel() not in (n, 1):
            raise ValueError(f"{op_name}: {label} has {t.numel()} elements, expected {n} or 1")
    for label, t in named:
        if t.dtype != ref.dtype or t.device != ref.device:
            raise ValueError(f"{op_name}: {label} must have {ref_name}'s dtype and device")


def _zero_grads(tensors: Sequence[Optional[torch.Tensor]], need: Sequence[bool]):
    """The gradients of an empty input: zeros for the requested operands, ``None`` otherwise."""
    return [torch.zeros_like(t) if k else None for t, k in zip(tensors, need)]
