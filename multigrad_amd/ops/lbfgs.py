"""L-BFGS vector ops (``csrc/lbfgs.hip``) with PyTorch fallbacks for CPU tensors."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._ext import ext

__all__ = ["MultiDot", "lincomb_", "lincomb_cols_", "compact_diag_"]


class MultiDot:
    """``out[r, c] = A[r, :n] . B_c[:n]`` for up to 4 right-hand vectors, fp64 results,
    deterministic fixed-order reduction.  Workspace is allocated once."""

    def __init__(self, nrows_max: int, n: int, device):
        self.n = int(n)
        self.device = torch.device(device)
        self.out = torch.zeros(nrows_max * 4, dtype=torch.float64, device=self.device)
        if self.device.type == "cuda":
            ws = ext().multi_dot_workspace(nrows_max, self.n)
            self.ws = torch.zeros(ws, dtype=torch.float64, device=self.device)

    def __call__(self, A: torch.Tensor, nrows: int, B: Sequence[torch.Tensor]) -> torch.Tensor:
        nc = len(B)
        if self.device.type == "cuda":
            ext().multi_dot(A, int(nrows), list(B), self.n, self.out, self.ws)
            return self.out[:nrows * nc].view(nrows, nc)
        Bm = torch.stack([b[:self.n] for b in B]).double()
        res = A[:nrows, :self.n].double() @ Bm.T
        self.out[:nrows * nc] = res.reshape(-1)
        return self.out[:nrows * nc].view(nrows, nc)


def lincomb_(H: torch.Tensor, nrows: int, coef: torch.Tensor, alpha: float,
             x: Optional[torch.Tensor], y: torch.Tensor) -> torch.Tensor:
    """``y = alpha * x + sum_i coef[i] * H[i]`` (one fused pass on the GPU)."""
    n = y.numel()
    if not 0 <= nrows <= 256:
        raise ValueError(f"lincomb_ takes 0..256 rows, got {nrows}")
    if y.device.type == "cuda":
        ext().lincomb(H, int(nrows), coef, float(alpha), x, n, y)
        return y
    acc = torch.zeros(n, dtype=torch.float64)
    if x is not None:
        acc += alpha * x[:n].double()
    if nrows:
        acc += coef[:nrows].double() @ H[:nrows, :n].double()
    y.copy_(acc.to(y.dtype))
    return y


def lincomb_cols_(H: torch.Tensor, nrows: int, coef: torch.Tensor, alpha: float,
                  x: Optional[torch.Tensor], y: torch.Tensor, pre: Optional[torch.Tensor] = None,
                  post: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y[c] = post * (alpha * x[c] * pre + sum_i coef[i, c] * H[i])`` for the ``nc <= 4`` rows
    of ``y`` (``[nc, n]``; ``x`` likewise or ``None``, ``coef`` ``[nrows, nc]``) in one pass over
    the rows of ``H``.  Per element: the ``alpha x`` term first, then rows ``0..nrows-1`` by
    fused multiply-add, so results are bitwise reproducible."""
    nc, n = y.shape
    if not 1 <= nc <= 4:
        raise ValueError(f"lincomb_cols_ takes 1..4 columns, got {nc}")
    if coef.shape != (nrows, nc):
        raise ValueError(f"coef must be [{nrows}, {nc}], got {tuple(coef.shape)}")
    if y.device.type == "cuda":
        ext().lincomb_cols(H, int(nrows), coef.contiguous(), float(alpha), x, pre, post, n, y)
        return y
    acc = torch.zeros((nc, n), dtype=torch.float64)
    if x is not None:
        acc += alpha * x[:, :n].double()
        if pre is not None:
            acc *= pre[:n].double()
    if nrows:
        acc += coef[:nrows].double().T @ H[:nrows, :n].double()
    if post is not None:
        acc *= post[:n].double()
    y.copy_(acc.to(y.dtype))
    return y


def compact_diag_(H: torch.Tensor, rows: torch.Tensor, fac: torch.Tensor, Q: torch.Tensor,
                  h0: float, out: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[j] = (h0 + sum_ab W[a, j] Q[a, b] W[b, j]) * scale[j]**2`` with
    ``W[a] = fac[a] * H[rows[a]]`` (``rows`` int32 ``[k2]``, ``fac`` fp32 ``[k2]``, ``Q`` fp32
    symmetric ``[k2, k2]``, ``k2 <= 240``): the diagonal of a compact L-BFGS matrix."""
    n = out.numel()
    k2 = int(rows.numel())
    if not 1 <= k2 <= 240:
        raise ValueError(f"compact_diag_ takes 1..240 rows, got {k2}")
    if Q.shape != (k2, k2) or fac.numel() != k2:
        raise ValueError("Q must be [k2, k2] and fac [k2]")
    if out.device.type == "cuda":
        ext().compact_diag(H, rows.to(torch.int32).contiguous(), fac.contiguous(), Q.contiguous(),
                           float(h0), scale, n, out)
        return out
    W = H[rows.long(), :n].double() * fac.double()[:, None]
    acc = h0 + ((Q.double() @ W) * W).sum(0)
    if scale is not None:
        acc = acc * scale[:n].double() ** 2
    out.copy_(acc.to(out.dtype))
    return out
