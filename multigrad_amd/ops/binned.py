"""Gaussian-binned sum: a weighted histogram of per-object values, each smeared by a
Gaussian -- the shape of almost every summary statistic fitted with this library (stellar
mass and luminosity functions, any "count objects in bins, differentiably" model).

    out[k] = sum_i w_i * ( Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i) )

``mu``, ``sigma`` and ``weights`` are ordinary autograd tensors produced by arbitrary user
code; the binning is one fused op.  float32 device tensors run the gfx950 kernels of
``csrc/binned.hip`` (forward: per-thread bin accumulators, block sums into a slab, a
fixed-order reduce; backward: one recomputing pass, no residuals, no float atomics, so
results are bitwise reproducible).  Every other dtype or device runs the same
``autograd.Function`` with the forward and the analytic backward written in torch ops,
chunked over objects so that peak memory is ``O(chunk * nb)``.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._ext import ext

__all__ = ["gaussian_binned_sum", "MAX_BINS"]

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


def _torch_forward(mu, sigma, w, edges: Tuple[float, ...], chunk: int) -> torch.Tensor:
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    out = torch.zeros(len(edges) - 1, dtype=mu.dtype, device=mu.device)
    for lo in range(0, mu.numel(), chunk):
        hi = min(lo + chunk, mu.numel())
        z = (e[None, :] - mu[lo:hi, None]) / _bcast(sigma, lo, hi)[:, None]
        cdf = torch.special.ndtr(z)
        d = cdf[:, 1:] - cdf[:, :-1]
        if w is not None:
            d = d * _bcast(w, lo, hi)[:, None]
        out += d.sum(0)
    return out


def _torch_backward(mu, sigma, w, edges: Tuple[float, ...], g, need, chunk: int):
    """The kernel's formulas in torch ops: with z_e = (e_e - mu)/sigma, phi the normal pdf
    and h_e = g_{e-1} - g_e (g_{-1} = g_nb = 0),
    dmu = -(w/sigma) sum_e h_e phi(z_e), dsigma = -(w/sigma) sum_e h_e z_e phi(z_e),
    dw = sum_k g_k dPhi_k; a broadcast operand receives the sum over objects."""
    n = mu.numel()
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    zero = g.new_zeros(1)
    h = torch.cat([zero, g]) - torch.cat([g, zero])
    dmu = torch.empty_like(mu) if need[0] else None
    dsig = (torch.zeros_like(sigma) if sigma.numel() == 1 else torch.empty_like(sigma)) \
        if need[1] else None
    dw = (torch.zeros_like(w) if w.numel() == 1 else torch.empty_like(w)) if need[2] else None
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        s = _bcast(sigma, lo, hi)
        z = (e[None, :] - mu[lo:hi, None]) / s[:, None]
        if need[0] or need[1]:
            hphi = h[None, :] * (torch.exp(-0.5 * z * z) * _INV_SQRT_2PI)
            c = -1.0 / s if w is None else -_bcast(w, lo, hi) / s
            if need[0]:
                dmu[lo:hi] = c * hphi.sum(1)
            if need[1]:
                ds = c * (hphi * z).sum(1)
                if sigma.numel() == 1:
                    dsig += ds.sum()
                else:
                    dsig[lo:hi] = ds
        if need[2]:
            cdf = torch.special.ndtr(z)
            d = ((cdf[:, 1:] - cdf[:, :-1]) * g[None, :]).sum(1)
            if w.numel() == 1:
                dw += d.sum()
            else:
                dw[lo:hi] = d
    return dmu, dsig, dw


def _native(mu: torch.Tensor) -> bool:
    return mu.is_cuda and mu.dtype == torch.float32


class _GaussianBinnedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, w, edges, chunk):
        ctx.edges, ctx.chunk = edges, chunk
        ctx.shapes = (mu.shape, sigma.shape, None if w is None else w.shape)
        mu_f = mu.detach().reshape(-1).contiguous()
        sig_f = sigma.detach().reshape(-1).contiguous()
        w_f = None if w is None else w.detach().reshape(-1).contiguous()
        ctx.save_for_backward(mu_f, sig_f, w_f)
        if mu_f.numel() == 0:
            return mu_f.new_zeros(len(edges) - 1)
        if _native(mu_f):
            return ext().binned_forward(mu_f, sig_f, w_f, list(edges))
        return _torch_forward(mu_f, sig_f, w_f, edges, chunk)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sigma, w = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                w is not None and ctx.needs_input_grad[2])
        if not any(need):
            return None, None, None, None, None
        if mu.numel() == 0:
            grads = [torch.zeros_like(t) if k else None for t, k in zip((mu, sigma, w), need)]
        elif _native(mu):
            grads = ext().binned_backward(mu, sigma, w, list(ctx.edges), g.contiguous().float(),
                                          *need)
        else:
            grads = _torch_backward(mu, sigma, w, ctx.edges, g.to(mu.dtype), need, ctx.chunk)
        out = [None if gr is None else gr.reshape(shp) for gr, shp in zip(grads, ctx.shapes)]
        return out[0], out[1], out[2], None, None


def gaussian_binned_sum(mu: torch.Tensor, sigma: torch.Tensor, edges: Sequence[float],
                        weights: Optional[torch.Tensor] = None, *,
                        chunk: Optional[int] = None) -> torch.Tensor:
    """``out[k] = sum_i w_i (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))``.

    Parameters
    ----------
    mu : tensor of any shape (treated as flat), the N per-object means.
    sigma : tensor of N elements, or of one element (broadcast), the Gaussian widths (> 0).
    edges : **host** sequence, numpy array or CPU tensor of ``nb + 1`` strictly increasing
        bin edges, ``1 <= nb <= 32``.  A device tensor raises ``TypeError``: convert it once
        at setup, since reading it back would synchronise with the host in every step (and
        cannot be captured into a graph).
    weights : optional tensor of N elements or one element (broadcast); ``None`` means 1.
    chunk : objects per chunk of the torch path (default 65536); ignored by the kernels.

    Returns the ``[nb]`` tensor of bin sums in ``mu``'s dtype, differentiable (first order)
    with respect to ``mu``, ``sigma`` and ``weights``.  float32 device inputs run the HIP
    kernels (absolute accuracy of the float32 erf: each edge CDF within ~1.6e-7, so a bin is
    within ``2.2e-7 * sum_i |w_i|``; bitwise reproducible; no host sync, graph-capturable);
    every other dtype or device runs chunked torch ops in the input dtype.
    """
    if not isinstance(mu, torch.Tensor) or not isinstance(sigma, torch.Tensor):
        raise TypeError("gaussian_binned_sum: mu and sigma must be tensors")
    e = _host_edges(edges)
    n = mu.numel()
    if sigma.numel() not in (n, 1):
        raise ValueError(f"gaussian_binned_sum: sigma has {sigma.numel()} elements, "
                         f"expected {n} or 1")
    if weights is not None and weights.numel() not in (n, 1):
        raise ValueError(f"gaussian_binned_sum: weights has {weights.numel()} elements, "
                         f"expected {n} or 1")
    for name, t in (("sigma", sigma), ("weights", weights)):
        if t is not None and (t.dtype != mu.dtype or t.device != mu.device):
            raise ValueError(f"gaussian_binned_sum: {name} must have mu's dtype and device")
    if not mu.dtype.is_floating_point:
        raise ValueError("gaussian_binned_sum: floating-point inputs required")
    return _GaussianBinnedSum.apply(mu, sigma, weights, e, int(chunk or _CHUNK))
