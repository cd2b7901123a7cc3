"""Two-axis Gaussian-binned sum: a weighted joint histogram of two per-object values, each
smeared by an independent Gaussian -- counts in (stellar mass x colour), (mass x specific
star-formation rate), (magnitude x redshift).

    out[j, k] = sum_i w_i * Px_i[j] * Py_i[k]
    Px_i[j]   = Phi((ex[j+1] - mux_i)/sigx_i) - Phi((ex[j] - mux_i)/sigx_i)      (Py likewise)

It is still a one-point statistic that adds across shards, so it fits ``OnePointModel``
unchanged; the 1-D op cannot express it (a sum of outer products is not a product of sums).
The five operands are ordinary autograd tensors produced by arbitrary user code.  float32
device tensors run the gfx950 kernels of ``csrc/binned2d.hip``; every other dtype or device
runs the same ``autograd.Function`` with the forward (``out += (Px*w)^T @ Py`` per chunk) and
the analytic backward written in torch ops, so that peak memory is ``O(chunk * (nbx + nby))``.

Forward kernel: a workgroup of 256 threads takes tiles of 256 objects; every thread writes
the ``w*Px`` and ``Py`` of one object as a row of LDS, then every thread accumulates a 4x4
register tile of cells over a slice of the rows.  No float atomics: bitwise reproducible for
a fixed N, shape and device.

Summation depth of one cell (the longest chain of rounded float32 additions), with
``C = (NBX/4)*(NBY/4)`` cell tiles of the padded sizes and ``B`` workgroups (at most one
chip-filling round):

* ``256 / (256/C) = C`` products (at most 64) into fresh registers per tile of objects,
* one addition per tile into the workgroup's running total: ``ceil(N / (256 B))``,
* the fold of the ``256/C`` slices: four interleaved chains, ``64/C + 2`` (at most 66),
* the slab reduction: ``ceil(B / (4 * 1024/32)) + 2`` row additions and a 5-level tree.

At ``N = 1e8`` on a 256-CU device that is a few hundred additions per cell instead of the
``N / B ~ 1e5`` of a plain per-thread accumulator.

Backward kernel: per-object parallel, recomputing from the inputs (no residuals).  With the
cotangent ``G[nbx, nby]`` and the unweighted ``Px``, ``Py`` of an object:
``u = G Py``, ``v = G^T Px``, ``dw = Px . u``; with ``hx_e = u[e-1] - u[e]``
(``u[-1] = u[nbx] = 0``), ``z_e = (ex[e] - mux)/sigx`` and ``phi`` the normal pdf,
``dmux = -(w/sigx) sum_e hx_e phi(z_e)`` and ``dsigx = -(w/sigx) sum_e hx_e z_e phi(z_e)``;
the y axis uses ``v`` and ``ey`` in the same way.  This is the 1-D op's backward with the
constant edge weights replaced by per-object ones.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from ._binned_common import (_CHUNK, _INV_SQRT_2PI, MAX_BINS, _bcast, _check_operands,
                             _host_edges, _native, _zero_grads)
from ._ext import ext

__all__ = ["gaussian_binned_sum_2d", "MAX_BINS"]


def _axis(mu, sigma, e, lo, hi):
    """z [n, nb+1] and the unweighted bin probabilities [n, nb] of one chunk."""
    z = (e[None, :] - mu[lo:hi, None]) / _bcast(sigma, lo, hi)[:, None]
    cdf = torch.special.ndtr(z)
    return z, cdf[:, 1:] - cdf[:, :-1]


def _torch_forward(mux, sigx, muy, sigy, w, ex: Tuple[float, ...], ey: Tuple[float, ...],
                   chunk: int) -> torch.Tensor:
    tx = torch.tensor(ex, dtype=mux.dtype, device=mux.device)
    ty = torch.tensor(ey, dtype=mux.dtype, device=mux.device)
    out = torch.zeros(len(ex) - 1, len(ey) - 1, dtype=mux.dtype, device=mux.device)
    for lo in range(0, mux.numel(), chunk):
        hi = min(lo + chunk, mux.numel())
        _, px = _axis(mux, sigx, tx, lo, hi)
        _, py = _axis(muy, sigy, ty, lo, hi)
        if w is not None:
            px = px * _bcast(w, lo, hi)[:, None]
        out += px.t() @ py
    return out


def _edge_sums(h_inner, z):
    """sum_e h_e phi(z_e) and sum_e h_e z_e phi(z_e) with h_e = t[e-1] - t[e], t padded by 0."""
    zero = h_inner.new_zeros(h_inner.shape[0], 1)
    h = torch.cat([zero, h_inner], 1) - torch.cat([h_inner, zero], 1)
    hphi = h * (torch.exp(-0.5 * z * z) * _INV_SQRT_2PI)
    return hphi.sum(1), (hphi * z).sum(1)


def _torch_backward(mux, sigx, muy, sigy, w, ex, ey, g, need, chunk: int):
    """The kernel's formulas (module docstring) in torch ops; a broadcast operand receives the
    sum over objects."""
    n = mux.numel()
    tx = torch.tensor(ex, dtype=mux.dtype, device=mux.device)
    ty = torch.tensor(ey, dtype=mux.dtype, device=mux.device)
    ops = (mux, sigx, muy, sigy, w)
    grads = [None if not k else (torch.zeros_like(t) if t.numel() == 1 and n != 1
                                 else torch.empty_like(t)) for t, k in zip(ops, need)]

    def put(i, val, lo, hi):
        if ops[i].numel() == 1 and n != 1:
            grads[i] += val.sum()
        else:
            grads[i][lo:hi] = val

    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        zx, px = _axis(mux, sigx, tx, lo, hi)
        zy, py = _axis(muy, sigy, ty, lo, hi)
        u = py @ g.t()          # [n, nbx]
        wt = None if w is None else _bcast(w, lo, hi)
        if need[4]:
            put(4, (px * u).sum(1), lo, hi)
        if need[0] or need[1]:
            sx = _bcast(sigx, lo, hi)
            c = -1.0 / sx if wt is None else -wt / sx
            a, b = _edge_sums(u, zx)
            if need[0]:
                put(0, c * a, lo, hi)
            if need[1]:
                put(1, c * b, lo, hi)
        if need[2] or need[3]:
            v = px @ g          # [n, nby]
            sy = _bcast(sigy, lo, hi)
            c = -1.0 / sy if wt is None else -wt / sy
            a, b = _edge_sums(v, zy)
            if need[2]:
                put(2, c * a, lo, hi)
            if need[3]:
                put(3, c * b, lo, hi)
    return grads


class _GaussianBinnedSum2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mux, sigx, muy, sigy, w, ex, ey, chunk):
        ctx.ex, ctx.ey, ctx.chunk = ex, ey, chunk
        ops = (mux, sigx, muy, sigy, w)
        ctx.shapes = tuple(None if t is None else t.shape for t in ops)
        flat = [None if t is None else t.detach().reshape(-1).contiguous() for t in ops]
        ctx.save_for_backward(*flat)
        if flat[0].numel() == 0:
            return flat[0].new_zeros(len(ex) - 1, len(ey) - 1)
        if _native(flat[0]):
            return ext().binned2d_forward(*flat, list(ex), list(ey))
        return _torch_forward(*flat, ex, ey, chunk)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flat = ctx.saved_tensors
        need = [t is not None and ctx.needs_input_grad[i] for i, t in enumerate(flat)]
        if not any(need):
            return (None,) * 8
        mux = flat[0]
        if mux.numel() == 0:
            grads = _zero_grads(flat, need)
        elif _native(mux):
            grads = ext().binned2d_backward(*flat, list(ctx.ex), list(ctx.ey),
                                            g.contiguous().float(), need)
        else:
            grads = _torch_backward(*flat, ctx.ex, ctx.ey, g.to(mux.dtype), need, ctx.chunk)
        out = [None if gr is None else gr.reshape(shp) for gr, shp in zip(grads, ctx.shapes)]
        return (*out, None, None, None)


def gaussian_binned_sum_2d(mu_x: torch.Tensor, sigma_x: torch.Tensor, mu_y: torch.Tensor,
                           sigma_y: torch.Tensor, edges_x: Sequence[float],
                           edges_y: Sequence[float], weights: Optional[torch.Tensor] = None, *,
                           chunk: Optional[int] = None) -> torch.Tensor:
    """``out[j, k] = sum_i w_i Px_i[j] Py_i[k]``, the joint Gaussian-smeared histogram.

    Parameters
    ----------
    mu_x, mu_y : tensors of N elements each, of any shape (treated as flat).
    sigma_x, sigma_y : tensors of N elements, or of one element (broadcast), the widths (> 0).
    edges_x, edges_y : **host** sequences, numpy arrays or CPU tensors of ``nbx + 1`` and
        ``nby + 1`` strictly increasing finite edges, ``1 <= nbx, nby <= 32``.  A device
        tensor raises ``TypeError``, as in :func:`~multigrad_amd.ops.binned.gaussian_binned_sum`.
    weights : optional tensor of N elements or one element (broadcast); ``None`` means 1.
    chunk : objects per chunk of the torch path (default 65536); ignored by the kernels.

    Returns the ``[nbx, nby]`` tensor of cell sums in ``mu_x``'s dtype, differentiable (first
    order only; second order and a forward-mode rule are offered by ``gaussian_binned_sum``
    alone: under ``torch.autograd.forward_ad`` this op raises torch's ``NotImplementedError``,
    and ``OnePointModel.calc_sumstats_jacobian_from_params`` then works in reverse mode) with
    respect to each
    of the five tensor operands; a broadcast operand receives the sum over objects.  float32 device inputs run the HIP kernels: no host synchronisation,
    launches on the current stream (graph-capturable), bitwise reproducible, and per cell
    ``|out - exact| <= 4.4e-7 * sum_i |w_i| + 2e-5 * |exact|`` (both factors of a cell carry
    the 2.2e-7 absolute error of the float32 Phi difference; the second term is float32
    accumulation).  Every other dtype or device runs chunked torch ops in the input dtype.
    """
    ops = (("mu_x", mu_x), ("sigma_x", sigma_x), ("mu_y", mu_y), ("sigma_y", sigma_y))
    for name, t in ops:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"gaussian_binned_sum_2d: {name} must be a tensor")
    ex = _host_edges(edges_x)
    ey = _host_edges(edges_y)
    n = mu_x.numel()
    if mu_y.numel() != n:
        raise ValueError(f"gaussian_binned_sum_2d: mu_y has {mu_y.numel()} elements, expected {n}")
    _check_operands("gaussian_binned_sum_2d", "mu_x", mu_x, ops[1:] + (("weights", weights),))
    if not mu_x.dtype.is_floating_point:
        raise ValueError("gaussian_binned_sum_2d: floating-point inputs required")
    return _GaussianBinnedSum2d.apply(mu_x, sigma_x, mu_y, sigma_y, weights, ex, ey,
                                      int(chunk or _CHUNK))
