"""Multi-channel Gaussian-binned sum: several weighted histograms over the same per-object
bin masses -- a stellar-mass function next to a quenched-weighted count and the sum of a
colour or a star-formation rate in the same mass bins.

    out[c, k] = sum_i w_{c,i} * ( Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i) )

Row ``c`` is ``gaussian_binned_sum(mu, sigma, edges, weights[c])``.  ``C`` calls of that op
repeat its dominant cost, the edge CDFs (one ``v_rcp`` + one ``v_exp`` each), ``C`` times in
the forward and in the backward, read ``mu`` and ``sigma`` again and write ``C`` full ``dmu``
/ ``dsigma`` for autograd to add up.  This op evaluates the CDFs once per object and pays
``C`` FMAs per bin on top; ``dmu`` / ``dsigma`` are summed over the channels in registers and
stored once.

float32 device tensors run the gfx950 kernels of ``csrc/binned_multi.hip`` in passes of up
to four channels (``C <= 4``: one forward and one backward launch, plus the fixed-order
reduces).  Every other dtype or device runs the same ``autograd.Function`` in chunked torch
ops: one table ``dPhi[chunk, nb]`` per chunk and ``out += W^T @ dPhi``, peak memory
``O(chunk * (nb + C))``.  With ``h_c[e] = g[c, e-1] - g[c, e]`` (``g[c, -1] = g[c, nb] = 0``),
``H_i[e] = sum_c w_{c,i} h_c[e]``, ``z_e = (e_e - mu_i)/sigma_i`` and ``phi`` the normal pdf,
the analytic backward is

    dmu_i = -(1/sigma_i) sum_e H_i[e] phi(z_e),   dsigma_i = -(1/sigma_i) sum_e H_i[e] z_e phi(z_e),
    dw_{c,i} = sum_k g[c, k] dPhi_i[k],

and a broadcast operand receives the sum over objects.

Accuracy of the kernels against float64 on the float32-rounded inputs (the arithmetic per
channel is that of ``gaussian_binned_sum``): per row and bin
``|out - ref| <= 2.2e-7 * sum_i |w_{c,i}| + 2e-5 * |ref|``; weight gradients rtol 2e-4, atol
``2e-5 * max|ref|``; ``dmu`` / ``dsigma`` are sums over channels whose terms may cancel, so
with ``t_{c,i}`` channel c's contribution and ``A_i = sum_c |t_{c,i}|``,
``|g_i - ref_i| <= 2e-4 * A_i + 2e-5 * max_i A_i`` (for a broadcast sigma with the sums over
i).  The accumulation chain of one ``out[c, k]`` is that of the single op:
``N / (4 * 256 * B)`` quads of four FMAs into one register of a thread (``B`` workgroups, at
most one chip-filling round), a 6-level wave butterfly, 4 wave totals, and the slab
reduction (``ceil(B * NB / 4096) + 2`` row additions and a ``log2(1024 / NB)``-level tree,
``NB`` the bin count padded to 4 / 8 / 16 / 32); no float atomics, bitwise reproducible for a
fixed N, C, shapes and device.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from ._binned_common import (_CHUNK, _INV_SQRT_2PI, MAX_BINS, _bcast, _check_operands,
                             _host_edges, _native, _zero_grads)
from ._ext import ext
from .binned import gaussian_binned_sum

__all__ = ["gaussian_binned_sum_multi", "MAX_CHANNELS", "MAX_BINS"]

MAX_CHANNELS = 8  # kMaxChannels in csrc/binned_multi.hip


def _weight_matrix(ws, lo: int, hi: int, like: torch.Tensor) -> torch.Tensor:
    """The weights of one chunk as [hi - lo, C] (None: ones, one element: broadcast)."""
    cols = []
    for w in ws:
        if w is None:
            cols.append(like.new_ones(hi - lo))
        elif w.numel() == 1:
            cols.append(w.expand(hi - lo))
        else:
            cols.append(w[lo:hi])
    return torch.stack(cols, dim=1)


def _torch_forward(mu, sigma, ws, edges: Tuple[float, ...], chunk: int) -> torch.Tensor:
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    out = torch.zeros(len(ws), len(edges) - 1, dtype=mu.dtype, device=mu.device)
    for lo in range(0, mu.numel(), chunk):
        hi = min(lo + chunk, mu.numel())
        z = (e[None, :] - mu[lo:hi, None]) / _bcast(sigma, lo, hi)[:, None]
        cdf = torch.special.ndtr(z)
        out += _weight_matrix(ws, lo, hi, mu).T @ (cdf[:, 1:] - cdf[:, :-1])
    return out


def _torch_backward(mu, sigma, ws, edges: Tuple[float, ...], g, need_mu, need_sigma, need_w,
                    chunk: int):
    """The kernel's formulas in torch ops (module docstring); returns
    ``[dmu, dsigma, dw_0, ..., dw_{C-1}]`` with ``None`` for what was not asked for."""
    n = mu.numel()
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    zero = g.new_zeros(g.shape[0], 1)
    h = torch.cat([zero, g], dim=1) - torch.cat([g, zero], dim=1)  # [C, nb + 1]

    def grad_like(t):
        return torch.zeros_like(t) if t.numel() == 1 and n != 1 else torch.empty_like(t)

    dmu = torch.empty_like(mu) if need_mu else None
    dsig = grad_like(sigma) if need_sigma else None
    dws = [grad_like(w) if k else None for w, k in zip(ws, need_w)]
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        s = _bcast(sigma, lo, hi)
        z = (e[None, :] - mu[lo:hi, None]) / s[:, None]
        if need_mu or need_sigma:
            H = _weight_matrix(ws, lo, hi, mu) @ h  # [chunk, nb + 1]
            hphi = H * (torch.exp(-0.5 * z * z) * _INV_SQRT_2PI)
            if need_mu:
                dmu[lo:hi] = -hphi.sum(1) / s
            if need_sigma:
                ds = -(hphi * z).sum(1) / s
                if sigma.numel() == 1 and n != 1:
                    dsig += ds.sum()
                else:
                    dsig[lo:hi] = ds
        if any(need_w):
            cdf = torch.special.ndtr(z)
            dW = (cdf[:, 1:] - cdf[:, :-1]) @ g.T  # [chunk, C]
            for c, dw in enumerate(dws):
                if dw is None:
                    continue
                if dw.numel() == 1 and n != 1:
                    dw += dW[:, c].sum()
                else:
                    dw[lo:hi] = dW[:, c]
    return [dmu, dsig] + dws


class _GaussianBinnedSumMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, sigma, edges, chunk, *weights):
        ctx.edges, ctx.chunk = edges, chunk
        ctx.shapes = [mu.shape, sigma.shape] + [None if w is None else w.shape for w in weights]
        mu_f = mu.detach().reshape(-1).contiguous()
        sig_f = sigma.detach().reshape(-1).contiguous()
        ws = [None if w is None else w.detach().reshape(-1).contiguous() for w in weights]
        ctx.has_w = [w is not None for w in ws]
        ctx.save_for_backward(mu_f, sig_f, *[w for w in ws if w is not None])
        if mu_f.numel() == 0:
            return mu_f.new_zeros(len(ws), len(edges) - 1)
        if _native(mu_f):
            return ext().binned_multi_forward(mu_f, sig_f, ws, list(edges))
        return _torch_forward(mu_f, sig_f, ws, edges, chunk)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sigma, *given = ctx.saved_tensors
        given = iter(given)
        ws = [next(given) if has else None for has in ctx.has_w]
        need_mu, need_sigma = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = [w is not None and ctx.needs_input_grad[4 + c] for c, w in enumerate(ws)]
        none = (None,) * (4 + len(ws))
        if not (need_mu or need_sigma or any(need_w)):
            return none
        need = [need_mu, need_sigma] + need_w
        if mu.numel() == 0:
            grads = _zero_grads([mu, sigma] + ws, need)
        elif _native(mu):
            grads = ext().binned_multi_backward(mu, sigma, ws, list(ctx.edges),
                                                g.contiguous().float(), need_mu, need_sigma,
                                                need_w)
        else:
            grads = _torch_backward(mu, sigma, ws, ctx.edges, g.to(mu.dtype), need_mu,
                                    need_sigma, need_w, ctx.chunk)
        out = [None if gr is None else gr.reshape(shp) for gr, shp in zip(grads, ctx.shapes)]
        return (out[0], out[1], None, None) + tuple(out[2:])


def gaussian_binned_sum_multi(mu: torch.Tensor, sigma: torch.Tensor, edges: Sequence[float],
                              weights: Sequence[Optional[torch.Tensor]], *,
                              chunk: Optional[int] = None) -> torch.Tensor:
    """``out[c, k] = sum_i w_{c,i} (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))``.

    Parameters
    ----------
    mu : tensor of any shape (treated as flat), the N per-object means.
    sigma : tensor of N elements, or of one element (broadcast), the Gaussian widths (> 0).
    edges : **host** sequence, numpy array or CPU tensor of ``nb + 1`` strictly increasing
        bin edges, ``1 <= nb <= 32``.  A device tensor raises ``TypeError`` (convert it once
        at setup), as in ``gaussian_binned_sum``.
    weights : list or tuple of ``1 <= C <= 8`` entries, one per channel: ``None`` (weight
        1), a tensor of N elements, or a tensor of one element (broadcast), in ``mu``'s
        dtype and on its device.  Separate tensors, not an ``[N, C]`` tensor: stacking
        per-channel autograd tensors would cost a pass over ``N * C`` floats per step.
    chunk : objects per chunk of the torch path (default 65536); ignored by the kernels.

    Returns the ``[C, nb]`` tensor in ``mu``'s dtype; row ``c`` is the value of
    ``gaussian_binned_sum(mu, sigma, edges, weights[c])``.  Differentiable (first order only;
    second order and a forward-mode rule are offered by ``gaussian_binned_sum``
    alone: under ``torch.autograd.forward_ad`` this op raises torch's ``NotImplementedError``,
    and ``OnePointModel.calc_sumstats_jacobian_from_params`` then works in reverse mode) with
    respect to ``mu``, ``sigma`` and every weight tensor that requires grad; a broadcast
    operand receives the sum over objects, an operand that does not require grad costs no
    store, and a tensor given in several channels gets the sum of its channel gradients.
    ``N == 0`` gives zeros.

    float32 device inputs run the HIP kernels: no host sync, graph-capturable, no float
    atomics, bitwise reproducible.  Accuracy against float64 on the float32-rounded inputs:
    per row and bin ``|out - ref| <= 2.2e-7 * sum_i |w_{c,i}| + 2e-5 * |ref|``; weight
    gradients rtol 2e-4 / atol ``2e-5 * max|ref|``; ``dmu`` and ``dsigma``, whose channel
    terms ``t_{c,i}`` may cancel, ``|g_i - ref_i| <= 2e-4 * A_i + 2e-5 * max_i A_i`` with
    ``A_i = sum_c |t_{c,i}|``.  Every other dtype or device runs chunked torch ops in the
    input dtype.
    """
    name = "gaussian_binned_sum_multi"
    if not isinstance(mu, torch.Tensor) or not isinstance(sigma, torch.Tensor):
        raise TypeError(f"{name}: mu and sigma must be tensors")
    e = _host_edges(edges)
    if isinstance(weights, torch.Tensor) or not isinstance(weights, (list, tuple)):
        raise ValueError(f"{name}: `weights` must be a list or tuple with one entry per "
                         "channel (None or a tensor), not a single tensor")
    C = len(weights)
    if C < 1 or C > MAX_CHANNELS:
        raise ValueError(f"{name}: `weights` needs 1 <= C <= {MAX_CHANNELS} channels, got {C}")
    _check_operands(name, "mu", mu, (("sigma", sigma),))
    for c, w in enumerate(weights):
        if w is None:
            continue
        if not isinstance(w, torch.Tensor):
            raise ValueError(f"{name}: weights[{c}] must be None or a tensor")
        _check_operands(name, "mu", mu, ((f"weights[{c}]", w),))
    if not mu.dtype.is_floating_point:
        raise ValueError(f"{name}: floating-point inputs required")
    if C == 1:
        return gaussian_binned_sum(mu, sigma, e, weights[0], chunk=chunk).unsqueeze(0)
    return _GaussianBinnedSumMulti.apply(mu, sigma, e, int(chunk or _CHUNK), *weights)
