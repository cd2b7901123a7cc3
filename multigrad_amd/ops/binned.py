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

The op is twice differentiable: the first backward is itself an ``autograd.Function`` of
``(mu, sigma, w, g)`` whose backward (``csrc/binned_hvp.hip`` for float32 device tensors, the
same formulas in chunked torch ops otherwise) is one more recomputing pass.  Third order
raises torch's ``once_differentiable`` error.

The op also has a forward-mode rule (``torch.autograd.forward_ad``): the tangent of the bin
sums is again a binned sum (``csrc/binned_jvp.hip`` for float32 device tensors, the same
formulas in chunked torch ops otherwise), so a tangent costs one pass that writes nothing of
length N.  The first backward has no forward rule (no forward-over-reverse).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from ._binned_common import (_CHUNK, _INV_SQRT_2PI, MAX_BINS, _bcast, _check_operands,
                             _host_edges, _native, _zero_grads)
from ._ext import ext

__all__ = ["gaussian_binned_sum", "MAX_BINS"]


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


def _torch_jvp(mu, sigma, w, edges: Tuple[float, ...], tmu, tsigma, tw, chunk: int):
    """The tangent kernel's formulas (csrc/binned_jvp.hip) in torch ops: with
    z_e = (e_e - mu)/sigma and phi the normal pdf, the edge term of object i is
    E_e = -(1/sigma)(tmu + z_e tsigma) phi(z_e) and
    tout_k = sum_i [w_i (E_{k+1} - E_k) + tw_i dPhi_k].
    A tangent that is None is a zero; a broadcast operand has a one-element tangent."""
    if tmu is None and tsigma is None:  # linear in w: the forward with tw as the weights
        return _torch_forward(mu, sigma, tw, edges, chunk)
    n = mu.numel()
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    out = torch.zeros(len(edges) - 1, dtype=mu.dtype, device=mu.device)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        s = _bcast(sigma, lo, hi)
        z = (e[None, :] - mu[lo:hi, None]) / s[:, None]
        t = None if tmu is None else tmu[lo:hi, None]
        if tsigma is not None:
            zs = z * _bcast(tsigma, lo, hi)[:, None]
            t = zs if t is None else t + zs
        c = -1.0 / s if w is None else -_bcast(w, lo, hi) / s
        E = (c[:, None] * _INV_SQRT_2PI) * torch.exp(-0.5 * z * z) * t
        d = E[:, 1:] - E[:, :-1]
        if tw is not None:
            cdf = torch.special.ndtr(z)
            d = d + (cdf[:, 1:] - cdf[:, :-1]) * _bcast(tw, lo, hi)[:, None]
        out += d.sum(0)
    return out


def _torch_backward2(mu, sigma, w, edges: Tuple[float, ...], g, a, b, c, need, chunk: int):
    """Gradients of sum_i (a_i dmu_i + b_i dsigma_i + c_i dw_i) with respect to (mu, sigma, w,
    g), the kernel's formulas (csrc/binned_hvp.hip) in torch ops: with the moments
    M_n = sum_e h_e z_e^n phi(z_e),
    d/dmu = (w/sigma^2)[-a M1 + b (M0 - M2)] - c M0/sigma,
    d/dsigma = (w/sigma^2)[a (M0 - M2) + b (2 M1 - M3)] - c M1/sigma,
    d/dw = -(a M0 + b M1)/sigma and d/dg_k = T_{k+1} - T_k with
    T_e = sum_i [-(w_i/sigma_i)(a_i + b_i z_ie) phi(z_ie) + c_i Phi(z_ie)].
    A cotangent that is None is a zero; a broadcast operand has a one-element cotangent and
    receives the sum over objects."""
    n = mu.numel()
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    zero = g.new_zeros(1)
    h = torch.cat([zero, g]) - torch.cat([g, zero])
    obj = need[0] or need[1] or need[2]

    def alloc(t):
        return torch.zeros_like(t) if t.numel() == 1 else torch.empty_like(t)

    gmu = torch.empty_like(mu) if need[0] else None
    gsig = alloc(sigma) if need[1] else None
    gw = alloc(w) if need[2] else None
    T = torch.zeros_like(e) if need[3] else None
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        s = _bcast(sigma, lo, hi)
        z = (e[None, :] - mu[lo:hi, None]) / s[:, None]
        phi = torch.exp(-0.5 * z * z) * _INV_SQRT_2PI
        ws = 1.0 / s if w is None else _bcast(w, lo, hi) / s
        ac = None if a is None else a[lo:hi]
        bc = None if b is None else _bcast(b, lo, hi)
        cc = None if c is None else _bcast(c, lo, hi)
        if obj:
            hphi = h[None, :] * phi
            M0 = hphi.sum(1)
            M1 = (hphi * z).sum(1)
            M2 = (hphi * z * z).sum(1)
            dm = torch.zeros_like(M0)
            ds = torch.zeros_like(M0)
            dw = torch.zeros_like(M0)
            if ac is not None:
                dm = dm - ws / s * ac * M1
                ds = ds + ws / s * ac * (M0 - M2)
                dw = dw - ac * M0 / s
            if bc is not None:
                M3 = (hphi * z * z * z).sum(1)
                dm = dm + ws / s * bc * (M0 - M2)
                ds = ds + ws / s * bc * (2.0 * M1 - M3)
                dw = dw - bc * M1 / s
            if cc is not None:
                dm = dm - cc * M0 / s
                ds = ds - cc * M1 / s
            if need[0]:
                gmu[lo:hi] = dm
            for out, val in ((gsig, ds), (gw, dw)):
                if out is None:
                    continue
                if out.numel() == 1:
                    out += val.sum()
                else:
                    out[lo:hi] = val
        if need[3]:
            if ac is not None:
                T -= ((ws * ac)[:, None] * phi).sum(0)
            if bc is not None:
                T -= ((ws * bc)[:, None] * (z * phi)).sum(0)
            if cc is not None:
                T += (torch.broadcast_to(cc, (hi - lo,))[:, None] * torch.special.ndtr(z)).sum(0)
    gg = T[1:] - T[:-1] if need[3] else None
    return gmu, gsig, gw, gg


class _GaussianBinnedSumBackward(torch.autograd.Function):
    """The first backward as a function of (mu, sigma, w, g), so that it can be differentiated
    once more.  All tensors are flat and contiguous; ``need`` selects which of (dmu, dsigma,
    dw) are computed (the others are None)."""

    @staticmethod
    def forward(ctx, mu, sigma, w, g, edges, chunk, need):
        ctx.set_materialize_grads(False)
        ctx.edges, ctx.chunk = edges, chunk
        ctx.save_for_backward(mu, sigma, w, g)
        if mu.numel() == 0:
            grads = _zero_grads((mu, sigma, w), need)
        elif _native(mu):
            grads = ext().binned_backward(mu, sigma, w, list(edges), g, *need)
        else:
            grads = _torch_backward(mu, sigma, w, edges, g, need, chunk)
        return tuple(grads)

    @staticmethod
    @once_differentiable
    def backward(ctx, a, b, c):
        mu, sigma, w, g = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                w is not None and ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        if not any(need) or (a is None and b is None and c is None):
            return (None,) * 7
        if mu.numel() == 0:
            grads = _zero_grads((mu, sigma, w, g), need)
        elif _native(mu):
            a, b, c = (None if t is None else t.contiguous() for t in (a, b, c))
            grads = ext().binned_backward2(mu, sigma, w, list(ctx.edges), g, a, b, c, *need)
        else:
            grads = _torch_backward2(mu, sigma, w, ctx.edges, g, a, b, c, need, ctx.chunk)
        return (*grads, None, None, None)


class _GaussianBinnedSum(torch.autograd.Function):
    """The forward, on flat contiguous operands (gaussian_binned_sum flattens them with
    differentiable views, so that the saved tensors are the caller's graph)."""

    @staticmethod
    def forward(ctx, mu, sigma, w, edges, chunk):
        ctx.edges, ctx.chunk = edges, chunk
        # a missing tangent reaches jvp as None; backward materialises its own zero
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mu, sigma, w)
        ctx.save_for_forward(mu, sigma, w)
        if mu.numel() == 0:
            return mu.new_zeros(len(edges) - 1)
        if _native(mu):
            return ext().binned_forward(mu, sigma, w, list(edges))
        return _torch_forward(mu, sigma, w, edges, chunk)

    @staticmethod
    def jvp(ctx, tmu, tsigma, tw, _edges, _chunk):
        """Forward mode (``torch.autograd.forward_ad``): the tangent of the bin sums is again
        a binned sum, so nothing of length N is written.  A ``None`` tangent is a zero and is
        never materialised."""
        mu, sigma, w = ctx.saved_tensors
        if w is None:
            tw = None
        if mu.numel() == 0 or (tmu is None and tsigma is None and tw is None):
            return mu.new_zeros(len(ctx.edges) - 1)
        if _native(mu):
            tmu, tsigma, tw = (None if t is None else t.reshape(-1).contiguous()
                               for t in (tmu, tsigma, tw))
            return ext().binned_jvp(mu, sigma, w, list(ctx.edges), tmu, tsigma, tw)
        tmu, tsigma, tw = (None if t is None else t.reshape(-1) for t in (tmu, tsigma, tw))
        return _torch_jvp(mu, sigma, w, ctx.edges, tmu, tsigma, tw, ctx.chunk)

    @staticmethod
    def backward(ctx, g):
        mu, sigma, w = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                w is not None and ctx.needs_input_grad[2])
        if not any(need):
            return None, None, None, None, None
        if g is None:
            g = mu.new_zeros(len(ctx.edges) - 1)
        g = g.contiguous().float() if _native(mu) else g.to(mu.dtype)
        dmu, dsigma, dw = _GaussianBinnedSumBackward.apply(mu, sigma, w, g, ctx.edges, ctx.chunk,
                                                           need)
        return dmu, dsigma, dw, None, None


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

    Returns the ``[nb]`` tensor of bin sums in ``mu``'s dtype, differentiable to second order
    (``create_graph=True``, ``torch.autograd.functional.hessian``,
    ``OnePointModel.calc_hvp_from_params``) with respect to ``mu``, ``sigma`` and ``weights``;
    with ``create_graph=False`` the first-order results are bitwise those of the first-order
    kernels alone.  float32 device inputs run the HIP
    kernels (absolute accuracy of the float32 erf: each edge CDF within ~1.6e-7, so a bin is
    within ``2.2e-7 * sum_i |w_i|``; bitwise reproducible; no host sync, graph-capturable);
    every other dtype or device runs chunked torch ops in the input dtype.  Second-order
    outputs of the kernels carry no derived float32 bound; their contract is relative to the
    float32 ``ndtr`` composite under torch's double backward: per output, against float64 on
    the float32-rounded inputs, ``max|op - ref| <= 2 max|composite - ref| + 2e-5 max|ref|``
    (the factor 2 is measured, not derived: profiles/binned_hvp/README.md).

    Forward mode (``torch.autograd.forward_ad``, also under ``torch.no_grad()``): tangents of
    ``mu``, ``sigma`` and ``weights`` (a missing one is a zero, a broadcast operand has a
    one-element tangent) give the tangent ``tout[k] = sum_i (w_i (E_i[k+1] - E_i[k]) +
    tw_i dPhi_i[k])``, ``E_i[e] = -(1/sigma_i) phi(z_e) (tmu_i + z_e tsigma_i)``; the kernel
    is within the first-order gradient contract term by term, ``|t_k - ref_k| <= 2e-4 A_k +
    2e-5 max_k A_k`` with ``A_k`` the sum over objects of the absolute terms.
    """
    if not isinstance(mu, torch.Tensor) or not isinstance(sigma, torch.Tensor):
        raise TypeError("gaussian_binned_sum: mu and sigma must be tensors")
    e = _host_edges(edges)
    _check_operands("gaussian_binned_sum", "mu", mu, (("sigma", sigma), ("weights", weights)))
    if not mu.dtype.is_floating_point:
        raise ValueError("gaussian_binned_sum: floating-point inputs required")
    flat = [None if t is None else t.reshape(-1).contiguous() for t in (mu, sigma, weights)]
    return _GaussianBinnedSum.apply(*flat, e, int(chunk or _CHUNK))
