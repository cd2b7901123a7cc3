"""Per-group Gaussian-binned sum: the same smeared histogram once per sample -- a stellar-mass
function per redshift slice or survey field, a conditional mass function per host-mass bin, a
richness function per cluster.

    out[g, k] = sum_{i : index_i = g} w_i * ( Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i) )

    plan = GroupIndex(index, num_groups)                      # once, at setup
    smf = plan.binned_sum(mu, sigma, edges, weights)          # [num_groups, nb]

``G`` calls of ``gaussian_binned_sum`` cost ``G`` launches and ``G`` full-length gradients;
the ``ndtr`` table followed by ``plan.segment_sum`` writes and re-reads ``N * nb`` floats.
This op fuses the binning into the reduce-by-key of the plan.

float32 device tensors on a plan of ``N < 2**31`` objects run the gfx950 kernels of
``csrc/binned_group.hip``.  The forward works over the plan's sorted positions (operands read
through ``perm`` when the plan has one): one workgroup per chunk of 1024 positions, four per
thread; the run structure of a chunk is computed once from the keys, then the edges are walked
and every bin's four ``w * dPhi`` values go through one segmented scan (thread, 64 lanes, wave
aggregates in LDS).  Runs inside a chunk are stored to ``out[g, k]``, runs that cross a chunk
edge leave partials in two carry slots per chunk, and the carry list is reduced by the same
kernel, level after level, until one chunk remains.  On the objects' level, where the keys are
sorted, a full chunk whose first and last key are equal holds one key and skips the scan; the
carry lists have unused slots between their keys and always take the scan.
The backward runs per object in the original order, recomputes from the inputs (no residuals)
and reads the cotangent row of object ``i`` through ``ids[i]``:

    dmu_i = -(w_i/sigma_i) sum_e h[g_i, e] phi(z_ie),   dsigma_i = -(w_i/sigma_i) sum_e h[g_i, e] z_ie phi(z_ie),
    dw_i = sum_k G[g_i, k] dPhi_ik,                     h[g, e] = G[g, e-1] - G[g, e]  (G[g, -1] = G[g, nb] = 0)

and a broadcast operand receives the sum over objects (block sum, slab, fixed-order reduce).
No float atomics, no data-dependent order (bitwise reproducible for a fixed plan, shapes and
device), no host synchronisation, launches on the current stream (graph-capturable).

Every other dtype or device, and plans of ``N >= 2**31``, run the same ``autograd.Function``
in chunked torch ops: a ``dPhi[chunk, nb]`` table per chunk and
``out.index_add_(0, ids[lo:hi], w * dPhi)``; peak memory ``O(chunk * nb)``.

Summation order of the kernels: the longest chain of rounded additions to ``out[g, k]`` for a
group of ``L`` objects is that of ``segment_sum``, ``summation_depth(L) <= 4 + 2 *
ceil(log2(max(L, 2)))`` (:func:`multigrad_amd.ops.groups.summation_depth`; a single-key chunk
takes 2 + 6 + 2 = 10 additions, fewer than the 13 of the scan it replaces), after one rounded
product ``w_i * dPhi_ik`` per term.  Accuracy against float64 on the float32-rounded inputs and
edges, per group and bin:

    |out[g, k] - ref| <= 3.2e-7 * W_g + 2e-5 * A_gk,   W_g = sum_{i in g} |w_i|,   A_gk = sum_{i in g} |w_i| dPhi_ik

(3.2e-7: two edge CDFs at their 1.6e-7 absolute class, a worst case since a group may hold one
object; the second term covers the accumulation, ``(depth + 1) * 2**-24 * A_gk`` with the
depth far below 335).  Gradients: per element rtol 2e-4 plus atol ``2e-5 * max|ref|``; for a
reduced (broadcast) gradient ``|g - ref| <= 2e-4 * sum_i |t_i| + 2e-5 * max_i |t_i|`` with
``t_i`` the per-object terms.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from ._binned_common import (_CHUNK, _INV_SQRT_2PI, MAX_BINS, _bcast, _check_operands,
                             _host_edges, _zero_grads)
from ._ext import ext
from .groups import GroupIndex

__all__ = ["gaussian_binned_sum_by_group", "MAX_BINS"]


def _torch_forward(plan, mu, sigma, w, edges: Tuple[float, ...], chunk: int) -> torch.Tensor:
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    out = torch.zeros(plan.num_groups, len(edges) - 1, dtype=mu.dtype, device=mu.device)
    for lo in range(0, mu.numel(), chunk):
        hi = min(lo + chunk, mu.numel())
        z = (e[None, :] - mu[lo:hi, None]) / _bcast(sigma, lo, hi)[:, None]
        cdf = torch.special.ndtr(z)
        d = cdf[:, 1:] - cdf[:, :-1]
        if w is not None:
            d = d * _bcast(w, lo, hi)[:, None]
        out.index_add_(0, plan.ids[lo:hi], d)
    return out


def _torch_backward(plan, mu, sigma, w, edges: Tuple[float, ...], g, need, chunk: int):
    """The kernel's formulas in torch ops (module docstring), with the cotangent row of object
    i taken from row ``ids[i]`` of ``g``; a broadcast operand receives the sum over objects."""
    n = mu.numel()
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    zero = g.new_zeros(g.shape[0], 1)
    h = torch.cat([zero, g], dim=1) - torch.cat([g, zero], dim=1)  # [G, nb + 1]
    dmu = torch.empty_like(mu) if need[0] else None
    dsig = (torch.zeros_like(sigma) if sigma.numel() == 1 else torch.empty_like(sigma)) \
        if need[1] else None
    dw = (torch.zeros_like(w) if w.numel() == 1 else torch.empty_like(w)) if need[2] else None
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        ids = plan.ids[lo:hi]
        s = _bcast(sigma, lo, hi)
        z = (e[None, :] - mu[lo:hi, None]) / s[:, None]
        if need[0] or need[1]:
            hphi = torch.index_select(h, 0, ids) * (torch.exp(-0.5 * z * z) * _INV_SQRT_2PI)
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
            d = ((cdf[:, 1:] - cdf[:, :-1]) * torch.index_select(g, 0, ids)).sum(1)
            if w.numel() == 1:
                dw += d.sum()
            else:
                dw[lo:hi] = d
    return dmu, dsig, dw


class _GaussianBinnedSumByGroup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, mu, sigma, w, edges, chunk):
        ctx.plan, ctx.edges, ctx.chunk = plan, edges, chunk
        ctx.shapes = [mu.shape, sigma.shape, None if w is None else w.shape]
        mu_f = mu.detach().reshape(-1).contiguous()
        sig_f = sigma.detach().reshape(-1).contiguous()
        w_f = None if w is None else w.detach().reshape(-1).contiguous()
        ctx.has_w = w_f is not None
        ctx.save_for_backward(mu_f, sig_f, *([w_f] if ctx.has_w else []))
        nb = len(edges) - 1
        if mu_f.numel() == 0 or plan.num_groups == 0:
            return mu_f.new_zeros(plan.num_groups, nb)
        if plan._native(mu_f):
            return ext().binned_group_forward(plan.sorted_ids, plan.perm, mu_f, sig_f, w_f,
                                              list(edges), plan.num_groups)
        return _torch_forward(plan, mu_f, sig_f, w_f, edges, chunk)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sigma, *rest = ctx.saved_tensors
        w = rest[0] if ctx.has_w else None
        plan = ctx.plan
        need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2],
                w is not None and ctx.needs_input_grad[3])
        none = (None,) * 6
        if not any(need):
            return none
        if mu.numel() == 0:
            grads = _zero_grads((mu, sigma, w), need)
        elif plan._native(mu):
            grads = ext().binned_group_backward(plan.ids, mu, sigma, w, list(ctx.edges),
                                                g.contiguous().float(), *need)
        else:
            grads = _torch_backward(plan, mu, sigma, w, ctx.edges, g.to(mu.dtype), need,
                                    ctx.chunk)
        out = [None if gr is None else gr.reshape(shp) for gr, shp in zip(grads, ctx.shapes)]
        return (None, out[0], out[1], out[2], None, None)


def gaussian_binned_sum_by_group(plan: GroupIndex, mu: torch.Tensor, sigma: torch.Tensor,
                                 edges: Sequence[float],
                                 weights: Optional[torch.Tensor] = None, *,
                                 chunk: Optional[int] = None) -> torch.Tensor:
    """``out[g, k] = sum_{i in g} w_i (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))``.

    Parameters
    ----------
    plan : :class:`~multigrad_amd.ops.groups.GroupIndex`, the group of each of N objects.
    mu : tensor of ``plan.n`` elements, any shape (treated as flat), the per-object means.
    sigma : tensor of ``plan.n`` elements, or of one element (broadcast), the widths (> 0).
    edges : **host** sequence, numpy array or CPU tensor of ``nb + 1`` strictly increasing
        bin edges, ``1 <= nb <= 32``.  A device tensor raises ``TypeError`` (convert it once
        at setup), as in ``gaussian_binned_sum``.
    weights : optional tensor of ``plan.n`` elements or one element (broadcast); ``None``
        means 1.
    chunk : objects per chunk of the torch path (default 65536); ignored by the kernels.

    All tensors share one floating dtype and live on the plan's device; non-contiguous inputs
    are copied.  Returns the ``[plan.num_groups, nb]`` tensor in ``mu``'s dtype; row ``g`` is
    the value of ``gaussian_binned_sum`` over the objects of group ``g``, and a group without
    objects is exactly 0 (``N == 0`` gives zeros, ``num_groups == 0`` a ``[0, nb]`` tensor).

    Differentiable (first order only; second order and a forward-mode rule are offered by
    ``gaussian_binned_sum`` alone: a second-order request raises torch's
    ``once_differentiable`` error, and under ``torch.autograd.forward_ad`` this op raises
    torch's ``NotImplementedError``, which
    ``OnePointModel.calc_sumstats_jacobian_from_params(mode="auto")`` answers with reverse
    mode) with respect to ``mu``, ``sigma`` and ``weights``; a broadcast operand receives the
    sum over objects and an operand that does not require grad costs no store.

    float32 device inputs on a plan of ``N < 2**31`` run the HIP kernels: no host sync,
    graph-capturable, no float atomics, bitwise reproducible for a fixed plan.  Accuracy
    against float64 on the float32-rounded inputs: per group and bin
    ``|out[g, k] - ref| <= 3.2e-7 * W_g + 2e-5 * A_gk`` with ``W_g = sum_{i in g} |w_i|`` (a
    one-element weight counts ``L_g * |w|``) and ``A_gk = sum_{i in g} |w_i| dPhi_ik``;
    gradients per element rtol 2e-4 plus atol ``2e-5 * max|ref|``, a reduced (broadcast)
    gradient ``|g - ref| <= 2e-4 * sum_i |t_i| + 2e-5 * max_i |t_i|`` with ``t_i`` the
    per-object terms.  Every other dtype or device runs chunked torch ops in the input dtype.
    """
    name = "gaussian_binned_sum_by_group"
    if not isinstance(plan, GroupIndex):
        raise TypeError(f"{name}: `plan` must be a GroupIndex")
    if not isinstance(mu, torch.Tensor) or not isinstance(sigma, torch.Tensor):
        raise TypeError(f"{name}: mu and sigma must be tensors")
    if weights is not None and not isinstance(weights, torch.Tensor):
        raise TypeError(f"{name}: weights must be None or a tensor")
    e = _host_edges(edges)
    n = plan.n
    if mu.numel() != n:
        raise ValueError(f"{name}: mu has {mu.numel()} elements, expected {n} (the plan's N)")
    if not mu.dtype.is_floating_point:
        raise ValueError(f"{name}: mu must be a floating-point tensor")
    for operand in (("sigma", sigma), ("weights", weights)):
        _check_operands(name, "mu", mu, (operand,))
    if mu.device != plan.device:
        raise ValueError(f"{name}: operands live on {mu.device}, the plan on {plan.device}; "
                         f"build the GroupIndex from an index on the operands' device")
    return _GaussianBinnedSumByGroup.apply(plan, mu, sigma, weights, e, int(chunk or _CHUNK))
