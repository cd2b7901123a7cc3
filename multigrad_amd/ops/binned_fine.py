"""Gaussian-binned sum over many fine bins, up to 4096: a photometric-redshift distribution, a
colour or magnitude distribution at 0.05 mag, a luminosity function over ten magnitudes, a
finely binned mass function that is merged later under several binnings.

    out[k] = sum_i w_i * ( Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i) )

    bins = FineBins(edges, device)                     # once, at setup
    nz = bins.sum(mu, sigma, weights)                  # [nb]

``gaussian_binned_sum`` and its variants stop at 32 bins: they keep one accumulator per bin in
registers and evaluate every edge for every object.  With fine bins an object of width sigma
reaches only the bins within a few sigma of its mean, and this op's cost follows those bins.

``nb <= 32`` calls ``gaussian_binned_sum`` with the plan's host edges (bitwise the single op).
For ``33 <= nb <= 4096`` float32 device tensors run the gfx950 kernels of
``csrc/binned_fine.hip``:

* Window.  Object ``i`` contributes to the bins that overlap ``(mu_i - T sigma_i, mu_i +
  T sigma_i)``, ``T = 5.5``; the first and last such bin are found by binary search over the
  edges in LDS and are evaluated at their true edges.  Bins wholly outside get nothing: per
  object and side at most ``Phi(-5.5) = 1.9e-8`` of the weight is dropped.
* Forward.  A scatter to data-dependent bins has no fixed float summation order, so every term
  ``t = w_i dPhi_ik`` is rounded once to float32 and then accumulated exactly as a 64-bit
  fixed-point integer ``q = rint(t 2^s)``, ``s = 30 - e`` with ``max_i |w_i| = m 2^e``,
  ``m in [0.5, 1)``: an int64 histogram per workgroup in LDS, 64-bit integer atomics into a
  zero-filled device buffer, and a last kernel ``out[k] = float(double(acc[k]) 2^-s)``.
  Integer addition is associative, so the result is bitwise independent of arrival order, of
  the grid and of the order of the objects.  ``max |w|`` comes from a max-reduction kernel and
  stays on the device; no weights or a one-element weight skip it (``dPhi`` is accumulated at
  ``s = 30`` and the last kernel multiplies by ``w``).  A non-finite weight or term, or a NaN
  ``mu`` or ``sigma``, makes every bin NaN.  When a quarter of a wave's lanes start at the same
  bin (wide objects), windows of 8 bins or more are walked cyclically from a start spread over
  the window by lane, so that the wave's adds go to different LDS addresses; the order does not
  change the integer sums.
* Backward.  Per object in the original order, recomputing from the inputs (no residuals), the
  cotangent and the edges in LDS, over the edges of the window only:
  ``dmu = -(w/sigma) sum_e h_e phi(z_e)``, ``dsigma = -(w/sigma) sum_e h_e z_e phi(z_e)``,
  ``dw = sum_k g_k dPhi_k``, ``h_e = g_{e-1} - g_e``; the dropped edge terms carry at most
  ``phi(5.5) = 1.1e-7`` of a central term.  A broadcast operand receives the sum over objects
  (block sum, slab, fixed-order reduce).

No float atomics, no host synchronisation, launches on the current stream (graph-capturable).
Every other dtype or device runs the same ``autograd.Function`` in chunked torch ops: the dense
``dPhi[chunk, nb]`` table without truncation and the analytic backward of
``ops/binned.py``; the default chunk keeps ``chunk * nb <= 2**21`` elements.

Accuracy of the kernels against float64 on the float32-rounded inputs and edges, untruncated.
With ``W_k`` the sum of ``|w_i|`` over the objects whose window reaches bin ``k``, ``n_k`` their
number, ``A_k = sum_i |w_i| dPhi_ik`` and ``W = sum_i |w_i|``:

    |out[k] - ref[k]| <= 3.2e-7 W_k + 1e-6 A_k + 2^-30 max|w| n_k + 2e-8 (W - W_k)

(two edge CDFs at their 1.6e-7 class; a few float32 roundings of the term and the result; the
fixed-point rounding; the truncation).  Gradients: per element rtol 2e-4 plus atol
``2e-5 * max|ref|``; a reduced (broadcast) gradient within ``2e-4 * sum_i |t_i| + 2e-5 *
max_i |t_i|`` with ``t_i`` the per-object terms.  Known weakness: the fixed-point grid is set by
the largest weight, so a weight far below ``max |w|`` is resolved only to ``2^-30 max |w|``.

Which to call (profiles/binned_fine/README.md has the measurements, forward + backward on one
MI355X against ``ceil(nb / 32)`` calls of ``gaussian_binned_sum`` on 33-edge slices): with sigma
up to 2 bin widths the op is 6-14 times faster at 256 bins and 73-148 times at 4096, at 8 widths
2 and 25 times; at 64 bins it wins 1.5-3.5 times up to 2 widths and loses at 8 widths (0.6-0.7),
where a window covers every bin.  The crossover is a window of about half the bins,
``11 sigma = 0.5 (e[nb] - e[0])``: where sigma spans more of the range than that, every object
reaches most bins and the slices do the same work without the searches and the LDS histogram.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ._binned_common import _CHUNK, MAX_BINS, _check_operands, _native, _zero_grads
from ._ext import ext
from .binned import _torch_backward, _torch_forward, gaussian_binned_sum

__all__ = ["FineBins", "gaussian_binned_sum_fine", "MAX_FINE_BINS"]

MAX_FINE_BINS = 4096  # kFineMaxBins in csrc/binned_fine.hip
_TABLE = 1 << 21  # elements of the dPhi table of one chunk of the torch path


def _fine_edges(edges) -> Tuple[float, ...]:
    if isinstance(edges, torch.Tensor):
        if edges.device.type != "cpu":
            raise TypeError(
                "FineBins: `edges` must live on the host (a sequence, a numpy array "
                "or a CPU tensor); convert a device tensor once at setup (tuple(edges.tolist())) "
                "-- reading it back on every call would be a host sync inside a captured step")
        edges = edges.detach().double().numpy()
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    nb = e.size - 1
    if nb < 1 or nb > MAX_FINE_BINS:
        raise ValueError(f"FineBins: need 1 <= nb <= {MAX_FINE_BINS} bins, got {nb}")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("FineBins: `edges` must be finite and strictly increasing")
    return tuple(float(v) for v in e)


class FineBins:
    """The plan of :func:`gaussian_binned_sum_fine`, built once at setup.

    ``edges`` is a **host** sequence, numpy array or CPU tensor of ``nb + 1`` finite, strictly
    increasing values, ``1 <= nb <= 4096`` (``ValueError`` otherwise; a device tensor raises
    ``TypeError``).  Construction is the only place that touches the host: it validates, keeps
    the host tuple (``edges``) and puts a float32 copy on ``device`` (``edges_dev``), which the
    kernels read.  Attributes: ``nb``, ``edges``, ``edges_dev``, ``device``.
    """

    def __init__(self, edges, device=None):
        self.edges = _fine_edges(edges)
        self.nb = len(self.edges) - 1
        self.device = torch.empty(0, device=device).device  # "cuda" -> the current device
        self.edges_dev = torch.tensor(self.edges, dtype=torch.float32, device=self.device)

    def sum(self, mu, sigma, weights=None, *, chunk=None):
        """``gaussian_binned_sum_fine(self, mu, sigma, weights, chunk=chunk)``."""
        return gaussian_binned_sum_fine(self, mu, sigma, weights, chunk=chunk)

    def __repr__(self):
        return (f"FineBins(nb={self.nb}, range=({self.edges[0]:g}, {self.edges[-1]:g}), "
                f"device={self.device})")


class _GaussianBinnedSumFine(torch.autograd.Function):
    """On flat contiguous operands; 33 <= nb <= 4096."""

    @staticmethod
    def forward(ctx, bins, mu, sigma, w, chunk):
        ctx.bins, ctx.chunk = bins, chunk
        ctx.has_w = w is not None
        ctx.save_for_backward(mu, sigma, *([w] if ctx.has_w else []))
        if mu.numel() == 0:
            return mu.new_zeros(bins.nb)
        if _native(mu):
            return ext().binned_fine_forward(mu, sigma, w, bins.edges_dev)
        return _torch_forward(mu, sigma, w, bins.edges, chunk)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sigma, *rest = ctx.saved_tensors
        w = rest[0] if ctx.has_w else None
        need = (ctx.needs_input_grad[1], ctx.needs_input_grad[2],
                w is not None and ctx.needs_input_grad[3])
        if not any(need):
            return (None,) * 5
        if mu.numel() == 0:
            grads = _zero_grads((mu, sigma, w), need)
        elif _native(mu):
            grads = ext().binned_fine_backward(mu, sigma, w, ctx.bins.edges_dev,
                                               g.contiguous().float(), *need)
        else:
            grads = _torch_backward(mu, sigma, w, ctx.bins.edges, g.to(mu.dtype), need, ctx.chunk)
        return (None, grads[0], grads[1], grads[2], None)


def gaussian_binned_sum_fine(bins: FineBins, mu: torch.Tensor, sigma: torch.Tensor,
                             weights: Optional[torch.Tensor] = None, *,
                             chunk: Optional[int] = None) -> torch.Tensor:
    """``out[k] = sum_i w_i (Phi((e[k+1] - mu_i)/sigma_i) - Phi((e[k] - mu_i)/sigma_i))`` over the
    ``nb <= 4096`` bins of a :class:`FineBins` plan; also ``bins.sum(mu, sigma, weights)``.

    Parameters
    ----------
    bins : :class:`FineBins`, built once at setup from host edges.
    mu : tensor of any shape (treated as flat), the N per-object means.
    sigma : tensor of N elements, or of one element (broadcast), the Gaussian widths (> 0).
    weights : optional tensor of N elements or one element (broadcast); ``None`` means 1.
    chunk : objects per chunk of the torch path (default: ``2**21 // nb``, at most 65536, so
        that the ``dPhi`` table of a chunk stays at a few tens of MB); ignored by the kernels.

    All tensors share one floating dtype and live on the plan's device; non-contiguous inputs
    are copied.  Returns the ``[nb]`` tensor in ``mu``'s dtype (``N == 0`` gives zeros).

    Differentiable (first order only: a second-order request raises torch's
    ``once_differentiable`` error, and under ``torch.autograd.forward_ad`` the op raises
    torch's ``NotImplementedError``, which
    ``OnePointModel.calc_sumstats_jacobian_from_params(mode="auto")`` answers with reverse
    mode) with respect to ``mu``, ``sigma`` and ``weights``; a broadcast operand receives the
    sum over objects and an operand that does not require grad costs no store.

    ``nb <= 32`` is ``gaussian_binned_sum`` on the plan's host edges, bitwise.  For
    ``33 <= nb <= 4096`` float32 device inputs run the HIP kernels: an object visits only the
    bins within 5.5 sigma of its mean, the forward accumulates exact 64-bit fixed-point
    integers (bitwise reproducible and independent of the order of the objects), no host sync,
    graph-capturable.  Accuracy against float64 on the float32-rounded inputs and edges:
    ``|out[k] - ref[k]| <= 3.2e-7 W_k + 1e-6 A_k + 2^-30 max|w| n_k + 2e-8 (W - W_k)`` with
    ``W_k`` / ``n_k`` the summed ``|w_i|`` / the number of the objects whose window reaches bin
    ``k``, ``A_k = sum_i |w_i| dPhi_ik`` and ``W = sum_i |w_i|``; gradients per element rtol
    2e-4 plus atol ``2e-5 * max|ref|``, a reduced (broadcast) gradient
    ``|g - ref| <= 2e-4 * sum_i |t_i| + 2e-5 * max_i |t_i|``.  A weight far below ``max |w|`` is
    resolved only to ``2^-30 max |w|``.  Every other dtype or device runs chunked torch ops in
    the input dtype, untruncated.  Where sigma spans a large part of the range, calls of
    ``gaussian_binned_sum`` on 33-edge slices are the better choice (module docstring).
    """
    name = "gaussian_binned_sum_fine"
    if not isinstance(bins, FineBins):
        raise TypeError(f"{name}: `bins` must be a FineBins")
    if not isinstance(mu, torch.Tensor) or not isinstance(sigma, torch.Tensor):
        raise TypeError(f"{name}: mu and sigma must be tensors")
    if weights is not None and not isinstance(weights, torch.Tensor):
        raise TypeError(f"{name}: weights must be None or a tensor")
    if not mu.dtype.is_floating_point:
        raise ValueError(f"{name}: mu must be a floating-point tensor")
    for operand in (("sigma", sigma), ("weights", weights)):
        _check_operands(name, "mu", mu, (operand,))
    if mu.device != bins.device:
        raise ValueError(f"{name}: mu lives on {mu.device}, the plan on {bins.device}; build "
                         f"the FineBins on the operands' device")
    if bins.nb <= MAX_BINS:
        return gaussian_binned_sum(mu, sigma, bins.edges, weights, chunk=chunk)
    flat = [None if t is None else t.reshape(-1).contiguous() for t in (mu, sigma, weights)]
    chunk = int(chunk) if chunk else max(1, min(_CHUNK, _TABLE // bins.nb))
    return _GaussianBinnedSumFine.apply(bins, *flat, chunk)
