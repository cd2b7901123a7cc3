"""Group gather and segment sum: the broadcast of per-group parameters to their objects and
its transpose -- the defining pair of a hierarchical model (one or a few parameters per
population, halo or sample, many objects each).

    plan = GroupIndex(index, num_groups)      # once, at setup
    a_i, s_i = plan.gather(a, sigma)          # [G] tensors -> [N] tensors, values[index]
    tot, = plan.segment_sum(m_i)              # [N] tensors -> [G] tensors, sum over each group

The group index is fixed for the life of a fit, so everything that depends on it -- the range
check, a stable sort, the per-group counts -- is done once by :class:`GroupIndex`.  The two ops
are each other's transpose and each one's backward is the other, so both are differentiable to
any order, and the backward of a gather is a fixed-order segmented sum over the sorted objects:
no sort per step, no float atomics, bitwise reproducible, no host synchronisation (it captures
into a HIP graph).  float32 device tensors run the gfx950 kernels of ``csrc/groups.hip``; every
other dtype or device runs ``index_select`` / ``index_add_``.

Accuracy of ``segment_sum`` (float32 kernels): for a group ``g`` of ``L`` objects

    |sum - exact| <= summation_depth(L) * 2**-24 * sum_{i in g} |x_i|

the standard bound of a summation order whose longest path has ``summation_depth(L)`` rounded
additions, with ``summation_depth(L) <= 4 + 2 * ceil(log2(max(L, 2)))``.  ``gather`` is exact.
"""
from __future__ import annotations

import functools
from typing import Tuple

import torch

from ._ext import ext
from .smf import stable_population_sort

__all__ = ["GroupIndex", "group_gather", "segment_sum", "summation_depth", "CHUNK"]

CHUNK = 1024  # kChunk in csrc/groups.hip: sorted positions per workgroup chunk
_THREAD = 4   # consecutive entries per thread
_WAVE = 64
_INT32_MAX = 2 ** 31


def _ceil_log2(n: int) -> int:
    return max(0, (int(n) - 1).bit_length())


def _chunk_depth(n: int) -> int:
    """Rounded additions on the longest path to the sum of ``n`` consecutive entries of one
    chunk, for the worst placement of the run: 3 in a thread's registers, ``ceil(log2(lanes))``
    in the scan over the lanes the run touches, 3 when it spans waves (2 to fold up to three
    wave aggregates, 1 to join them with the lanes of the own wave), 1 to add the own thread's
    entries.  Additions of an exact 0 (identities, padding) are not rounded, so the depth is
    also at most ``n - 1``."""
    if n <= 1:
        return 0
    threads = 1 + (n + _THREAD - 2) // _THREAD      # a run may start on a thread's last entry
    lanes = min(threads, _WAVE)
    waves = 3 if threads > 1 else 0                 # any two threads may sit in two waves
    return min(n - 1, (_THREAD - 1) + _ceil_log2(lanes) + waves + 1)


@functools.lru_cache(maxsize=None)
def _run_depth(n: int) -> int:
    """Worst case over placements for a run of ``n`` entries on any level: inside one chunk,
    or across ``c`` chunks, whose partials (two slots per inner chunk, one per outer chunk)
    form a run of ``2 (c - 1)`` entries on the next level."""
    if n <= 2:
        return max(0, n - 1)
    inside = _chunk_depth(n) if n <= CHUNK else 0
    chunks = 1 + (n - 1 + CHUNK - 1) // CHUNK
    across = _chunk_depth(min(n - 1, CHUNK)) + _run_depth(2 * (chunks - 1))
    return max(inside, across)


def summation_depth(L: int) -> int:
    """The number of rounded additions on the longest path to the sum of a group of ``L``
    objects in the order ``segment_sum``'s kernels use, for the worst placement of the group
    in the sorted order; ``<= 4 + 2 * ceil(log2(max(L, 2)))``.  The error contract follows:
    ``|sum - exact| <= summation_depth(L) * 2**-24 * sum |x_i|``."""
    L = int(L)
    return min(max(L - 1, 0), _run_depth(L))


class GroupIndex:
    """The plan of a fixed group index: ``index`` holds the group id in ``[0, num_groups)`` of
    each of N objects (int32 or int64, any shape, treated as flat, on any device).

    Construction does all the work that depends on ``index`` and is the only place that reads
    the device back: the range check (``ValueError``), a stable sort
    (:func:`~multigrad_amd.ops.smf.stable_population_sort`), the per-group ``counts`` and
    ``offsets``.  ``is_sorted`` tells whether ``index`` was already non-decreasing (population
    shards are); the permutation is then ``None``.  Plans of ``N >= 2**31`` objects are valid
    but run the torch ops.
    """

    def __init__(self, index: torch.Tensor, num_groups: int):
        if not isinstance(index, torch.Tensor) or index.dtype not in (torch.int32, torch.int64):
            raise TypeError("GroupIndex: `index` must be an int32 or int64 tensor")
        num_groups = int(num_groups)
        if num_groups < 0 or num_groups >= _INT32_MAX:
            raise ValueError(f"GroupIndex: num_groups must be in [0, 2**31), got {num_groups}")
        flat = index.detach().reshape(-1)
        self.n = flat.numel()
        self.num_groups = num_groups
        self.device = flat.device
        if self.n:
            lo, hi = (int(v) for v in torch.stack([flat.min(), flat.max()]).tolist())
            if lo < 0 or hi >= num_groups:
                raise ValueError(f"GroupIndex: group ids must lie in [0, {num_groups}), "
                                 f"got [{lo}, {hi}]")
        self.ids = flat.to(torch.int32).contiguous()
        if self.n:
            sorted_ids, order, counts = stable_population_sort(self.ids, num_groups)
            self.is_sorted = bool(torch.equal(sorted_ids, self.ids))
        else:
            sorted_ids, order = self.ids, None
            counts = torch.zeros(num_groups, dtype=torch.int64, device=self.device)
            self.is_sorted = True
        self.counts = counts.to(torch.int64)
        self.offsets = torch.cumsum(self.counts, 0) - self.counts
        if self.is_sorted:
            self.sorted_ids, self.perm = self.ids, None
        else:
            self.sorted_ids = sorted_ids.to(torch.int32).contiguous()
            self.perm = (order.to(torch.int32) if self.n < _INT32_MAX else order).contiguous()

    def __repr__(self):
        return (f"GroupIndex(n={self.n}, num_groups={self.num_groups}, device={self.device}, "
                f"is_sorted={self.is_sorted})")

    def gather(self, *values: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """``values[index]`` for 1..k same-dtype ``[num_groups]`` tensors (four per launch):
        a tuple of contiguous ``[N]`` tensors, bitwise equal to the torch expression."""
        _check_operands("gather", self, values, self.num_groups)
        return _Gather.apply(self, *values)

    def segment_sum(self, *per_object: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """The sum over each group of 1..k same-dtype tensors of N elements (four per launch):
        a tuple of contiguous ``[num_groups]`` tensors; a group without objects gets exactly 0.
        See the module docstring for the float32 error contract."""
        _check_operands("segment_sum", self, per_object, self.n)
        return _SegmentSum.apply(self, *per_object)

    def binned_sum(self, mu, sigma, edges, weights=None, *, chunk=None) -> torch.Tensor:
        """The Gaussian-binned sum of every group, ``[num_groups, nb]``:
        :func:`~multigrad_amd.ops.binned_group.gaussian_binned_sum_by_group` on this plan."""
        from .binned_group import gaussian_binned_sum_by_group
        return gaussian_binned_sum_by_group(self, mu, sigma, edges, weights, chunk=chunk)

    # ---- the raw ops (no autograd) ----
    def _native(self, t: torch.Tensor) -> bool:
        return t.is_cuda and t.dtype == torch.float32 and self.n < _INT32_MAX

    def _gather_raw(self, values):
        v0 = values[0]
        if self.n == 0 or not self._native(v0):
            return tuple(torch.index_select(v.reshape(-1), 0, self.ids) for v in values)
        cols = [v.reshape(-1).contiguous() for v in values]
        return tuple(ext().group_gather(self.ids, cols, self.num_groups))

    def _segment_sum_raw(self, xs):
        x0 = xs[0]
        if self.n == 0 or self.num_groups == 0 or not self._native(x0):
            return tuple(torch.zeros(self.num_groups, dtype=x.dtype, device=x.device)
                         .index_add_(0, self.ids, x.reshape(-1)) for x in xs)
        cols = [x.reshape(-1).contiguous() for x in xs]
        return tuple(ext().group_segment_sum(self.sorted_ids, self.perm, cols, self.num_groups))


def _check_operands(name: str, plan: GroupIndex, ops, numel: int) -> None:
    if not ops:
        raise ValueError(f"{name}: at least one operand")
    first = ops[0]
    for t in ops:
        if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
            raise TypeError(f"{name}: operands must be floating-point tensors")
        if t.numel() != numel:
            raise ValueError(f"{name}: operand has {t.numel()} elements, expected {numel}")
        if t.dtype != first.dtype or t.device != first.device:
            raise ValueError(f"{name}: operands must share one dtype and device")
    if first.device != plan.device:
        raise ValueError(f"{name}: operands live on {first.device}, the plan on {plan.device}; "
                         f"build the GroupIndex from an index on the operands' device")


def _transpose(op, plan, grads, needs, shapes):
    """The other op applied to the gradients that are present and wanted, in one call; a
    missing (``None``) gradient is a zero column and is never materialised."""
    live = [i for i, g in enumerate(grads) if g is not None and needs[i]]
    out = [None] * len(grads)
    if live:
        for i, r in zip(live, op.apply(plan, *[grads[i] for i in live])):
            out[i] = r.reshape(shapes[i])
    return (None, *out)


def _tangents(raw, tangents, shapes):
    """Forward mode of a linear op: the raw op applied to the tangents.  A missing (``None``)
    tangent becomes zeros, since another operand of the same call has one."""
    ref = next(t for t in tangents if t is not None)
    return raw([ref.new_zeros(s) if t is None else t for t, s in zip(tangents, shapes)])


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *values):
        ctx.plan, ctx.shapes = plan, [v.shape for v in values]
        ctx.set_materialize_grads(False)
        return plan._gather_raw(values)

    @staticmethod
    def backward(ctx, *grads):
        return _transpose(_SegmentSum, ctx.plan, grads, ctx.needs_input_grad[1:], ctx.shapes)

    @staticmethod
    def jvp(ctx, _plan, *tangents):
        return _tangents(ctx.plan._gather_raw, tangents, ctx.shapes)


class _SegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *per_object):
        ctx.plan, ctx.shapes = plan, [x.shape for x in per_object]
        ctx.set_materialize_grads(False)
        return plan._segment_sum_raw(per_object)

    @staticmethod
    def backward(ctx, *grads):
        return _transpose(_Gather, ctx.plan, grads, ctx.needs_input_grad[1:], ctx.shapes)

    @staticmethod
    def jvp(ctx, _plan, *tangents):
        return _tangents(ctx.plan._segment_sum_raw, tangents, ctx.shapes)


def group_gather(plan: GroupIndex, *values: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """``plan.gather(*values)``."""
    return plan.gather(*values)


def segment_sum(plan: GroupIndex, *per_object: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """``plan.segment_sum(*per_object)``."""
    return plan.segment_sum(*per_object)
