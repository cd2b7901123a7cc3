"""Where the fused engine's data and its peers are: the collective decisions of a setup
(re-partition by owner, owner-mode bounds, the two-shot peer-memory context) and the
assembly of sharded vectors."""
from __future__ import annotations

import torch

from ._stream import on_engine_stream
from ..utils.trace import trace


def assemble(x, t: torch.Tensor) -> torch.Tensor:
    """Collective: ``[..., P_pad]`` in the internal order from every rank's ``[..., n_local]``
    (identical leading shape on all ranks) of an owner-mode or ZeRO engine ``x`` (or the
    ``_EngineLayout`` of one): one all-gather of equal pieces -- owner ranges padded to the
    longest -- then every rank's slices put in place."""
    lead = tuple(t.shape[:-1])
    piece = t.contiguous()
    if x.owner:
        piece = torch.zeros(lead + (max(x.lengths),), dtype=t.dtype, device=t.device)
        piece[..., :t.shape[-1]] = t
    gathered = piece.reshape((1,) + tuple(piece.shape))
    if x.size > 1:
        gathered = torch.empty((x.size,) + tuple(piece.shape), dtype=t.dtype, device=t.device)
        x.comm.all_gather_into_tensor(gathered.reshape(-1), piece.reshape(-1))
    full = torch.empty(lead + (x.P_pad,), dtype=t.dtype, device=t.device)
    for r in range(x.size):
        if x.owner:
            a, b = x.pb[r], x.pb[r + 1]
            full[..., a:b] = gathered[r][..., :b - a]
            continue
        for s in x.slices:  # rank r's 1/W of the chunk, where this rank keeps its own
            a = x.pb[s.chunk] + r * s.n
            full[..., a:a + s.n] = gathered[r][..., s.o:s.o + s.n]
    return full


class _PlacementMixin:
    def _maybe_repartition(self) -> None:
        """Collective: move the model's data to the parameter owners once (see
        ``repartition`` in ``__init__``); a model without ``engine_repartition``, or whose
        data already follow the owners, is left as it is."""
        if not self.repartition or self.repartitioned is not None:
            return
        md = self.model
        fn = getattr(md, "engine_repartition", None)
        if fn is None:
            return
        trace("engine: re-partition by owner")
        info = fn()
        self.repartitioned = dict(info) if info else {}
        trace(f"engine: re-partition done {self.repartitioned}")

    def _owner_units(self, md, J):
        """Owner-mode unit bounds if the model's data placement allows it on every rank."""
        if not self.allow_owner or (self.size == 1 and not self.force_owner):
            return None
        fn = getattr(md, "engine_owner_units", None)
        ub = fn() if fn is not None else None
        if ub is None and self.size == 1 and self.force_owner:
            ub = [0, J]
        ok = ub is not None and len(ub) == self.size + 1 and ub[0] == 0 and ub[-1] == J \
            and all(x <= y for x, y in zip(ub, ub[1:]))
        if ok:
            lo, hi = md.engine_support_units()
            ok = hi <= lo or (ub[self.rank] <= lo and hi <= ub[self.rank + 1])
        flag = torch.tensor([1 if ok else 0], dtype=torch.int64)
        self.comm.all_reduce(flag, op="min")
        return [int(u) for u in ub] if int(flag[0]) == 1 else None

    def _assemble(self, own: torch.Tensor) -> torch.Tensor:
        """Collective: the full (internal order) vector(s) from every rank's local ones."""
        return assemble(self, own)[..., :self.P]

    def _connect_twoshot(self, numel: int):
        """The two-shot context for ``numel`` floats (kept across setups of the same
        size), connecting it now if needed -- collective; None: use RCCL."""
        from ..parallel.xgmi import acquire_twoshot, release_twoshot, twoshot_enabled
        if not twoshot_enabled() or self.size > 8:
            return None
        ts = self._ts_keep
        if ts is not None:
            torch.cuda.synchronize()  # no exchange of a previous run still in flight
        if ts is not None and ts.numel == numel:
            return ts
        if ts is not None:
            release_twoshot(self.comm, ts)
            self._ts_keep = None
        self._ts_keep = acquire_twoshot(self.comm, numel)
        return self._ts_keep

    @on_engine_stream
    def close(self) -> None:
        """Give the engine's peer-memory exchange context back to the communicator's pool
        (collective: every rank closes its engine).  The engine cannot step afterwards."""
        from ..parallel.xgmi import release_twoshot
        if self._ts_keep is not None:
            release_twoshot(self.comm, self._ts_keep)
        self._ts_keep = None
        self.twoshot = None
        self.ready = False
        self.closed = True
        self.graph = None
        self._gkey = None
