"""Re-layout of the fused engine's parameter order while a fit runs.

A fit can move populations across the Euler-Maclaurin limit (the reference's own SMF
fit takes sigma from 0.5 to 0.2 dex on 0.1-dex bins, tests/smf_example/
smf_grad_descent.py:103,113): the lane classes laid out at setup then no longer
match, narrow populations sit scattered in wide groups and most groups take the
per-edge path (1% scattered narrow populations: ~47% of the groups).  Every
MULTIGRAD_RELAYOUT_EVERY (16) steps the engine measures on the device, without a host sync,
the share of groups the forward at the current parameters sends down the per-edge
path (model.engine_relayout_probe), reads it back a few steps later, and when it
differs from the share the classes were laid out for by more than
MULTIGRAD_RELAYOUT_MARGIN it re-classifies at the step boundary: the lanes are rebuilt
on the GPU (ops/_schedule.py:build_lanes_torch, ms) and theta / m / v / u / bounds are
permuted into the new internal order.  Trajectory rows keep the order they were
written in; each row range is mapped back to the user order with its own permutation.
"""
from __future__ import annotations

import time
from typing import Optional

import torch

from ._stream import on_engine_stream
from ..optim.transforms import Bounds


class _RelayoutMixin:
    _PROBE_DELAY = 4

    def _relayout_reset(self) -> None:
        self.relayout_every = self.cfg.relayout_every
        self.relayout_margin = self.cfg.relayout_margin
        self._relayout_on = False
        self._probe_step = self._probe_host = self._probe_ev = self._share_ref = None
        self._probe_last = 0
        self.relayouts = []
        # trajectory row ranges and the user -> internal map they were written with
        self._segs = [(0, self.inv_pidx)]

    def _relayout_init(self) -> None:
        md = self.model
        self._relayout_reset()
        # (one slice: the probe is off under ZeRO, whose slices are cut from the order)
        self._relayout_on = bool(
            self.relayout_every > 0 and self.cfg.relayout and self.device.type == "cuda"
            and (self.size == 1 or self.owner) and self.pidx is not None
            and hasattr(md, "engine_relayout_probe") and hasattr(md, "engine_layout_share"))
        self._share_ref = self._probe_now() if self._relayout_on else None

    @staticmethod
    def _param_order(md, P: int, upp: int, dev):
        """``(pidx, inv_pidx)``: internal -> user and user -> internal parameter index of
        the model's unit order (``engine_param_perm``), or ``(None, None)``."""
        perm = getattr(md, "engine_param_perm", lambda: None)()
        if perm is None:
            return None, None
        perm = torch.as_tensor(perm, device=dev).to(torch.int64)
        ar = torch.arange(upp, device=dev, dtype=torch.int64)
        pidx = (perm[:, None] * upp + ar).reshape(-1)      # internal -> user index
        inv = torch.empty_like(pidx)
        inv[pidx] = torch.arange(P, device=dev)            # user -> internal index
        return pidx, inv

    def _probe_now(self) -> Optional[float]:
        """The probe's per-edge share at the current parameters (host sync)."""
        v = self.model.engine_relayout_probe(self.theta, self.slices[0].chunk)
        return None if v is None else float(v)

    def _maybe_relayout(self) -> None:
        """Step-boundary hook: launch the device probe every ``relayout_every`` steps and act
        on its value ``_PROBE_DELAY`` steps later (deterministic step: owner ranks vote)."""
        if not self._relayout_on or self._tuning or self._capturing:
            return
        k = self.step_host
        if self._probe_step is None:
            if k - self._probe_last < self.relayout_every:
                return
            v = self.model.engine_relayout_probe(self.theta, self.slices[0].chunk)
            if v is None:
                self._relayout_on = False
                return
            if self._probe_host is None:
                self._probe_host = torch.zeros(1, dtype=torch.float32, pin_memory=True)
                self._probe_ev = torch.cuda.Event()
            self._probe_host.copy_(v.reshape(1), non_blocking=True)
            self._probe_ev.record()
            self._probe_step = k
            return
        if k - self._probe_step < self._PROBE_DELAY:
            return
        self._probe_ev.synchronize()  # recorded _PROBE_DELAY steps ago: normally long done
        f_cur = float(self._probe_host[0])
        self._probe_step, self._probe_last = None, k
        # the probe's share right after the last (re)layout is the reference: a drift by
        # more than the margin either way means populations crossed the limit since
        f_ref = self._share_ref if self._share_ref is not None else 0.0
        go = abs(f_cur - f_ref) > self.relayout_margin
        if self.owner and self.size > 1:
            flag = torch.tensor([1 if go else 0], dtype=torch.int64)
            self.comm.all_reduce(flag, op="max")
            go = bool(flag[0])
        if go and not self.relayout(reason=dict(step=k, share_probe=round(f_cur, 4),
                                                share_ref=round(f_ref, 4))):
            self._share_ref = f_cur  # classes unchanged: nothing to gain, stop re-trying

    @on_engine_stream
    def relayout(self, reason: Optional[dict] = None) -> bool:
        """Re-classify the lane groups at the current parameters and rebuild the layout
        (collective in owner mode).  Returns whether the classes changed."""
        md = self.model
        if self.pidx is None or not hasattr(md, "engine_layout_hint") or \
                (self.zero and not self.owner):  # ZeRO slices are cut from the order
            return False
        t0 = time.perf_counter()
        self.drain()
        P, dev = self.P, self.device
        s, = self.slices  # owner mode or replicated
        hi = min(s.b, P)
        full = self._assemble(self.theta[s.a:hi]) if self.owner else self.theta[:P]
        if not md.engine_layout_hint(self.to_user(full), band=self.cfg.relayout_band):
            return False
        old_inv = self.inv_pidx
        md.engine_set_chunks(self._ub)
        pidx, inv = self._param_order(md, P, self.upp, dev)
        g = old_inv[pidx]  # new internal position i holds old internal position g[i]
        n = hi - s.a
        loc = g[s.a:hi] - s.a  # the same permutation, of the local vectors
        self.theta[s.a:hi] = self.theta[g[s.a:hi]]
        for t in (self.m, self.v, self.u):
            if t is not None:
                t[:n] = t[:n][loc]
        if self.bounds is not None:
            bd = self.bounds
            pad = torch.arange(P, bd.lo.numel(), device=dev)
            gi = torch.cat([g, pad])
            self.bounds = Bounds(bd.lo[gi].contiguous(), bd.hi[gi].contiguous(),
                                 bd.kind[gi].contiguous())
            self.bounds_loc = self._local_bounds(self.bounds)
        if self.history.mode != "full":
            self.history.rows = [r[g] for r in self.history.rows]
        self.pidx, self.inv_pidx = pidx, inv
        self._segs.append((self.step_host + 1, inv))
        rows = [md.engine_fwd_rows(c) for c in range(self.C)]
        if sum(rows) * self.nS > self.slab.numel():
            self.slab = torch.zeros(sum(rows) * self.nS, dtype=torch.float32, device=dev)
        self.rows = rows
        self._bind()
        self.graph = None  # captured with the old layout's buffers
        torch.cuda.synchronize()
        self._share_ref = self._probe_now()
        rec = dict(reason or {}, step=self.step_host, seconds=round(time.perf_counter() - t0, 4),
                   share_new=round(self._share_ref, 4) if self._share_ref is not None else None,
                   share_layout=round(md.engine_layout_share(s.chunk), 4))
        self.relayouts.append(rec)
        return True

    def _traj_to_user(self, t: torch.Tensor) -> torch.Tensor:
        """Trajectory rows (internal order of the layout they were written in) -> user order."""
        segs = self._segs
        if self.pidx is None or len(segs) == 1:
            return self.to_user(t)
        out = torch.empty_like(t)
        n = t.shape[0]
        for i, (r0, inv) in enumerate(segs):
            r1 = segs[i + 1][0] if i + 1 < len(segs) else n
            r0, r1 = min(r0, n), min(r1, n)
            if r1 > r0:
                out[r0:r1] = t[r0:r1][..., inv]
        return out

    def _traj_rows_to_current(self, t: torch.Tensor) -> torch.Tensor:
        """Trajectory rows (each in the layout it was written in) -> the current internal
        order (columns: this rank's local elements)."""
        segs = self._segs
        if self.pidx is None or len(segs) == 1:
            return t
        base = self.slices[0].a  # several layouts: one slice (owner mode or replicated)
        cur = self._local_order()
        out = t.clone()
        n = t.shape[0]
        for i, (r0, inv) in enumerate(segs[:-1]):
            r1 = min(segs[i + 1][0], n)
            if r1 > min(r0, n):
                out[r0:r1, :cur.numel()] = t[r0:r1][:, inv[cur] - base]
        return out
