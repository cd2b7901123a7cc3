"""The fused engine as an L-BFGS objective over each rank's owned parameters, and the map
between the user's parameter order and that vector (``FusedAdamEngine.lbfgs_objective``)."""
from __future__ import annotations

import math

import torch

from ._placement import assemble


class _EngineObjective:
    """Loss and gradient over the engine's owned parameter slices.

    ZeRO (world > 1): x is the concatenation of this rank's slices of every chunk; an
    evaluation all-gathers the chunks, runs forward + loss + per-chunk VJP, and
    reduce-scatters the gradient back to the owned slices -- L-BFGS vectors and history
    are sharded 1/W and its dot products are all-reduced by the optimizer.  With the
    two-shot peer-memory context up, the all-gather is its mode 5 (each rank pushes its
    slices into every rank's parameter region) and the reduce-scatter its mode 4 (rank-order
    sum of the owned slices of every rank's gradient region): the evaluation makes no RCCL
    or host collective.  Otherwise RCCL reduce-scatter / all-gather on the same layout.
    Owner placement: x is the owned parameter range, whose gradient is complete locally
    (only the sumstats cross ranks, inside the forward's epilogue).
    Replicated: x is the full (padded) parameter vector and the gradient is all-reduced.
    """

    def __init__(self, eng):
        self.e = eng
        self.comm = eng.comm
        self.sharded = eng.zero or eng.owner
        self.device = eng.device
        self.ts = eng.twoshot if (eng.zero and not eng.owner) else None
        self.n_local = sum(s.n for s in eng.slices)
        self._nev = 0
        # MULTIGRAD_LBFGS_FAULT=<rank>:<evaluation> (tests): that rank skips the whole
        # evaluation number ``evaluation`` (1-based) -- every exchange in it
        r, _, k = (eng.cfg.lbfgs_fault or "").partition(":")
        self._fault = (int(r), int(k or 1)) if r and eng.size > 1 else None

    def local_box(self, param_bounds):
        """``(lo, hi)`` of this objective's vector (user-order spec -> internal order,
        padding unbounded, then this rank's owned slices) for the device L-BFGS-B."""
        from ..optim.lbfgsb import bounds_arrays
        e = self.e
        lo_u, hi_u = bounds_arrays(param_bounds, e.P)
        out = []
        for arr, fill in ((lo_u, -math.inf), (hi_u, math.inf)):
            v = torch.full((e.P_pad,), fill, dtype=torch.float32, device=self.device)
            if arr is not None:
                t = torch.as_tensor(arr, dtype=torch.float32, device=self.device)
                v[:e.P] = t[e.pidx] if e.pidx is not None else t
            out.append(e._local(v).contiguous())
        return out[0], out[1]

    def x0(self) -> torch.Tensor:
        return self.e._local(self.e.theta).clone()

    def _load(self, x: torch.Tensor):
        e = self.e
        gather = e.zero and not e.owner
        for s in e.slices:
            xs = x[s.o:s.o + s.n]
            if self.ts is not None:
                # this rank's slice into every rank's parameter region (its own included);
                # the launch returns when every rank's slice of the chunk has landed here
                self.ts.all_gather_(xs, s.a, s.n)
                continue
            e.theta[s.a:s.b].copy_(xs)
            if gather:
                e._all_gather(s)

    def __call__(self, x: torch.Tensor):
        loss, g = self.device_call(x)
        f = float(loss.double().item())
        self.e.check("L-BFGS evaluation")
        return f, g

    def check(self, where: str = "L-BFGS") -> None:
        """Collective: raise :class:`~multigrad_amd.parallel.xgmi.CollectiveTimeout` on every
        rank if any peer-memory exchange of the engine's evaluations timed out (the two-shot
        reduce-scatter / all-gather of the ZeRO evaluations, the one-shot sumstats) -- their
        results were NaN-poisoned.  :meth:`device_call` does not sync, so the optimizers call
        this at the end of a run, next to their reducer's check."""
        self.e.check(where, collective=True)

    def device_call(self, x: torch.Tensor):
        """``(loss, grad)`` with the loss left on the device (1-element tensor), so the
        optimizer can fetch it together with its own reductions in one copy."""
        e, md = self.e, self.e.model
        self._nev += 1
        if self._fault == (e.rank, self._nev):
            # test hook: this rank skips the gradient exchange of one evaluation, so its
            # peers' bounded waits time out (the engine's error word, NaN-poisoned slices)
            return e.loss, e.g_loc if (e.zero and not e.owner) else e.grad
        self._load(x)
        e._forward_loss()
        if e.owner:
            s, = e.slices
            md.engine_vjp_into(e.theta, e.h, e.grad, chunk=s.chunk)
            g = e.grad[s.a:s.b]
        elif e.zero:
            works = []
            for s in e.slices:
                md.engine_vjp_into(e.theta, e.h, e.grad, chunk=s.chunk)
                if self.ts is not None:
                    self.ts.reduce_scatter_(e.g_loc[s.o:s.o + s.n], s.a, s.n)
                else:
                    works.append(e._reduce_scatter(s))
            for w in works:
                w.wait()
            g = e.g_loc
        else:
            for c in range(e.C):
                md.engine_vjp_into(e.theta, e.h, e.grad, chunk=c if e.C > 1 else None)
            if e.size > 1:
                e.comm.all_reduce(e.grad)
            g = e.grad
        return e.loss, g

    def vector_layout(self) -> "_EngineLayout":
        """The mapping between the user's parameter order and this objective's vector, as
        it stands now (it owns what it needs: usable after the engine is closed)."""
        return _EngineLayout(self.e)

    def full(self, x: torch.Tensor) -> torch.Tensor:
        """The full parameter vector (model order) for the optimizer's vector x."""
        self._load(x)
        self.e.drain()
        if self.e.owner:
            return self.e.params().clone()
        return self.e.to_user(self.e.theta[:self.e.P]).clone()


class _EngineLayout:
    """User parameter order <-> the vector of an :class:`_EngineObjective` (last dimension;
    leading batch dimensions allowed in both directions).

    Replicated: permute to the internal order and pad.  Owner placement: permute and take
    the owned range; back by an all-gather of equal padded pieces.  ZeRO: the owned slice of
    every chunk, concatenated; back by one all-gather of the local vectors, placed chunk by
    chunk (``_placement.assemble``).  Padding entries are zero
    in every optimizer vector, so they drop out.  It never touches ``engine.theta`` and owns
    (copies of) the index data it needs, so it works after the engine is closed or re-laid
    out; on several ranks ``from_local`` is collective."""

    def __init__(self, eng):
        self.comm, self.size, self.rank = eng.comm, eng.size, eng.rank
        self.device = eng.device
        self.P, self.P_pad = int(eng.P), int(eng.P_pad)
        self.pidx = None if eng.pidx is None else eng.pidx.clone()
        self.inv_pidx = None if eng.pidx is None else eng.inv_pidx.clone()
        self.pb, self.lengths = list(eng.pb), list(eng.lengths)
        self.owner, self.zero = bool(eng.owner), bool(eng.zero) and not eng.owner
        # replicated: the whole padded vector, nothing to cut
        self.slices = tuple(eng.slices) if (self.owner or self.zero) else ()
        self.n_local = sum(s.n for s in self.slices) if self.slices else self.P_pad

    def to_local(self, v: torch.Tensor) -> torch.Tensor:
        v = v.to(self.device)
        if self.pidx is not None:
            v = v[..., self.pidx]
        if self.P_pad > self.P:
            v = torch.cat([v, v.new_zeros(v.shape[:-1] + (self.P_pad - self.P,))], -1)
        if self.slices:
            v = torch.cat([v[..., s.a:s.b] for s in self.slices], -1)
        return v.contiguous()

    def from_local(self, t: torch.Tensor) -> torch.Tensor:
        full = assemble(self, t) if self.slices else t
        full = full[..., :self.P]
        return full[..., self.inv_pidx] if self.inv_pidx is not None else full.clone()
