"""Fused, device-resident Adam engine (HIP kernels + stream-ordered RCCL collectives).

The generic path (``OnePointModel.run_adam``) runs the distributed chain rule through
autograd with Python in the loop.  Models that expose the *engine protocol* run instead
as a fixed sequence of device operations per step, with no host synchronisation:

    forward per chunk      (HIP kernel -> per-workgroup slab rows)
    slab reduce            (fixed-order sum)                               -> S
    all-reduce(S)          (RCCL, latency bound, K floats)
    loss + edge weights    (1 tiny kernel)                                 -> loss, h
    VJP per chunk          (segmented per-population kernel)               -> g_c
    ZeRO-1 (world > 1, default):
        reduce-scatter(g_c)  issued right after VJP_c on RCCL's stream, so it overlaps
                             VJP_{c+1} on the compute stream
        fused Adam on the owned 1/W slice of chunk c (as soon as RS_c lands)
        all-gather(theta_c)  overlapping Adam_{c+1} and, across the step boundary, the
                             next step's forward of chunk c-1...
    replicated (world == 1, or zero=False):
        all-reduce(g) + fused Adam over every parameter

RS + AG move exactly the bytes of one all-reduce, but the optimizer work and the Adam
state drop to 1/W per GPU and every collective hides behind compute of a neighbouring
chunk.  Parameters stay bitwise identical across ranks (each slice has one owner).

Owner mode (world > 1, model data placed by parameter ownership): when the model
reports unit bounds ``engine_owner_units() -> [W+1]`` and every rank's data touches only
units inside its own range (``engine_support_units()``, verified collectively at setup),
the chunks ARE the ranks' ranges.  Rank r's gradient on its range is then complete
locally and zero elsewhere, so the step is

    forward(own chunk) -> all-reduce(S) -> loss -> VJP(own chunk) -> Adam(own chunk)

with the K-float sumstat all-reduce as the only collective: the dense P-float
gradient reduction of data parallelism (reference multigrad/multigrad.py:531-532)
is provably all zeros outside the owner's range and is not sent.  Parameters, moments and
trajectory are sharded by owner and assembled on request.

What a rank updates is one list of slices (``_Slice``) in every placement: a range of
``theta`` and the range of the rank's local vectors (``m``, ``v``, ``u``, ``bounds_loc``,
``g_loc``, the columns of ``traj_loc``) that holds it -- the rank's range in owner mode, its
1/W of every chunk under ZeRO, the whole padded vector otherwise.  Every update takes its
arguments from ``_adam_args``; the placements differ only in the collectives of a step.

On a single GPU the whole step is captured once into a HIP graph and replayed; the
device step counter inside the Adam kernel makes the replay self-advancing.  This
replaces the reference's per-step host round trips (4 host crossings per
Adam step, 2 of them pickled broadcasts).

Engine protocol (implemented by :class:`~multigrad_amd.models.population.PopulationSMFModel`):
``engine_units() -> (J, params_per_unit)``, ``engine_set_chunks(unit_bounds)``,
``engine_nS()``, ``engine_fwd_rows(chunk)``, ``engine_forward_chunk(theta, slab, chunk)
-> rows``, ``engine_reduce(slab, rows, S)``, ``engine_loss_into(S, loss, h)``,
``engine_vjp_into(theta, h, grad, chunk)``, optionally ``engine_param_perm()`` (the
unit order the model wants the engine vectors in) and ``engine_layout_hint(guess)`` (the
starting parameters, before ``engine_set_chunks``, for a data layout that depends on
them).  Every method works on CPU tensors too (PyTorch reference math), which is how the
multi-rank orchestration is tested on gloo.

Here: construction, setup, the step path, the reads and ``run_adam``.  Settings:
``_settings.py``; setup-time tuning: ``_tune.py``; data placement and peers: ``_placement.py``;
re-layout: ``_relayout.py``; checkpoints: ``_state.py``; L-BFGS objective: ``_objective.py``.
"""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple, Optional

import torch

from ._placement import _PlacementMixin
from ._objective import _EngineLayout, _EngineObjective  # noqa: F401  (_EngineLayout: imported from here)
from ._relayout import _RelayoutMixin
from ._settings import _Settings
from ._state import _StateMixin
from ._stream import EngineStream, make_engine_stream, on_engine_stream
from ._tune import _TuneMixin
from ..optim.adam import History
from ..optim.transforms import Bounds, KIND_NONE
from ..ops.adam import adam_step_
from ..utils.profiling import PhaseTimer
from ..utils.trace import trace

__all__ = ["FusedAdamEngine", "plan_chunks"]


def plan_chunks(J: int, upp: int, world: int, nchunks: int):
    """Unit-aligned chunk boundaries whose parameter counts are multiples of 4*world
    (float4 lanes on every reduce-scatter slice); the last chunk is padded.

    Returns (unit_bounds, param_bounds, P_pad, chunk_lengths)."""
    q = 4 * world
    a = q // math.gcd(q, upp)  # units per alignment block
    C = max(1, min(int(nchunks), J))
    ub = sorted({min(J, int(round(c * J / C / a)) * a) for c in range(C)} | {0, J})
    ub = [u for u in ub if u <= J]
    # drop empty chunks (duplicates already removed); keep J as the final bound
    pb = [u * upp for u in ub]
    last = pb[-1] - pb[-2]
    P_pad = pb[-2] + (-(-last // q) * q if last else 0)
    lengths = [pb[i + 1] - pb[i] for i in range(len(pb) - 2)] + [P_pad - pb[-2]]
    return ub, pb, P_pad, lengths


class _Slice(NamedTuple):
    """One range of parameters this rank updates."""
    chunk: Optional[int]  # what the model protocol takes (None: one replicated chunk)
    a: int                # [a, b) in theta
    b: int
    o: int                # [o, o + n) in the rank's local vectors
    n: int
    step: int             # row of step_dev (and the slice's index in ``engine.slices``)


def _cut(t: torch.Tensor, o: int, n: int) -> torch.Tensor:
    """``t[o:o + n]`` (``t`` itself where that is all of it)."""
    return t if (o == 0 and n == t.numel()) else t[o:o + n]


class FusedAdamEngine(_TuneMixin, _RelayoutMixin, _StateMixin, _PlacementMixin):
    """Device-resident Adam for a model implementing the engine protocol.

    Parameters
    ----------
    model : the model (its ``comm`` is used for the collectives)
    graph : capture the step into a HIP graph (default: on for a single GPU rank;
        ``MULTIGRAD_GRAPH`` overrides)
    zero : shard the optimizer across ranks (reduce-scatter / all-gather); default on
        for more than one rank (``MULTIGRAD_ZERO``)
    chunks : number of parameter chunks for collective/compute overlap (default 1 on a
        single rank, 4 otherwise; ``MULTIGRAD_CHUNKS``)
    owner : owner mode (see the module docstring): default whenever the model's data
        placement allows it on more than one rank (``MULTIGRAD_OWNER``)

    With ZeRO the parameter all-gathers run on a second communicator (its own RCCL
    stream), so the all-gather of chunk c overlaps the reduce-scatter of chunk c+1
    instead of queueing behind it; the trajectory is stored sharded (each rank records
    the slices it owns, written by the Adam kernel) and assembled by one all-gather when
    it is requested -- the analogue of the reference's end-of-run trajectory broadcast.
    """

    @property
    def graph(self):
        """The captured one-step graph (None: capture on first use).  Dropping it also
        drops the graph of a block of steps."""
        return self._graph

    @graph.setter
    def graph(self, g):
        self._graph = g
        if g is None:
            self._kgraph = None

    def __init__(self, model, comm=None, graph: Optional[bool] = None,
                 zero: Optional[bool] = None, chunks: Optional[int] = None,
                 owner: Optional[bool] = None, repartition: Optional[bool] = None):
        cfg = self.cfg = _Settings()
        self.model = model
        self.comm = model.comm if comm is None else comm
        self.size = 1 if self.comm is None else self.comm.size
        self.rank = 0 if self.comm is None else self.comm.rank
        z = zero if cfg.zero is None else cfg.zero
        self.zero = (self.size > 1) if z is None else bool(z) and self.size > 1
        # owner mode: None = whenever the model's placement allows it on >1 rank; True =
        # also on a single rank (exercises the owner schedule); False = never
        o = owner if cfg.owner is None else cfg.owner
        self.allow_owner = True if o is None else bool(o)
        self.force_owner = bool(o)
        self.owner = False
        # re-partition a data-parallel (hashed) shard by parameter owner at setup: one
        # all-to-all-v of the data (model.engine_repartition), after which owner mode needs
        # only the sumstat all-reduce per step.  None = on for several ranks unless owner
        # mode or ZeRO was asked for explicitly; MULTIGRAD_REPARTITION overrides
        r = repartition if cfg.repartition is None else cfg.repartition
        if r is None:
            r = self.size > 1 and self.allow_owner and z is None
        self.repartition = bool(r) and self.size > 1 and self.allow_owner
        self.repartitioned = None  # the model's re-partition record, once done
        # kept across setup() calls of this engine (a model's cached engine serves every
        # run_* call, models/population.py fused_engine): device buffers of the same shape,
        # the autotune verdicts and -- when every buffer and scalar a graph captured is
        # unchanged -- the captured graphs (the analogue of JAX's jit cache)
        self._bufs = {}
        self._tune_cache = {}
        self._gkey = None
        self.stats = {"setups": 0, "captures": 0, "trial_steps": 0, "layouts": 0}
        self.closed = False
        self.fuse_vjp_adam = cfg.fused_vjp_adam
        # slab reduction (+ one-shot cross-rank sum) + loss in one launch
        self.fuse_epilogue = cfg.fused_epilogue
        self.oneshot = None
        # two-shot xGMI reduce-scatter -> Adam -> all-gather of the dense gradient (ZeRO
        # mode on GPUs; parallel/xgmi.py): None = RCCL collectives
        self.twoshot = None
        self._ts_keep = None  # the acquired two-shot context (kept across setups)
        nc = chunks if chunks is not None else cfg.chunks or None
        self._chunks_explicit = nc is not None
        self._chunks_override = None  # the chunk count setup() measured or is measuring
        self.nchunks_req = nc if nc is not None else (1 if self.size == 1 else 4)
        self.comm_ag = None  # second communicator (own RCCL stream) for parameter all-gathers
        g = graph if cfg.graph is None else cfg.graph
        self._graph_auto = g is None
        self.use_graph = (self.size == 1) if g is None else bool(g)
        # whole-loop capture (the analogue of the reference's lax.scan over the optimizer
        # loop, multigrad/mpi4jax/multigrad.py:57-58): graph mode replays graphs of
        # graph_steps unrolled steps, so the ~10 us host launch and the ~10 us device gap
        # between consecutive graph launches are paid once per block, not per step
        # (profiles/graph_modes/); MULTIGRAD_GRAPH_STEPS, 1 = one step per graph
        self.graph_steps = cfg.graph_steps
        # direct step() calls replay graphs only on request (engine/generic.py step())
        self.step_replay = cfg.step_replay
        self._kgraph = None
        self.graph = None
        self._capturing = False
        self._es = None  # the engine's own stream (stream(), engine/_stream.py)
        # eager launches of a pipelined step that read/advance the device step counter like
        # graph replays do (benchmarks/graph_modes.py "eager-dev": separates the cost of the
        # device counter from the cost of graph dispatch); MULTIGRAD_DEVICE_STEP=1
        self.device_step = cfg.device_step
        self.pending = False
        self.pipeline = False
        self.capturable = False
        self.ready = False
        # per-phase HIP-event timing of eager steps (MULTIGRAD_PROFILE=1 or bench.py
        # --profile-phases); never active inside a graph capture
        self.timer = PhaseTimer()
        # ---- (re)built by every _setup(); nothing is created anywhere else
        self.device = None
        self.upp = self.P = self.P_pad = self.C = self.nS = self.step_host = self.nsteps = 0
        self.pb, self.lengths, self.rows, self._ub, self._fwd_chunks = [], [], [], [], []
        self.slices, self._bound = (), []  # what this rank updates, and the views that takes
        self.pidx = self.inv_pidx = None
        self.lr = self.b1 = self.b2 = self.eps = 0.0
        self.legacy = False
        self.theta = self.grad = self.S = self.slab = self.h = self.loss = self.step_dev = None
        # this rank's vectors, indexed by the slices' [o, o + n): moments, the gradient shard
        # (ZeRO), the sharded trajectory (columns) and, for a bounded fit, u = T(theta) with
        # its part of the box; ``bounds`` is the whole box (internal order, padded)
        self.m = self.v = self.g_loc = self.traj_loc = self.u = self.bounds_loc = None
        self.bounds = self.history = self.history_mode = None
        self._ag, self.ev_vjp, self.ev_ts, self._ts_pending = [], [], [], []
        self.comm_stream = self._x_pending = None
        self.ts_blocks = cfg.twoshot_blocks
        self.ts_side = self.ts_fused = self.ts_fused_ok = self.rccl_exchange = False
        self.tuning = None
        self._tuning = False
        self._fault_c, self._fault_seen = None, set()  # test hook (_inject_fault)
        self._relayout_reset()

    def _buf(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        """A zeroed device buffer, the one of the previous setup when the shape matches."""
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
            self._bufs[name] = t
        else:
            t.zero_()
        return t

    # ------------------------------------------------------------------ stream
    def _engine_stream(self):
        self._es = make_engine_stream(self._es, self.device if self.device is not None
                                      else self.model.param_device())
        return self._es

    def _stream_wanted(self) -> bool:
        """Launch on the engine stream while a graph may be replayed: graph mode, or any
        captured graph still held (eager steps between replays belong there too)."""
        return bool(self.use_graph or self._graph is not None or self._kgraph is not None)

    def stream(self):
        """Context manager: the engine's own HIP stream becomes current (ordered after the
        caller's stream on entry, before it on exit).  Every public method runs its launches
        there, never on the legacy default stream (engine/_stream.py: graph replays after
        default-stream launches and a host synchronisation compute garbage on this runtime)."""
        return EngineStream(self, always=False)

    # ------------------------------------------------------------------ setup
    @on_engine_stream(always=True)
    def setup(self, guess, nsteps: int, param_bounds=None, learning_rate: float = 0.01,
              b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, history="full",
              legacy_bounds_jacobian: bool = False, tune: bool = True):
        """Allocate the device state for ``nsteps`` steps from ``guess`` (collective).
        ``tune=False``: no setup-time measurement (the default schedule is kept).

        Hashed placement on several GPUs with the two-shot exchange and no explicit chunk
        count: the two-chunk layout (whose exchange may overlap the VJP on a side stream) is
        timed against one chunk (one cross-rank rendezvous per step instead of two) and,
        when the overlapped two-chunk schedule won, against four overlapped chunks
        (``MULTIGRAD_MAX_CHUNKS``, default 4); the fastest is kept -- all by the same
        setup-time measurement as the rest of the schedule (``_tune.py``)."""
        kw = dict(param_bounds=param_bounds, learning_rate=learning_rate, b1=b1, b2=b2,
                  eps=eps, history=history, legacy_bounds_jacobian=legacy_bounds_jacobian)
        self.cfg = self.cfg.reread()
        self._maybe_repartition()
        ck = ("chunks", self.size, bool(param_bounds is None), history == "full")
        # the chunk count this engine measured before (hashed two-shot schedule)
        self._chunks_override = None if self._chunks_explicit else self._tune_cache.get(ck)
        self._setup(guess, nsteps, tune=tune, **kw)
        if tune:
            self._tune_chunks(ck, guess, nsteps, kw)
        return self

    def _setup(self, guess, nsteps: int, param_bounds=None, learning_rate: float = 0.01,
               b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, history="full",
               legacy_bounds_jacobian: bool = False, tune: bool = True):
        md, cfg = self.model, self.cfg
        dev = md.param_device()
        self.device = dev
        if dev.type != "cuda":
            self.use_graph = False
        J, upp = md.engine_units()
        P = J * upp
        self.upp = upp
        owner_ub = self._owner_units(md, J)
        self.owner = owner_ub is not None
        self.twoshot = None
        W = self.size if (self.zero and not self.owner) else 1
        if self.owner:
            ub = owner_ub
            pb = [u * upp for u in ub]
            P_pad = P
            lengths = [pb[i + 1] - pb[i] for i in range(len(pb) - 1)]
        else:
            if self.zero and dev.type == "cuda":
                # two-shot: 2 chunks by default when the overlapped schedule may be chosen
                # (side stream auto), else 1 -- each chunk is one more cross-rank rendezvous
                nch = self._chunks_override or (
                    self.nchunks_req if self._chunks_explicit
                    else (2 if cfg.side_stream == "auto" else 1))
                ub, pb, P_pad, lengths = plan_chunks(J, upp, W, nch)
                self.twoshot = self._connect_twoshot(P_pad)  # collective
            if self.twoshot is None:
                ub, pb, P_pad, lengths = plan_chunks(J, upp, W, self.nchunks_req)
        hint = getattr(md, "engine_layout_hint", None)
        changed = True
        if hint is not None:  # e.g. lanes grouped by forward path at the starting point
            changed = bool(hint(guess))
        cur = getattr(md, "engine_chunks_current", None)
        if changed or cur is None or not cur(ub):
            # (a model that reports its current chunks keeps its layout when neither the
            # chunks nor the layout classes changed: no rebuild on a repeated run)
            trace(f"engine: layout ({'owner' if self.owner else 'dense'}, {len(ub) - 1} chunks)")
            md.engine_set_chunks(ub)
            self.stats["layouts"] += 1
        self._ub = list(ub)
        if self.size > 1 and dev.type == "cuda" and self.fuse_epilogue:
            from ..parallel.xgmi import get_oneshot
            trace("engine: one-shot connect")
            self.oneshot = get_oneshot(self.comm)  # collective (all ranks run setup)
            trace(f"engine: one-shot {'up' if self.oneshot is not None else 'unavailable'}")
        # Internal order: models may keep the engine vectors in their own unit order
        # (e.g. the lanes layout's slot order, for coalesced parameter/gradient access).
        # It must keep every chunk's units inside the chunk, and be the same on all ranks;
        # user-facing values (guess, bounds, params, trajectory) are permuted at the edge.
        self.pidx, self.inv_pidx = self._param_order(md, P, upp, dev)
        self.P, self.P_pad, self.pb, self.lengths = P, P_pad, pb, lengths
        self.C = len(lengths)
        # what this rank updates: its own range (owner mode), its 1/W of every chunk (ZeRO),
        # everything (replicated)
        r = self.rank
        if self.owner:
            self.slices = (_Slice(r, pb[r], pb[r + 1], 0, pb[r + 1] - pb[r], 0),)
        elif self.zero:
            n = [L // W for L in lengths]
            self.slices = tuple(_Slice(c, pb[c] + r * n[c], pb[c] + (r + 1) * n[c], sum(n[:c]),
                                       n[c], c) for c in range(self.C))
        else:
            self.slices = (_Slice(None, 0, P_pad, 0, P_pad, 0),)
        self._fwd_chunks = [r] if self.owner else list(range(self.C))
        nloc = sum(s.n for s in self.slices)
        self.lr, self.b1, self.b2, self.eps = float(learning_rate), float(b1), float(b2), float(eps)
        self.legacy = bool(legacy_bounds_jacobian)
        p0 = torch.as_tensor(guess).detach().reshape(-1).to(device=dev, dtype=torch.float32)
        assert p0.numel() == P, f"guess has {p0.numel()} params, model expects {P}"
        f32 = dict(dtype=torch.float32, device=dev)
        bounds = Bounds.from_spec(param_bounds, P, device=dev)
        if self.pidx is not None:
            p0 = p0[self.pidx]
            if bounds is not None:
                bounds = Bounds(bounds.lo[self.pidx].contiguous(), bounds.hi[self.pidx].contiguous(),
                                bounds.kind[self.pidx].contiguous())
        if bounds is not None and P_pad > P:
            pad = P_pad - P
            bounds = Bounds(torch.cat([bounds.lo, torch.full((pad,), -math.inf, **f32)]),
                            torch.cat([bounds.hi, torch.full((pad,), math.inf, **f32)]),
                            torch.cat([bounds.kind, torch.full((pad,), KIND_NONE, dtype=torch.int8,
                                                               device=dev)]))
        old_b = self.bounds
        if bounds is not None and old_b is not None and bounds.lo.shape == old_b.lo.shape and \
                torch.equal(bounds.lo, old_b.lo) and torch.equal(bounds.hi, old_b.hi):
            bounds = old_b  # the same box: the same tensors (graphs captured on them stay valid)
        self.bounds = bounds
        if self.twoshot is not None:
            # parameters and gradient live in the exported peer-memory regions
            theta = self.twoshot.theta
            theta.zero_()
            self.grad = self.twoshot.grad
            self.grad.zero_()
        else:
            theta = self._buf("theta", P_pad)
            self.grad = self._buf("grad", P_pad)
        theta[:P] = p0
        if bounds is not None:  # the recorded start is T^-1(T(guess)), as the reference
            theta.copy_(bounds.inverse(bounds.forward(theta)))
        self.theta = theta
        nS = md.engine_nS()
        self.nS = nS
        self.rows = [md.engine_fwd_rows(c) for c in range(self.C)]
        self.S = self._buf("S", nS)
        self.slab = self._buf("slab", max(1, sum(self.rows)) * nS)
        self.h = self._buf("h", nS + 1)
        self.loss = self._buf("loss", 1)
        self.step_dev = self._buf("step_dev", (self.C, 2), torch.int32)
        self.m = self._buf("m", nloc)
        self.v = self._buf("v", nloc)
        self.g_loc = self._buf("g_loc", nloc) if W > 1 else None
        # bounded: Adam runs on u = T(theta) of the rank's slices, p = T^-1(u) lands in theta
        self.bounds_loc = self._local_bounds(bounds)
        self.u = None
        if bounds is not None:
            self.u = self._buf("u", nloc)
            self.u.copy_(self.bounds_loc.forward(self._local(theta)))
        self.step_host = 0
        self.nsteps = int(nsteps)
        sharded = self.zero or self.owner
        hmode = history if not (sharded and history == "full") else "last"
        self.history = History(hmode, nsteps, theta[:P].detach().clone(),
                               buf=self._bufs.get("history") if hmode == "full" else None)
        if hmode == "full":
            self._bufs["history"] = self.history.buf
        self.traj_loc = None
        self.history_mode = history
        if sharded and history == "full":
            self.traj_loc = self._buf("traj_loc", (self.nsteps + 1, nloc))
            self.traj_loc[0] = self._local(theta)
        if W > 1 and self.comm_ag is None and self.twoshot is None and cfg.ag_comm:
            self.comm_ag = self.comm.split(0)
        self._ag = [None] * self.C
        self.comm_stream = None
        self.ts_side = False
        # hashed placement with the two-shot context up: RCCL reduce-scatter / all-gather
        # stays available as an autotune candidate (on the same buffers and shard layout)
        self.rccl_exchange = self.twoshot is not None and cfg.hashed_exchange == "rccl"
        self.ts_blocks = cfg.twoshot_blocks
        if self.twoshot is not None and self.C > 1 and cfg.side_stream != "off":
            # overlapped schedule: the two-shot exchange of chunk c runs on a side stream as
            # soon as the VJP of chunk c is done (overlapping the VJP of chunk c+1), and the
            # next step's forward of chunk c waits only for that chunk's exchange; its grid
            # is capped so the compute kernels keep most CUs.  "auto" (default) times both
            # schedules on this machine at setup (_autotune) and keeps the faster: with
            # two ranks sharing one GPU the side stream only adds event waits, across xGMI
            # it hides part of the exchange behind compute.
            self.comm_stream = torch.cuda.Stream(device=dev)
            self.ev_vjp = [torch.cuda.Event() for _ in range(self.C)]
            self.ev_ts = [torch.cuda.Event() for _ in range(self.C)]
            self.ts_side = cfg.side_stream == "on"
        self._ts_pending = [False] * self.C
        # fused exchange ("ts_fused"): the two-shot exchange of chunk c-1 runs in the first
        # workgroups of chunk c's VJP launch and the last chunk's in the next step's first
        # forward launch (csrc/twoshot.h) -- overlap with compute on ONE stream, no events.
        # >= 2 chunks on a model whose kernels carry it (bounded fits: modes 2 / 3).
        # MULTIGRAD_TWOSHOT_FUSED: auto (an autotune candidate), on (always, no tuning), off
        self._x_pending = None  # packed exchange of the last chunk, for the next launch
        self.ts_fused_ok = bool(
            cfg.twoshot_fused != "off" and self.twoshot is not None and self.C > 1
            and getattr(md, "engine_fused_exchange_ok", lambda: False)())
        self.ts_fused = self.ts_fused_ok and cfg.twoshot_fused == "on"
        if self.ts_fused:
            self.ts_side = False
        self.pending = False
        ok = getattr(md, "engine_pipeline_ok", None)
        pchunk = self.slices[0].chunk
        self.pipeline = bool(
            cfg.pipeline and self.fuse_vjp_adam
            and (self.owner or (not self.zero and self.C == 1 and self.size == 1))
            and ok is not None and hasattr(md, "engine_forward_update_chunk")
            and (ok(pchunk) if bounds is None else ok(pchunk, bounded=True)))
        # a step can be captured when every collective in it is a peer-memory kernel with
        # its sequence number in device memory (one-shot sumstats, two-shot gradient) --
        # RCCL/gloo calls are not captured
        # (the fused exchange carries a step's last exchange into the next step: eager only)
        self.capturable = dev.type == "cuda" and not self.ts_fused and (
            self.size == 1 or (self.oneshot is not None and self.fuse_epilogue and
                               (self.owner or (self.twoshot is not None and not self.ts_side))))
        if self._graph_auto:
            # a pipelined step is two launches (forward+update, epilogue); replaying them
            # from a graph measured 1-5% slower than eager launches (tools/archive/graph_ab_full.sh).
            # Multi-rank steps are capturable (MULTIGRAD_GRAPH=1, tested bitwise against
            # eager) but replays measured 7x slower than the 4 eager launches of the hashed
            # step with two ranks on one GPU (profiles/twoshot_2rank.md): eager by default.
            self.use_graph = self.capturable and not self.pipeline and self.size == 1
        elif self.use_graph and not self.capturable:
            self.use_graph = False  # e.g. RCCL collectives in the step: eager launches
        self._bind()
        gk = self._graph_key()
        if gk != self._gkey:  # a buffer or scalar the captured graphs baked in changed
            self.graph = None
            self._gkey = gk
        self.tuning = None
        self._tuning = False
        self._relayout_init()
        self.ready = True
        if self.size > 1 and dev.type == "cuda":
            # line the ranks up before the first peer-memory exchange: a kernel waits for
            # its peers at most MULTIGRAD_ONESHOT_TIMEOUT, and the setup above (data layout,
            # sorts, first code-object loads) takes different times on different ranks
            torch.cuda.synchronize()
            self.comm.barrier()
        self.stats["setups"] += 1
        cands = self._candidates() if (tune and dev.type == "cuda" and cfg.autotune != "off") else []
        if cands:
            self._autotune(cands, min_window_s=1e-3 * cfg.autotune_window_ms)
        return self

    def _local(self, t: torch.Tensor) -> torch.Tensor:
        """This rank's part of a full (internal order) vector, last dimension: its slices
        side by side, as the local vectors hold them (``t`` itself where that is all)."""
        if len(self.slices) == 1:
            s = self.slices[0]
            return t if (s.a == 0 and s.b >= t.shape[-1]) else t[..., s.a:s.b]
        return torch.cat([t[..., s.a:s.b] for s in self.slices], -1)

    def _local_bounds(self, bounds: Optional[Bounds]) -> Optional[Bounds]:
        if bounds is None:
            return None
        return Bounds(self._local(bounds.lo).contiguous(), self._local(bounds.hi).contiguous(),
                      self._local(bounds.kind).contiguous())

    def _bind(self) -> None:
        """Per slice, the arguments of its update launches that depend only on the setup
        (:meth:`_adam_args`): views of the local vectors, of theta and of the trajectory,
        built once instead of per step.  Rebuilt wherever one of those tensors is re-bound
        (``_setup``, ``relayout``; a loaded checkpoint and the autotune's restore copy into
        the same tensors)."""
        traj = self.traj_loc if self.traj_loc is not None else (
            self.history.buf if self.history.mode == "full" else None)
        flat = None if traj is None else traj.reshape(-1)
        bl = self.bounds_loc
        self._bound = []
        for s in self.slices:
            # replicated with a full trajectory: its rows are P long, so the update covers
            # the real parameters only and the kernel writes exactly one row
            n = self.P if (s.chunk is None and traj is not None) else s.n
            th = _cut(self.theta, s.a, n)
            self._bound.append(dict(
                u=th if self.u is None else _cut(self.u, s.o, n), m=_cut(self.m, s.o, n),
                v=_cut(self.v, s.o, n),
                g=_cut(self.grad, s.a, n) if self.g_loc is None else _cut(self.g_loc, s.o, n),
                p=None if self.u is None else th, step=self.step_dev[s.step], lr=self.lr,
                b1=self.b1, b2=self.b2, eps=self.eps,
                bounds=None if bl is None else Bounds(_cut(bl.lo, s.o, n), _cut(bl.hi, s.o, n),
                                                      _cut(bl.kind, s.o, n)),
                legacy=self.legacy, traj_base=None if flat is None else flat[s.o:],
                traj_stride=0 if traj is None else traj.shape[1]))

    def _adam_args(self, s: _Slice, host_step: Optional[int]) -> dict:
        """Everything an update of slice ``s`` takes, named as :func:`adam_step_` names it:
        the ``u`` / ``m`` / ``v`` / ``g`` / ``p`` views, the slice's step counter, its part of
        the box, the trajectory base and row stride (none while the autotune steps run) and
        the Adam scalars."""
        if self._tuning:
            return dict(self._bound[s.step], traj_base=None, traj_stride=0, host_step=host_step)
        return dict(self._bound[s.step], host_step=host_step)

    def _adam(self, s: _Slice, host_step: Optional[int]) -> None:
        adam_step_(**self._adam_args(s, host_step))

    def _graph_key(self):
        """Everything a captured step bakes in: the identity of every buffer it reads or
        writes and the launch scalars.  Equal keys across setups keep the graphs."""
        ids = [id(t) for t in (
            self.theta, self.grad, self.S, self.slab, self.h, self.loss, self.step_dev, self.m,
            self.v, self.u, self.g_loc, self.traj_loc, self.oneshot, self.twoshot)]
        for b in (self.bounds, self.bounds_loc):
            ids += [None] if b is None else [id(b.lo), id(b.hi), id(b.kind)]
        ids.append(id(self.history.buf) if self.history.mode == "full" else None)
        md = self.model
        epoch = getattr(md, "engine_layout_epoch", None)
        return (tuple(ids), self.lr, self.b1, self.b2, self.eps, self.legacy, self.pipeline,
                self.owner, self.zero, self.C, None if epoch is None else epoch())

    # ------------------------------------------------------------------ helpers
    def _ts_args(self, s: _Slice, max_blocks: int):
        """Slice ``s``'s two-shot exchange (reduce-scatter -> Adam -> all-gather; bounded
        fits: Adam on u, modes 2 / 3) as the arguments of ``twoshot.step`` / ``.pack``."""
        A = self._adam_args(s, self._hstep())
        bnd = A["bounds"]
        mode = 1 if bnd is None else (3 if self.legacy else 2)
        return (s.a, s.n, mode), dict(
            m=A["m"], v=A["v"], u=None if bnd is None else A["u"], bounds=bnd,
            traj=A["traj_base"], traj_stride=A["traj_stride"], step=A["step"],
            host_step=A["host_step"], lr=self.lr, b1=self.b1, b2=self.b2, eps=self.eps,
            max_blocks=max_blocks)

    def _ts_pack(self, c: int) -> bytes:
        """Chunk c's two-shot exchange as packed launch arguments for a compute launch that
        carries it (fused exchange)."""
        pos, kw = self._ts_args(self.slices[c], self.ts_blocks)
        return self.twoshot.pack(*pos, **kw)

    def _flush_exchange(self):
        """Launch the pending exchange of the last chunk on its own (fused exchange)."""
        if self._x_pending is not None:
            from ..ops._ext import ext
            xs, self._x_pending = self._x_pending, None
            if not self._inject_fault():
                ext().xgmi_twoshot_launch_packed(xs)

    def _twoshot_update(self, c: int):
        """Chunk c: dense-gradient reduce-scatter + Adam on the owned slice + all-gather,
        one launch on the side stream after the chunk's VJP."""
        side = self.ts_side
        if self._inject_fault():
            return  # test hook: this rank skips one exchange, so its peers time out
        if side:
            self.ev_vjp[c].record(torch.cuda.current_stream())
            self.comm_stream.wait_event(self.ev_vjp[c])
        pos, kw = self._ts_args(self.slices[c], self.ts_blocks if side else 0)
        with torch.cuda.stream(self.comm_stream) if side else contextlib.nullcontext():
            self.twoshot.step(*pos, **kw)
        if side:
            self.ev_ts[c].record(self.comm_stream)
            self._ts_pending[c] = True

    def _reduce_scatter(self, s: _Slice):
        """ZeRO over RCCL: start the sum of chunk ``s.chunk``'s gradient into this rank's
        shard of it."""
        pa, L = self.pb[s.chunk], self.lengths[s.chunk]
        return self.comm.reduce_scatter_tensor(self._bound[s.step]["g"], self.grad[pa:pa + L],
                                               async_op=True)

    def _all_gather(self, s: _Slice) -> None:
        """ZeRO over RCCL: start the all-gather of chunk ``s.chunk``'s parameters from every
        rank's slice of it (joined by :meth:`_drain`)."""
        pa, L = self.pb[s.chunk], self.lengths[s.chunk]
        agc = self.comm_ag if self.comm_ag is not None else self.comm
        self._ag[s.chunk] = agc.all_gather_into_tensor(self.theta[pa:pa + L],
                                                       self.theta[s.a:s.b], async_op=True)

    def _ph(self, name: str):
        if self._capturing or not self.timer.enabled:
            return contextlib.nullcontext()
        return self.timer.phase(name)

    def _drain(self, c):
        """Wait for chunk c's parameter all-gather (stream-ordered)."""
        if self._ts_pending[c]:
            torch.cuda.current_stream().wait_event(self.ev_ts[c])
            self._ts_pending[c] = False
        w = self._ag[c]
        if w is None:
            return
        w.wait()
        self._ag[c] = None

    def _drain_all(self):
        self._flush_exchange()
        for c in range(self.C):
            self._drain(c)

    @on_engine_stream
    def drain(self):
        """Join pending parameter all-gathers and exchanges and apply a pending (pipelined)
        update."""
        self._drain_all()
        if self.pending:
            self.pending = False
            s, = self.slices  # pipelined: owner mode or one replicated chunk
            hs = self._hstep(self.step_host - 1)
            if self.bounds is not None:
                # residual VJP and the bounded Adam kernel (csrc/adam.hip; the end of a run
                # or a checkpoint)
                self.model.engine_vjp_into(self.theta, self.h, self.grad, chunk=s.chunk)
                self._adam(s, hs)
            else:
                ok = self._fused_vjp_adam(s, hs)
                assert ok, "pipelined engine lost its fused VJP + Adam path"

    # ------------------------------------------------------------------ one step
    def _update_args(self, step_idx: int) -> dict:
        """Arguments of the pending (pipelined) VJP + Adam of step ``step_idx``."""
        s = self.slices[0]
        A = self._adam_args(s, self._hstep(step_idx))
        args = dict(h=self.h, m=A["m"], v=A["v"], unit_offset=s.a // self.upp, step=A["step"],
                    host_step=A["host_step"], lr=self.lr, b1=self.b1, b2=self.b2, eps=self.eps,
                    traj=A["traj_base"], traj_stride=A["traj_stride"])
        bnd = A["bounds"]
        if bnd is not None:  # bounded: Adam on u (indexed like m, v), p = T^-1(u)
            args.update(u=A["u"], lo=bnd.lo, hi=bnd.hi, legacy=self.legacy)
        return args

    def _forward_loss(self, update: bool = False):
        md = self.model
        row = 0
        fused = getattr(md, "engine_reduce_loss_into", None)
        fused_ok = (fused is not None and self.fuse_epilogue
                    and (self.size == 1 or self.oneshot is not None) and self.slab.is_cuda)
        advance = None
        # the last chunk's forward host call also issues the epilogue launch (one host call
        # per step fewer; ops/smf.py:smf_forward_into, csrc/smf_lanes.hip:smf_forward_lanes)
        fold = fused_ok and self.cfg.fold_epilogue and \
            getattr(md, "engine_forward_epilogue_ok", lambda: False)()
        chunks = self._fwd_chunks
        folded = False
        with self._ph("forward"):
            for i, c in enumerate(chunks):
                self._drain(c)
                epi = None
                if fold and i == len(chunks) - 1:
                    epi = dict(slab=self.slab, row0=row, S=self.S, loss=self.loss, h=self.h,
                               oneshot=self.oneshot if self.size > 1 else None, advance=None)
                kw = {} if epi is None else {"epilogue": epi}
                if update:  # the previous step's VJP + Adam, fused into this forward
                    args = self._update_args(self.step_host - 1)
                    if fused_ok and args["host_step"] is None:
                        # device step counter: advanced by the epilogue launch, not a kernel
                        args["defer_advance"] = True
                        advance = args["step"]
                    if epi is not None:
                        epi["advance"] = advance
                    n = md.engine_forward_update_chunk(self.theta, self.slab[row * self.nS:], c,
                                                       args, **kw)
                else:
                    if i == 0 and self._x_pending is not None:
                        # the previous step's exchange of the last chunk, in this launch's
                        # first workgroups (this chunk's parameters are already complete)
                        kw["exchange"] = self._x_pending
                        self._x_pending = None
                        if self._inject_fault():
                            del kw["exchange"]
                    n = md.engine_forward_chunk(self.theta, self.slab[row * self.nS:], c, **kw)
                folded = epi is not None
                row += n
        if folded:
            return
        if fused_ok:
            with self._ph("sumstat_epilogue"):
                if fused(self.slab, row, self.S, self.loss, self.h, self.oneshot,
                         advance=advance):
                    return
        assert advance is None, "the step counter advance was deferred to the epilogue"
        with self._ph("forward"):
            md.engine_reduce(self.slab, row, self.S)
        if self.size > 1:
            with self._ph("sumstat_allreduce"):
                self.comm.all_reduce(self.S)
        with self._ph("loss"):
            md.engine_loss_into(self.S, self.loss, self.h)

    def _enqueue_step(self):
        """One step's launches.  The placements differ in the collectives only; every update
        takes its arguments from :meth:`_adam_args`."""
        md = self.model
        if self.pipeline:
            # step k = [VJP + Adam of step k-1 fused into the forward of step k] + epilogue;
            # the update of step k stays pending until the next step or drain()
            self._forward_loss(update=self.pending)
            self.pending = True
            return
        self._forward_loss()
        hs = self._hstep()
        if self.owner:  # the gradient of the own range is complete locally: no collective
            s = self.slices[0]
            if not self._fused_vjp_adam(s, hs):
                with self._ph("vjp"):
                    md.engine_vjp_into(self.theta, self.h, self.grad, chunk=s.chunk)
                with self._ph("adam"):
                    self._adam(s, hs)
        elif self.zero and self.twoshot is not None and not self.rccl_exchange and self.ts_fused:
            # VJP_0, [VJP_1 + X_0], ..., [VJP_{C-1} + X_{C-2}]; X_{C-1} rides on the next
            # step's first forward launch (or drain())
            for c in range(self.C):
                xs = self._ts_pack(c - 1) if c > 0 else None
                with self._ph("vjp"):
                    md.engine_vjp_into(self.theta, self.h, self.grad, chunk=c, exchange=xs)
            self._x_pending = self._ts_pack(self.C - 1)
        elif self.zero and self.twoshot is not None and not self.rccl_exchange:
            for c in range(self.C):
                with self._ph("vjp"):
                    md.engine_vjp_into(self.theta, self.h, self.grad, chunk=c)
                self._twoshot_update(c)
        elif self.zero:
            rs = []
            for s in self.slices:
                with self._ph("vjp"):
                    md.engine_vjp_into(self.theta, self.h, self.grad, chunk=s.chunk)
                rs.append(self._reduce_scatter(s))
            for s, w in zip(self.slices, rs):
                with self._ph("grad_reduce_scatter_wait"):
                    w.wait()
                with self._ph("adam"):
                    self._adam(s, hs)
                self._all_gather(s)
        elif self.C == 1 and self._fused_vjp_adam(self.slices[0], hs):
            pass
        else:
            with self._ph("vjp"):
                for c in range(self.C):
                    md.engine_vjp_into(self.theta, self.h, self.grad,
                                       chunk=c if self.C > 1 else None)
            if self.size > 1:
                with self._ph("grad_allreduce"):
                    self.comm.all_reduce(self.grad)
            with self._ph("adam"):
                self._adam(self.slices[0], hs)

    def _fused_vjp_adam(self, s: _Slice, host_step: Optional[int]) -> bool:
        """Fused VJP + Adam when the gradient is complete locally (owner mode, or one
        replicated chunk), the parameters are unbounded and the model offers it."""
        md = self.model
        fn = getattr(md, "engine_vjp_adam_into", None)
        if fn is None or not self.fuse_vjp_adam or self.bounds is not None:
            return False
        with self._ph("vjp_adam"):
            A = self._adam_args(s, host_step)
            return bool(fn(self.theta, self.h, A["m"], A["v"], s.a // self.upp, A["step"],
                           host_step, self.lr, self.b1, self.b2, self.eps,
                           traj_base=A["traj_base"], traj_stride=A["traj_stride"], chunk=s.chunk))

    def _hstep(self, idx: Optional[int] = None):
        """The 0-based step for eager launches; None inside a graph capture and for every
        launch of a graph-mode engine (the Adam kernels then keep the step in device
        memory, so graph replays and eager launches -- e.g. direct step() calls, which
        launch eagerly -- agree)."""
        if self._capturing or self.use_graph or (self.device_step and self.pipeline):
            return None
        return self.step_host if idx is None else idx

    def _capture(self, k: int = 1):
        """Capture ``k`` consecutive steps into one graph (k = 1: ``self.graph``; k > 1:
        the block graph).  Every step inside reads and advances the device step counter,
        so a block replays exactly like k one-step replays."""
        md = self.model
        prep = getattr(md, "engine_prepare", None)
        if prep is not None:
            prep(list(self._fwd_chunks))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        torch.cuda.current_stream().wait_stream(s)
        from .generic import _no_gc
        g = torch.cuda.CUDAGraph()
        pend = self.pending
        self._capturing = True
        try:
            with _no_gc():  # no CUDAGraph may be freed by the collector during a capture
                with torch.cuda.graph(g):
                    for _ in range(int(k)):
                        self._enqueue_step()  # pipelined: sets pending for the next one
        finally:
            self._capturing = False
            self.pending = pend
        self.stats["captures"] += 1
        if k == 1:
            self.graph = g
        else:
            self._kgraph = (int(k), g)

    def _block_ok(self) -> bool:
        """Whether steps may run as replays of a multi-step graph: graph mode, and no
        per-step host work (the trajectory rows are written on the device)."""
        return (self.use_graph and self.graph_steps > 1 and
                (self.history.mode == "full" or self.traj_loc is not None))

    def _run_steps(self, n: int):
        """``n`` steps without the host-side history bookkeeping: blocks of
        ``graph_steps`` steps replayed from one graph where allowed, the rest one by one."""
        n = int(n)
        K = self.graph_steps
        while n > 0:
            if n >= K and self._block_ok() and (self.pending or not self.pipeline):
                if self._kgraph is None or self._kgraph[0] != K:
                    self._capture(K)
                self._kgraph[1].replay()
                if self.pipeline:
                    self.pending = True
                self.step_host += K
                n -= K
            else:
                self._raw_step()
                n -= 1
            self._maybe_relayout()

    @on_engine_stream
    def steps(self, n: int):
        """Enqueue ``n`` optimizer steps (asynchronous on GPU): :meth:`step` ``n`` times,
        with blocks of ``graph_steps`` steps replayed from one graph in graph mode."""
        assert self.ready, "call setup() first"
        n = int(n)
        if n <= 0:
            return
        if not self._block_ok():
            for _ in range(n):
                self._step(replay=True)
            return
        if self.step_host + n > self.nsteps and self.history.mode == "full":
            raise RuntimeError("more steps than the trajectory buffer was sized for")
        self._run_steps(n)

    def _raw_step(self, replay: bool = True):
        if replay and self.use_graph and (self.pending or not self.pipeline):
            if self.graph is None:
                self._capture()
            self.graph.replay()
            if self.pipeline:
                self.pending = True
        else:
            self._enqueue_step()
        self.step_host += 1

    @on_engine_stream
    def step(self):
        """Enqueue one optimizer step (asynchronous on GPU).  A direct call launches eagerly
        even in graph mode unless ``step_replay`` is set (``MULTIGRAD_STEP_REPLAY=1``), as
        :meth:`GraphAdamEngine.step <multigrad_amd.engine.generic.GraphAdamEngine.step>`;
        :meth:`steps` and ``run_adam`` replay."""
        self._step(replay=self.step_replay)

    def _step(self, replay: bool = True):
        assert self.ready, "call setup() first"
        if self.step_host >= self.nsteps and self.history.mode == "full":
            raise RuntimeError("more steps than the trajectory buffer was sized for")
        self._raw_step(replay)
        self._record_history()
        self._maybe_relayout()

    def _record_history(self) -> None:
        """Host-side trajectory bookkeeping after a step (history "last" / stride)."""
        if self.history.mode != "full" and self.traj_loc is None:
            st = self.history.stride
            due = self.step_host == self.history.nsteps or (st and self.step_host % st == 0)
            if self.pipeline and not due:
                return
            self.drain()
            if not self.owner:
                self.history.record(self.step_host - 1, self.theta[:self.P])
            elif due:  # (collective)
                self.history.record(self.step_host - 1, self._assemble(self._local_theta()))

    def to_user(self, t: torch.Tensor) -> torch.Tensor:
        """Engine (internal) parameter order -> the model's parameter order (last dim)."""
        if self.pidx is None:
            return t
        return t[..., self.inv_pidx]

    @on_engine_stream
    def trajectory(self) -> torch.Tensor:
        """The recorded parameter trajectory (assembled across ranks where it is sharded)."""
        self.drain()
        self.check("trajectory", collective=True)
        if self.traj_loc is None:
            if self.history.mode == "full":
                out = self._traj_to_user(self.history.result())
                if out.untyped_storage().data_ptr() == self.history.buf.untyped_storage().data_ptr():
                    out = out.clone()  # the buffer is the engine's: a later run rewrites it
                return out
            return self.to_user(self.history.result())
        rows = self.step_host + 1
        return self._traj_to_user(self._assemble(self.traj_loc[:rows].contiguous()))

    @on_engine_stream
    def params(self) -> torch.Tensor:
        self.drain()
        self.check("params", collective=True)
        if self.owner:
            return self.to_user(self._assemble(self._local_theta()))
        # a copy: theta may be the peer-memory region a later engine reuses
        return self.to_user(self.theta[:self.P]).clone()

    @on_engine_stream
    def last_loss(self) -> float:
        loss = float(self.loss.item())
        self.check("last_loss")
        return loss

    @on_engine_stream
    def check(self, where: str = "", collective: bool = False) -> None:
        """Raise :class:`~multigrad_amd.parallel.xgmi.CollectiveTimeout` if a peer-memory
        exchange of this engine (one-shot sumstats, two-shot gradient) timed out -- its
        results are NaN-poisoned; a host sync.

        ``collective=True`` all-reduces the verdict so every rank raises together (used
        where the caller goes on to a collective: ``params``, ``trajectory``,
        checkpoints, the periodic check of :meth:`run_adam`); ``last_loss`` and
        ``state_dict`` check locally."""
        where = where or f"engine step {self.step_host}"
        comm = self.comm if collective else None
        for ctx in (self.twoshot, self.oneshot):
            if ctx is not None:
                ctx.check(where, comm=comm)

    def grad_collective_name(self) -> str:
        """Human-readable name of the per-step gradient collective (bench records)."""
        if self.size == 1:
            return "none (1 rank)"
        if self.owner:
            return "none: owner-local gradients, sumstat all-reduce only"
        if self.zero and self.twoshot is not None and self.rccl_exchange:
            return ("RCCL reduce-scatter + all-gather (ZeRO-1), measured faster than the "
                    "two-shot kernel at setup")
        if self.zero and self.twoshot is not None:
            if self.ts_fused:
                sched = (f", {self.C} chunks, each exchange in the first workgroups of the "
                         f"next compute launch (fused exchange, one stream, no events)")
            elif self.ts_side:
                sched = f", {self.C} chunks on a side stream overlapping compute"
            else:
                sched = f", {self.C} chunk(s) on the compute stream"
            return ("xGMI two-shot kernel: reduce-scatter + Adam + all-gather in one launch per "
                    "chunk (self-tested)" + sched)
        if self.zero:
            return "RCCL reduce-scatter + all-gather (ZeRO-1)"
        return "RCCL all-reduce"

    def comm_bytes_per_step(self) -> int:
        """Bytes this rank sends through collectives in one step: the sumstat exchange,
        plus the dense-gradient exchange of the hashed placement (reduce-scatter and
        parameter all-gather, or an all-reduce: 2 (W-1)/W of the vector either way)."""
        W = self.size
        if W == 1:
            return 0
        nbytes = 4 * self.nS * (W - 1)  # one-shot push (RCCL moves about as much)
        if not self.owner:
            nbytes += int(2 * (W - 1) * (self.P_pad // W) * 4)
        return nbytes

    def sumstat_collective_name(self) -> str:
        if self.size == 1:
            return "none (1 rank)"
        return "xGMI one-shot kernel (self-tested)" if self.oneshot is not None else "RCCL"

    # ------------------------------------------------------------------ L-BFGS objective
    def lbfgs_objective(self, guess):
        """Objective over this rank's optimizer-owned parameters for
        :func:`multigrad_amd.optim.lbfgs.lbfgs_minimize` (sharded under ZeRO)."""
        self.setup(guess, nsteps=1, history="last", tune=False)  # it never runs optimizer steps
        return _EngineObjective(self)

    # ------------------------------------------------------------------ driver
    @on_engine_stream(always=True)
    def run_adam(self, guess, nsteps: int = 100, param_bounds=None, learning_rate: float = 0.01,
                 b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, history="full",
                 legacy_bounds_jacobian: bool = False, callback=None,
                 checkpoint_path: Optional[str] = None, checkpoint_every: int = 0,
                 resume_from: Optional[str] = None, **unused):
        """Adam with the reference's return contract: trajectory ``(nsteps+1, P)``.

        ``checkpoint_path``/``checkpoint_every`` write a resumable state every k steps
        (owner-/ZeRO-sharded runs write one file per rank, ``<path>.rank<r>``);
        ``resume_from`` continues such a run (same number of ranks and placement)."""
        if unused:
            raise TypeError(f"unsupported run_adam options for the fused engine: {sorted(unused)}")
        self.setup(guess, nsteps, param_bounds, learning_rate, b1, b2, eps, history,
                   legacy_bounds_jacobian)
        start = self.load_checkpoint(resume_from) if resume_from is not None else 0
        from ..utils.hooks import StepHooks, driver_guard
        hooks = StepHooks(self.comm, callback)  # MULTIGRAD_CHECK_EVERY / MULTIGRAD_METRICS
        err_every = self.cfg.err_check_every
        err_every = err_every if (self.oneshot is not None or self.twoshot is not None) else 0
        ck_every = checkpoint_every if checkpoint_path else 0
        with driver_guard(self.comm):
            comm_bytes = self.comm_bytes_per_step()
            i, end = start, int(nsteps)
            while i < end:
                # steps up to the next host event run as one call (graph blocks)
                n = 1 if hooks.active else min(
                    [end - i] + [e - i % e for e in (err_every, ck_every) if e])
                self.steps(n)
                i += n
                if hooks.active:
                    hooks(i - 1, self.loss, self, self.params, comm_bytes=comm_bytes)
                if err_every and i % err_every == 0:
                    self.check(collective=True)
                if ck_every and i % ck_every == 0:
                    self.save_checkpoint(checkpoint_path)
            return self.trajectory()
