"""Setup-time tuning of the fused engine: which schedule (and, for the hashed two-shot
exchange, how many chunks) runs fastest on this machine -- measured, not assumed."""
from __future__ import annotations

import math
import time
from typing import Optional

import torch

from ..utils.trace import trace


def _best_ms(tuning) -> float:
    """Fastest measured candidate of an autotune record (dropped candidates have no time)."""
    ms = [c["ms"] for c in tuning["candidates"] if c.get("ms") is not None]
    return min(ms) if ms else math.inf


class _TuneMixin:
    def _setup_chunks(self, n: int, guess, nsteps: int, kw: dict) -> None:
        """Set up again with ``n`` chunks, without tuning."""
        self._chunks_override = n
        self._setup(guess, nsteps, tune=False, **kw)

    def _tune_chunks(self, ck, guess, nsteps: int, kw: dict) -> None:
        """Hashed placement on several GPUs with the two-shot exchange and no explicit chunk
        count (see :meth:`setup`): time one chunk and, when the overlapped two-chunk schedule
        won, four overlapped chunks against the two just tuned; keep the fastest."""
        tun = self.tuning
        if not (tun and self.twoshot is not None and not self.owner and self.C == 2
                and not self._chunks_explicit and "ts_side" in tun["chosen"]
                and not tun.get("budget_skipped") and not tun.get("cached")):
            return
        window_s = 1e-3 * self.cfg.autotune_window_ms
        t2 = _best_ms(tun)
        self._setup_chunks(1, guess, nsteps, kw)
        cands = [{"ts_side": False, "rccl_exchange": False}]
        if self.cfg.hashed_exchange != "twoshot":
            cands.append({"ts_side": False, "rccl_exchange": True})
        self._autotune(cands, min_window_s=window_s)
        t1 = _best_ms(self.tuning)
        tun1 = self.tuning
        chunk_times = {"1": t1, "2": t2}
        tuned = {1: tun1, 2: tun}
        current = 1
        if self.cfg.max_chunks >= 4 and t2 < t1:
            # the overlapped schedule won with two chunks: four give the exchange of each
            # chunk a shorter wait behind its VJP and the next forward a shorter wait behind
            # its exchange (one more cross-rank rendezvous per extra chunk)
            self._setup_chunks(4, guess, nsteps, kw)
            if self.C == 4 and self.comm_stream is not None:
                self._autotune([{"ts_side": True, "rccl_exchange": False}], min_window_s=window_s)
                chunk_times["4"] = _best_ms(self.tuning)
                tuned[4] = self.tuning
                current = 4
        best = min(tuned, key=lambda c: chunk_times[str(c)])
        if best != current:
            self._setup_chunks(best, guess, nsteps, kw)
            for k, v in tuned[best]["chosen"].items():
                setattr(self, k, v)
            self.graph = None
        self.tuning = dict(tuned[best], chunks=dict(chunk_times, chosen=best))
        self._tune_cache[ck] = best
        dropped = [dict(d, chunks=n) for n, t in tuned.items() for d in t.get("dropped", [])]
        if dropped:  # candidates dropped in any of the chunk-count tunings, with the reason
            self.tuning["dropped"] = dropped

    def _candidates(self) -> list:
        """The schedules (dicts of engine attributes) this setup has to choose between."""
        cfg = self.cfg
        cands = []
        if self.comm_stream is not None and cfg.side_stream == "auto" and not self.use_graph and \
                cfg.hashed_exchange != "rccl" and not self.ts_fused:
            # hashed: where the exchange runs -- two-shot on the compute stream, on the side
            # stream, or RCCL's reduce-scatter / all-gather (measured, not assumed;
            # MULTIGRAD_HASHED_EXCHANGE=twoshot|rccl pins it)
            cands = [{"ts_side": False, "rccl_exchange": False, "ts_fused": False},
                     {"ts_side": True, "rccl_exchange": False, "ts_fused": False}]
            if self.ts_fused_ok:
                cands.append({"ts_side": False, "rccl_exchange": False, "ts_fused": True})
            if cfg.hashed_exchange != "twoshot":
                cands.append({"ts_side": False, "rccl_exchange": True, "ts_fused": False})
        elif self._graph_auto and self.capturable and (self.size == 1 or self.owner):
            # eager launches vs one-step replays vs replays of blocks of steps
            cands = [{"use_graph": False}, {"use_graph": True, "graph_steps": 1}]
            if self.graph_steps > 1 and (self.history.mode == "full" or self.traj_loc is not None):
                cands.append({"use_graph": True, "graph_steps": self.graph_steps})
        return cands

    def _tune_key(self, cands):
        return (tuple(tuple(sorted(c.items())) for c in cands), self.P, self.size, self.owner,
                self.zero, self.pipeline, self.C, self.history.mode == "full",
                self.traj_loc is not None, self.bounds is None)

    def _autotune(self, cands, warm: int = 2, min_window_s: float = 0.008, **kw):
        cfg = self.cfg
        key = self._tune_key(cands)
        hit = self._tune_cache.get(key)
        if hit is not None and hit.get("budget_skipped"):
            # a short run kept the default schedule before: again, unless this run's budget
            # (from the probe step time measured then) now affords the windows
            est = hit["step_ms_probe"] * 1e-3
            budget = cfg.tune_budget * est * max(1, self.nsteps)
            extra = warm + (self.graph_steps if any(c.get("use_graph") for c in cands) else 0)
            if cfg.autotune == "on" or \
                    int(budget / max(est, 1e-9) / (len(cands) * cfg.autotune_rounds)) - extra >= 8:
                hit = None
        if hit is not None:
            # this engine timed these candidates before (a repeated run_* call): no trial
            # steps, the verdict is applied as it is
            changed = False
            now = dict(use_graph=self.use_graph, graph_steps=self.graph_steps,
                       ts_side=self.ts_side, ts_fused=self.ts_fused,
                       rccl_exchange=self.rccl_exchange)  # what candidates assign
            for k, v in hit["chosen"].items():
                if now[k] != v:
                    setattr(self, k, v)
                    # use_graph / graph_steps choose whether (and which) graphs replay; the
                    # graphs themselves stay valid (their buffers are in the graph key)
                    changed = changed or k not in ("use_graph", "graph_steps")
            if changed:
                self.graph = None
            self.tuning = dict(hit, cached=True)
            trace(f"engine: autotune verdict cached {hit['chosen']}")
            return
        trace(f"engine: autotune {cands}")
        try:
            self._autotune_impl(cands, warm, min_window_s, **kw)
        finally:
            trace(f"engine: autotune done {self.tuning}")
        if self.tuning is not None:
            self._tune_cache[key] = {k: v for k, v in self.tuning.items() if k != "cached"}

    def _autotune_impl(self, cands, warm: int = 2, min_window_s: float = 0.008,
                       max_reps: int = 400):
        """Collective: time each candidate schedule (a dict of engine attributes) over a
        window of at least ``min_window_s`` of work after ``warm`` steps, with syncs only
        at the window edges; keep the candidate whose slowest rank was fastest, then
        restore the optimizer state.  No trajectory rows are written while tuning, so the
        recorded trajectory is that of the real steps alone.

        Besides picking the schedule measured fastest on this machine (eager launches vs
        graph replay; the hashed exchange on the compute or a side stream), the window
        length brings the GPU to its working clock before the first real step: after a
        cold start the same step ran 0.88 ms and ~0.64 ms only after ~15 ms of work
        (profiles/step_timeline.md)."""
        cfg = self.cfg
        state = [t for t in (self.theta, self.m, self.v, self.step_dev, self.u) if t is not None]
        saved = [t.clone() for t in state]
        multi = self.size > 1

        def restore():  # (copies into the same tensors: the per-slice views stay valid)
            self._drain_all()
            torch.cuda.synchronize()
            for t, v in zip(state, saved):
                t.copy_(v)
            self.pending = False
            self.step_host = 0

        def apply(c):
            for k, v in c.items():
                setattr(self, k, v)
            self.graph = None

        def window(n):
            self._drain_all()
            torch.cuda.synchronize()
            if multi:
                self.comm.barrier()
            t0 = time.perf_counter()
            self._run_steps(n)
            self._drain_all()
            torch.cuda.synchronize()
            dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
            if multi:
                self.comm.all_reduce(dt, op="max")
            return float(dt) / n

        from ..parallel.xgmi import CollectiveTimeout

        def verdict(c):
            """Collective: None if every rank's peer-memory exchanges of candidate ``c``
            completed, else the reason (and the protocols are reset on every rank, so the
            next candidate starts clean)."""
            ctxs = [x for x in (self.twoshot, self.oneshot) if x is not None]
            if not multi or not ctxs:
                return None
            flags = torch.zeros(self.size, dtype=torch.int64)
            flags[self.rank] = int(any(int(x.err.item()) for x in ctxs))
            self.comm.all_reduce(flags)
            bad = [r for r in range(self.size) if int(flags[r])]
            if not bad:
                return None
            for x in ctxs:
                x.reset(self.comm)
            return f"peer-memory exchange timed out on rank(s) {bad}"

        cands = [dict(c) for c in cands]
        dropped = []
        self._fault_seen = set()
        self._tuning = True
        try:
            apply(cands[0])
            for _ in range(warm):
                self._raw_step()
            est = window(2)
            reps = int(min(max_reps, max(8, math.ceil(min_window_s / max(est, 1e-6)))))
            restore()
            why = verdict(cands[0])
            if why is not None:  # the probe of the first candidate already failed
                dropped.append(dict(cands[0], reason=why))
            self.stats["trial_steps"] += warm + 2
            # MULTIGRAD_AUTOTUNE_ROUNDS (2) rounds, the order reversed every other round, the
            # best window of each candidate kept: a single pass in a fixed order let the
            # clock ramp of the first windows decide (the headline's eager candidate timed
            # 0.470 ms against 0.455 for 16-step replays in the first window, while
            # alternating runs measured eager 0.438 vs 0.447, profiles/graph_modes)
            rounds = cfg.autotune_rounds
            budget_s = None
            if cfg.autotune == "auto":
                # at most MULTIGRAD_TUNE_BUDGET of the requested run (est: the slowest rank's
                # step, identical on every rank, so every rank takes the same branch)
                budget_s = cfg.tune_budget * est * max(1, self.nsteps)
                extra = warm + (self.graph_steps if any(c.get("use_graph") for c in cands) else 0)
                fit = int(budget_s / max(est, 1e-9) / (len(cands) * rounds)) - extra
                if fit < 8 and why is None:
                    apply(cands[0])
                    self.tuning = {"chosen": cands[0], "budget_skipped": True,
                                   "budget_ms": round(1e3 * budget_s, 3),
                                   "step_ms_probe": round(1e3 * est, 4)}
                    self._settle(est, restore, budget_s=budget_s)
                    if multi:
                        torch.cuda.synchronize()
                        self.comm.barrier()
                    return
                reps = max(8, min(reps, fit))
            times = [math.inf] * len(cands)
            for r in range(rounds):
                order = list(range(len(cands)))
                if r % 2:
                    order.reverse()
                for i in order:
                    c = cands[i]
                    if any(d.items() >= c.items() for d in dropped):
                        times[i] = math.inf
                        continue
                    apply(c)
                    self._fault_c = c
                    for _ in range(warm):
                        self._raw_step()
                    if self._block_ok():
                        self._run_steps(self.graph_steps)  # capture (and first replay) untimed
                    t = window(reps)
                    self.stats["trial_steps"] += warm + reps
                    self._fault_c = None
                    restore()
                    why = verdict(c)
                    if why is not None:
                        dropped.append(dict(c, reason=why))
                        times[i] = math.inf
                        continue
                    times[i] = min(times[i], t)
            if all(math.isinf(t) for t in times) and self.twoshot is not None:
                # no peer-memory schedule survived: the RCCL exchange on the same buffers
                fb = {k: False for k in cands[0]}
                fb["rccl_exchange"] = True
                if fb in cands:
                    times[cands.index(fb)] = math.inf
                apply(fb)
                for _ in range(warm):
                    self._raw_step()
                t = window(reps)
                restore()
                why = verdict(fb)
                if why is not None:
                    raise CollectiveTimeout(f"setup autotune: every exchange schedule failed ({why})")
                if fb not in cands:
                    cands.append(fb)
                    times.append(t)
                else:
                    times[cands.index(fb)] = t
            self.check("setup autotune", collective=multi)
        finally:
            self._tuning = False
            self._fault_c = None
        if all(math.isinf(t) for t in times):
            raise CollectiveTimeout(f"setup autotune: every candidate failed: {dropped}")
        best = min(range(len(cands)), key=lambda i: times[i])
        apply(cands[best])
        self.tuning = {"candidates": [dict(c, ms=round(1e3 * t, 4) if math.isfinite(t) else None)
                                      for c, t in zip(cands, times)],
                       "chosen": cands[best], "steps_per_window": reps, "rounds": rounds}
        if dropped:
            self.tuning["dropped"] = dropped
        if self.use_graph:
            # capture the real (trajectory-writing) step now rather than inside the first
            # timed step
            pend = self.pending
            self.pending = self.pipeline
            self._capture()
            if self._block_ok():
                self._capture(self.graph_steps)
            self.pending = pend
        used = rounds * len(cands) * (reps + warm) * est
        self._settle(est, restore, budget_s=None if budget_s is None else max(0.0, budget_s - used))
        if multi:
            torch.cuda.synchronize()
            self.comm.barrier()

    def _settle(self, step_s: float, restore, budget_s: Optional[float] = None) -> None:
        """End the setup with ``MULTIGRAD_SETTLE_MS`` (60) of eager steps (no trajectory
        rows; the optimizer state is restored afterwards), so the first real steps do not
        start from an idle GPU.  Measured on one MI355X (profiles/narrow_sweep/README.md):
        after the ~0.1 s of host work that follows the autotune windows, the forward kernel
        ran 410 us for a few steps, then 500-585 us and only back at ~445 us after ~50 steps
        -- the power controller's transient after an idle gap; a 20-step timing from there
        measured ~1850 steps/s against ~2250 in steady state."""
        ms = self.cfg.settle_ms
        if budget_s is not None:  # MULTIGRAD_AUTOTUNE=auto: what is left of the tuning budget
            ms = min(ms, 1e3 * budget_s)
        if ms <= 0 or self.device.type != "cuda" or (budget_s is not None and ms < 1e3 * step_s):
            return
        n = int(min(2000, max(1, math.ceil(1e-3 * ms / max(step_s, 1e-5)))))
        self.stats["trial_steps"] += n
        use_graph = self.use_graph
        self._tuning = True
        self.use_graph = False  # eager launches: the captured graphs write trajectory rows
        try:
            for _ in range(n):
                self._raw_step()
            restore()
        finally:
            self._tuning = False
            self.use_graph = use_graph

    def _inject_fault(self) -> bool:
        """Test hook ``MULTIGRAD_AUTOTUNE_FAULT=<attr>=<0|1>:<rank>``: while the setup
        autotune times a candidate with that attribute value, the given rank skips one
        two-shot exchange (once per matching candidate and tuning), so its peers' exchange times
        out (bounded wait) -- the way an exchange that fails on a real xGMI node shows up."""
        spec, c = self.cfg.autotune_fault, self._fault_c
        if not spec or c is None:
            return False
        cond, _, rank = spec.partition(":")
        key, _, val = cond.partition("=")
        if key not in c or bool(c[key]) != (val.strip() == "1") or int(rank or 0) != self.rank:
            return False
        ck = tuple(sorted(c.items()))
        if ck in self._fault_seen:
            return False  # once per matching candidate
        self._fault_seen.add(ck)
        return True
