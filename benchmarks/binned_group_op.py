"""The per-group Gaussian-binned-sum op against what a user writes without it, on one MI355X.

(a) op level: forward + backward (all gradients: mu, sigma and per-object weights) of
    ``plan.binned_sum`` at nb = 10 for N = 1e4, 4e6 and 1e8 and G = 4, 64 and 1e4 groups, on a
    sorted and on a shuffled index, against
      composite: the ``ndtr`` table (laid out ``[nb + 1, N]``, so that its rows are contiguous)
                 followed by ``plan.segment_sum`` over the nb rows of bin masses;
      calls    : for G <= 64, G calls of ``gaussian_binned_sum`` on slices of operands that
                 were sorted by group at setup (so this side pays no gather per step).
(b) end to end: ``GraphAdamEngine`` steps/s of ``SampleBinnedPopulationSMFModel`` on the op
    against the same model with ``_sums`` written as the composite, at 2e5 parameters / 4e6
    halos, both captured (marginal cost per step, as benchmarks/binned_op.py).

The sides run alternately, ``--pairs`` times; one JSON line per row, with the largest relative
differences of the outputs and gradients.  ``--profile`` adds one ``torch.profiler`` pass of
each side (per-kernel microseconds).  ``--cpu`` runs tiny sizes on the CPU (a functional
check of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time
from dataclasses import dataclass

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

NB = 10
SIZES = [1e4, 4e6, 1e8]
GROUPS = [4, 64, 10_000]
MAX_CALLS_G = 64


def _edges(nb):
    """float32-representable edges, so that all sides bin alike."""
    return tuple(float(torch.tensor(9.0 + 1.5 * k / nb, dtype=torch.float32))
                 for k in range(nb + 1))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, dev):
    g = torch.Generator().manual_seed(1)
    spec = ((9.0, 1.5), (0.1, 0.4), (0.5, 1.0))  # mu, sigma, weights
    return tuple((lo + span * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
                 for lo, span in spec)


def _group_fb(plan, ops, edges, cot):
    out = plan.binned_sum(ops[0], ops[1], edges, ops[2])
    return out.detach(), torch.autograd.grad(out, ops, cot)


def composite_sums(plan, mu, sigma, edges_t, w=None):
    """The bin masses as an [nb + 1, N] ndtr table, then plan.segment_sum over its nb rows."""
    cdf = torch.special.ndtr((edges_t[:, None] - mu[None, :]) / sigma[None, :])
    d = cdf[1:] - cdf[:-1]
    if w is not None:
        d = d * w[None, :]
    return torch.stack(plan.segment_sum(*d.unbind(0)), dim=1)


def _composite_fb(plan, ops, edges_t, cot):
    out = composite_sums(plan, ops[0], ops[1], edges_t, ops[2])
    return out.detach(), torch.autograd.grad(out, ops, cot)


def _calls_fb(sorted_ops, bounds, edges, cot):
    """G calls of the single op on slices of the operands sorted by group."""
    from multigrad_amd.ops import gaussian_binned_sum
    rows = [gaussian_binned_sum(*(t[lo:hi] for t in sorted_ops[:2]), edges, sorted_ops[2][lo:hi])
            for lo, hi in bounds]
    out = torch.stack(rows)
    return out.detach(), torch.autograd.grad(out, sorted_ops, cot)


def _time_calls(fn, dev, min_s, max_calls=2000):
    """Seconds per call over a window of at least ``min_s`` (host clock around a device
    synchronise)."""
    fn()
    _sync(dev)
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 8 == 0 or calls >= max_calls or dev.type == "cpu":
            _sync(dev)
            dt = time.perf_counter() - t0
            if dt >= min_s or calls >= max_calls:
                return dt / calls


def _kernel_us(fn, dev):
    """Device microseconds per kernel name over one profiled call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    _sync(dev)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        _sync(dev)
    rows = {}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
            us = getattr(ev, "device_time", None)
            us = ev.cuda_time if us is None else us
            rows[ev.name] = round(rows.get(ev.name, 0.0) + float(us), 2)
    return rows


def _rel(a, b):
    return float((a - b).abs().max() / a.abs().max().clamp_min(1e-30))


def op_level(rows, dev, pairs, min_s, profile):
    """Returns whether the op beat the composite in every pair of every row of N >= 4e6 (the
    expectation); the other rows and the calls side are reported as they fall."""
    from multigrad_amd.ops import GroupIndex
    edges = _edges(NB)
    edges_t = torch.tensor(edges, device=dev)
    ok = True
    for n, G, shuffled in rows:
        ops = _op_inputs(n, dev)
        gen = torch.Generator().manual_seed(2)
        index = torch.randint(0, G, (n,), generator=gen)
        index = (index if shuffled else index.sort().values).to(dev)
        plan = GroupIndex(index, G)
        cot = (torch.linspace(0.5, 1.5, NB, device=dev)[None, :] *
               (1.0 + (torch.arange(G, device=dev) % 5)[:, None] / 4.0))
        sides = {"group": lambda: _group_fb(plan, ops, edges, cot),
                 "composite": lambda: _composite_fb(plan, ops, edges_t, cot)}
        if G <= MAX_CALLS_G:
            order = slice(None) if plan.perm is None else plan.perm.long()
            sorted_ops = tuple(t.detach()[order].clone().requires_grad_(True) for t in ops)
            off = plan.offsets.tolist() + [n]
            bounds = [(off[g], off[g + 1]) for g in range(G) if off[g + 1] > off[g]]
            live = torch.tensor([g for g in range(G) if off[g + 1] > off[g]], device=dev)
            sides["calls"] = lambda: _calls_fb(sorted_ops, bounds, edges, cot[live])
        got = sides["group"]()
        ref = sides["composite"]()
        err = _rel(ref[0], got[0])
        gerr = max(_rel(a, b) for a, b in zip(ref[1], got[1]))
        del ref, got
        for p in range(pairs):
            t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
            if n >= 4e6:
                ok = ok and t["group"] < t["composite"]
            row = {"bench": "op", "n": n, "G": G, "nb": NB, "shuffled": shuffled, "pair": p,
                   "group_ms": round(t["group"] * 1e3, 4),
                   "composite_ms": round(t["composite"] * 1e3, 4),
                   "speedup_vs_composite": round(t["composite"] / t["group"], 2),
                   "group_us_per_1e6_objects": round(t["group"] * 1e12 / n, 2),
                   "max_rel_out_diff": err, "max_rel_grad_diff": gerr}
            if "calls" in t:
                row["calls_ms"] = round(t["calls"] * 1e3, 4)
                row["speedup_vs_calls"] = round(t["calls"] / t["group"], 2)
            print(json.dumps(row), flush=True)
        if profile and dev.type == "cuda":
            print(json.dumps({"bench": "op_kernels", "n": n, "G": G, "nb": NB,
                              "shuffled": shuffled,
                              "kernel_us": {k: _kernel_us(f, dev) for k, f in sides.items()}}),
                  flush=True)
        del ops, sides, plan
    return ok


def end_to_end(params, halos, steps, dev, pairs, repeats, min_s):
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (SampleBinnedPopulationSMFModel,
                                                       sample_population_data)

    @dataclass(eq=False)
    class CompositeModel(SampleBinnedPopulationSMFModel):
        def _sums(self, mu, sigma):
            return composite_sums(self.samples, mu, sigma, self.aux_data["edges"])

    data = make_population_data(params, halos, seed=5, device=dev)
    aux = sample_population_data(data)
    models = {"composite": CompositeModel(aux_data=aux),
              "group": SampleBinnedPopulationSMFModel(aux_data=aux)}
    guess = data["guess"]
    graph = True if dev.type == "cuda" else False

    captured = {}

    def run(m, n):
        eng = GraphAdamEngine(m, graph=graph)
        traj = eng.run_adam(guess, nsteps=n, learning_rate=1e-3)
        captured[type(m).__name__] = bool(eng.use_graph and eng.fallback_reason is None)
        return traj

    def window(m):
        """K: ``steps``, or as many more as make the K steps between the two runs last
        ``min_s``."""
        _sync(dev)
        t0 = time.perf_counter()
        run(m, steps)
        _sync(dev)
        t1 = time.perf_counter()
        run(m, 2 * steps)
        _sync(dev)
        per_step = max((time.perf_counter() - t1) - (t1 - t0), 1e-9) / steps
        return max(steps, min(int(min_s / per_step) + 1, 20 * steps))

    def steps_per_s(m, k):
        # marginal cost per step, (t(2K) - t(K)) / K: setup and capture do not count
        ts = []
        for n in (k, 2 * k):
            best = float("inf")
            for _ in range(repeats):
                _sync(dev)
                t0 = time.perf_counter()
                traj = run(m, n)
                _sync(dev)
                best = min(best, time.perf_counter() - t0)
            ts.append(best)
        return k / max(ts[1] - ts[0], 1e-9), traj

    for m in models.values():
        run(m, 3)  # warm-up (kernel loading)
    ks = {k: window(m) for k, m in models.items()}
    ok = True
    for p in range(pairs):
        r = {k: steps_per_s(m, ks[k]) for k, m in models.items()}
        ok = ok and r["group"][0] > r["composite"][0]
        # both trajectories hold at least 2 * steps rows: compare the same step
        diff = float((r["group"][1][2 * steps] - r["composite"][1][2 * steps]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos, "pair": p,
                          "window_steps": ks, "graph_captured": dict(captured),
                          "composite_steps_per_s": round(r["composite"][0], 2),
                          "group_steps_per_s": round(r["group"][0], 2),
                          "speedup": round(r["group"][0] / r["composite"][0], 2),
                          "max_param_diff_after_2k_steps": diff}), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--max-size", type=float, default=1e8, help="drop op-level rows above this N")
    ap.add_argument("--min-size", type=float, default=0, help="drop op-level rows below this N")
    ap.add_argument("--params", type=int, default=200_000)
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=300,
                    help="K of the marginal cost (t(2K) - t(K)) / K")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true",
                    help="one torch.profiler pass of each side per op-level row")
    ap.add_argument("--skip", default="", choices=["", "op", "e2e"])
    a = ap.parse_args(argv)
    rows = [(int(n), G, s) for n in SIZES if a.min_size <= n <= a.max_size for G in GROUPS
            for s in (False, True)]
    if a.cpu:
        dev = torch.device("cpu")
        rows, a.params, a.halos, a.steps = [(1000, 4, False), (5000, 70, True)], 200, 4000, 3
        a.pairs, a.repeats, a.min_seconds = 1, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_group_op.py measures on a GPU; use --cpu for a functional "
                             "check")
        dev = torch.device("cuda", 0)
    out = {}
    if a.skip != "op":
        out["group_faster_than_composite_in_every_pair_from_4e6"] = bool(
            op_level(rows, dev, a.pairs, a.min_seconds, a.profile))
    if a.skip != "e2e":
        out["group_model_faster_in_every_pair"] = bool(
            end_to_end(a.params, a.halos, a.steps, dev, a.pairs, a.repeats, a.min_seconds))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
