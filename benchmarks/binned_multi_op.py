"""The multi-channel Gaussian-binned-sum op against C calls of the single op on one MI355X.

(a) op level: forward + backward (all gradients: mu, sigma and C per-object weights) of
    ``gaussian_binned_sum_multi`` against C calls of ``gaussian_binned_sum`` stacked, with
    autograd adding up the C ``dmu`` / ``dsigma``, at nb = 10: N = 1e4, 4e6 and 1e8 for
    C = 2 and 4, and C = 8 at N = 4e6.
(b) end to end: ``GraphAdamEngine`` steps/s of ``ConditionalBinnedPopulationSMFModel`` on
    the op against the same model with ``_sums`` made of three single-op calls at 2e5
    parameters / 4e6 halos, both captured (marginal cost per step, as
    benchmarks/binned_op.py).

The baseline is always C calls of the single op.  The two sides run alternately, ``--pairs``
times; one JSON line per row, with the largest relative differences of the outputs and
gradients between the two sides.  ``--profile`` adds one ``torch.profiler`` pass of each side
(per-kernel microseconds).  ``--cpu`` runs tiny sizes on the CPU (a functional check of the
script, not a measurement).
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
ROWS = [(1e4, 2), (1e4, 4), (4e6, 2), (4e6, 4), (4e6, 8), (1e8, 2), (1e8, 4)]  # (N, C)


def _edges(nb):
    """float32-representable edges, so that both sides bin alike."""
    return tuple(float(torch.tensor(9.0 + 1.5 * k / nb, dtype=torch.float32))
                 for k in range(nb + 1))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, C, dev):
    g = torch.Generator().manual_seed(1)
    spec = ((9.0, 1.5), (0.1, 0.4)) + ((0.5, 1.0),) * C  # mu, sigma, C weights
    return tuple((lo + span * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
                 for lo, span in spec)


def _calls_fb(ops, edges, G):
    """Forward + backward of C calls of the single op."""
    from multigrad_amd.ops import gaussian_binned_sum
    out = torch.stack([gaussian_binned_sum(ops[0], ops[1], edges, w) for w in ops[2:]])
    return out.detach(), torch.autograd.grad(out, ops, G)


def _multi_fb(ops, edges, G):
    from multigrad_amd.ops import gaussian_binned_sum_multi
    out = gaussian_binned_sum_multi(ops[0], ops[1], edges, list(ops[2:]))
    return out.detach(), torch.autograd.grad(out, ops, G)


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


def op_level(rows, dev, pairs, min_s, profile):
    """Returns whether the multi op won every pair of the largest N (the criterion); the
    other rows are reported as they fall."""
    from multigrad_amd.utils.profiling import count_device_ops
    edges = _edges(NB)
    big = max(n for n, _ in rows)
    ok = True
    for n, C in rows:
        ops = _op_inputs(n, C, dev)
        G = (torch.linspace(0.5, 1.5, NB, device=dev)[None, :] *
             (1.0 + torch.arange(C, device=dev)[:, None] / 4.0))
        sides = {"calls": lambda: _calls_fb(ops, edges, G),
                 "multi": lambda: _multi_fb(ops, edges, G)}
        ref, got = sides["calls"](), sides["multi"]()
        err = float((ref[0] - got[0]).abs().max() / ref[0].abs().max())
        gerr = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(ref[1], got[1]))
        del ref, got
        dev_ops = {k: count_device_ops(f) for k, f in sides.items()}
        for p in range(pairs):
            t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
            if n == big:
                ok = ok and t["multi"] < t["calls"]
            print(json.dumps({"bench": "op", "n": n, "C": C, "nb": NB, "pair": p,
                              "calls_ms": round(t["calls"] * 1e3, 4),
                              "multi_ms": round(t["multi"] * 1e3, 4),
                              "speedup": round(t["calls"] / t["multi"], 2),
                              "multi_us_per_1e6_objects": round(t["multi"] * 1e12 / n, 2),
                              "device_ops": dev_ops, "max_rel_out_diff": err,
                              "max_rel_grad_diff": gerr}), flush=True)
        if profile and dev.type == "cuda":
            print(json.dumps({"bench": "op_kernels", "n": n, "C": C, "nb": NB,
                              "kernel_us": {k: _kernel_us(f, dev) for k, f in sides.items()}}),
                  flush=True)
        del ops, sides
    return ok


def end_to_end(params, halos, steps, dev, pairs, repeats, min_s):
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (ConditionalBinnedPopulationSMFModel,
                                                       conditional_population_data)
    from multigrad_amd.ops import gaussian_binned_sum

    @dataclass(eq=False)
    class ThreeCallModel(ConditionalBinnedPopulationSMFModel):
        def _sums(self, mu, sigma, weights):
            return torch.stack([gaussian_binned_sum(mu, sigma, self.edges, w) for w in weights])

    data = make_population_data(params, halos, seed=5, device=dev)
    aux = conditional_population_data(data)
    models = {"calls": ThreeCallModel(aux_data=aux),
              "multi": ConditionalBinnedPopulationSMFModel(aux_data=aux)}
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
        ok = ok and r["multi"][0] > r["calls"][0]
        # both trajectories hold at least 2 * steps rows: compare the same step
        diff = float((r["multi"][1][2 * steps] - r["calls"][1][2 * steps]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos, "pair": p,
                          "window_steps": ks, "graph_captured": dict(captured),
                          "calls_steps_per_s": round(r["calls"][0], 2),
                          "multi_steps_per_s": round(r["multi"][0], 2),
                          "speedup": round(r["multi"][0] / r["calls"][0], 2),
                          "max_param_diff_after_2k_steps": diff}), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--max-size", type=float, default=1e8, help="drop op-level rows above this N")
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
    rows = [(int(n), C) for n, C in ROWS if n <= a.max_size]
    if a.cpu:
        dev = torch.device("cpu")
        rows, a.params, a.halos, a.steps = [(1000, 2), (5000, 4), (1000, 8)], 200, 4000, 3
        a.pairs, a.repeats, a.min_seconds = 1, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_multi_op.py measures on a GPU; use --cpu for a functional "
                             "check")
        dev = torch.device("cuda", 0)
    out = {}
    if a.skip != "op":
        out["multi_faster_in_every_pair_at_largest_n"] = bool(
            op_level(rows, dev, a.pairs, a.min_seconds, a.profile))
    if a.skip != "e2e":
        out["multi_model_faster_in_every_pair"] = bool(
            end_to_end(a.params, a.halos, a.steps, dev, a.pairs, a.repeats, a.min_seconds))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
