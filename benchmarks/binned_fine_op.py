"""The fine Gaussian-binned-sum op against what a user writes without it, on one MI355X.

(a) op level: forward + backward (all gradients: mu, sigma and per-object weights) of
    ``FineBins.sum`` for N = 4e6 and 1e8, nb = 64, 256, 1024 and 4096 uniform bins and
    sigma = 0.5, 2 and 8 bin widths, plus one contention row (every mu inside two bins), against
      slices: ``ceil(nb / 32)`` calls of ``gaussian_binned_sum`` on 33-edge slices, concatenated;
      dense : the ``ndtr`` table (laid out ``[nb + 1, N]``) summed over objects, where the table
              fits (``N * nb <= --dense-limit`` elements).
(b) end to end: ``GraphAdamEngine`` steps/s of ``FineBinnedPopulationSMFModel`` on the op against
    the same model with ``_sums`` written as the slices composite, both captured (marginal cost
    per step, as benchmarks/binned_op.py).

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

SIZES = [4e6, 1e8]
NBS = [64, 256, 1024, 4096]
RATIOS = [0.5, 2.0, 8.0]
E0, E1 = 9.0, 11.0


def _edges(nb):
    """float32-representable edges, so that all sides bin alike."""
    return tuple(float(v) for v in torch.linspace(E0, E1, nb + 1, dtype=torch.float64).float())


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, nb, ratio, dev, contention=False):
    g = torch.Generator().manual_seed(1)
    width = (E1 - E0) / nb
    if contention:  # every mean inside the two bins in the middle of the range
        mu = 0.5 * (E0 + E1) + width * (2.0 * torch.rand(n, generator=g) - 1.0)
    else:
        mu = E0 + (E1 - E0) * torch.rand(n, generator=g)
    sigma = ratio * width * (0.75 + 0.5 * torch.rand(n, generator=g))
    w = 0.5 + torch.rand(n, generator=g)
    return tuple(t.to(dev).requires_grad_(True) for t in (mu, sigma, w))


def slices_sums(mu, sigma, edges, w=None):
    """``gaussian_binned_sum`` on 33-edge slices of the host edges, concatenated."""
    from multigrad_amd.ops import gaussian_binned_sum
    return torch.cat([gaussian_binned_sum(mu, sigma, edges[k:k + 33], w)
                      for k in range(0, len(edges) - 1, 32)])


def dense_sums(mu, sigma, edges_t, w=None):
    cdf = torch.special.ndtr((edges_t[:, None] - mu[None, :]) / sigma[None, :])
    d = cdf[1:] - cdf[:-1]
    if w is not None:
        d = d * w[None, :]
    return d.sum(1)


def _fb(fn, ops, cot):
    out = fn()
    return out.detach(), torch.autograd.grad(out, ops, cot)


def _time_calls(fn, dev, min_s, max_calls=2000):
    """Seconds per call over a window of at least ``min_s`` (host clock around a device
    synchronise)."""
    fn()
    _sync(dev)
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 8 == 0 or calls >= max_calls or dev.type == "cpu" or \
                time.perf_counter() - t0 >= min_s:
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


def op_level(rows, dev, pairs, min_s, profile, dense_limit):
    """Returns whether the op beat the slices composite in every pair of every row with
    nb >= 256 and sigma <= 2 widths (the expectation); the other rows are reported as they
    fall."""
    from multigrad_amd.ops import FineBins
    ok = True
    for n, nb, ratio, contention in rows:
        edges = _edges(nb)
        bins = FineBins(edges, device=dev)
        edges_t = torch.tensor(edges, device=dev)
        ops = _op_inputs(n, nb, ratio, dev, contention)
        cot = torch.linspace(0.5, 1.5, nb, device=dev)
        sides = {"fine": lambda: _fb(lambda: bins.sum(*ops), ops, cot),
                 "slices": lambda: _fb(lambda: slices_sums(ops[0], ops[1], edges, ops[2]), ops,
                                       cot)}
        if n * nb <= dense_limit:
            sides["dense"] = lambda: _fb(lambda: dense_sums(ops[0], ops[1], edges_t, ops[2]),
                                         ops, cot)
        got = sides["fine"]()
        ref = sides["slices"]()
        err = _rel(ref[0], got[0])
        gerr = max(_rel(a, b) for a, b in zip(ref[1], got[1]))
        del ref, got
        for p in range(pairs):
            t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
            if nb >= 256 and ratio <= 2.0 and not contention:
                ok = ok and t["fine"] < t["slices"]
            row = {"bench": "op", "n": n, "nb": nb, "sigma_over_width": ratio,
                   "contention": contention, "pair": p,
                   "fine_ms": round(t["fine"] * 1e3, 4),
                   "slices_ms": round(t["slices"] * 1e3, 4),
                   "speedup_vs_slices": round(t["slices"] / t["fine"], 2),
                   "fine_us_per_1e6_objects": round(t["fine"] * 1e12 / n, 2),
                   "max_rel_out_diff": err, "max_rel_grad_diff": gerr}
            if "dense" in t:
                row["dense_ms"] = round(t["dense"] * 1e3, 4)
                row["speedup_vs_dense"] = round(t["dense"] / t["fine"], 2)
            print(json.dumps(row), flush=True)
        if profile and dev.type == "cuda":
            print(json.dumps({"bench": "op_kernels", "n": n, "nb": nb, "sigma_over_width": ratio,
                              "contention": contention,
                              "kernel_us": {k: _kernel_us(f, dev) for k, f in sides.items()
                                            if k != "dense"}}), flush=True)
        del ops, sides, bins
    return ok


def end_to_end(params, halos, refine, steps, dev, pairs, repeats, min_s):
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (FineBinnedPopulationSMFModel,
                                                       fine_population_data)

    @dataclass(eq=False)
    class SlicesModel(FineBinnedPopulationSMFModel):
        def _sums(self, mu, sigma):
            return slices_sums(mu, sigma, self.edges)

    data = make_population_data(params, halos, seed=5, device=dev)
    aux = fine_population_data(data, refine=refine)
    models = {"slices": SlicesModel(aux_data=aux),
              "fine": FineBinnedPopulationSMFModel(aux_data=aux)}
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
        ok = ok and r["fine"][0] > r["slices"][0]
        diff = float((r["fine"][1][2 * steps] - r["slices"][1][2 * steps]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos,
                          "nb": models["fine"].bins.nb, "pair": p, "window_steps": ks,
                          "graph_captured": dict(captured),
                          "slices_steps_per_s": round(r["slices"][0], 2),
                          "fine_steps_per_s": round(r["fine"][0], 2),
                          "speedup": round(r["fine"][0] / r["slices"][0], 2),
                          "max_param_diff_after_2k_steps": diff}), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--max-size", type=float, default=1e8, help="drop op-level rows above this N")
    ap.add_argument("--min-size", type=float, default=0, help="drop op-level rows below this N")
    ap.add_argument("--dense-limit", type=float, default=1.1e9,
                    help="largest N * nb for which the dense ndtr table is measured")
    ap.add_argument("--params", type=int, default=200_000)
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--refine", type=int, default=32, help="fine bins per coarse bin (e2e)")
    ap.add_argument("--steps", type=int, default=100,
                    help="K of the marginal cost (t(2K) - t(K)) / K")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--profile", action="store_true",
                    help="one torch.profiler pass of each side per op-level row")
    ap.add_argument("--skip", default="", choices=["", "op", "e2e"])
    a = ap.parse_args(argv)
    rows = [(int(n), nb, r, False) for n in SIZES if a.min_size <= n <= a.max_size for nb in NBS
            for r in RATIOS]
    rows += [(int(n), 1024, 2.0, True) for n in SIZES[:1] if a.min_size <= n <= a.max_size]
    if a.cpu:
        dev = torch.device("cpu")
        rows = [(1000, 40, 2.0, False), (3000, 100, 0.5, True)]
        a.params, a.halos, a.steps, a.refine = 200, 4000, 3, 8
        a.pairs, a.repeats, a.min_seconds = 1, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_fine_op.py measures on a GPU; use --cpu for a functional "
                             "check")
        dev = torch.device("cuda", 0)
    out = {}
    if a.skip != "op":
        out["fine_faster_than_slices_in_every_pair_from_256_bins_at_sigma_le_2"] = bool(
            op_level(rows, dev, a.pairs, a.min_seconds, a.profile, a.dense_limit))
    if a.skip != "e2e":
        out["fine_model_faster_in_every_pair"] = bool(
            end_to_end(a.params, a.halos, a.refine, a.steps, dev, a.pairs, a.repeats,
                       a.min_seconds))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
