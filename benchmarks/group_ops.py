"""The group gather / segment-sum ops against their torch expressions on one MI355X.

(a) op level: forward + backward of ``GroupIndex.gather`` of two columns against
    ``v[index]`` + autograd (whose backward is ``index_put_(accumulate=True)``: a sort and
    an atomic scatter per call), at G = 1e5 groups with N = 1e4, 4e6 and 1e8 objects, for a
    sorted and a shuffled index; and one row with one group holding every object,
    ``segment_sum`` against ``x.sum()``.
(b) end to end: ``GraphAdamEngine`` steps/s of ``GroupedBinnedPopulationSMFModel`` against
    ``BinnedPopulationSMFModel`` at 2e5 parameters / 4e6 halos (marginal cost per step, as
    benchmarks/binned_op.py, with K >= 300 raised until K steps last the timing window).

The two sides run alternately, ``--pairs`` times; one JSON line per row.  ``--profile``
adds a ``torch.profiler`` kernel table of one eager step of each model of (b).  ``--cpu``
runs tiny sizes on the CPU (a functional check of the script, not a measurement).
"""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


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


def _pairs(row, sides, dev, pairs, min_s):
    from multigrad_amd.utils.profiling import count_device_ops
    ops = {k: count_device_ops(f) for k, f in sides.items()}
    ok = True
    for p in range(pairs):
        t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
        ok = ok and t["new"] < t["torch"]
        print(json.dumps(dict(row, pair=p, torch_ms=round(t["torch"] * 1e3, 4),
                              new_ms=round(t["new"] * 1e3, 4),
                              speedup=round(t["torch"] / t["new"], 2), device_ops=ops)),
              flush=True)
    return ok


def op_level(sizes, groups, dev, pairs, min_s):
    """Returns whether the new side won every pair at N >= 4e6 (smaller sizes are reported,
    not judged: there both sides are bound by the host)."""
    from multigrad_amd.ops import GroupIndex
    ok = True
    for n in sizes:
        g = min(groups, n)
        gen = torch.Generator(device=dev).manual_seed(1)   # inputs are made on the device
        base = torch.sort(torch.randint(0, g, (n,), generator=gen, device=dev)).values
        for order in ("sorted", "shuffled"):
            ids = base if order == "sorted" else \
                base[torch.randperm(n, generator=gen, device=dev)]
            plan = GroupIndex(ids, g)
            a = torch.randn(g, generator=gen, device=dev).requires_grad_(True)
            s = torch.rand(g, generator=gen, device=dev).requires_grad_(True)
            ga = torch.randn(n, generator=gen, device=dev)
            gs = torch.randn(n, generator=gen, device=dev)

            def torch_side():
                return torch.autograd.grad((a[ids], s[ids]), (a, s), (ga, gs))

            def new_side():
                return torch.autograd.grad(plan.gather(a, s), (a, s), (ga, gs))

            ref, got = torch_side(), new_side()
            diff = max(float((r - o).abs().max() / r.abs().max()) for r, o in zip(ref, got))
            del ref, got
            row = {"bench": "gather", "n": n, "groups": g, "index": order,
                   "max_rel_grad_diff": diff}
            won = _pairs(row, {"torch": torch_side, "new": new_side}, dev, pairs, min_s)
            ok = ok and (won or n < 4_000_000)
            del plan, ids, a, s, ga, gs
        del base
    # one group holding everything: the shape of torch.sum
    n = max(sizes)
    plan = GroupIndex(torch.zeros(n, dtype=torch.int32, device=dev), 1)
    x = torch.randn(n, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    diff = abs(float(plan.segment_sum(x)[0]) - float(x.sum())) / float(x.abs().sum())
    row = {"bench": "one-group-sum", "n": n, "groups": 1, "diff_over_abs_sum": diff}
    won = _pairs(row, {"torch": lambda: x.sum(), "new": lambda: plan.segment_sum(x)}, dev, pairs,
                 min_s)
    return ok and (won or n < 4_000_000)


def _models(params, halos, dev):
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       GroupedBinnedPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(params, halos, seed=5, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    return {"torch": BinnedPopulationSMFModel(aux_data=aux),
            "new": GroupedBinnedPopulationSMFModel(aux_data=aux)}, data["guess"]


def end_to_end(params, halos, steps, dev, pairs, repeats, min_s):
    from multigrad_amd.engine.generic import GraphAdamEngine
    models, guess = _models(params, halos, dev)
    graph = dev.type == "cuda"

    def run(m, n):
        return GraphAdamEngine(m, graph=graph).run_adam(guess, nsteps=n, learning_rate=1e-3)

    def window(m):
        """K: ``steps``, or as many more as make the K steps between the two runs last
        ``min_s`` (a 0.2 ms step needs more than 300 of them to rise above the jitter of
        engine setup and capture)."""
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
        ok = ok and r["new"][0] > r["torch"][0]
        # both trajectories hold at least 2 * steps rows: compare the same step
        diff = float((r["new"][1][2 * steps] - r["torch"][1][2 * steps]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos, "pair": p,
                          "window_steps": {"binned": ks["torch"], "grouped": ks["new"]},
                          "binned_steps_per_s": round(r["torch"][0], 2),
                          "grouped_steps_per_s": round(r["new"][0], 2),
                          "speedup": round(r["new"][0] / r["torch"][0], 2),
                          "max_final_param_diff": diff}), flush=True)
    return ok


def step_kernel_table(params, halos, dev, calls=10, top=12):
    """Device time per kernel of one eager ``calc_loss_and_grad_from_params`` of each model."""
    models, guess = _models(params, halos, dev)
    for name, m in models.items():
        for _ in range(3):
            m.calc_loss_and_grad_from_params(guess)
        _sync(dev)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                m.calc_loss_and_grad_from_params(guess)
            _sync(dev)
        us, cnt = collections.Counter(), collections.Counter()
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                us[e.name[:110]] += e.device_time
                cnt[e.name[:110]] += 1
        label = {"torch": "binned", "new": "grouped"}[name]
        print(json.dumps({"bench": "step_kernels", "model": label,
                          "device_us_per_step": round(sum(us.values()) / calls, 1)}), flush=True)
        for k, v in us.most_common(top):
            print(json.dumps({"bench": "step_kernels", "model": label, "kernel": k,
                              "calls_per_step": cnt[k] / calls,
                              "us_per_step": round(v / calls, 1)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--sizes", type=float, nargs="*", default=[1e4, 4e6, 1e8])
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--params", type=int, default=200_000)
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=300,
                    help="smallest K of the marginal cost (t(2K) - t(K)) / K; K grows until the "
                         "K steps last --min-seconds")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--skip", default="", choices=["", "op", "e2e"])
    ap.add_argument("--profile", action="store_true",
                    help="also print the kernel table of one eager step of each model")
    a = ap.parse_args(argv)
    if a.cpu:
        dev = torch.device("cpu")
        a.sizes, a.groups, a.params, a.halos, a.steps = [1000, 5000], 50, 200, 4000, 3
        a.pairs, a.repeats, a.min_seconds, a.profile = 1, 1, 0.0, False
    else:
        if not torch.cuda.is_available():
            raise SystemExit("group_ops.py measures on a GPU; use --cpu for a functional check")
        dev = torch.device("cuda", 0)
    ok = True
    if a.skip != "op":
        ok = op_level([int(s) for s in a.sizes], a.groups, dev, a.pairs, a.min_seconds) and ok
    if a.skip != "e2e":
        ok = end_to_end(a.params, a.halos, a.steps, dev, a.pairs, a.repeats,
                        a.min_seconds) and ok
    if a.profile:
        step_kernel_table(a.params, a.halos, dev)
    print(json.dumps({"new_faster_in_every_judged_pair": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
