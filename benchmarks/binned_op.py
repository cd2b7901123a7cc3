"""The fused Gaussian-binned-sum op against its torch composite on one MI355X.

(a) op level: forward + backward of ``gaussian_binned_sum`` against the plain
    ``ndtr((edges - mu)/sigma)`` expression + autograd, per-object sigma and weights,
    nb = 10, at N = 1e4, 4e6 and 1e8 (the composite is chunked over objects only where
    its N x (nb+1) intermediates do not fit in device memory).
(b) end to end: ``GraphAdamEngine`` steps/s of ``BinnedPopulationSMFModel`` against
    ``TorchPopulationSMFModel`` at 2e5 parameters / 4e6 halos (marginal cost per step, as
    benchmarks/generic_engine.py).

The two sides run alternately, ``--pairs`` times; one JSON line per row.  ``--cpu`` runs
tiny sizes on the CPU (a functional check of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

NB = 10
EDGES = tuple(9.0 + 0.15 * k for k in range(NB + 1))
COMPOSITE_CHUNK = 1 << 24  # objects per composite call when the intermediates would not fit


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, dev):
    g = torch.Generator().manual_seed(1)
    mu = (9.0 + 1.5 * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    sigma = (0.1 + 0.4 * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    w = (0.5 + torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    return mu, sigma, w


def _composite_fits(n, dev):
    """About a dozen [N, nb+1] float32 intermediates live at the peak of forward + backward."""
    if dev.type != "cuda":
        return True
    return 12 * 4 * n * (NB + 1) < 0.6 * torch.cuda.mem_get_info(dev)[0] or n <= COMPOSITE_CHUNK


def _composite_fb(mu, sigma, w, gS):
    """Forward + backward of the torch composite; chunked over objects (each chunk's graph
    is freed by its backward) when the [N, nb+1] intermediates would not fit."""
    e = torch.tensor(EDGES, dtype=mu.dtype, device=mu.device)
    n = mu.numel()
    if _composite_fits(n, mu.device):
        cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma[:, None])
        out = ((cdf[:, 1:] - cdf[:, :-1]) * w[:, None]).sum(0)
        return out.detach(), torch.autograd.grad(out, (mu, sigma, w), gS)
    out = torch.zeros(NB, dtype=mu.dtype, device=mu.device)
    grads = [torch.empty_like(t) for t in (mu, sigma, w)]
    for lo in range(0, n, COMPOSITE_CHUNK):
        sl = slice(lo, min(lo + COMPOSITE_CHUNK, n))
        leaves = [t.detach()[sl].requires_grad_(True) for t in (mu, sigma, w)]
        cdf = torch.special.ndtr((e[None, :] - leaves[0][:, None]) / leaves[1][:, None])
        o = ((cdf[:, 1:] - cdf[:, :-1]) * leaves[2][:, None]).sum(0)
        for dst, gr in zip(grads, torch.autograd.grad(o, leaves, gS)):
            dst[sl] = gr
        out += o.detach()
    return out, tuple(grads)


def _fused_fb(mu, sigma, w, gS):
    from multigrad_amd.ops import gaussian_binned_sum
    out = gaussian_binned_sum(mu, sigma, EDGES, w)
    return out.detach(), torch.autograd.grad(out, (mu, sigma, w), gS)


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


def op_level(sizes, dev, pairs, min_s):
    from multigrad_amd.utils.profiling import count_device_ops
    ok = True
    for n in sizes:
        mu, sigma, w = _op_inputs(n, dev)
        gS = torch.linspace(0.5, 1.5, NB, device=dev)
        sides = {"composite": lambda: _composite_fb(mu, sigma, w, gS),
                 "fused": lambda: _fused_fb(mu, sigma, w, gS)}
        ref, got = sides["composite"](), sides["fused"]()
        err = float((ref[0] - got[0]).abs().max() / ref[0].abs().max())
        gerr = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(ref[1], got[1]))
        del ref, got
        ops = {k: count_device_ops(f) for k, f in sides.items()}
        for p in range(pairs):
            t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
            ok = ok and t["fused"] < t["composite"]
            print(json.dumps({"bench": "op", "n": n, "nb": NB, "pair": p,
                              "composite_ms": round(t["composite"] * 1e3, 4),
                              "fused_ms": round(t["fused"] * 1e3, 4),
                              "speedup": round(t["composite"] / t["fused"], 2),
                              "device_ops": ops, "composite_chunked": not _composite_fits(n, dev),
                              "max_rel_out_diff": err,
                              "max_rel_grad_diff": gerr}), flush=True)
        del mu, sigma, w
    return ok


def end_to_end(params, halos, steps, dev, pairs, repeats):
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(params, halos, seed=5, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    models = {"composite": TorchPopulationSMFModel(aux_data=aux),
              "fused": BinnedPopulationSMFModel(aux_data=aux)}
    guess = data["guess"]
    graph = True if dev.type == "cuda" else False

    def run(m, n):
        return GraphAdamEngine(m, graph=graph).run_adam(guess, nsteps=n, learning_rate=1e-3)

    def steps_per_s(m):
        # marginal cost per step, (t(2K) - t(K)) / K: setup and capture do not count
        ts = []
        for n in (steps, 2 * steps):
            best = float("inf")
            for _ in range(repeats):
                _sync(dev)
                t0 = time.perf_counter()
                traj = run(m, n)
                _sync(dev)
                best = min(best, time.perf_counter() - t0)
            ts.append(best)
        return steps / max(ts[1] - ts[0], 1e-9), traj

    for m in models.values():
        run(m, 3)  # warm-up (kernel loading)
    ok = True
    for p in range(pairs):
        r = {k: steps_per_s(m) for k, m in models.items()}
        ok = ok and r["fused"][0] > r["composite"][0]
        diff = float((r["fused"][1][-1] - r["composite"][1][-1]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos, "pair": p,
                          "composite_steps_per_s": round(r["composite"][0], 2),
                          "fused_steps_per_s": round(r["fused"][0], 2),
                          "speedup": round(r["fused"][0] / r["composite"][0], 2),
                          "max_final_param_diff": diff}), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--sizes", type=float, nargs="*", default=[1e4, 4e6, 1e8])
    ap.add_argument("--params", type=int, default=200_000)
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=300,
                    help="K of the marginal cost (t(2K) - t(K)) / K; a window of a few tens of "
                         "steps at this size measures host jitter of setup and capture")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--skip", default="", choices=["", "op", "e2e"])
    a = ap.parse_args(argv)
    if a.cpu:
        dev = torch.device("cpu")
        a.sizes, a.params, a.halos, a.steps = [1000, 5000], 200, 4000, 3
        a.pairs, a.repeats, a.min_seconds = 1, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_op.py measures on a GPU; use --cpu for a functional check")
        dev = torch.device("cuda", 0)
    ok = True
    if a.skip != "op":
        ok = op_level([int(s) for s in a.sizes], dev, a.pairs, a.min_seconds) and ok
    if a.skip != "e2e":
        ok = end_to_end(a.params, a.halos, a.steps, dev, a.pairs, a.repeats) and ok
    print(json.dumps({"fused_faster_in_every_pair": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
