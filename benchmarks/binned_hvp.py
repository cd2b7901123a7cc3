"""Hessian-vector products through the fused Gaussian-binned-sum op against its float32
torch composite on one MI355X.

(a) op level: one Hessian-vector product of a scalar of the bin sums with respect to
    (mu, sigma, w) -- ``grad(grad(f, x, create_graph=True), x, v)`` -- through
    ``gaussian_binned_sum`` (second backward: csrc/binned_hvp.hip) and through the plain
    ``ndtr((edges - mu)/sigma)`` expression with torch's own double backward; per-object
    sigma and weights, nb = 10, N = 1e4 and 4e6.  ``linear``: f = sum_k gS_k out_k (the
    cotangent of the op is a constant: no gradient of g); ``quadratic``: f = sum_k gS_k out_k^2
    (the whole second backward).  Each row also has the op's forward + first backward on the
    same inputs (the floor: it reads the same operands) and the peak device memory of both
    sides above the inputs.
(b) model level: ``calc_hvp_from_params`` of ``BinnedPopulationSMFModel`` against
    ``TorchPopulationSMFModel`` at 2e5 parameters / 4e6 halos.

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


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, dev):
    g = torch.Generator().manual_seed(1)
    mu = (9.0 + 1.5 * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    sigma = (0.1 + 0.4 * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    w = (0.5 + torch.rand(n, generator=g)).to(dev).requires_grad_(True)
    vs = tuple(torch.randn(n, generator=g).to(dev) for _ in range(3))
    return (mu, sigma, w), vs


def _composite(mu, sigma, w):
    e = torch.tensor(EDGES, dtype=mu.dtype, device=mu.device)
    cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma[:, None])
    return ((cdf[:, 1:] - cdf[:, :-1]) * w[:, None]).sum(0)


def _fused(mu, sigma, w):
    from multigrad_amd.ops import gaussian_binned_sum
    return gaussian_binned_sum(mu, sigma, EDGES, w)


def _hvp(fn, leaves, vs, gS, scalar):
    out = fn(*leaves)
    f = (gS * out).sum() if scalar == "linear" else (gS * out * out).sum()
    grads = torch.autograd.grad(f, leaves, create_graph=True)
    return torch.autograd.grad(grads, leaves, vs)


def _first_order(leaves, gS):
    return torch.autograd.grad(_fused(*leaves), leaves, gS)


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


def _peak_mib(fn, dev):
    """Peak device memory of one call above what is allocated before it."""
    if dev.type != "cuda":
        return None
    _sync(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    _sync(dev)
    return round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)


def op_level(sizes, dev, pairs, min_s):
    ok = True
    for n in sizes:
        leaves, vs = _op_inputs(n, dev)
        gS = torch.linspace(0.5, 1.5, NB, device=dev)
        for scalar in ("linear", "quadratic"):
            sides = {"composite": lambda: _hvp(_composite, leaves, vs, gS, scalar),
                     "fused": lambda: _hvp(_fused, leaves, vs, gS, scalar)}
            ref, got = sides["composite"](), sides["fused"]()
            err = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(ref, got))
            del ref, got
            peak = {k: _peak_mib(f, dev) for k, f in sides.items()}
            for p in range(pairs):
                t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
                t1 = _time_calls(lambda: _first_order(leaves, gS), dev, min_s)
                ok = ok and t["fused"] < t["composite"]
                print(json.dumps({"bench": "op_hvp", "scalar": scalar, "n": n, "nb": NB, "pair": p,
                                  "composite_ms": round(t["composite"] * 1e3, 4),
                                  "fused_ms": round(t["fused"] * 1e3, 4),
                                  "speedup": round(t["composite"] / t["fused"], 2),
                                  "fused_first_order_ms": round(t1 * 1e3, 4),
                                  "peak_mib": peak, "max_rel_hvp_diff": err}), flush=True)
        del leaves, vs
    return ok


def model_level(params, halos, dev, pairs, min_s):
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
    v = torch.randn(guess.numel(), generator=torch.Generator().manual_seed(2)).to(dev)
    sides = {k: (lambda m=m: m.calc_hvp_from_params(guess, v)) for k, m in models.items()}
    ref, got = sides["composite"](), sides["fused"]()
    err = float((ref - got).abs().max() / ref.abs().max())
    del ref, got
    peak = {k: _peak_mib(f, dev) for k, f in sides.items()}
    ok = True
    for p in range(pairs):
        t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
        ok = ok and t["fused"] < t["composite"]
        print(json.dumps({"bench": "model_hvp", "params": params, "halos": halos, "pair": p,
                          "composite_ms": round(t["composite"] * 1e3, 4),
                          "fused_ms": round(t["fused"] * 1e3, 4),
                          "speedup": round(t["composite"] / t["fused"], 2),
                          "peak_mib": peak, "max_rel_hvp_diff": err}), flush=True)
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--sizes", type=float, nargs="*", default=[1e4, 4e6])
    ap.add_argument("--params", type=int, default=200_000)
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--skip", default="", choices=["", "op", "model"])
    a = ap.parse_args(argv)
    if a.cpu:
        dev = torch.device("cpu")
        a.sizes, a.params, a.halos, a.pairs, a.min_seconds = [1000, 5000], 200, 4000, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_hvp.py measures on a GPU; use --cpu for a functional check")
        dev = torch.device("cuda", 0)
    ok = True
    if a.skip != "op":
        ok = op_level([int(s) for s in a.sizes], dev, a.pairs, a.min_seconds) and ok
    if a.skip != "model":
        ok = model_level(a.params, a.halos, dev, a.pairs, a.min_seconds) and ok
    print(json.dumps({"fused_faster_in_every_pair": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
