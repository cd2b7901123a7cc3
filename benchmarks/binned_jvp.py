"""Forward mode of the fused Gaussian-binned-sum op, and the sumstat Jacobian built on it, on
one MI355X.

(a) op level: one tangent of ``gaussian_binned_sum`` along (tmu, tsigma) under
    ``torch.autograd.forward_ad`` (csrc/binned_jvp.hip) beside the op's forward and its
    first backward (gradients of mu and sigma) on the same inputs, and beside the float32
    ``ndtr((edges - mu)/sigma)`` composite under torch's own forward AD; N = 4e6, nb = 10,
    per-object and broadcast sigma, no weights.  Calls are timed with a host clock around
    a device synchronise, so each figure includes the launches and the dual-tensor
    plumbing of a call.
(b) model level: ``calc_sumstats_jacobian_from_params`` of
    ``GroupedBinnedPopulationSMFModel`` with ``mode="forward"`` against ``mode="reverse"``
    at 8 and 64 parameters, 4e6 halos, K = 10 sumstats.

The sides run alternately, ``--pairs`` times; one JSON line per row.  ``--cpu`` runs tiny
sizes on the CPU (a functional check of the script, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.autograd.forward_ad as fwad

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

NB = 10
EDGES = tuple(9.0 + 0.15 * k for k in range(NB + 1))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _composite(mu, sigma):
    e = torch.tensor(EDGES, dtype=mu.dtype, device=mu.device)
    cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma.reshape(-1, 1))
    return (cdf[:, 1:] - cdf[:, :-1]).sum(0)


def _fused(mu, sigma):
    from multigrad_amd.ops import gaussian_binned_sum
    return gaussian_binned_sum(mu, sigma, EDGES)


def _tangent(fn, ops, tans):
    with torch.no_grad(), fwad.dual_level():
        out = fn(*[fwad.make_dual(t, d) for t, d in zip(ops, tans)])
        return fwad.unpack_dual(out).tangent


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


def op_level(n, dev, pairs, min_s):
    g = torch.Generator().manual_seed(1)
    mu = (9.0 + 1.5 * torch.rand(n, generator=g)).to(dev)
    sig_n = (0.1 + 0.4 * torch.rand(n, generator=g)).to(dev)
    tmu, tsig_n = (torch.randn(n, generator=g).to(dev) for _ in range(2))
    gS = torch.linspace(0.5, 1.5, NB, device=dev)
    for mode in ("per-object", "broadcast"):
        sigma, tsigma = (sig_n, tsig_n) if mode == "per-object" else (sig_n[:1].clone(),
                                                                      tsig_n[:1].clone())
        ops, tans = (mu, sigma), (tmu, tsigma)
        leaves = [t.clone().requires_grad_(True) for t in ops]

        def forward():
            with torch.no_grad():
                return _fused(*ops)

        def forward_backward():
            return torch.autograd.grad(_fused(*leaves), leaves, gS)

        sides = {"jvp": lambda: _tangent(_fused, ops, tans), "forward": forward,
                 "forward_backward": forward_backward,
                 "composite_jvp": lambda: _tangent(_composite, ops, tans)}
        ref, got = sides["composite_jvp"](), sides["jvp"]()
        err = float((ref - got).abs().max() / ref.abs().max())
        del ref, got
        for p in range(pairs):
            t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
            row = {"bench": "op_jvp", "sigma": mode, "n": n, "nb": NB, "pair": p}
            row.update({k + "_ms": round(v * 1e3, 4) for k, v in t.items()})
            # the tangent call runs the forward kernel too (the primal), so the tangent
            # kernel's own share is the difference
            row["jvp_minus_forward_ms"] = round((t["jvp"] - t["forward"]) * 1e3, 4)
            row["backward_ms"] = round((t["forward_backward"] - t["forward"]) * 1e3, 4)
            row["max_rel_diff_to_composite"] = err
            print(json.dumps(row), flush=True)


def model_level(params, halos, dev, pairs, min_s):
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(params, halos, seed=5, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))
    guess = data["guess"]
    sides = {m: (lambda m=m: model.calc_sumstats_jacobian_from_params(guess, mode=m))
             for m in ("forward", "reverse")}
    jf, jr = sides["forward"]()[1], sides["reverse"]()[1]
    err = float((jf - jr).abs().max() / jr.abs().max())
    for p in range(pairs):
        t = {k: _time_calls(f, dev, min_s, max_calls=200) for k, f in sides.items()}
        print(json.dumps({"bench": "model_jacobian", "params": params, "halos": halos,
                          "sumstats": int(jf.shape[0]), "pair": p,
                          "forward_ms": round(t["forward"] * 1e3, 3),
                          "reverse_ms": round(t["reverse"] * 1e3, 3),
                          "reverse_over_forward": round(t["reverse"] / t["forward"], 2),
                          "max_rel_diff": err}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true", help="tiny sizes on the CPU (functional check)")
    ap.add_argument("--size", type=float, default=4e6)
    ap.add_argument("--params", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--halos", type=int, default=4_000_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--skip", default="", choices=["", "op", "model"])
    a = ap.parse_args(argv)
    if a.cpu:
        dev = torch.device("cpu")
        a.size, a.params, a.halos, a.pairs, a.min_seconds = 5000, [8], 4000, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned_jvp.py measures on a GPU; use --cpu for a functional check")
        dev = torch.device("cuda", 0)
    if a.skip != "op":
        op_level(int(a.size), dev, a.pairs, a.min_seconds)
    if a.skip != "model":
        for params in a.params:
            model_level(params, a.halos, dev, a.pairs, a.min_seconds)


if __name__ == "__main__":
    main()
