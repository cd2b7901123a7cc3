"""The fused two-axis Gaussian-binned-sum op against its torch composite on one MI355X.

(a) op level: forward + backward of ``gaussian_binned_sum_2d`` against the plain composite
    (two ``ndtr`` tables + ``einsum('ij,ik->jk')`` + autograd), per-object sigmas and
    weights, at N = 1e4, 4e6 and 1e8 and at 10x10 and 32x8 cells (the composite is chunked
    over objects only where its N x (nb+1) tables do not fit in device memory).
(b) end to end: ``GraphAdamEngine`` steps/s of ``JointBinnedPopulationSMFModel`` on the op
    against the same model on the composite at 2e5 parameters / 4e6 halos (marginal cost
    per step, as benchmarks/binned_op.py).

The baseline is always the torch composite.  The two sides run alternately, ``--pairs``
times; one JSON line per row, with the largest relative differences of the outputs and
gradients between the two sides and each side's output error against the float64 torch path.  ``--profile`` adds one ``torch.profiler`` pass of the fused
side (per-kernel microseconds).  ``--cpu`` runs tiny sizes on the CPU (a functional check of
the script, not a measurement).
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

GRIDS = [(10, 10), (32, 8)]
COMPOSITE_CHUNK = 1 << 23  # objects per composite call when the tables would not fit


def _edges(nbx, nby):
    """float32-representable edges, so that every side and the float64 check bin alike."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    return (tuple(f32(9.0 + 1.5 * k / nbx) for k in range(nbx + 1)),
            tuple(f32(-12.0 + 2.0 * k / nby) for k in range(nby + 1)))


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _op_inputs(n, dev):
    g = torch.Generator().manual_seed(1)
    spec = ((9.0, 1.5), (0.1, 0.4), (-12.5, 3.0), (0.2, 0.6), (0.5, 1.0))  # mux sigx muy sigy w
    return tuple((lo + span * torch.rand(n, generator=g)).to(dev).requires_grad_(True)
                 for lo, span in spec)


def _composite_fits(n, nbx, nby, dev):
    """About a dozen float32 copies of the two [N, nb+1] tables live at the peak."""
    if dev.type != "cuda":
        return True
    need = 12 * 4 * n * (nbx + nby + 2)
    return need < 0.6 * torch.cuda.mem_get_info(dev)[0] or n <= COMPOSITE_CHUNK


def _composite(mux, sigx, muy, sigy, w, ex, ey):
    def table(mu, sigma, e):
        cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma[:, None])
        return cdf[:, 1:] - cdf[:, :-1]
    px, py = table(mux, sigx, ex), table(muy, sigy, ey)
    if w is not None:
        px = px * w[:, None]
    return torch.einsum("ij,ik->jk", px, py)


def _composite_fb(ops, edges, G):
    """Forward + backward of the torch composite; chunked over objects (each chunk's graph
    is freed by its backward) when the tables would not fit."""
    dev = ops[0].device
    ex, ey = (torch.tensor(e, dtype=ops[0].dtype, device=dev) for e in edges)
    n = ops[0].numel()
    if _composite_fits(n, G.shape[0], G.shape[1], dev):
        out = _composite(*ops, ex, ey)
        return out.detach(), torch.autograd.grad(out, ops, G)
    out = torch.zeros_like(G)
    grads = [torch.empty_like(t) for t in ops]
    for lo in range(0, n, COMPOSITE_CHUNK):
        sl = slice(lo, min(lo + COMPOSITE_CHUNK, n))
        leaves = [t.detach()[sl].requires_grad_(True) for t in ops]
        o = _composite(*leaves, ex, ey)
        for dst, gr in zip(grads, torch.autograd.grad(o, leaves, G)):
            dst[sl] = gr
        out += o.detach()
    return out, tuple(grads)


def _fused_fb(ops, edges, G):
    from multigrad_amd.ops import gaussian_binned_sum_2d
    out = gaussian_binned_sum_2d(*ops[:4], edges[0], edges[1], ops[4], chunk=1 << 20)
    return out.detach(), (torch.autograd.grad(out, ops, G) if G is not None else None)


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


def op_level(sizes, grids, dev, pairs, min_s, profile):
    from multigrad_amd.utils.profiling import count_device_ops
    ok = True
    for n in sizes:
        ops = _op_inputs(n, dev)
        for nbx, nby in grids:
            edges = _edges(nbx, nby)
            G = torch.linspace(0.5, 1.5, nbx * nby, device=dev).reshape(nbx, nby)
            sides = {"composite": lambda: _composite_fb(ops, edges, G),
                     "fused": lambda: _fused_fb(ops, edges, G)}
            ref, got = sides["composite"](), sides["fused"]()
            err = float((ref[0] - got[0]).abs().max() / ref[0].abs().max())
            # which side the difference belongs to: both against the float64 torch path
            out64 = _fused_fb([t.detach().double() for t in ops], edges, None)[0]
            err64 = {k: float((v[0].double() - out64).abs().max() / out64.abs().max())
                     for k, v in (("composite", ref), ("fused", got))}
            del out64
            gerr = max(float((a - b).abs().max() / a.abs().max())
                       for a, b in zip(ref[1], got[1]))
            del ref, got
            dev_ops = {k: count_device_ops(f) for k, f in sides.items()}
            for p in range(pairs):
                t = {k: _time_calls(f, dev, min_s) for k, f in sides.items()}
                ok = ok and t["fused"] < t["composite"]
                print(json.dumps({"bench": "op", "n": n, "nbx": nbx, "nby": nby, "pair": p,
                                  "composite_ms": round(t["composite"] * 1e3, 4),
                                  "fused_ms": round(t["fused"] * 1e3, 4),
                                  "speedup": round(t["composite"] / t["fused"], 2),
                                  "device_ops": dev_ops,
                                  "composite_chunked": not _composite_fits(n, nbx, nby, dev),
                                  "max_rel_out_diff": err,
                                  "max_rel_out_err_vs_float64": err64,
                                  "max_rel_grad_diff": gerr}), flush=True)
            if profile and dev.type == "cuda":
                print(json.dumps({"bench": "op_kernels", "n": n, "nbx": nbx, "nby": nby,
                                  "fused_kernel_us": _kernel_us(sides["fused"], dev)}), flush=True)
        del ops
    return ok


def end_to_end(params, halos, steps, dev, pairs, repeats, min_s):
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (JointBinnedPopulationSMFModel,
                                                       joint_population_data)

    @dataclass(eq=False)
    class CompositeJointModel(JointBinnedPopulationSMFModel):
        def __post_init__(self):
            super().__post_init__()  # device edges once: a captured step cannot upload them
            self.dev_edges = tuple(torch.tensor(e, dtype=torch.float32, device=dev)
                                   for e in (self.edges, self.edges_y))

        def _cells(self, mu_x, sigma_x, mu_y, sigma_y):
            return _composite(mu_x, sigma_x, mu_y, sigma_y, None, *self.dev_edges)

    data = make_population_data(params, halos, seed=5, device=dev)
    aux = joint_population_data(data)
    models = {"composite": CompositeJointModel(aux_data=aux),
              "fused": JointBinnedPopulationSMFModel(aux_data=aux)}
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
        ok = ok and r["fused"][0] > r["composite"][0]
        # both trajectories hold at least 2 * steps rows: compare the same step
        diff = float((r["fused"][1][2 * steps] - r["composite"][1][2 * steps]).abs().max())
        print(json.dumps({"bench": "e2e", "params": params, "halos": halos, "pair": p,
                          "window_steps": ks, "graph_captured": dict(captured),
                          "composite_steps_per_s": round(r["composite"][0], 2),
                          "fused_steps_per_s": round(r["fused"][0], 2),
                          "speedup": round(r["fused"][0] / r["composite"][0], 2),
                          "max_param_diff_after_2k_steps": diff}), flush=True)
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
    ap.add_argument("--profile", action="store_true",
                    help="one torch.profiler pass of the fused side per op-level row")
    ap.add_argument("--skip", default="", choices=["", "op", "e2e"])
    a = ap.parse_args(argv)
    if a.cpu:
        dev = torch.device("cpu")
        a.sizes, a.params, a.halos, a.steps = [1000, 5000], 200, 4000, 3
        a.pairs, a.repeats, a.min_seconds = 1, 1, 0.0
    else:
        if not torch.cuda.is_available():
            raise SystemExit("binned2d_op.py measures on a GPU; use --cpu for a functional check")
        dev = torch.device("cuda", 0)
    ok = True
    if a.skip != "op":
        ok = op_level([int(s) for s in a.sizes], GRIDS, dev, a.pairs, a.min_seconds,
                      a.profile) and ok
    if a.skip != "e2e":
        ok = end_to_end(a.params, a.halos, a.steps, dev, a.pairs, a.repeats, a.min_seconds) and ok
    print(json.dumps({"fused_faster_in_every_pair": bool(ok)}), flush=True)


if __name__ == "__main__":
    main()
