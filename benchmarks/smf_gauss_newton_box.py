"""Cost of the box-constrained Gauss-Newton fit of the population SMF model on one GPU.

In one process, the sides of each comparison alternating, ``--rounds`` windows of at least
``--window`` seconds each (work that ends in a device synchronise), best / median / worst:

(a) one ``box_dual_pass`` at ``K = nbins``: the fused kernel against the composition of the
    existing ops (``lincomb_cols_``, torch clamp and compares, ``MultiDot``,
    ``weighted_gram``: three passes over ``J``), each with and without writing ``delta``, and
    a copy of the bytes the fused pass needs (``(K + 3) 4 P``, plus ``4 P`` for ``delta``), at
    ``--small-params`` and ``--num-params`` columns;
(b) the fit of part (d) of ``benchmarks/smf_gauss_newton.py`` (against ``--adam-steps`` steps
    of Adam from the same guess, ``gtol`` as given) inside a physical box on ``a`` and
    ``log10 sigma`` for each ``--max-step``.

Prints markdown tables and one JSON line; ``--out`` also writes the tables to a file.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

import torch  # noqa: E402

from multigrad_amd.models.population import PopulationSMFModel, make_population_data  # noqa: E402
from multigrad_amd.ops.box_dual import (box_dual_pass, box_dual_pass_composed,  # noqa: E402
                                        vector_loads)
from smf_gauss_newton import compare, sync, table  # noqa: E402


def bench_pass(n, a, dev):
    K = a.nbins
    g = torch.Generator(device=dev).manual_seed(2)
    J = torch.randn(K, n, generator=g, device=dev)
    coef = torch.randn(K, generator=g, device=dev, dtype=torch.float64)
    d = torch.rand(n, generator=g, device=dev) + 0.1
    lam = 0.3
    scale = K ** 0.5 / lam
    lo = -scale * torch.rand(n, generator=g, device=dev)
    hi = scale * torch.rand(n, generator=g, device=dev)
    delta = torch.empty(n, device=dev)
    ref = box_dual_pass_composed(J.double(), coef, d.double(), lam, lo.double(), hi.double())
    out = box_dual_pass(J, coef, d, lam, lo, hi)
    comp = box_dual_pass_composed(J, coef, d, lam, lo, hi)
    top = ref[:-1].abs().max()
    err = {"fused": float((out[:-1] - ref[:-1]).abs().max() / top),
           "composition": float((comp[:-1] - ref[:-1]).abs().max() / top)}
    free = {"fused": int(out[-1]), "composition": int(comp[-1]), "float64": int(ref[-1])}
    nb, nbd = (K + 3) * 4 * n, (K + 4) * 4 * n
    src, srcd = torch.empty(nb // 8, device=dev), torch.empty(nbd // 8, device=dev)
    dst, dstd = torch.empty_like(src), torch.empty_like(srcd)
    sides = [("fused pass", lambda: box_dual_pass(J, coef, d, lam, lo, hi)),
             ("composition", lambda: box_dual_pass_composed(J, coef, d, lam, lo, hi)),
             ("copy, same bytes", lambda: dst.copy_(src)),
             ("fused pass, delta written", lambda: box_dual_pass(J, coef, d, lam, lo, hi, delta)),
             ("composition, delta written",
              lambda: box_dual_pass_composed(J, coef, d, lam, lo, hi, delta)),
             ("copy, same bytes with delta", lambda: dstd.copy_(srcd))]
    times, calls = compare(sides, a.rounds, a.window)
    share = times["copy, same bytes"][0] / times["fused pass"][0]
    title = (f"(a) one pass, K = {K}, P = {n}; largest error of v, W, s against the float64 "
             f"composition, relative to the largest entry: fused {err['fused']:.1e}, composition "
             f"{err['composition']:.1e}; free columns {free}; 16-byte loads: "
             f"{vector_loads(J, d, lo, hi, delta)}; the fused pass runs at {share:.2f} of "
             "the copy rate (MB needed is the fused pass's for every side; the composition reads "
             "J three times)")
    nbytes = {name: (nbd if "delta" in name else nb) for name, _ in sides}
    return table(title, times, calls, nbytes)


def bench_fit(model, data, a):
    guess = data["guess"]
    sync()
    t0 = time.perf_counter()
    traj = model.run_adam(guess, nsteps=a.adam_steps, learning_rate=a.adam_lr, history="last")
    sync()
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    traj = model.run_adam(guess, nsteps=a.adam_steps, learning_rate=a.adam_lr, history="last")
    sync()
    t_adam = time.perf_counter() - t0
    adam_loss = float(model.calc_loss_from_params(traj[-1]))
    bounds = torch.empty(guess.numel(), 2, dtype=torch.float64)
    bounds[0::2, 0], bounds[0::2, 1] = a.a_range
    bounds[1::2, 0], bounds[1::2, 1] = a.sigma_range
    lines = [f"(b) fit from the guess, {guess.numel()} parameters, {model.shard.n} halos, a in "
             f"{list(a.a_range)}, log10 sigma in {list(a.sigma_range)}, gtol {a.gtol:g} (single "
             "runs, wall time, the first fit carries the first-call costs; the Adam figure is the "
             "second of two runs)", "",
             f"Adam, {a.adam_steps} steps at lr {a.adam_lr}: loss {adam_loss:.3e} in {t_adam:.3f} s "
             f"(first run {t_first:.3f} s)", "",
             "| max_step | loss | iterations | Jacobians | loss evaluations | inner passes | "
             "unconverged solves | active | s | at or below Adam | message |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    rec = {"adam_loss": adam_loss, "adam_s": t_adam, "adam_first_run_s": t_first, "fits": []}
    for cap in a.max_step:
        sync()
        t0 = time.perf_counter()
        res = model.run_gauss_newton_box(guess, param_bounds=bounds, max_step=cap,
                                         maxsteps=a.maxsteps, gtol=a.gtol)
        sync()
        dt = time.perf_counter() - t0
        active = int((res.active != 0).sum())
        rec["fits"].append({"max_step": cap, "loss": float(res.fun), "nit": int(res.nit),
                            "njev": int(res.njev), "nfev": int(res.nfev),
                            "inner_passes": int(res.inner_passes),
                            "inner_unconverged": int(res.inner_unconverged), "active": active,
                            "s": dt, "success": bool(res.success), "message": res.message,
                            "damping": res.damping, "damping_floor": res.damping_floor})
        lines.append(f"| {cap} | {float(res.fun):.3e} | {res.nit} | {res.njev} | {res.nfev} | "
                     f"{res.inner_passes} | {res.inner_unconverged} | {active} | {dt:.3f} | "
                     f"{'yes' if res.fun <= adam_loss else 'no'} | {res.message} |")
    return "\n".join(lines), rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--num-params", type=int, default=10_000_000)
    ap.add_argument("--num-halos", type=int, default=1 << 27)
    ap.add_argument("--small-params", type=int, default=200_000)
    ap.add_argument("--nbins", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--adam-steps", type=int, default=1000)
    ap.add_argument("--adam-lr", type=float, default=0.01)
    ap.add_argument("--maxsteps", type=int, default=50)
    ap.add_argument("--gtol", type=float, default=0.0, help="gradient tolerance of the fits in (b)")
    ap.add_argument("--max-step", type=float, nargs="+", default=[0.07, 0.1, 0.3, 1.0])
    ap.add_argument("--a-range", type=float, nargs=2, default=[-4.0, 0.0])
    ap.add_argument("--sigma-range", type=float, nargs=2, default=[-1.5, 0.5])
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/smf_gauss_newton_box.py needs a GPU")
    dev = torch.device("cuda", 0)
    tables, rec = [], {}

    def emit(name, out):
        tables.append(out[0])
        rec[name] = out[1]
        print(out[0] + "\n", flush=True)

    if "a" in a.parts:
        emit("pass_small", bench_pass(a.small_params, a, dev))
        emit("pass_large", bench_pass(a.num_params, a, dev))
    if "b" in a.parts:
        data = make_population_data(a.num_params, a.num_halos, seed=0, device=dev, nbins=a.nbins)
        model = PopulationSMFModel(aux_data=data)
        model.set_target_from_truth()
        emit("fit", bench_fit(model, data, a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n\n".join(tables) + "\n")
    print(json.dumps({"metric": "box-constrained Gauss-Newton cost",
                      "device": torch.cuda.get_device_name(0), "num_params": a.num_params,
                      "num_halos": a.num_halos, "nbins": a.nbins, "rounds": a.rounds,
                      "window_s": a.window, "results": rec}))


if __name__ == "__main__":
    main()
