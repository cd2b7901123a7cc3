"""Cost of the Gaussian-prior vector work (csrc/prior.hip) and of a trajectory and an L-BFGS
iteration with a prior on the headline model, one GPU.  The method of benchmarks/hmc.py:
variants alternating inside one process, ``--rounds`` rounds, host clock around work that ends
in a device synchronise.

(a) For every ``--n`` (default 1e7, where six 40 MB vectors sit at the edge of the 256 MiB
    Infinity Cache, and 4e7, where nothing is cache-resident), per-element ``inv_mass``,
    ``b != 0``, each with and without the energies:
    ``hmc_leapfrog_prior_`` with a per-element and with a broadcast prior;
    ``gaussian_prior_grad_`` on p (``c = -ap``, from the input q) followed by
    ``hmc_leapfrog_``, the two-pass composition that computes the same update;
    ``hmc_leapfrog_`` alone, the flat case.
    Bytes are what the update needs: q, p, g, inv_mass read and q, p written, 24 per element,
    plus mean and inv_var, 32 per element, for a per-element prior.
(b) ``hmc_sample`` over the engine objective of the headline population model with a
    per-element prior against the flat run, alternating: time per leapfrog step, with the
    time of a call without iterations (set-up and the first evaluation; with a prior also the
    copy of its mean and inverse variance to the device) taken off; one evaluation through
    the objective, bare (``device_call``) and through ``PriorObjective.partial_call``; and
    ``lbfgs_minimize`` over both: iterations and evaluations per second (the two runs
    minimise different functions, so their line searches differ).

Prints a markdown table and one JSON line; ``--out`` also writes the table to a file.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from multigrad_amd.ops.hmc import hmc_leapfrog_, hmc_workspace  # noqa: E402
from multigrad_amd.ops.prior import (gaussian_prior_grad_, hmc_leapfrog_prior_,  # noqa: E402
                                     prior_workspace)


def leapfrog_variants(n, dev, rounds, calls, sync):
    gen = torch.Generator(device=dev).manual_seed(0)
    q, p, g, m = (torch.randn(n, generator=gen, device=dev) for _ in range(4))
    im = 0.5 + torch.rand(n, generator=gen, device=dev)
    w = 0.5 + torch.rand(n, generator=gen, device=dev)
    m1, w1 = m[:1].clone(), w[:1].clone()
    en = torch.zeros(2, dtype=torch.float64, device=dev)
    ke, pen = en[0:1], en[1:2]
    ws, pws = hmc_workspace(dev), prior_workspace(dev)
    ea, eb, eap = 1e-3, 1e-3, 1e-3  # small steps: q and p stay O(1) over the timed calls

    def two_pass(energies):
        # the prior's half of the momentum update first (it reads the input q), then the
        # flat leapfrog: p' = (p - ap w (q - m)) - a g
        gaussian_prior_grad_(q, p, m, w, -eap, p, pen if energies else None, pws)
        hmc_leapfrog_(q, p, g, im, ea, eb, ke if energies else None, ws)

    variants = [
        ("hmc_leapfrog_prior_, per-element prior", 32,
         lambda: hmc_leapfrog_prior_(q, p, g, im, ea, eb, m, w, eap)),
        ("hmc_leapfrog_prior_, broadcast prior", 24,
         lambda: hmc_leapfrog_prior_(q, p, g, im, ea, eb, m1, w1, eap)),
        ("gaussian_prior_grad_ + hmc_leapfrog_ (two passes)", 32, lambda: two_pass(False)),
        ("hmc_leapfrog_ (flat)", 24, lambda: hmc_leapfrog_(q, p, g, im, ea, eb)),
        ("hmc_leapfrog_prior_, per-element prior, ke and pen", 32,
         lambda: hmc_leapfrog_prior_(q, p, g, im, ea, eb, m, w, eap, ke, pen, pws)),
        ("hmc_leapfrog_prior_, broadcast prior, ke and pen", 24,
         lambda: hmc_leapfrog_prior_(q, p, g, im, ea, eb, m1, w1, eap, ke, pen, pws)),
        ("gaussian_prior_grad_ + hmc_leapfrog_ (two passes), ke and pen", 32,
         lambda: two_pass(True)),
        ("hmc_leapfrog_ (flat), ke", 24, lambda: hmc_leapfrog_(q, p, g, im, ea, eb, ke, ws)),
    ]
    # the fused pass and the composition agree before anything is timed
    q0, p0 = q.clone(), p.clone()
    variants[4][2]()
    qa, pa, ea_f = q.clone(), p.clone(), en.clone()
    q.copy_(q0)
    p.copy_(p0)
    two_pass(True)
    agree = max(float((q - qa).abs().max()), float((p - pa).abs().max()))
    agree_en = float(((en - ea_f).abs() / ea_f.abs()).max())
    del q0, p0, qa, pa
    for _, _, fn in variants:
        fn()
    sync()
    times = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, _, fn in variants:
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / calls)
    lines = [f"(a) n = {n}, {rounds} rounds of {calls} calls, alternating; device {dev}; "
             f"max |fused - two passes| = {agree:.2e} (q, p), energies differ by {agree_en:.1e} "
             "relative", "",
             "| variant | best us | median us | worst us | MB needed | TB/s at best |",
             "|---|---|---|---|---|---|"]
    rec = {}
    for name, per, _ in variants:
        t = sorted(times[name])
        best, med, worst = t[0], t[len(t) // 2], t[-1]
        rec[name] = {"us": [v * 1e6 for v in times[name]], "bytes": per * n}
        lines.append(f"| {name} | {best * 1e6:.1f} | {med * 1e6:.1f} | {worst * 1e6:.1f} | "
                     f"{per * n / 1e6:.0f} | {per * n / best / 1e12:.2f} |")
    # every alternating pair: the fused pass against the composition of the same round
    for fused, comp in ((0, 2), (4, 6)):
        a, b = times[variants[fused][0]], times[variants[comp][0]]
        lines.append(f"\nfused / two passes per round ({variants[fused][0]}): "
                     + ", ".join(f"{x / y:.3f}" for x, y in zip(a, b)))
    return lines, {"n": n, "agreement": agree, "agreement_energies": agree_en, "variants": rec}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, nargs="+", default=[10_000_000, 40_000_000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--params", type=int, default=10_000_000)
    ap.add_argument("--halos", type=int, default=1 << 27)
    ap.add_argument("--iters", type=int, default=10, help="HMC iterations per timed window")
    ap.add_argument("--lbfgs-iters", type=int, default=8, help="L-BFGS iterations per window")
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("benchmarks/prior.py needs a GPU")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    lines, out = [], {"metric": "prior cost", "device": str(dev), "leapfrog": []}
    for n in a.n:
        part, rec = leapfrog_variants(n, dev, a.rounds, a.calls, sync)
        lines += part + [""]
        out["leapfrog"].append(rec)
        if dev.type == "cuda":
            torch.cuda.empty_cache()

    if not a.skip_model:
        from multigrad_amd.models.population import PopulationSMFModel, make_population_data
        from multigrad_amd.optim.hmc import hmc_sample
        from multigrad_amd.optim.lbfgs import lbfgs_minimize
        from multigrad_amd.optim.prior import GaussianPrior, PriorObjective
        L = 10
        data = make_population_data(a.params, a.halos, seed=1234, device=dev)
        model = PopulationSMFModel(aux_data=data)
        model.set_target_from_truth()
        eng = model.fused_engine()
        obj = eng.lbfgs_objective(data["guess"])
        g0 = data["guess"].double().cpu().numpy()
        prior = GaussianPrior(g0, np.linspace(0.5, 2.0, g0.size))
        kw = dict(warmup=0, nleapfrog=L, step_size=1e-4, history="moments", track=[0, 1])
        runs = {"flat": dict(), "per-element prior": dict(prior=prior)}
        for extra in runs.values():
            hmc_sample(obj, nsamples=2, **kw, **extra)  # warm-up: code objects, buffers
        sync()
        step = {k: [] for k in runs}
        setup = {k: [] for k in runs}
        acc = {}
        for _ in range(a.rounds):
            for name, extra in runs.items():
                sync()
                t0 = time.perf_counter()
                hmc_sample(obj, nsamples=0, **kw, **extra)
                sync()
                t1 = time.perf_counter()
                res = hmc_sample(obj, nsamples=a.iters, **kw, **extra)
                sync()
                t2 = time.perf_counter()
                setup[name].append(t1 - t0)
                step[name].append(((t2 - t1) - (t1 - t0)) / (a.iters * L))
                acc[name] = res.accept_rate
        lines += [f"(b) {a.params} parameters, {a.halos} halos, L = {L}, {a.rounds} rounds of "
                  f"{a.iters} iterations, alternating (vector length {obj.n_local})", "",
                  "| hmc_sample, per leapfrog step | best ms | median ms | worst ms | accept | "
                  "call without iterations, median ms |", "|---|---|---|---|---|---|"]
        for name, t in step.items():
            s = sorted(t)
            lines.append(f"| {name} | {s[0] * 1e3:.3f} | {s[len(s) // 2] * 1e3:.3f} | "
                         f"{s[-1] * 1e3:.3f} | {acc[name]:.2f} | "
                         f"{sorted(setup[name])[len(s) // 2] * 1e3:.1f} |")
        lines.append("\nprior / flat per round: "
                     + ", ".join(f"{x / y:.3f}" for x, y in zip(step["per-element prior"],
                                                                 step["flat"])))
        # the device L-BFGS over the same objective
        objs = {"bare": obj, "PriorObjective": PriorObjective(obj, prior, 1.0)}
        x = obj.x0()
        calls = {"bare": lambda: obj.device_call(x),
                 "PriorObjective": lambda: objs["PriorObjective"].partial_call(x, device=True)}
        if dev.type != "cuda":
            calls = {"bare": lambda: obj(x), "PriorObjective": lambda: objs["PriorObjective"](x)}
        ev = {k: [] for k in calls}
        for fn in calls.values():
            fn()
        for _ in range(a.rounds):
            for name, fn in calls.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(20):
                    fn()
                sync()
                ev[name].append((time.perf_counter() - t0) / 20)
        lines += ["", "one evaluation through the objective, 20 calls per window, alternating", "",
                  "| objective | best ms | median ms | worst ms |", "|---|---|---|---|"]
        for name, t in ev.items():
            s = sorted(t)
            lines.append(f"| {name} | {s[0] * 1e3:.3f} | {s[len(s) // 2] * 1e3:.3f} | "
                         f"{s[-1] * 1e3:.3f} |")
        okw = dict(maxiter=a.lbfgs_iters, hess_inv=False, ftol=0.0, gtol=0.0)
        for o in objs.values():
            lbfgs_minimize(o, **dict(okw, maxiter=2))
        sync()
        rate = {k: [] for k in objs}
        for _ in range(a.rounds):
            for name, o in objs.items():
                sync()
                t0 = time.perf_counter()
                res = lbfgs_minimize(o, **okw)
                sync()
                dt = time.perf_counter() - t0
                rate[name].append((res.nit / dt, res.nfev / dt, int(res.nit), int(res.nfev)))
        lines += ["", f"device L-BFGS, {a.lbfgs_iters} iterations per window, alternating", "",
                  "| objective | iterations/s best | median | worst | evaluations/s best | "
                  "iterations, evaluations of the last window |", "|---|---|---|---|---|---|"]
        for name, r in rate.items():
            its = sorted((v[0] for v in r), reverse=True)
            evs = max(v[1] for v in r)
            lines.append(f"| {name} | {its[0]:.1f} | {its[len(its) // 2]:.1f} | {its[-1]:.1f} | "
                         f"{evs:.1f} | {r[-1][2]}, {r[-1][3]} |")
        out["trajectory"] = {"params": a.params, "halos": a.halos, "L": L,
                             "step_ms": {k: [t * 1e3 for t in v] for k, v in step.items()},
                             "setup_ms": {k: [t * 1e3 for t in v] for k, v in setup.items()},
                             "eval_ms": {k: [t * 1e3 for t in v] for k, v in ev.items()},
                             "lbfgs": {k: [list(v) for v in r] for k, r in rate.items()}}
        if not getattr(eng, "cached", False):
            eng.close()
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(table + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
