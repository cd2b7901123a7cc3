"""Cost of the HMC vector work (csrc/hmc.hip) and of a trajectory on the headline model, one GPU.

(a) ``hmc_leapfrog_`` at ``n = 1e7`` (per-element ``inv_mass``, ``b != 0``), with and without
    the fp64 kinetic energy, against the same update written in torch ops
    (``p.add_(g, alpha=-a); q.addcmul_(inv_mass, p, value=b)`` and, for the energy,
    ``0.5 * (p.double() ** 2 * inv_mass).sum()``) -- in one process, alternating, ``--rounds``
    rounds of ``--calls`` calls.  Bytes are what the update needs: q, p, g, inv_mass read and
    q, p written (24 bytes per element); the rate is those bytes over the time of a call.
(b) Iterations of ``hmc_sample`` with 10 leapfrog steps over the engine objective of the
    headline population model (``bench.py``'s: ``--params`` parameters, ``--halos`` halos),
    ``history="moments"``: wall time per iteration / 10 = ms per leapfrog step (momentum
    draw, 11 leapfrog launches, 10 evaluations, one device->host copy, the commit), beside the
    time of one bare evaluation (``obj.device_call``).

Prints a markdown table and one JSON line; ``--out`` also writes the table to a file.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

import torch  # noqa: E402

from multigrad_amd.ops.hmc import hmc_leapfrog_, hmc_workspace  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--params", type=int, default=10_000_000)
    ap.add_argument("--halos", type=int, default=1 << 27)
    ap.add_argument("--iters", type=int, default=5, help="HMC iterations per timed window")
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    dev = torch.device(a.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        raise SystemExit("benchmarks/hmc.py needs a GPU")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    # ------------------------------------------------------------------ (a) the leapfrog pass
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(0)
    q, p, g = (torch.randn(n, generator=gen, device=dev) for _ in range(3))
    im = 0.5 + torch.rand(n, generator=gen, device=dev)
    ke = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = hmc_workspace(dev)
    ea, eb = 1e-3, 1e-3  # small steps: q and p stay O(1) over the timed calls

    def torch_update():
        p.add_(g, alpha=-ea)
        q.addcmul_(im, p, value=eb)

    def torch_update_ke():
        torch_update()
        return 0.5 * (p.double() ** 2 * im).sum()

    variants = [
        ("hmc_leapfrog_", lambda: hmc_leapfrog_(q, p, g, im, ea, eb)),
        ("torch ops", torch_update),
        ("hmc_leapfrog_ with ke_out", lambda: hmc_leapfrog_(q, p, g, im, ea, eb, ke, ws)),
        ("torch ops with fp64 energy", torch_update_ke),
    ]
    # the two agree before anything is timed
    q0, p0 = q.clone(), p.clone()
    hmc_leapfrog_(q, p, g, im, ea, eb, ke, ws)
    qa, pa, ka = q.clone(), p.clone(), float(ke)
    q.copy_(q0)
    p.copy_(p0)
    kb = float(torch_update_ke())
    agree = max(float((q - qa).abs().max()), float((p - pa).abs().max()))
    agree_ke = abs(ka - kb) / kb
    for _, fn in variants:
        fn()
    sync()
    times = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            sync()
            times[name].append((time.perf_counter() - t0) / a.calls)
    nbytes = 24 * n
    lines = [f"(a) n = {n}, {a.rounds} rounds of {a.calls} calls, alternating; device {dev}; "
             f"max |fused - torch| = {agree:.2e} (q, p), energies differ by {agree_ke:.1e} relative",
             "",
             "| variant | best us | median us | worst us | MB needed | TB/s at best |",
             "|---|---|---|---|---|---|"]
    rec = {}
    for name, _ in variants:
        t = sorted(times[name])
        best, med, worst = t[0], t[len(t) // 2], t[-1]
        rec[name] = {"best_us": best * 1e6, "median_us": med * 1e6, "worst_us": worst * 1e6,
                     "bytes": nbytes}
        lines.append(f"| {name} | {best * 1e6:.1f} | {med * 1e6:.1f} | {worst * 1e6:.1f} | "
                     f"{nbytes / 1e6:.0f} | {nbytes / best / 1e12:.2f} |")
    out = {"metric": "hmc cost", "n": n, "device": str(dev), "agreement": agree,
           "agreement_ke": agree_ke, "leapfrog": rec}
    del q, p, g, im, q0, p0, qa, pa

    # ------------------------------------------------------------------ (b) a trajectory
    if not a.skip_model:
        from multigrad_amd.models.population import PopulationSMFModel, make_population_data
        from multigrad_amd.optim.hmc import hmc_sample
        L = 10
        data = make_population_data(a.params, a.halos, seed=1234, device=dev)
        model = PopulationSMFModel(aux_data=data)
        model.set_target_from_truth()
        eng = model.fused_engine()
        obj = eng.lbfgs_objective(data["guess"])
        x = obj.x0()
        call = getattr(obj, "device_call", None) if dev.type == "cuda" else obj
        for _ in range(3):
            call(x)
        sync()
        ev = []
        for _ in range(a.rounds):
            sync()
            t0 = time.perf_counter()
            for _ in range(20):
                call(x)
            sync()
            ev.append((time.perf_counter() - t0) / 20)
        kw = dict(warmup=0, nleapfrog=L, step_size=1e-4, history="moments", track=[0, 1])
        hmc_sample(obj, nsamples=2, **kw)  # warm-up: code objects, buffers
        sync()
        it = []
        res = None
        for _ in range(a.rounds):
            sync()
            t0 = time.perf_counter()
            res = hmc_sample(obj, nsamples=a.iters, **kw)
            sync()
            # one evaluation per call of hmc_sample is the initial one, not a trajectory's
            it.append((time.perf_counter() - t0) / (a.iters * L + 1))
        ev.sort()
        it.sort()
        lines += ["",
                  f"(b) {a.params} parameters, {a.halos} halos, L = {L}, {a.rounds} rounds of "
                  f"{a.iters} iterations (accept rate {res.accept_rate:.2f}, vector length "
                  f"{obj.n_local})",
                  "",
                  "| per leapfrog step | best ms | median ms | worst ms |",
                  "|---|---|---|---|",
                  f"| hmc_sample, time / evaluations | {it[0] * 1e3:.3f} | "
                  f"{it[len(it) // 2] * 1e3:.3f} | {it[-1] * 1e3:.3f} |",
                  f"| bare evaluation (device_call) | {ev[0] * 1e3:.3f} | "
                  f"{ev[len(ev) // 2] * 1e3:.3f} | {ev[-1] * 1e3:.3f} |"]
        out["trajectory"] = {"params": a.params, "halos": a.halos, "L": L,
                             "step_ms": [t * 1e3 for t in it], "eval_ms": [t * 1e3 for t in ev],
                             "accept_rate": res.accept_rate}
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
