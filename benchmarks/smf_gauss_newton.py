"""Cost of the dual Gauss-Newton fit of the population SMF model on one GPU.

In one process, the sides of each comparison alternating, ``--rounds`` windows of at least
``--window`` seconds each (work that ends in a device synchronise), best / median / worst:

(a) ``smf_jacobian_into`` (one pass over the lanes residuals) against ``nb`` residual VJPs
    with unit cotangents on the same shard, at ``--small-params`` and ``--num-params``
    parameters with ~27 halos per population, with the bytes each side needs;
(b) ``weighted_gram`` at ``K = nbins``, ``n = --num-params`` against torch's composite
    ``(J * w) @ J.T`` in float32 and in float64, and a copy of the same number of bytes;
(c) the parts of one dual iteration on the headline model: forward (one loss evaluation),
    Jacobian (residual forward + Jacobian pass), ``compact_diag_``, ``weighted_gram``, and
    one trial (step pass + vector add + loss evaluation);
(d) the Gauss-Newton iterations and wall time until a trial loss is at or below the loss
    ``run_adam`` reaches in ``--adam-steps`` steps from the same guess.  ``--gtol`` (default 0)
    is the fit's gradient tolerance: the drivers' default of 1e-8 on ``max |grad|`` is an
    absolute bound, and at 1e7 parameters every entry of the gradient is that small long
    before the loss has converged (a parameter's share of the loss falls as 1 / P).

Prints markdown tables and one JSON line; ``--out`` also writes the tables to a file.
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MULTIGRAD_PROGRESS", "0")

import torch  # noqa: E402

from multigrad_amd.models.population import PopulationSMFModel, make_population_data  # noqa: E402
from multigrad_amd.ops import smf as S  # noqa: E402
from multigrad_amd.ops.gram import weighted_gram  # noqa: E402
from multigrad_amd.optim import gauss_newton as gn  # noqa: E402


def sync():
    torch.cuda.synchronize()


def timed(fn, calls):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) / calls


def compare(sides, rounds, window):
    """``{name: sorted seconds per call}``: every side warmed, its calls per window sized
    from one timed call, then ``rounds`` rounds with the sides alternating."""
    calls = {}
    for name, fn in sides:
        fn()
        calls[name] = max(1, math.ceil(window / max(timed(fn, 2), 1e-7)))
    times = {name: [] for name, _ in sides}
    for _ in range(rounds):
        for name, fn in sides:
            times[name].append(timed(fn, calls[name]))
    return {k: sorted(v) for k, v in times.items()}, calls


def table(title, times, calls, nbytes=None):
    lines = [title, "", "| side | calls/window | best ms | median ms | worst ms | MB needed | TB/s at best |",
             "|---|---|---|---|---|---|---|"]
    rec = {}
    for name, t in times.items():
        best, med, worst = t[0], t[len(t) // 2], t[-1]
        nb = None if nbytes is None else nbytes.get(name)
        rec[name] = {"best_ms": best * 1e3, "median_ms": med * 1e3, "worst_ms": worst * 1e3,
                     "bytes": nb, "calls_per_window": calls[name]}
        lines.append(f"| {name} | {calls[name]} | {best * 1e3:.3f} | {med * 1e3:.3f} | {worst * 1e3:.3f} | "
                     + ("not counted | |" if nb is None else f"{nb / 1e6:.0f} | {nb / best / 1e12:.2f} |"))
    return "\n".join(lines), rec


def bench_jacobian(num_params, a, dev):
    npop = num_params // 2
    data = make_population_data(num_params, 27 * npop, seed=0, device=dev, nbins=a.nbins)
    shard, bins, th = data["shard"], data["bins"], data["guess"]
    assert shard.layout == "lanes" and not shard.vjp_recompute
    nb = bins.nb
    out = torch.zeros(bins.nbp, device=dev)
    S.smf_forward_into(th, shard, bins, True, out, resid=True)
    one = torch.empty(nb, num_params, device=dev)
    many = torch.empty(nb, num_params, device=dev)
    hs = S._unit_edge_weights(bins, dev)

    def one_pass():
        S.smf_jacobian_into(th, shard, bins, True, one, residuals_ready=True)

    def nb_pass():
        for k in range(nb):
            S.smf_vjp_into(th, shard, bins, True, hs[k], many[k], residuals_ready=True)

    one_pass()
    nb_pass()
    agree = float((one - many).abs().max() / many.abs().max())
    resid = shard.resid.numel() * 4
    ids = shard.nslots * 8                       # slot population + slot part
    write = nb * num_params * 4
    nbytes = {"one pass": resid + ids + num_params * 4 + write,
              f"{nb} VJP passes": nb * (resid + ids + num_params * 4) + write}
    times, calls = compare([("one pass", one_pass), (f"{nb} VJP passes", nb_pass)], a.rounds, a.window)
    title = (f"(a) Jacobian, {num_params} parameters, {shard.n} halos, {nb} bins, {shard.ngroups} lane "
             f"groups; max |one pass - VJPs| / max |VJPs| = {agree:.2e}")
    return table(title, times, calls, nbytes)


def bench_gram(a, dev):
    K, n = a.nbins, a.num_params
    g = torch.Generator(device=dev).manual_seed(2)
    J = torch.randn(K, n, generator=g, device=dev)
    w = torch.rand(n, generator=g, device=dev) + 0.1
    nbytes = (K + 1) * n * 4
    src = torch.empty(nbytes // 8, device=dev)
    dst = torch.empty_like(src)
    ref = (J.double() * w.double()) @ J.double().T
    err = {"weighted_gram": float((weighted_gram(J, w) - ref).abs().max() / ref.abs().max()),
           "torch float32": float((((J * w) @ J.T).double() - ref).abs().max() / ref.abs().max())}
    sides = [("weighted_gram", lambda: weighted_gram(J, w)),
             ("torch float32 (J * w) @ J.T", lambda: (J * w) @ J.T),
             ("torch float64 composite", lambda: (J.double() * w.double()) @ J.double().T),
             ("copy, same bytes", lambda: dst.copy_(src))]
    times, calls = compare(sides, a.rounds, a.window)
    share = times["copy, same bytes"][0] / times["weighted_gram"][0]
    title = (f"(b) weighted Gram, K = {K}, n = {n}; relative error against the float64 composite: "
             f"weighted_gram {err['weighted_gram']:.1e}, torch float32 {err['torch float32']:.1e}; "
             f"weighted_gram runs at {share:.2f} of the copy rate (MB needed is the kernel's "
             f"(K + 1) n floats for every side; the composites move more)")
    return table(title, times, calls, {name: nbytes for name, _ in sides})


def bench_iteration(model, guess, a):
    """(c): the parts of one dual iteration, each in its own windows."""
    loss, c, J, H, used = model._gauss_newton_factors(guess)
    fac = gn._DualFactors(J, c, H, [])
    Hp = fac.L @ fac.L.T
    x = guess.reshape(-1)
    sides = [("forward (loss evaluation)", lambda: model.calc_loss_from_params(guess)),
             ("Jacobian (forward + one pass)",
              lambda: model.calc_partial_sumstats_and_jacobian_from_params(guess)),
             ("compact_diag_", lambda: gn._diag_jhj(J, Hp)),
             ("weighted_gram", lambda: weighted_gram(J, fac.inv_d)),
             ("trial (step, add, loss)",
              lambda: model.calc_loss_from_params((x + fac.step(1e-3)).reshape(guess.shape)))]
    times, calls = compare(sides, a.rounds, a.window)
    title = (f"(c) parts of one dual iteration, {guess.numel()} parameters, {model.shard.n} halos, "
             f"jac_mode {used}")
    return table(title, times, calls)


def bench_fit(model, guess, a):
    """(d): Gauss-Newton against ``--adam-steps`` steps of Adam from the same guess."""
    sync()
    t0 = time.perf_counter()
    traj = model.run_adam(guess, nsteps=a.adam_steps, learning_rate=a.adam_lr, history="last")
    sync()
    t_adam_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    traj = model.run_adam(guess, nsteps=a.adam_steps, learning_rate=a.adam_lr, history="last")
    sync()
    t_adam = time.perf_counter() - t0
    adam_loss = float(model.calc_loss_from_params(traj[-1]))
    log, jacs = [], [0]
    loss_fn, factors_fn = model.calc_loss_from_params, model._gauss_newton_factors

    def loss_wrapper(p, **k):
        v = loss_fn(p, **k)
        log.append((time.perf_counter(), float(v), jacs[0]))
        return v

    def factors_wrapper(*args, **k):
        jacs[0] += 1
        return factors_fn(*args, **k)

    model.calc_loss_from_params, model._gauss_newton_factors = loss_wrapper, factors_wrapper
    try:
        sync()
        t0 = time.perf_counter()
        res = model.run_gauss_newton(guess, maxsteps=a.maxsteps, solver="dual", gtol=a.gtol)
        sync()
        t_gn = time.perf_counter() - t0
    finally:
        del model.calc_loss_from_params, model._gauss_newton_factors
    hit = next(((t - t0, i + 1, j) for i, (t, v, j) in enumerate(log) if v <= adam_loss), None)
    rec = {"adam_steps": a.adam_steps, "adam_lr": a.adam_lr, "adam_loss": adam_loss,
           "adam_s": t_adam, "adam_first_run_s": t_adam_first, "gn_loss": float(res.fun),
           "gn_nit": int(res.nit), "gn_njev": int(res.njev), "gn_nfev": int(res.nfev),
           "gn_s": t_gn, "gn_gtol": a.gtol, "gn_message": res.message, "gn_jac_mode": res.jac_mode,
           "gn_reached_adam_loss": None if hit is None else
           {"s": hit[0], "loss_evaluations": hit[1], "jacobians": hit[2]}}
    lines = [f"(d) fit from the guess, {guess.numel()} parameters, {model.shard.n} halos (single runs, "
             "wall time; the Adam figure is the second of two runs, its engine and graphs warm)", "",
             f"- Adam, {a.adam_steps} steps at lr {a.adam_lr}: loss {adam_loss:.3e} in {t_adam:.3f} s "
             f"(first run {t_adam_first:.3f} s)",
             f"- Gauss-Newton (dual, {res.jac_mode} Jacobian, gtol {a.gtol:g}): loss {float(res.fun):.3e} after {res.nit} "
             f"iterations, {res.njev} Jacobians, {res.nfev} loss evaluations, {t_gn:.3f} s: {res.message}"]
    if hit is None:
        lines.append("- Gauss-Newton did not reach Adam's loss")
    else:
        lines.append(f"- Gauss-Newton was at or below Adam's loss after {hit[0]:.3f} s: {hit[2]} Jacobians, "
                     f"{hit[1]} loss evaluations")
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
    ap.add_argument("--gtol", type=float, default=0.0, help="gradient tolerance of the fit in (d)")
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/smf_gauss_newton.py needs a GPU")
    dev = torch.device("cuda", 0)
    tables, rec = [], {}

    def emit(name, out):
        tables.append(out[0])
        rec[name] = out[1]
        print(out[0] + "\n", flush=True)

    if "a" in a.parts:
        emit("jacobian_small", bench_jacobian(a.small_params, a, dev))
        emit("jacobian_large", bench_jacobian(a.num_params, a, dev))
    if "b" in a.parts:
        emit("gram", bench_gram(a, dev))
    if "c" in a.parts or "d" in a.parts:
        data = make_population_data(a.num_params, a.num_halos, seed=0, device=dev, nbins=a.nbins)
        model = PopulationSMFModel(aux_data=data)
        model.set_target_from_truth()
        if "c" in a.parts:
            emit("iteration", bench_iteration(model, data["guess"], a))
        if "d" in a.parts:
            emit("fit", bench_fit(model, data["guess"], a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n\n".join(tables) + "\n")
    print(json.dumps({"metric": "dual Gauss-Newton cost", "device": torch.cuda.get_device_name(0),
                      "num_params": a.num_params, "num_halos": a.num_halos, "nbins": a.nbins,
                      "rounds": a.rounds, "window_s": a.window, "results": rec}))


if __name__ == "__main__":
    main()
