"""Bounded Gauss-Newton fit of the population SMF model: every population's ``a`` and
``log10 sigma`` stay inside a physical box and no parameter moves by more than ``--max-step``
in one iteration (``OnePointModel.run_gauss_newton_box``).  Prints the fit beside the
unconstrained dual fit and Adam, and how many parameters ended on a bound.

    python examples/population_gauss_newton_box.py [--num-params P] [--num-halos N] [--max-step D]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from multigrad_amd.models.population import PopulationSMFModel, make_population_data  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-params", type=int, default=2000)
    ap.add_argument("--num-halos", type=int, default=54_000)
    ap.add_argument("--max-step", type=float, default=0.3)
    ap.add_argument("--adam-steps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(a.num_params, a.num_halos, seed=3, device=dev)
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()
    guess = data["guess"]

    # a in [-4, 0], log10 sigma in [-1.5, 0.5]: the rows alternate as the parameters do
    bounds = torch.tensor([[-4.0, 0.0], [-1.5, 0.5]], dtype=torch.float64).repeat(a.num_params // 2, 1)
    box = model.run_gauss_newton_box(guess, param_bounds=bounds, max_step=a.max_step, gtol=0.0)
    dual = model.run_gauss_newton(guess, solver="dual", gtol=0.0)
    traj = model.run_adam(guess, nsteps=a.adam_steps, learning_rate=0.01)
    adam_loss = float(model.calc_loss_from_params(traj[-1]))

    print(f"Gauss-Newton in the box ({box.jac_mode} Jacobian): loss {float(box.fun):.3e} after "
          f"{box.nit} iterations ({box.njev} Jacobians, {box.nfev} loss evaluations, "
          f"{box.inner_passes} inner passes, {box.inner_unconverged} unconverged solves): {box.message}")
    print(f"Gauss-Newton, unconstrained dual: loss {float(dual.fun):.3e} after {dual.nit} iterations: "
          f"{dual.message}")
    print(f"Adam: loss {adam_loss:.3e} after {a.adam_steps} steps")
    x = box.x.double().cpu()
    print(f"parameters on a bound: {int((box.active != 0).sum())} of {x.numel()}; a in "
          f"[{float(x[0::2].min()):.3f}, {float(x[0::2].max()):.3f}], log10 sigma in "
          f"[{float(x[1::2].min()):.3f}, {float(x[1::2].max()):.3f}]")
    assert bool(((x >= bounds[:, 0]) & (x <= bounds[:, 1])).all())
    assert box.solver == "dual-box"
