"""Gauss-Newton at any parameter count: fit the population SMF model by damped Gauss-Newton
steps in the dual (K x K) form.  The dense form needs the [P, P] Gauss-Newton matrix; the
dual form keeps only the [K, P] sumstat Jacobian, written in one pass over the forward's
residuals (``jac_mode == "native"``), and solves a K x K system per trial step, so the same
call works at 2e3 and at 1e7 parameters.  ``res.hess_inv`` is an operator on the device:
the example prints the range of its diagonal.

    python examples/population_gauss_newton.py [--num-params P] [--num-halos N] [--maxsteps M]
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
    ap.add_argument("--maxsteps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(a.num_params, a.num_halos, seed=3, device=dev)
    model = PopulationSMFModel(aux_data=data)
    model.set_target_from_truth()

    start = float(model.calc_loss_from_params(data["guess"]))
    res = model.run_gauss_newton(data["guess"], maxsteps=a.maxsteps, solver="dual")
    diag = res.hess_inv.diagonal()
    print(f"start: loss {start:.3e} ({a.num_params} parameters, {a.num_halos} halos, {dev})")
    print(f"Gauss-Newton ({res.solver} solve, jac_mode {res.jac_mode}): loss {float(res.fun):.3e} "
          f"nit {res.nit} njev {res.njev} nfev {res.nfev}: {res.message}")
    print(f"hess_inv diagonal: largest {float(diag.max()):.3e} smallest {float(diag.min()):.3e}")
    assert res.success and res.x.device.type == dev.type and float(res.fun) < start
