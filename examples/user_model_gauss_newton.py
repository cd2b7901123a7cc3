"""Gauss-Newton fit and Fisher errors: fit a small population model that bins with
``gaussian_binned_sum`` (GroupedBinnedPopulationSMFModel) by damped Gauss-Newton steps on
the forward-mode sumstat Jacobian, print the iterations beside 100 steps of Adam, and the
Fisher 1-sigma errors beside those from the exact Hessian (``2 H^-1``, as in
examples/user_model_errors.py).

    python examples/user_model_gauss_newton.py [--num-pops J] [--num-halos N] [--adam-steps K]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from multigrad_amd.models.population import PopulationSMFModel, make_population_data  # noqa: E402
from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,  # noqa: E402
                                                   torch_population_data)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-pops", type=int, default=4)
    ap.add_argument("--num-halos", type=int, default=20_000)
    ap.add_argument("--adam-steps", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(2 * a.num_pops, a.num_halos, seed=3, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))

    res = model.run_gauss_newton(data["guess"])
    traj = model.run_adam(data["guess"], nsteps=a.adam_steps, learning_rate=0.01)
    adam_loss = float(model.calc_loss_from_params(traj[-1]))
    print(f"Gauss-Newton ({res.jac_mode} Jacobian): loss {float(res.fun):.3e} after {res.nit} "
          f"iterations ({res.njev} Jacobians, {res.nfev} loss evaluations): {res.message}")
    print(f"Adam: loss {adam_loss:.3e} after {a.adam_steps} steps")

    best = torch.as_tensor(res.x, dtype=torch.float32, device=dev)
    # Reading the loss (the mean over K bins of the squared log10 residuals) as a chi-square
    # makes 2 H^-1 the covariance at the optimum; the same reading gives the sumstats the
    # variances var(S_k) = K (ln(10) S_k)^2, and the Fisher matrix is then H/2 where the
    # residuals vanish.  Only the sum over the populations is observed, so some directions
    # are (nearly) unconstrained: eigenvalues below RTOL of the largest are left out (pinv).
    RTOL = 1e-4
    S = model.calc_sumstats_from_params(best).double()
    F = model.calc_fisher_from_params(best, S.numel() * (math.log(10.0) * S) ** 2).cpu()
    H = model.calc_hessian_from_params(best).double().cpu()
    fisher = torch.linalg.pinv(F, rtol=RTOL, hermitian=True).diagonal().clamp_min(0).sqrt()
    exact = (2.0 * torch.linalg.pinv(H, rtol=RTOL, hermitian=True)).diagonal().clamp_min(0).sqrt()
    print("param      fitted     truth   1-sigma (Fisher)   1-sigma (2 H^-1)")
    for i, (x, t, f, e) in enumerate(zip(best.tolist(), data["truth"].tolist(), fisher.tolist(),
                                         exact.tolist())):
        print(f"{i:5d} {x:11.4f} {t:9.4f} {f:18.3e} {e:18.3e}")
    assert res.success and torch.isfinite(F).all()
