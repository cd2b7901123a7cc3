"""Error bars from the exact Hessian: fit a small population model that bins with
``gaussian_binned_sum`` (GroupedBinnedPopulationSMFModel), then invert
``calc_hessian_from_params`` at the optimum and print the 1-sigma errors beside the diagonal
of the L-BFGS approximation ``res.hess_inv`` (rank <= history, from a few (s, y) pairs).

    python examples/user_model_errors.py [--num-pops J] [--num-halos N] [--num-steps K]
"""
import argparse
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
    ap.add_argument("--num-steps", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(2 * a.num_pops, a.num_halos, seed=3, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))
    res = model.run_bfgs(data["guess"], maxsteps=a.num_steps, method="device")
    best = torch.as_tensor(res.x, dtype=torch.float32, device=dev)
    H = model.calc_hessian_from_params(best).double().cpu()
    # reading the loss as a chi-square (unit errors on the log residuals), the parameter
    # covariance is 2 H^-1.  Only the sum over the populations is observed, so some
    # directions are (nearly) unconstrained: eigenvalues below RTOL of the largest are left
    # out (pinv), and the errors are those within the constrained directions.
    RTOL = 1e-4
    ev = torch.linalg.eigvalsh(H)
    cov = 2.0 * torch.linalg.pinv(H, rtol=RTOL, hermitian=True)
    exact = cov.diagonal().clamp_min(0).sqrt()
    approx = (2.0 * torch.as_tensor(res.hess_inv.diagonal()).double().cpu()).clamp_min(0).sqrt()
    kept = int((ev.abs() > RTOL * ev.abs().max()).sum())
    print(f"loss {float(res.fun):.3e} after {int(res.nit)} iterations; Hessian eigenvalues "
          f"{float(ev[0]):.3e} .. {float(ev[-1]):.3e}, {kept} of {ev.numel()} directions "
          "constrained")
    print("param      fitted     truth   1-sigma (exact Hessian)   1-sigma (L-BFGS hess_inv)")
    for i, (x, t, e, q) in enumerate(zip(best.tolist(), data["truth"].tolist(), exact.tolist(),
                                         approx.tolist())):
        print(f"{i:5d} {x:11.4f} {t:9.4f} {e:25.3e} {q:27.3e}")
    assert torch.isfinite(H).all() and torch.equal(H, H.T)
