"""Posterior samples beside the Hessian's error bars: fit the grouped binned population model
of ``examples/user_model_errors.py`` (GroupedBinnedPopulationSMFModel), then draw from
``exp(-loss_scale * loss)`` with ``run_hmc`` and print the standard deviation of the draws
beside the 1-sigma errors from the exact Hessian at the optimum.

    python examples/user_model_posterior.py [--num-pops J] [--num-halos N] [--nsamples S]

Reading the loss as a chi-square with errors ``sigma`` on the log residuals, the posterior is
``exp(-loss / (2 sigma^2))``: ``loss_scale = 1 / (2 sigma^2)``.  Only the sum over the
populations is observed, so some directions are nearly unconstrained: there the Gaussian
approximation (cut off at RTOL below) and the chain (which wanders, and needs more draws than
the stiff directions) are not expected to agree.
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
    ap.add_argument("--num-halos", type=int, default=2000)
    ap.add_argument("--nsamples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=0.001, help="error on the log residuals")
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(2 * a.num_pops, a.num_halos, seed=3, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))
    fit = model.run_gauss_newton(data["guess"])
    best = torch.as_tensor(fit.x, dtype=torch.float32, device=dev)
    scale = 1.0 / (2.0 * a.sigma ** 2)
    # Gaussian approximation: covariance (loss_scale H)^-1 within the constrained directions
    RTOL = 1e-4
    H = model.calc_hessian_from_params(best).double().cpu()
    ev = torch.linalg.eigvalsh(H)
    kept = int((ev.abs() > RTOL * ev.abs().max()).sum())
    hess = (torch.linalg.pinv(H, rtol=RTOL, hermitian=True).diagonal() / scale).clamp_min(0).sqrt()
    res = model.run_hmc(best, nsamples=a.nsamples, warmup=a.warmup, nleapfrog=4, step_size=1e-3,
                        loss_scale=scale, randkey=0, jitter=0.2)
    post = res.samples.double().std(0).cpu()
    print(f"loss {float(fit.fun):.3e} at the optimum; {kept} of {ev.numel()} Hessian directions "
          f"constrained; HMC: {a.nsamples} draws after {a.warmup} warm-up iterations, accept rate "
          f"{res.accept_rate:.2f}, step {res.step_size:.3g}, {res.n_divergent} divergent, "
          f"{res.nfev} evaluations")
    print("param      fitted  posterior mean   posterior std (HMC)   1-sigma (exact Hessian)")
    for i, (x, m, s, h) in enumerate(zip(best.tolist(), res.mean.tolist(), post.tolist(),
                                         hess.tolist())):
        print(f"{i:5d} {x:11.4f} {m:15.4f} {s:21.3e} {h:25.3e}")
    assert torch.isfinite(res.samples).all() and res.n_divergent == 0
