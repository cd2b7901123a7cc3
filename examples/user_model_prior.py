"""A Gaussian prior on the parameters: a MAP fit, then posterior samples with the same prior.

    python examples/user_model_prior.py [--num-pops J] [--num-halos N] [--nsamples S]

The grouped binned population model of ``examples/user_model_posterior.py`` observes only the
sum over the populations, so some directions of its parameter space are nearly unconstrained:
with a flat prior the posterior is improper there and the chain wanders.  ``GaussianPrior``
puts a width on every parameter (``None`` in the list leaves one flat).  Reading the loss as a
chi-square with errors ``sigma`` on the log residuals, the posterior is
``exp(-(loss_scale * loss + penalty))`` with ``loss_scale = 1 / (2 sigma^2)`` -- the prior is a
density and is not scaled -- and its maximum is what
``run_bfgs(prior=..., prior_weight=1 / loss_scale)`` finds.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from multigrad_amd import GaussianPrior  # noqa: E402
from multigrad_amd.models.population import PopulationSMFModel, make_population_data  # noqa: E402
from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,  # noqa: E402
                                                   torch_population_data)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-pops", type=int, default=4)
    ap.add_argument("--num-halos", type=int, default=2000)
    ap.add_argument("--nsamples", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--sigma", type=float, default=0.01, help="error on the log residuals")
    ap.add_argument("--width", type=float, default=0.05, help="prior width of every parameter")
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_population_data(2 * a.num_pops, a.num_halos, seed=3, device=dev)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    model = GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data))
    guess = data["guess"]
    scale = 1.0 / (2.0 * a.sigma ** 2)
    # centred on the guess; the last parameter stays flat
    widths = [a.width] * (guess.numel() - 1) + [None]
    prior = GaussianPrior(guess.double().cpu().numpy(), widths)
    flat = model.run_bfgs(guess, method="device", maxsteps=200)
    fit = model.run_bfgs(guess, method="device", maxsteps=200, prior=prior,
                         prior_weight=1.0 / scale)
    print(f"MAP: objective {fit.fun:.3e} = loss {fit.fun - fit.prior_penalty / scale:.3e} + "
          f"penalty {fit.prior_penalty:.3e} / loss_scale, {fit.nit} iterations; "
          f"the fit without a prior ends at loss {flat.fun:.3e}")
    res = model.run_hmc(fit.x, nsamples=a.nsamples, warmup=a.warmup, nleapfrog=4, step_size=1e-3,
                        loss_scale=scale, randkey=0, jitter=0.2, prior=prior)
    post = res.samples.double().std(0).cpu()
    print(f"posterior: {a.nsamples} draws after {a.warmup} warm-up iterations, accept rate "
          f"{res.accept_rate:.2f}, step {res.step_size:.3g}, {res.n_divergent} divergent")
    print("param  prior mean  prior width   flat fit        MAP  posterior mean  posterior std")
    for i, (m, x0, x, pm, s) in enumerate(zip(guess.tolist(), flat.x.tolist(), fit.x.tolist(),
                                              res.mean.tolist(), post.tolist())):
        w = "flat" if widths[i] is None else f"{widths[i]:.3g}"
        print(f"{i:5d} {m:11.4f} {w:>12} {x0:10.4f} {x:10.4f} {pm:15.4f} {s:14.3e}")
    assert torch.isfinite(res.samples).all() and res.n_divergent == 0
    assert fit.prior_penalty >= 0 and res.potential.min() >= 0
