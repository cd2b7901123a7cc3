"""A user-written fit of a finely binned stellar-mass function on the fine binning op: the mass
is p0 + p1 (x - 12) with scatter exp(p2) -- plain torch -- and the Gaussian-smeared histogram
has 160 bins of 0.0125 dex, sixteen per coarse bin, so that it can be merged later under any
binning.  A ``FineBins`` plan is built once from the host edges; ``bins.sum`` then visits, for
every halo, only the bins within 5.5 sigma of its mass (HIP kernels on a GPU, torch ops on the
CPU).  The fitted fine sumstats, merged back to the ten coarse bins, are printed beside those of
the same model on ``gaussian_binned_sum`` with the coarse edges.

    python examples/user_model_fine.py [--num-halos N] [--num-steps K]
"""
import argparse
import os
import sys
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multigrad_amd as mg  # noqa: E402
from multigrad_amd.ops import FineBins, gaussian_binned_sum  # noqa: E402

REFINE = 16
COARSE = tuple(9.5 + 0.2 * k for k in range(11))   # host edges: set once, never read back
FINE = tuple(COARSE[k // REFINE] + (COARSE[k // REFINE + 1] - COARSE[k // REFINE]) *
             (k % REFINE) / REFINE for k in range(10 * REFINE)) + (COARSE[-1],)


@dataclass(eq=False)
class MyModel(mg.OnePointModel):
    aux_data: dict = None

    def __post_init__(self):
        super().__post_init__()
        self.bins = FineBins(FINE, device=self.aux_data["x"].device)   # once, at setup

    def mass_and_scatter(self, params):
        x = self.aux_data["x"]
        return params[0] + params[1] * (x - 12.0), torch.exp(params[2]).reshape(1)

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        mass, sigma = self.mass_and_scatter(params)               # one width for all: broadcast
        return self.bins.sum(mass, sigma) / self.aux_data["x"].numel()

    def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
        return torch.mean((torch.log10(sumstats + 1e-6) - self.aux_data["target"]) ** 2)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-halos", type=int, default=20_000)
    ap.add_argument("--num-steps", type=int, default=300)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    gen = torch.Generator().manual_seed(1)
    x = 11.0 + 2.5 * torch.rand(a.num_halos, generator=gen)
    model = MyModel(aux_data=dict(x=x.to(dev)))
    truth = torch.tensor([10.5, 0.8, -2.5], device=dev)          # scatter 0.08 dex: 6.5 fine bins
    model.aux_data["target"] = torch.log10(model.calc_partial_sumstats_from_params(truth) + 1e-6)
    guess = truth + torch.tensor([0.1, -0.05, 0.3], device=dev)
    traj = model.run_adam(guess, nsteps=a.num_steps, learning_rate=0.02)
    first, last = (float(model.calc_loss_from_params(p)) for p in (traj[0], traj[-1]))
    print("truth ", truth.tolist())
    print("fitted", [round(v, 4) for v in traj[-1].tolist()], f"loss {first:.3e} -> {last:.3e}")
    fine = model.calc_partial_sumstats_from_params(traj[-1])
    merged = fine.reshape(-1, REFINE).sum(1)
    mass, sigma = model.mass_and_scatter(traj[-1])
    coarse = gaussian_binned_sum(mass, sigma, COARSE) / a.num_halos
    print(f"{model.bins}: {fine.numel()} fine sumstats")
    print("merged to the coarse bins", [round(v, 5) for v in merged.tolist()])
    print("the coarse model         ", [round(v, 5) for v in coarse.tolist()])
    assert float((merged - coarse).abs().max()) < 1e-5, "merged fine bins differ from the coarse op"
    assert last < 0.05 * first, "the fit did not reduce the loss"
