"""A user-written multi-statistic fit on the multi-channel binning op: in the same stellar-mass
bins, the counts, a quenched-weighted count and the summed star-formation rate.  The mass is
p0 + p1 (x - 12) with scatter exp(p2), the quenched probability is sigmoid(3 (mass - p3)) and
the star-formation rate a fixed per-halo observable -- all plain torch -- and the three
Gaussian-smeared histograms come from one ``gaussian_binned_sum_multi`` call (HIP kernels on
a GPU, torch ops on the CPU): the edge CDFs are evaluated once for the three statistics.

    python examples/user_model_conditional.py [--num-halos N] [--num-steps K]
"""
import argparse
import os
import sys
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multigrad_amd as mg  # noqa: E402
from multigrad_amd.ops import gaussian_binned_sum_multi  # noqa: E402

EDGES = tuple(9.0 + 0.25 * k for k in range(11))   # host edges: set once, never read back


@dataclass(eq=False)
class MyModel(mg.OnePointModel):
    aux_data: dict = None

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        x, sfr = self.aux_data["x"], self.aux_data["sfr"]
        mass = params[0] + params[1] * (x - 12.0)
        sigma = torch.exp(params[2]).reshape(1)               # one width for all: broadcast
        quenched = torch.sigmoid(3.0 * (mass - params[3]))    # a weight with a gradient
        sums = gaussian_binned_sum_multi(mass, sigma, EDGES, [None, quenched, sfr])
        return sums.reshape(-1) / x.numel()

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
    sfr = 0.5 + torch.rand(a.num_halos, generator=gen)
    model = MyModel(aux_data=dict(x=x.to(dev), sfr=sfr.to(dev)))
    truth = torch.tensor([10.5, 0.8, -1.2, 10.3], device=dev)
    model.aux_data["target"] = torch.log10(model.calc_partial_sumstats_from_params(truth) + 1e-6)
    guess = truth + torch.tensor([0.3, -0.1, 0.2, 0.2], device=dev)
    traj = model.run_adam(guess, nsteps=a.num_steps, learning_rate=0.02)
    first, last = (float(model.calc_loss_from_params(p)) for p in (traj[0], traj[-1]))
    print("truth ", truth.tolist())
    print("fitted", [round(v, 4) for v in traj[-1].tolist()], f"loss {first:.3e} -> {last:.3e}")
    assert last < 0.05 * first, "the fit did not reduce the loss"
