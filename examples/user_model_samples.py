"""A user-written fit of one stellar-mass function per sample (three survey fields here) on the
per-group binning op: the mass is p0 + p1 (x - 12) with scatter exp(p2) -- plain torch -- and
every halo belongs to one field.  A ``GroupIndex`` over the field ids is built once; the three
Gaussian-smeared histograms then come from one ``plan.binned_sum`` call (HIP kernels on a GPU,
torch ops on the CPU) instead of one masked call per field.

    python examples/user_model_samples.py [--num-halos N] [--num-steps K]
"""
import argparse
import os
import sys
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multigrad_amd as mg  # noqa: E402
from multigrad_amd.ops import GroupIndex  # noqa: E402

EDGES = tuple(9.0 + 0.25 * k for k in range(11))   # host edges: set once, never read back
NFIELDS = 3


@dataclass(eq=False)
class MyModel(mg.OnePointModel):
    aux_data: dict = None

    def __post_init__(self):
        super().__post_init__()
        self.fields = GroupIndex(self.aux_data["field"], NFIELDS)   # the sort happens here, once

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        x = self.aux_data["x"]
        mass = params[0] + params[1] * (x - 12.0)
        sigma = torch.exp(params[2]).reshape(1)               # one width for all: broadcast
        smf = self.fields.binned_sum(mass, sigma, EDGES)      # [NFIELDS, nb]
        return (smf / self.aux_data["count"][:, None]).reshape(-1)

    def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
        return torch.mean((torch.log10(sumstats + 1e-6) - self.aux_data["target"]) ** 2)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-halos", type=int, default=20_000)
    ap.add_argument("--num-steps", type=int, default=300)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    gen = torch.Generator().manual_seed(1)
    field = torch.randint(0, NFIELDS, (a.num_halos,), generator=gen)
    # the fields differ in depth: field f holds halos above 11 + 0.3 f
    x = 11.0 + 0.3 * field + (2.5 - 0.3 * field) * torch.rand(a.num_halos, generator=gen)
    count = torch.bincount(field, minlength=NFIELDS).float()
    model = MyModel(aux_data=dict(x=x.to(dev), field=field.to(dev), count=count.to(dev)))
    truth = torch.tensor([10.5, 0.8, -1.2], device=dev)
    model.aux_data["target"] = torch.log10(model.calc_partial_sumstats_from_params(truth) + 1e-6)
    guess = truth + torch.tensor([0.3, -0.1, 0.2], device=dev)
    traj = model.run_adam(guess, nsteps=a.num_steps, learning_rate=0.02)
    first, last = (float(model.calc_loss_from_params(p)) for p in (traj[0], traj[-1]))
    print("truth ", truth.tolist())
    print("fitted", [round(v, 4) for v in traj[-1].tolist()], f"loss {first:.3e} -> {last:.3e}")
    smf = model.calc_partial_sumstats_from_params(traj[-1]).reshape(NFIELDS, -1)
    for f in range(NFIELDS):
        print(f"field {f} SMF", [round(v, 4) for v in smf[f].tolist()])
    assert last < 0.05 * first, "the fit did not reduce the loss"
