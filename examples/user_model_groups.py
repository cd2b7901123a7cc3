"""A user-written hierarchical model on the group ops: every group (a sample, a population)
has its own offset, all share one width.  The offsets are broadcast to the objects by
``GroupIndex.gather`` -- its backward is a fixed-order segmented sum, not a sort and an atomic
scatter per step -- and the histogram is ``gaussian_binned_sum`` (HIP kernels on a GPU, torch
ops on the CPU).

    python examples/user_model_groups.py [--num-groups G] [--num-objects N] [--num-steps K]
"""
import argparse
import os
import sys
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multigrad_amd as mg  # noqa: E402
from multigrad_amd.ops import GroupIndex, gaussian_binned_sum  # noqa: E402

EDGES = tuple(9.0 + 0.25 * k for k in range(11))  # host edges: set once, never read back


@dataclass(eq=False)
class MyModel(mg.OnePointModel):
    """Parameters: one offset per group, then the log of the shared width."""

    aux_data: dict = None

    def __post_init__(self):
        super().__post_init__()
        d = self.aux_data
        self.groups = GroupIndex(d["group"], d["num_groups"])   # once: range check and sort
        self.per_group = self.groups.counts.to(d["x"].dtype)

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        d = self.aux_data
        offset, = self.groups.gather(params[:-1])               # [G] -> [N]
        sigma = torch.exp(params[-1]).reshape(1)                 # one width for all: broadcast
        hist = gaussian_binned_sum(d["x"] + offset, sigma, EDGES) / d["x"].numel()
        # the mean shifted mass of every group, by the transpose op
        tot, = self.groups.segment_sum(d["x"] + offset)
        return torch.cat([hist, 0.01 * tot / self.per_group])

    def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
        return torch.mean((sumstats - self.aux_data["target"]) ** 2)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-groups", type=int, default=50)
    ap.add_argument("--num-objects", type=int, default=20_000)
    ap.add_argument("--num-steps", type=int, default=300)
    a = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    gen = torch.Generator().manual_seed(1)
    x = 9.5 + 1.5 * torch.rand(a.num_objects, generator=gen)
    group = torch.arange(a.num_objects) % a.num_groups          # every group has objects
    model = MyModel(aux_data=dict(x=x.to(dev), group=group.to(dev), num_groups=a.num_groups))
    truth = torch.cat([0.3 * torch.randn(a.num_groups, generator=gen),
                       torch.tensor([-1.2])]).to(dev)
    model.aux_data["target"] = model.calc_partial_sumstats_from_params(truth)
    guess = torch.cat([torch.zeros(a.num_groups), torch.tensor([-0.8])]).to(dev)
    traj = model.run_adam(guess, nsteps=a.num_steps, learning_rate=0.02)
    first, last = (float(model.calc_loss_from_params(p)) for p in (traj[0], traj[-1]))
    err = float((traj[-1][:-1] - truth[:-1]).abs().max())
    print(f"{a.num_groups} groups, {a.num_objects} objects ({model.groups}); "
          f"loss {first:.3e} -> {last:.3e}, largest offset error {err:.3f}")
    assert last < 0.05 * first, "the fit did not reduce the loss"
