"""The population SMF model written in plain PyTorch ops (no custom kernels).

This is what a user of the reference writes: a ``OnePointModel`` whose hooks are ordinary
differentiable array code (the reference's are ``jax.numpy``, tests/smf_example/
smf_grad_descent.py:32-82; here ``torch``).  It computes the same summed statistics as
:class:`~multigrad_amd.models.population.PopulationSMFModel` -- one ``(a, log10 sigma)``
pair per population, log-MSE loss -- through autograd, so it exercises the *generic*
device paths: the eager distributed chain rule (``OnePointModel._vjp``) and the
graph-captured generic engine (:mod:`multigrad_amd.engine.generic`).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops.binned import gaussian_binned_sum
from ..ops.binned2d import gaussian_binned_sum_2d
from ..ops.binned_fine import FineBins
from ..ops.binned_multi import gaussian_binned_sum_multi
from ..ops.groups import GroupIndex
from ..ops.smf import logmse_loss
from .onepoint import OnePointModel

__all__ = ["TorchPopulationSMFModel", "StochasticTorchPopulationSMFModel",
           "BinnedPopulationSMFModel", "GroupedBinnedPopulationSMFModel",
           "JointBinnedPopulationSMFModel", "ConditionalBinnedPopulationSMFModel",
           "SampleBinnedPopulationSMFModel", "FineBinnedPopulationSMFModel",
           "torch_population_data", "joint_population_data", "conditional_population_data",
           "sample_population_data", "fine_population_data"]


def torch_population_data(data: dict) -> dict:
    """Plain-tensor aux data (halo masses, population ids, bins) from
    :func:`~multigrad_amd.models.population.make_population_data` output, with the
    target SMF filled in (``PopulationSMFModel.set_target_from_truth`` first)."""
    sh = data["shard"]
    bins = data["bins"]
    dev = sh.x.device
    return dict(x=sh.x.float(), pop=sh.pop.long(),
                edges=torch.tensor(bins.edges, dtype=torch.float32, device=dev),
                scale=torch.tensor(bins.scale, dtype=torch.float32, device=dev),
                target=data["target_sumstats"].float().to(dev), eps=float(data["loss_eps"]),
                npop=int(data["npop"]))


@dataclass(eq=False)
class TorchPopulationSMFModel(OnePointModel):
    """``aux_data`` from :func:`torch_population_data`; parameters interleaved
    ``(a_c, log10 sigma_c)``."""

    aux_data: dict = None

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        return self._sumstats(params, self.aux_data["x"])

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a = th[:, 0][d["pop"]]
        sigma = torch.pow(10.0, th[:, 1])[d["pop"]]
        z = (d["edges"][None, :] - (x + a)[:, None]) / sigma[:, None]
        cdf = torch.special.ndtr(z)
        return (cdf[:, 1:] - cdf[:, :-1]).sum(0) * d["scale"]

    def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
        d = self.aux_data
        return logmse_loss(sumstats, d["target"].to(sumstats.dtype), d["eps"])


@dataclass(eq=False)
class StochasticTorchPopulationSMFModel(TorchPopulationSMFModel):
    """The same model with per-evaluation Monte-Carlo scatter: every halo's log mass is
    perturbed by ``scatter * N(0, 1)`` drawn from ``randkey.generator(device)`` -- a
    stochastic forward model, fitted with a fresh key per Adam step (reference
    multigrad/adam.py:59-62) or a constant one (``const_randkey``)."""

    scatter: float = 0.02

    def calc_partial_sumstats_from_params(self, params, randkey=None):
        x = self.aux_data["x"]
        if randkey is not None:
            x = x + self.scatter * torch.randn(x.shape, generator=randkey.generator(x.device),
                                               device=x.device, dtype=x.dtype)
        return self._sumstats(params, x)


@dataclass(eq=False)
class BinnedPopulationSMFModel(TorchPopulationSMFModel):
    """The same model and loss with the binning done by
    :func:`~multigrad_amd.ops.binned.gaussian_binned_sum`: what a user writes -- the gather
    and the parameter transforms in torch, the Gaussian-smeared histogram in the fused op.
    The bin edges are kept as a host tuple at construction (the op takes host edges, so a
    captured step never reads them back from the device)."""

    def __post_init__(self):
        super().__post_init__()
        self.edges = tuple(float(e) for e in self.aux_data["edges"].tolist())

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a = th[:, 0][d["pop"]]
        sigma = torch.pow(10.0, th[:, 1])[d["pop"]]
        return gaussian_binned_sum(x + a, sigma, self.edges, None) * d["scale"]


@dataclass(eq=False)
class GroupedBinnedPopulationSMFModel(BinnedPopulationSMFModel):
    """:class:`BinnedPopulationSMFModel` with the two gathers done by a
    :class:`~multigrad_amd.ops.groups.GroupIndex` built once from the population ids: the
    backward of ``a[pop]`` and ``sigma[pop]`` is then one fixed-order segmented sum of both
    gradient columns instead of a sort and an atomic scatter per step."""

    def __post_init__(self):
        super().__post_init__()
        self.groups = GroupIndex(self.aux_data["pop"], self.aux_data["npop"])

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a, sigma = self.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
        return gaussian_binned_sum(x + a, sigma, self.edges, None) * d["scale"]


@dataclass(eq=False)
class JointBinnedPopulationSMFModel(GroupedBinnedPopulationSMFModel):
    """A joint statistic on :func:`~multigrad_amd.ops.binned2d.gaussian_binned_sum_2d`: counts
    in (log stellar mass x a second observable ``y``), both axes smeared by the population's
    parameters -- ``mu_x = x + a``, ``sigma_x = sigma``, ``mu_y = y + y_slope * a``,
    ``sigma_y = y_width * sigma`` -- so all four per-object gradients flow.  ``aux_data`` from
    :func:`joint_population_data`: the per-halo ``y``, the host ``edges_y`` and ``scale`` /
    ``target`` of ``nbx * nby`` flattened cells.  With the default ``y_width`` the y smearing
    stays well inside a y bin, so widening a population never spills more out of the grid
    in y than it gains in x and every population's sigma gradient keeps one sign (at 1.5 a
    few change sign, and gradient elements that are near-cancellations cannot be compared
    between float32 implementations)."""

    y_slope: float = 0.5
    y_width: float = 0.5

    def __post_init__(self):
        super().__post_init__()
        self.edges_y = tuple(float(e) for e in self.aux_data["edges_y"])

    def _cells(self, mu_x, sigma_x, mu_y, sigma_y):
        return gaussian_binned_sum_2d(mu_x, sigma_x, mu_y, sigma_y, self.edges, self.edges_y)

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a, sigma = self.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
        cells = self._cells(x + a, sigma, d["y"] + self.y_slope * a, self.y_width * sigma)
        return cells.reshape(-1) * d["scale"]


def joint_population_data(data: dict, nby: int = 4, y_range=(-12.0, -10.0), seed: int = 0,
                          **model_kwargs) -> dict:
    """``aux_data`` of :class:`JointBinnedPopulationSMFModel` from
    :func:`~multigrad_amd.models.population.make_population_data` output: the second
    coordinate ``y`` is drawn independently of ``x`` so that ``mu_y`` at the mean true offset
    is uniform across ``nby`` equal bins of ``y_range`` (a small ``nby`` keeps every cell
    populated), the per-bin scale is repeated
    over the y bins, and the target is the model's own sumstats at ``data["truth"]``."""
    sh = data["shard"]
    bins = data["bins"]
    dev = sh.x.device
    n = sh.x.numel()
    gen = torch.Generator().manual_seed(1000 + seed)
    slope = float(model_kwargs.get("y_slope", JointBinnedPopulationSMFModel.y_slope))
    shift = slope * float(data["truth"].reshape(-1, 2)[:, 0].float().mean())
    y = (y_range[0] - shift + (y_range[1] - y_range[0]) * torch.rand(n, generator=gen)).to(dev)
    edges_y = tuple(float(y_range[0] + (y_range[1] - y_range[0]) * k / nby) for k in range(nby + 1))
    scale = torch.tensor(bins.scale, dtype=torch.float32, device=dev).repeat_interleave(nby)
    aux = dict(x=sh.x.float(), pop=sh.pop.long(), y=y,
               edges=torch.tensor(bins.edges, dtype=torch.float32, device=dev), edges_y=edges_y,
               scale=scale, target=torch.ones_like(scale), eps=float(data["loss_eps"]),
               npop=int(data["npop"]))
    model = JointBinnedPopulationSMFModel(aux_data=aux, **model_kwargs)
    with torch.no_grad():
        aux["target"] = model.calc_sumstats_from_params(
            data["truth"].to(dev, torch.float32)).float()
    return aux


@dataclass(eq=False)
class ConditionalBinnedPopulationSMFModel(GroupedBinnedPopulationSMFModel):
    """Three statistics over the same stellar-mass bins on
    :func:`~multigrad_amd.ops.binned_multi.gaussian_binned_sum_multi`, ``3 * nb`` sumstats:
    the counts (weight ``None``), a quenched-weighted count with
    ``q_i = sigmoid(q_slope * (x_i + a_i - q_mass))`` -- a weight that depends on the
    parameters, so its gradient flows through the op's weight gradient -- and the sum of a
    fixed per-halo observable ``y_i`` in ``[0.5, 1.5]`` (a weight that needs no gradient).
    ``aux_data`` from :func:`conditional_population_data`: the per-halo ``y`` and ``scale`` /
    ``target`` of ``3 * nb`` entries (the per-bin scale repeated per statistic).  All three
    weights are positive, so every sumstat is positive and the log-MSE loss applies."""

    q_slope: float = 2.0
    q_mass: float = 10.0

    def _sums(self, mu, sigma, weights):
        return gaussian_binned_sum_multi(mu, sigma, self.edges, weights)

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a, sigma = self.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
        mu = x + a
        q = torch.sigmoid(self.q_slope * (mu - self.q_mass))
        return self._sums(mu, sigma, (None, q, d["y"])).reshape(-1) * d["scale"]


def conditional_population_data(data: dict, seed: int = 0, **model_kwargs) -> dict:
    """``aux_data`` of :class:`ConditionalBinnedPopulationSMFModel` from
    :func:`~multigrad_amd.models.population.make_population_data` output: the per-halo
    observable ``y`` is uniform in ``[0.5, 1.5]``, the per-bin scale is repeated for the three
    statistics, and the target is the model's own sumstats at ``data["truth"]``."""
    sh = data["shard"]
    bins = data["bins"]
    dev = sh.x.device
    gen = torch.Generator().manual_seed(2000 + seed)
    y = (0.5 + torch.rand(sh.x.numel(), generator=gen)).to(dev)
    scale = torch.tensor(bins.scale, dtype=torch.float32, device=dev).repeat(3)
    aux = dict(x=sh.x.float(), pop=sh.pop.long(), y=y,
               edges=torch.tensor(bins.edges, dtype=torch.float32, device=dev),
               scale=scale, target=torch.ones_like(scale), eps=float(data["loss_eps"]),
               npop=int(data["npop"]))
    model = ConditionalBinnedPopulationSMFModel(aux_data=aux, **model_kwargs)
    with torch.no_grad():
        aux["target"] = model.calc_sumstats_from_params(
            data["truth"].to(dev, torch.float32)).float()
    return aux


@dataclass(eq=False)
class SampleBinnedPopulationSMFModel(GroupedBinnedPopulationSMFModel):
    """The stellar-mass function once per sample (a redshift slice, a survey field) on
    :func:`~multigrad_amd.ops.binned_group.gaussian_binned_sum_by_group`: every halo carries a
    sample id next to its population id, and the sumstats are the ``nsamples * nb`` per-sample
    SMFs, sample-major.  ``aux_data`` from :func:`sample_population_data`: the per-halo
    ``sample`` ids, ``nsamples`` and ``scale`` / ``target`` of ``nsamples * nb`` entries (the
    per-bin scale repeated per sample).  A second ``GroupIndex`` over the sample ids is built
    once; they are unsorted, so that plan carries a permutation."""

    def __post_init__(self):
        super().__post_init__()
        self.samples = GroupIndex(self.aux_data["sample"], self.aux_data["nsamples"])

    def _sums(self, mu, sigma):
        return self.samples.binned_sum(mu, sigma, self.edges)

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a, sigma = self.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
        return self._sums(x + a, sigma).reshape(-1) * d["scale"]


def sample_population_data(data: dict, nsamples: int = 3, seed: int = 0) -> dict:
    """``aux_data`` of :class:`SampleBinnedPopulationSMFModel` from
    :func:`~multigrad_amd.models.population.make_population_data` output: every halo gets a
    seeded, unsorted sample id in ``[0, nsamples)``, the per-bin scale is repeated per sample,
    and the target is the model's own sumstats at ``data["truth"]``."""
    sh = data["shard"]
    bins = data["bins"]
    dev = sh.x.device
    gen = torch.Generator().manual_seed(3000 + seed)
    sample = torch.randint(0, int(nsamples), (sh.x.numel(),), generator=gen).to(dev)
    scale = torch.tensor(bins.scale, dtype=torch.float32, device=dev).repeat(int(nsamples))
    aux = dict(x=sh.x.float(), pop=sh.pop.long(), sample=sample, nsamples=int(nsamples),
               edges=torch.tensor(bins.edges, dtype=torch.float32, device=dev),
               scale=scale, target=torch.ones_like(scale), eps=float(data["loss_eps"]),
               npop=int(data["npop"]))
    model = SampleBinnedPopulationSMFModel(aux_data=aux)
    with torch.no_grad():
        aux["target"] = model.calc_sumstats_from_params(
            data["truth"].to(dev, torch.float32)).float()
    return aux


@dataclass(eq=False)
class FineBinnedPopulationSMFModel(GroupedBinnedPopulationSMFModel):
    """The stellar-mass function in many fine bins on
    :func:`~multigrad_amd.ops.binned_fine.gaussian_binned_sum_fine`: the same model with every
    coarse bin split into equal parts, as one fits a finely binned SMF that is merged later
    under several binnings.  ``aux_data`` from :func:`fine_population_data`: ``edges``,
    ``scale`` and ``target`` of the fine bins (up to 4096).  The :class:`FineBins` plan is built
    once from the host edges; a captured step never reads them back.  This model's widths
    (0.1-0.3 dex over a range of 1 dex) make every halo reach every bin, the regime in which
    calls of ``gaussian_binned_sum`` on 33-edge slices are faster (profiles/binned_fine): it is
    here to exercise the op under the engines, not as its best case."""

    def __post_init__(self):
        super().__post_init__()
        self.bins = FineBins(self.edges, device=self.aux_data["x"].device)

    def _sums(self, mu, sigma):
        return self.bins.sum(mu, sigma)

    def _sumstats(self, params, x):
        d = self.aux_data
        th = params.reshape(-1, 2)
        a, sigma = self.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
        return self._sums(x + a, sigma) * d["scale"]


def fine_population_data(data: dict, refine: int = 8) -> dict:
    """``aux_data`` of :class:`FineBinnedPopulationSMFModel` from
    :func:`~multigrad_amd.models.population.make_population_data` output: every coarse bin is
    split into ``refine`` equal bins (every ``refine``-th fine edge is the coarse edge itself,
    so sums of ``refine`` consecutive fine bins are the coarse bins), the per-bin scale
    ``1 / (volume * width)`` follows the fine widths, and the target is the model's own
    sumstats at ``data["truth"]``."""
    sh = data["shard"]
    bins = data["bins"]
    dev = sh.x.device
    refine = int(refine)
    if refine < 1:
        raise ValueError("fine_population_data: refine must be at least 1")
    coarse = torch.tensor(bins.edges, dtype=torch.float64)
    frac = torch.arange(refine, dtype=torch.float64) / refine
    inner = coarse[:-1, None] + (coarse[1:] - coarse[:-1])[:, None] * frac[None, :]
    edges = torch.cat([inner.reshape(-1), coarse[-1:]]).float()
    scale = (torch.tensor(bins.scale, dtype=torch.float64) * refine).float()
    scale = scale.repeat_interleave(refine).to(dev)
    aux = dict(x=sh.x.float(), pop=sh.pop.long(), edges=edges.to(dev), scale=scale,
               target=torch.ones_like(scale), eps=float(data["loss_eps"]),
               npop=int(data["npop"]), refine=refine)
    model = FineBinnedPopulationSMFModel(aux_data=aux)
    with torch.no_grad():
        aux["target"] = model.calc_sumstats_from_params(
            data["truth"].to(dev, torch.float32)).float()
    return aux
