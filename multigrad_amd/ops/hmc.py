"""HMC vector ops (``csrc/hmc.hip``) with PyTorch fallbacks for CPU tensors.

Vectors are fp32 of ``n`` elements; every energy is an fp64 device scalar (``ke_out``, one
element), so the sampler can fetch it together with the potential in one copy.  On the GPU
each op is one streaming pass on the current stream (plus a one-workgroup reduce when an
energy is asked for) with no host sync; the CPU fallbacks use the same formulas."""
from __future__ import annotations

from typing import Optional

import torch

from ._ext import ext

__all__ = ["hmc_workspace", "hmc_leapfrog_", "hmc_momentum_", "hmc_commit_"]


def hmc_workspace(device) -> Optional[torch.Tensor]:
    """The fp64 slab the energy reductions of ``hmc_leapfrog_`` / ``hmc_momentum_`` need on
    ``device`` (``None`` on the CPU); allocate once per sampler."""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return torch.zeros(ext().hmc_workspace(), dtype=torch.float64, device=device)


def _ws(ke_out, ws, device):
    if ke_out is not None and ws is None:
        return hmc_workspace(device)
    return ws


def hmc_leapfrog_(q: torch.Tensor, p: torch.Tensor, g: torch.Tensor, inv_mass: torch.Tensor,
                  a: float, b: float, ke_out: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> None:
    """``p -= a g``; if ``b != 0``: ``q += b inv_mass p`` with the updated ``p``; if ``ke_out``
    is given: ``ke_out[0] = 1/2 sum p^2 inv_mass`` (products and sum in fp64 from the fp32
    values, fixed order: bitwise reproducible for a fixed ``n`` and device).  ``inv_mass`` has
    ``n`` elements or one (broadcast).  A trajectory of ``L`` steps is ``L + 1`` calls:
    ``(eps/2, eps)``, ``L - 1`` times ``(eps, eps)``, ``(eps/2, 0, ke_out)``."""
    if q.device.type == "cuda":
        ext().hmc_leapfrog(q, p, g, inv_mass, float(a), float(b), ke_out,
                           _ws(ke_out, ws, q.device))
        return
    m = inv_mass.double()
    pd = p.double() - float(a) * g.double()
    p.copy_(pd.to(p.dtype))
    if b != 0:
        q.copy_((q.double() + float(b) * m * p.double()).to(q.dtype))
    if ke_out is not None:
        p2 = p.double() ** 2
        ke_out[0] = 0.5 * ((p2 * m).sum() if m.numel() == p2.numel() else p2.sum() * m.reshape(()))


def hmc_momentum_(z: torch.Tensor, inv_mass: torch.Tensor, p: torch.Tensor,
                  ke_out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> None:
    """``p = z / sqrt(inv_mass)`` and, if ``ke_out`` is given, ``ke_out[0] = 1/2 sum z^2`` in
    fp64: the momentum of standard-normal ``z`` under the diagonal mass ``1 / inv_mass``, and
    its kinetic energy."""
    if z.device.type == "cuda":
        ext().hmc_momentum(z, inv_mass, p, ke_out, _ws(ke_out, ws, z.device))
        return
    torch.div(z, torch.sqrt(inv_mass), out=p)
    if ke_out is not None:
        ke_out[0] = 0.5 * (z.double() ** 2).sum()


def hmc_commit_(q: torch.Tensor, count: int, mean: Optional[torch.Tensor] = None,
                m2: Optional[torch.Tensor] = None, track_idx: Optional[torch.Tensor] = None,
                track_row: Optional[torch.Tensor] = None,
                sample_row: Optional[torch.Tensor] = None) -> None:
    """One pass over the kept position ``q``: the Welford update ``d = q - mean``,
    ``mean += d / count``, ``m2 += d (q - mean)`` (``count`` includes this vector; skipped
    without ``mean``), ``track_row[j] = q[track_idx[j]]`` (int64 indices; an index outside
    ``q`` leaves its entry as it is) and a copy of ``q`` into ``sample_row`` -- each optional."""
    if q.device.type == "cuda":
        ext().hmc_commit(q, int(count), mean, m2, track_idx, track_row, sample_row)
        return
    if mean is not None:
        d = q - mean
        mean.add_(d, alpha=1.0 / float(count))
        m2.addcmul_(d, q - mean)
    if track_idx is not None:
        ok = (track_idx >= 0) & (track_idx < q.numel())  # as the kernel: others keep their value
        track_row[ok] = q[track_idx[ok]]
    if sample_row is not None:
        sample_row.copy_(q)
