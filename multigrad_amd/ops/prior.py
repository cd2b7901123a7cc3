"""Gaussian-prior vector ops (``csrc/prior.hip``) with PyTorch fallbacks for CPU tensors.

The penalty is ``pen(x) = 1/2 sum w (x - m)^2`` with a mean ``m`` and an inverse variance
``w`` of ``n`` elements or of one element each (broadcast; where only one of the two has one
element it is expanded here).  Vectors are fp32, every energy is an fp64 device scalar, as
in :mod:`multigrad_amd.ops.hmc`.  On the GPU each op is one streaming pass on the current
stream (plus a one-workgroup reduce when an energy is asked for) with no host sync; the CPU
fallbacks use the same formulas in float64."""
from __future__ import annotations

from typing import Optional

import torch

from ._ext import ext

__all__ = ["prior_workspace", "gaussian_prior_grad_", "hmc_leapfrog_prior_"]


def prior_workspace(device) -> Optional[torch.Tensor]:
    """The fp64 slab the energy reductions of this module need on ``device`` (``None`` on the
    CPU): two energies, twice :func:`~multigrad_amd.ops.hmc.hmc_workspace`; allocate once."""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return torch.zeros(ext().prior_workspace(), dtype=torch.float64, device=device)


def _pair(mean: torch.Tensor, inv_var: torch.Tensor, n: int):
    """Both of ``n`` elements or both of one."""
    if mean.numel() != inv_var.numel():
        if mean.numel() == 1:
            mean = mean.expand(n).contiguous()
        elif inv_var.numel() == 1:
            inv_var = inv_var.expand(n).contiguous()
    return mean, inv_var


def _penalty64(x: torch.Tensor, mean: torch.Tensor, inv_var: torch.Tensor) -> torch.Tensor:
    d = x.double() - mean.double()
    return 0.5 * (d * d * inv_var.double()).sum()


def gaussian_prior_grad_(x: torch.Tensor, g: torch.Tensor, mean: torch.Tensor,
                         inv_var: torch.Tensor, c: float, out: torch.Tensor,
                         pen_out: Optional[torch.Tensor] = None,
                         ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out = g + c w (x - m)``: per element ``d = x - m`` in fp32, then
    ``out = fmaf(c w, d, g)``; ``out`` may be ``g`` itself.  If ``pen_out`` is given,
    ``pen_out[0] = 1/2 sum w (x - m)^2`` -- the unweighted penalty, products and sum in fp64
    from the fp32 values in a fixed order (bitwise reproducible for a fixed ``n`` and device).
    ``ws`` is :func:`prior_workspace` (allocated per call when missing).  Returns ``out``."""
    mean, inv_var = _pair(mean, inv_var, x.numel())
    if x.device.type == "cuda":
        if pen_out is not None and ws is None:
            ws = prior_workspace(x.device)
        ext().gaussian_prior_grad(x, g, mean, inv_var, float(c), out, pen_out, ws)
        return out
    if out.numel() != x.numel() or g.numel() != x.numel() or \
            mean.numel() not in (1, x.numel()):
        raise RuntimeError("gaussian_prior_grad_: x, g, out of n elements; mean, inv_var of n or 1")
    c32 = float(torch.tensor(float(c), dtype=torch.float32))
    d = (x - mean).double()
    val = g.double() + (c32 * inv_var.double()) * d
    if pen_out is not None:
        pen_out[0] = _penalty64(x, mean, inv_var)
    out.copy_(val.to(out.dtype))
    return out


def hmc_leapfrog_prior_(q: torch.Tensor, p: torch.Tensor, g: torch.Tensor,
                        inv_mass: torch.Tensor, a: float, b: float, mean: torch.Tensor,
                        inv_var: torch.Tensor, ap: float, ke_out: Optional[torch.Tensor] = None,
                        pen_out: Optional[torch.Tensor] = None,
                        ws: Optional[torch.Tensor] = None) -> None:
    """:func:`~multigrad_amd.ops.hmc.hmc_leapfrog_` with the prior's force taken from the
    position it reads: per element ``s = fmaf(-a, g, p)``, ``p' = fmaf(-(ap w), q - m, s)``
    with the input ``q``; if ``b != 0``: ``q' = fmaf(b inv_mass, p', q)``.  ``ke_out`` as in
    ``hmc_leapfrog_``; ``pen_out[0] = 1/2 sum w (q_in - m)^2`` in fp64 -- the call that ends
    a trajectory has ``b = 0``, so there it is the penalty at the final position.  Both
    energies come from the one pass.  A trajectory of ``L`` steps of size ``e`` is ``L + 1``
    calls: ``(a, b, ap) = (e/2 s, e, e/2)``, ``L - 1`` times ``(e s, e, e)``, and
    ``(e/2 s, 0, e/2, ke_out, pen_out)`` with ``s`` the loss scale (``g`` stays the gradient
    of the loss)."""
    mean, inv_var = _pair(mean, inv_var, q.numel())
    if q.device.type == "cuda":
        if (ke_out is not None or pen_out is not None) and ws is None:
            ws = prior_workspace(q.device)
        ext().hmc_leapfrog_prior(q, p, g, inv_mass, float(a), float(b), mean, inv_var, float(ap),
                                 ke_out, pen_out, ws)
        return
    m = inv_mass.double()
    if pen_out is not None:
        pen_out[0] = _penalty64(q, mean, inv_var)
    d = (q - mean).double()
    pd = (p.double() - float(a) * g.double()) - (float(ap) * inv_var.double()) * d
    p.copy_(pd.to(p.dtype))
    if b != 0:
        q.copy_((q.double() + float(b) * m * p.double()).to(q.dtype))
    if ke_out is not None:
        p2 = p.double() ** 2
        ke_out[0] = 0.5 * ((p2 * m).sum() if m.numel() == p2.numel() else p2.sum() * m.reshape(()))
