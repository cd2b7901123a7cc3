"""Float64 oracle of the bound transforms of ``optim/transforms.py`` / ``csrc/adam.h``,
shared by the CPU tests (``test_optim.py``) and the kernel tests (``test_adam_gpu.py``).

The one-sided forms are written so that nothing cancels: with ``t = sqrt(u^2+4) + |u|`` the
distance to the bound is ``h = t/2`` on the side away from the bound and ``h = 2/t`` on the
side towards it, and ``dp/du = h / sqrt(u^2+4)``.  (The textbook ``(u + sqrt(u^2+4))/2`` is
itself wrong by 6e-5 relative at ``u = -1e6`` in float64.)
"""
import math

import torch

E = 2.0 ** -24  # float32 unit roundoff
NONE, BOTH, LOW, HIGH = 0, 1, 2, 3


def dist64(u, kind):
    """Distance ``|p - bound|`` of a one-sided coordinate (``kind`` LOW or HIGH, scalar or
    tensor) at ``u``, and ``dp/du``, in float64."""
    u = u.double()
    r = torch.sqrt(u * u + 4.0)
    t = r + u.abs()
    towards = torch.where(torch.as_tensor(kind, device=u.device) == LOW, u < 0, u > 0)
    h = torch.where(towards, 2.0 / t, t / 2.0)
    return h, h / r


def inverse64(u, lo, hi, kind):
    """``p = T^-1(u)`` and ``dp/du`` in float64 for per-element ``lo``/``hi`` (``+-inf``
    where absent) and ``kind``."""
    u, lo, hi = u.double(), lo.double(), hi.double()
    h, d1 = dist64(u, kind)
    both = kind == BOTH
    s = torch.where(both, (hi - lo) / math.pi, torch.ones_like(u))
    mid = torch.where(both, (hi + lo) / 2.0, torch.zeros_like(u))
    r = u / s
    p = torch.where(both, mid + s * torch.atan(r), u)
    p = torch.where(kind == LOW, lo + h, p)
    p = torch.where(kind == HIGH, hi - h, p)
    d = torch.where(both, 1.0 / (1.0 + r * r), torch.ones_like(u))
    d = torch.where((kind == LOW) | (kind == HIGH), d1, d)
    return p, d


def ulp32(x):
    """Spacing of float32 at ``|x|`` (a float32 tensor)."""
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, math.inf)) - x).double()


def log_u(n=2048, lo=1e-3, hi=1e6, device=None):
    """``u`` log-spaced over ``+-[lo, hi]``, float32, both signs interleaved."""
    a = torch.logspace(math.log10(lo), math.log10(hi), n, dtype=torch.float64, device=device)
    return torch.stack([a, -a], 1).reshape(-1).float()


def random_boxes(n=4096, seed=5, device=None):
    """``n`` two-sided boxes, widths log-uniform in [1e-3, 10], lower edges in [-10, 10)."""
    g = torch.Generator().manual_seed(seed)
    w = 10.0 ** (-3.0 + 4.0 * torch.rand(n, generator=g, dtype=torch.float64))
    lo = (20.0 * torch.rand(n, generator=g, dtype=torch.float64) - 10.0).float()
    hi = (lo.double() + w).float()
    assert bool((hi > lo).all())
    return lo.to(device), hi.to(device)
