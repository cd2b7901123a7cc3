"""Forward mode (torch.autograd.forward_ad) of gaussian_binned_sum and the group ops on the
torch path, in float64 against forward AD of the ndtr composite."""
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwad

from multigrad_amd.ops import gaussian_binned_sum
from multigrad_amd.ops.groups import GroupIndex

F64 = torch.float64
SETS = {"mu": (True, False, False), "sigma": (False, True, False), "w": (False, False, True),
        "all": (True, True, True)}


def _composite(mu, sigma, edges, w=None):
    e = torch.as_tensor(edges, dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1)[:, None])
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1)[:, None]
    return d.sum(0)


def _edges(nb):
    return tuple(np.linspace(9.2, 10.4, nb + 1).tolist())


@functools.lru_cache(maxsize=None)
def _inputs(n, sigma_mode, w_mode):
    """(operands, tangents) in float64; a broadcast operand and its tangent have one element."""
    g = torch.Generator().manual_seed(n)
    mu = 9.0 + 1.6 * torch.rand(n, generator=g, dtype=F64)
    sigma = 0.1 + 0.4 * torch.rand(1 if sigma_mode == "broadcast" else n, generator=g, dtype=F64)
    w = None if w_mode == "none" else torch.randn(1 if w_mode == "broadcast" else n, generator=g,
                                                  dtype=F64)
    ops = (mu, sigma, w)
    tans = tuple(None if t is None else torch.randn(t.shape, generator=g, dtype=F64) for t in ops)
    return ops, tans


def _jvp(fn, ops, tans, which):
    """The tangent of fn(mu, sigma, w) along the tangents selected by ``which``."""
    with fwad.dual_level():
        args = [t if t is None or not k else fwad.make_dual(t, d)
                for t, d, k in zip(ops, tans, which)]
        return fwad.unpack_dual(fn(*args)).tangent


# without weights there is no weights tangent: "all" is then (mu, sigma)
MODES = [(w, t) for w in ("per-object", "broadcast", "none") for t in SETS
         if not (w == "none" and t == "w")]


@pytest.mark.parametrize("w_mode,which", MODES)
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("nb", [1, 10, 32])
@pytest.mark.parametrize("n", [1, 63, 1025])
def test_torch_jvp_matches_composite_fp64(n, nb, sigma_mode, w_mode, which):
    ops, tans = _inputs(n, sigma_mode, w_mode)
    edges = _edges(nb)
    ref = _jvp(lambda m, s, w: _composite(m, s, edges, w), ops, tans, SETS[which])
    got = _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w), ops, tans, SETS[which])
    assert got.shape == (nb,) and got.dtype == F64
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_chunked_jvp():
    ops, tans = _inputs(1025, "per-object", "per-object")
    edges = _edges(10)
    ref = _jvp(lambda m, s, w: _composite(m, s, edges, w), ops, tans, SETS["all"])
    got = _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w, chunk=100), ops, tans,
               SETS["all"])
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_jvp_under_no_grad():
    ops, tans = _inputs(63, "broadcast", "per-object")
    edges = _edges(10)
    ref = _jvp(lambda m, s, w: _composite(m, s, edges, w), ops, tans, SETS["all"])
    with torch.no_grad():
        got = _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w), ops, tans, SETS["all"])
    assert got is not None
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_missing_tangents_are_not_materialised():
    """With a tangent of the weights alone jvp receives None for mu and sigma (not zeros), so
    the tangent is the forward with tw as the weights, bit for bit."""
    from multigrad_amd.ops import binned
    ops, tans = _inputs(1025, "per-object", "per-object")
    edges = _edges(10)
    seen = []
    orig = binned._torch_jvp

    def spy(mu, sigma, w, e, tmu, tsigma, tw, chunk):
        seen.append((tmu, tsigma, tw))
        return orig(mu, sigma, w, e, tmu, tsigma, tw, chunk)

    binned._torch_jvp = spy
    try:
        got = _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w), ops, tans, SETS["w"])
    finally:
        binned._torch_jvp = orig
    assert len(seen) == 1 and seen[0][0] is None and seen[0][1] is None
    assert torch.equal(got, gaussian_binned_sum(ops[0], ops[1], edges, tans[2]))


def test_jvp_of_empty_input_is_zero():
    empty = torch.zeros(0, dtype=F64)
    with fwad.dual_level():
        out = gaussian_binned_sum(fwad.make_dual(empty, empty.clone()), empty, _edges(4), empty)
        value, tangent = fwad.unpack_dual(out)
    assert torch.equal(value, torch.zeros(4, dtype=F64))
    assert tangent is None or torch.equal(tangent, torch.zeros(4, dtype=F64))


@pytest.mark.parametrize("sigma_mode,w_mode", [("per-object", "per-object"),
                                               ("broadcast", "broadcast"), ("broadcast", "none")])
def test_adjoint_identity(sigma_mode, w_mode):
    """<g, jvp(t)> = <vjp(g), t> in float64."""
    ops, tans = _inputs(1025, sigma_mode, w_mode)
    edges = _edges(10)
    live = [i for i, t in enumerate(ops) if t is not None]
    g = torch.linspace(0.5, 1.5, 10, dtype=F64)
    tout = _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w), ops, tans,
                tuple(t is not None for t in ops))
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in ops]
    grads = torch.autograd.grad(gaussian_binned_sum(leaves[0], leaves[1], edges, leaves[2]),
                                [leaves[i] for i in live], g)
    lhs = float((g * tout).sum())
    rhs = float(sum((gr * tans[i]).sum() for gr, i in zip(grads, live)))
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), 1.0)


def test_group_ops_under_forward_ad():
    g = torch.Generator().manual_seed(5)
    index = torch.randint(0, 7, (300,), generator=g)
    plan = GroupIndex(index, 7)
    a, b, ta = (torch.randn(7, generator=g, dtype=F64) for _ in range(3))
    x, y, ty = (torch.randn(300, generator=g, dtype=F64) for _ in range(3))
    with fwad.dual_level():
        # b and x carry no tangent: zeros, since another operand of the call has one
        ga, gb = plan.gather(fwad.make_dual(a, ta), b)
        sx, sy = plan.segment_sum(x, fwad.make_dual(y, ty))
        tga, tgb, tsx, tsy = (fwad.unpack_dual(t).tangent for t in (ga, gb, sx, sy))
    zero = torch.zeros(7, dtype=F64)
    assert float((tga - ta[index]).abs().max()) <= 1e-12
    assert tgb is None or not tgb.any()
    assert tsx is None or not tsx.any()
    assert float((tsy - zero.index_add(0, index, ty)).abs().max()) <= 1e-12
    # composed: gather, then the binned sum, against indexing and the composite
    edges = _edges(5)
    pos = torch.rand(300, generator=g, dtype=F64) + 9.3

    def model(fn_gather, fn_sum, a_):
        return fn_sum(pos + fn_gather(a_), torch.full((1,), 0.3, dtype=F64))

    with fwad.dual_level():
        d = fwad.make_dual(a, ta)
        got = fwad.unpack_dual(model(lambda v: plan.gather(v)[0],
                                     lambda m, s: gaussian_binned_sum(m, s, edges), d)).tangent
        ref = fwad.unpack_dual(model(lambda v: v[index],
                                     lambda m, s: _composite(m, s, edges), d)).tangent
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


def test_reverse_mode_bits_unchanged_by_forward_ad():
    """Reverse-mode results after forward-AD use are bitwise those of a call made before it."""
    ops, tans = _inputs(1025, "per-object", "per-object")
    edges = _edges(10)
    g = torch.linspace(0.5, 1.5, 10, dtype=F64)

    def reverse():
        leaves = [t.clone().requires_grad_(True) for t in ops]
        out = gaussian_binned_sum(leaves[0], leaves[1], edges, leaves[2])
        return [out.detach()] + list(torch.autograd.grad(out, leaves, g))

    before = reverse()
    _jvp(lambda m, s, w: gaussian_binned_sum(m, s, edges, w), ops, tans, SETS["all"])
    after = reverse()
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_ops_without_a_forward_rule_raise():
    from multigrad_amd.ops.binned2d import gaussian_binned_sum_2d
    from multigrad_amd.ops.binned_multi import gaussian_binned_sum_multi
    ops, tans = _inputs(63, "per-object", "per-object")
    mu, sigma, w = ops
    with fwad.dual_level():
        d = fwad.make_dual(mu, tans[0])
        with pytest.raises(NotImplementedError):
            gaussian_binned_sum_2d(d, sigma, mu, sigma, _edges(4), _edges(3))
        with pytest.raises(NotImplementedError):
            gaussian_binned_sum_multi(d, sigma, _edges(4), (None, w))
