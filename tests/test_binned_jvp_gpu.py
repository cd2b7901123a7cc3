"""Forward-mode tangent of gaussian_binned_sum on the MI355X (csrc/binned_jvp.hip).

Oracle: float64 forward AD of the ndtr composite on the float32-rounded inputs, with the
shapes, the input generator and the sigma / w modes of test_binned_hvp_gpu.py; the tangents
(tmu, tsigma, tw) are that generator's seeded normals (a, b, c).

Bound: the project's first-order gradient contract applied term by term (the rule
gaussian_binned_sum_multi uses for its channel sums),

    |t_k - ref_k|  <=  2e-4 A_k + 2e-5 max_k A_k,
    A_k = sum_i ( |tmu_i dout_k/dmu_i| + |tsigma_i dout_k/dsigma_i| + |tw_i dPhi_ik| )

with A_k evaluated in float64.  The error of the float32 composite under torch's forward AD
on the device is printed beside the kernel's.
"""
import functools
import math
import os
import sys

import pytest
import torch
import torch.autograd.forward_ad as fwad

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_binned_hvp_gpu import SHAPES, _composite, _edges, _op, _operands  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SETS = {"mu": (True, False, False), "sigma": (False, True, False), "w": (False, False, True),
        "all": (True, True, True)}
MODES = [(w, t) for w in ("none", "per-object") for t in SETS if not (w == "none" and t == "w")]


def _jvp(fn, ops, tans, which, dtype, device, view=False):
    """The tangent of fn(mu, sigma[, w]) along the tangents selected by ``which``."""
    def put(t):
        t = t.to(device=device, dtype=dtype)
        if view:            # a 4-byte-offset pointer: the guarded scalar path
            t = torch.cat([t.new_zeros(1), t])[1:]
            assert t.data_ptr() % 16 == 4
        return t

    with fwad.dual_level():
        args = [fwad.make_dual(put(t), put(d)) if k else put(t)
                for t, d, k in zip(ops, tans, which)]
        tangent = fwad.unpack_dual(fn(*args)).tangent
    return tangent.detach()


@functools.lru_cache(maxsize=None)
def _oracle(n, nb, sigma_mode, w_mode, which):
    """(reference tangent, A) in float64 on the host."""
    ops, tans = _operands(n, sigma_mode, w_mode)
    edges = _edges(nb)
    sel = SETS[which]
    ref = _jvp(lambda m, s, ww=None: _composite(m, s, ww, edges), ops, tans, sel, torch.float64,
               "cpu")
    mu, sigma = ops[0].double(), ops[1].double()
    w = ops[2].double() if len(ops) == 3 else torch.ones(1, dtype=torch.float64)
    e = torch.tensor(edges, dtype=torch.float64)
    z = (e[None, :] - mu[:, None]) / sigma.reshape(-1, 1)
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    c = -(w / sigma).reshape(-1, 1)
    A = torch.zeros(nb, dtype=torch.float64)
    if sel[0]:
        A += (tans[0].double()[:, None] * c * (phi[:, 1:] - phi[:, :-1])).abs().sum(0)
    if sel[1]:
        zphi = z * phi
        A += (tans[1].double().reshape(-1, 1) * c * (zphi[:, 1:] - zphi[:, :-1])).abs().sum(0)
    if sel[2] and len(ops) == 3:
        cdf = torch.special.ndtr(z)
        A += (tans[2].double().reshape(-1, 1) * (cdf[:, 1:] - cdf[:, :-1])).abs().sum(0)
    return ref, A


def _run_case(n, nb, sigma_mode, w_mode, which, view=False):
    ops, tans = _operands(n, sigma_mode, w_mode)
    edges = _edges(nb)
    sel = SETS[which]
    ref, A = _oracle(n, nb, sigma_mode, w_mode, which)
    comp = _jvp(lambda m, s, ww=None: _composite(m, s, ww, edges), ops, tans, sel, torch.float32,
                DEV)
    got = _jvp(lambda m, s, ww=None: _op(m, s, ww, edges), ops, tans, sel, torch.float32, DEV,
               view=view)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (nb,)
    assert bool(torch.isfinite(got).all())
    err = (got.double().cpu() - ref).abs()
    err_c = (comp.double().cpu() - ref).abs()
    bound = 2e-4 * A + 2e-5 * A.max()
    print(f"n={n} nb={nb} {sigma_mode}/{w_mode} d{which}: op err {float(err.max()):.3e} "
          f"composite err {float(err_c.max()):.3e} max A {float(A.max()):.3e} "
          f"worst err/bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), (err, bound)
    return got


@pytest.mark.parametrize("w_mode,which", MODES)
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_jvp_matches_fp64(n, nb, sigma_mode, w_mode, which):
    _run_case(n, nb, sigma_mode, w_mode, which)


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", [(1023, 10), (1025, 17)])
def test_broadcast_weights(n, nb, sigma_mode, which):
    _run_case(n, nb, sigma_mode, "broadcast", which)


def test_misaligned_view_takes_the_guarded_path():
    got = _run_case(1023, 10, "per-object", "per-object", "all", view=True)
    # the same values from aligned tensors: same bits (the load path does not change the
    # arithmetic)
    again = _run_case(1023, 10, "per-object", "per-object", "all")
    assert torch.equal(got, again)


@pytest.mark.parametrize("sigma_mode,w_mode", [("per-object", "per-object"),
                                               ("broadcast", "none"), ("broadcast", "broadcast")])
@pytest.mark.parametrize("n,nb", [(1023, 10), (200_003, 32)])
def test_adjoint_identity_with_the_backward_kernel(n, nb, sigma_mode, w_mode):
    """|<g, jvp(t)> - <vjp(g), t>| <= 4.4e-4 sum_k |g_k| A_k: the contracts of the tangent
    kernel and of the existing backward kernel added, dots in float64."""
    ops, tans = _operands(n, sigma_mode, w_mode)
    edges = _edges(nb)
    _, A = _oracle(n, nb, sigma_mode, w_mode, "all")
    g = torch.linspace(0.5, 1.5, nb, dtype=torch.float64)
    tout = _jvp(lambda m, s, ww=None: _op(m, s, ww, edges), ops, tans, SETS["all"],
                torch.float32, DEV)
    leaves = [t.to(DEV).requires_grad_(True) for t in ops]
    out = _op(leaves[0], leaves[1], leaves[2] if len(leaves) == 3 else None, edges)
    grads = torch.autograd.grad(out, leaves, g.to(DEV, torch.float32))
    lhs = float((g * tout.double().cpu()).sum())
    rhs = float(sum((gr.double().cpu() * t.double()).sum() for gr, t in zip(grads, tans)))
    bound = 4.4e-4 * float((g.abs() * A).sum())
    print(f"n={n} nb={nb} {sigma_mode}/{w_mode}: <g,jvp> {lhs:.9e} <vjp,t> {rhs:.9e} "
          f"diff {abs(lhs - rhs):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_bitwise_deterministic():
    n, nb = 200_003, 10
    ops, tans = _operands(n, "broadcast", "per-object")
    fn = (lambda m, s, ww: _op(m, s, ww, _edges(nb)))
    a = _jvp(fn, ops, tans, SETS["all"], torch.float32, DEV)
    b = _jvp(fn, ops, tans, SETS["all"], torch.float32, DEV)
    assert torch.equal(a, b)


@pytest.mark.parametrize("w_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", [(1023, 10), (200_003, 32)])
def test_weights_tangent_alone_is_the_forward(n, nb, w_mode):
    ops, tans = _operands(n, "per-object", w_mode)
    edges = _edges(nb)
    got = _jvp(lambda m, s, ww: _op(m, s, ww, edges), ops, tans, SETS["w"], torch.float32, DEV)
    fwd = _op(ops[0].to(DEV), ops[1].to(DEV), tans[2].to(DEV), edges)
    assert torch.equal(got, fwd)


def test_jvp_under_no_grad():
    n, nb = 1025, 17
    ops, tans = _operands(n, "per-object", "per-object")
    edges = _edges(nb)
    fn = (lambda m, s, ww: _op(m, s, ww, edges))
    plain = _jvp(fn, ops, tans, SETS["all"], torch.float32, DEV)
    with torch.no_grad():
        quiet = _jvp(fn, ops, tans, SETS["all"], torch.float32, DEV)
    assert torch.equal(plain, quiet)
