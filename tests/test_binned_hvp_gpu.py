"""Second backward of gaussian_binned_sum on the MI355X (csrc/binned_hvp.hip) and the
model-level Hessian-vector product on the device.

Oracle: float64 autograd (double backward) of the ndtr expression on the float32-rounded
inputs, with the input generator of test_binned_gpu.py, cotangents a, b, c of (dmu, dsigma,
dw) drawn as seeded normals and g = linspace(0.5, 1.5, nb).

Tolerance: nothing in the project derives a float32 bound for second derivatives, so each
test also evaluates the same outputs with the float32 ndtr composite on the GPU through
torch's own double backward and asserts, per output,

    max |op - ref|  <=  2 * max |composite - ref|  +  2e-5 * max |ref|

(the factor 2 is measured, not derived, as in test_invhess_gpu.py; the floor is the absolute
term of the first-order contract).  Both errors are printed.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# (1, 1) .. (1023, 10): a ragged last quad in a single workgroup (outputs written directly);
# (1025, 17): the first size with two workgroups (slabs and the reduce); (200_003, 32): many
# slab rows and the widest dispatch
SHAPES = [(1, 1), (63, 4), (257, 5), (1023, 10), (1025, 17), (200_003, 32)]
NAMES = ("mu", "sigma", "w", "g")


def _edges(nb):
    # float32-representable edges (the kernels hold them in float32)
    return tuple(float(v) for v in np.linspace(9.2, 10.4, nb + 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """float32 inputs on the host: means around the bins, widths 0.1-0.5, weights of both
    signs with exact zeros (the generator of test_binned_gpu.py), and normal cotangents."""
    g = torch.Generator().manual_seed(seed + n)
    mu = 9.0 + 1.6 * torch.rand(n, generator=g)
    if n == 1:
        mu = torch.tensor([9.7])
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g)
    w = torch.randn(n, generator=g)
    w[::7] = 0.0
    if n == 1:
        w = torch.tensor([-1.3])
    a, b, c = (torch.randn(n, generator=g) for _ in range(3))
    return mu, sigma, w, a, b, c


def _composite(mu, sigma, w, edges):
    e = torch.tensor(edges, dtype=mu.dtype, device=mu.device)
    cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma.reshape(-1, 1))
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1, 1)
    return d.sum(0)


def _op(mu, sigma, w, edges):
    from multigrad_amd.ops import gaussian_binned_sum
    return gaussian_binned_sum(mu, sigma, edges, w)


def _second(fn, ops, cots, nb, dtype, device):
    """(first-order gradients, gradients of sum_i (a dmu + b dsigma + c dw) w.r.t. the operands
    and g) of ``fn`` in ``dtype`` on ``device``; ops / cots: (mu, sigma[, w]) and (a, b[, c])."""
    leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in ops]
    g = torch.linspace(0.5, 1.5, nb, dtype=torch.float64).to(device=device, dtype=dtype)
    g.requires_grad_(True)
    out = fn(*leaves)
    first = torch.autograd.grad(out, leaves, g, create_graph=True)
    second = torch.autograd.grad(first, leaves + [g],
                                 [c.to(device=device, dtype=dtype) for c in cots])
    return [t.detach() for t in first], [t.detach() for t in second]


def _operands(n, sigma_mode, w_mode):
    mu, sigma, w, a, b, c = _inputs(n)
    if sigma_mode == "broadcast":
        sigma, b = sigma[:1].clone(), b[:1].clone()
    if w_mode == "broadcast":
        w, c = torch.tensor([-0.7]), c[:1].clone()
    if w_mode == "none":
        return (mu, sigma), (a, b)
    return (mu, sigma, w), (a, b, c)


@functools.lru_cache(maxsize=None)
def _oracle(n, nb, sigma_mode, w_mode):
    ops, cots = _operands(n, sigma_mode, w_mode)
    edges = _edges(nb)
    fn = (lambda m, s, ww=None: _composite(m, s, ww, edges))
    return _second(fn, ops, cots, nb, torch.float64, "cpu")[1]


def _check(got, comp, ref, names, what=""):
    """The error-ratio rule of the module docstring; returns the ratios op/composite."""
    rows = {}
    for k, g, c, r in zip(names, got, comp, ref):
        g, c, r = (t.double().cpu().reshape(-1) for t in (g, c, r))
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), k
        scale = float(r.abs().max())
        e_op, e_c = float((g - r).abs().max()), float((c - r).abs().max())
        rows[k] = (e_op, e_c, scale)
        ratio = e_op / e_c if e_c > 0 else float("inf") if e_op > 0 else 0.0
        print(f"{what} d/d{k}: op err {e_op:.3e} composite err {e_c:.3e} max|ref| {scale:.3e} "
              f"ratio {ratio:.3f}")
    for k, (e_op, e_c, scale) in rows.items():   # every figure is printed before any assert
        assert e_op <= 2.0 * e_c + 2e-5 * scale, (k, e_op, e_c, scale)
    return rows


def _run_case(n, nb, sigma_mode, w_mode, view=False):
    ops, cots = _operands(n, sigma_mode, w_mode)
    edges = _edges(nb)
    ref = _oracle(n, nb, sigma_mode, w_mode)
    names = NAMES if len(ops) == 3 else ("mu", "sigma", "g")
    comp = _second(lambda m, s, ww=None: _composite(m, s, ww, edges), ops, cots, nb,
                   torch.float32, DEV)[1]

    def fn(m, s, ww=None):
        if view:        # a 4-byte-offset pointer: the guarded scalar path
            m = torch.cat([m.new_zeros(1), m])[1:]
            assert m.data_ptr() % 16 == 4
        return _op(m, s, ww, edges)

    got = _second(fn, ops, cots, nb, torch.float32, DEV)[1]
    for t, o in zip(got, list(ops) + [ref[-1]]):
        assert t.is_cuda and t.dtype == torch.float32 and t.shape == o.shape
    return got, _check(got, comp, ref, names, f"n={n} nb={nb} {sigma_mode}/{w_mode}")


@pytest.mark.parametrize("w_mode", ["none", "per-object"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_second_order_matches_fp64(n, nb, sigma_mode, w_mode):
    _run_case(n, nb, sigma_mode, w_mode)


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", [(1023, 10), (1025, 17)])
def test_broadcast_weights(n, nb, sigma_mode):
    _run_case(n, nb, sigma_mode, "broadcast")


def test_misaligned_view_takes_the_guarded_path():
    got, _ = _run_case(1023, 10, "per-object", "per-object", view=True)
    # the same values from aligned tensors: same bits (the load path does not change the
    # arithmetic)
    again, _ = _run_case(1023, 10, "per-object", "per-object")
    assert all(torch.equal(x, y) for x, y in zip(got, again))


# (cotangents left out, gradients asked for): every kernel variant (with and without the
# gradient of g, with and without Phi) and stores of one, two or three operands
SUBSETS = [("a", ("mu", "g")), ("b", ("sigma", "w")), ("c", NAMES), ("ab", ("g",)),
           ("bc", ("mu",)), ("ac", ("w", "g"))]


@pytest.mark.parametrize("drop,wrt", SUBSETS, ids=[f"no-{d}" for d, _ in SUBSETS])
def test_absent_cotangents_and_gradient_subsets(drop, wrt):
    """Cotangents left out (None, never materialised) and only some gradients requested (g
    requires grad only when its gradient is), against the float64 oracle with the same
    cotangents set to zero."""
    n, nb = 1023, 10
    ops, cots = _operands(n, "per-object", "per-object")
    edges = _edges(nb)
    zeroed = [torch.zeros_like(c) if k in drop else c for k, c in zip("abc", cots)]
    fn64 = (lambda m, s, ww: _composite(m, s, ww, edges))
    ref = _second(fn64, ops, zeroed, nb, torch.float64, "cpu")[1]
    comp = _second(fn64, ops, zeroed, nb, torch.float32, DEV)[1]
    leaves = [t.to(DEV).requires_grad_(True) for t in ops]
    g = torch.linspace(0.5, 1.5, nb, dtype=torch.float64).to(DEV, torch.float32)
    g.requires_grad_("g" in wrt)
    first = torch.autograd.grad(_op(*leaves, edges), leaves, g, create_graph=True)
    keep = [(f, c.to(DEV)) for k, f, c in zip("abc", first, cots) if k not in drop]
    idx = [NAMES.index(k) for k in wrt]
    targets = [(leaves + [g])[i] for i in idx]
    got = torch.autograd.grad([f for f, _ in keep], targets, [c for _, c in keep],
                              allow_unused=True)
    got = [torch.zeros_like(x) if t is None else t for t, x in zip(got, targets)]
    _check(got, [comp[i] for i in idx], [ref[i] for i in idx], wrt, f"without {drop}")


def test_bitwise_deterministic():
    n, nb = 200_003, 10
    ops, cots = _operands(n, "broadcast", "per-object")
    fn = (lambda m, s, ww: _op(m, s, ww, _edges(nb)))
    a = _second(fn, ops, cots, nb, torch.float32, DEV)[1]
    b = _second(fn, ops, cots, nb, torch.float32, DEV)[1]
    for k, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), k


def test_first_order_unchanged_by_create_graph():
    n, nb = 200_003, 17
    ops, cots = _operands(n, "broadcast", "per-object")
    edges = _edges(nb)
    with_graph = _second(lambda m, s, ww: _op(m, s, ww, edges), ops, cots, nb, torch.float32,
                         DEV)[0]
    leaves = [t.to(DEV).requires_grad_(True) for t in ops]
    g = torch.linspace(0.5, 1.5, nb, dtype=torch.float64).to(DEV, torch.float32)
    plain = torch.autograd.grad(_op(*leaves, edges), leaves, g)
    for k, x, y in zip(NAMES, with_graph, plain):
        assert torch.equal(x, y), k


def test_functional_hessian_runs_on_the_device():
    n, nb = 257, 5
    ops, _ = _operands(n, "broadcast", "none")
    edges = _edges(nb)
    gS = torch.linspace(0.5, 1.5, nb)

    def scalar(fn, dev, dtype):
        return lambda s: (fn(ops[0].to(dev, dtype), s, None, edges) ** 2 * gS.to(dev, dtype)).sum()

    ref = torch.autograd.functional.hessian(scalar(_composite, "cpu", torch.float64),
                                            ops[1].double())
    comp = torch.autograd.functional.hessian(scalar(_composite, DEV, torch.float32),
                                             ops[1].to(DEV))
    got = torch.autograd.functional.hessian(scalar(_op, DEV, torch.float32), ops[1].to(DEV))
    _check([got], [comp], [ref], ["sigma"], "hessian")


def test_model_hvp_matches_fp64_torch_model():
    """calc_hvp_from_params of GroupedBinnedPopulationSMFModel on the GPU against the float64
    CPU Hessian product of TorchPopulationSMFModel: 200 populations, 4000 halos; the composite
    of the error-ratio rule is the float32 TorchPopulationSMFModel on the GPU."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(400, 4000, seed=11, device="cpu")
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    guess = data["guess"]
    v = torch.randn(guess.numel(), generator=torch.Generator().manual_seed(1))

    def moved(dev, dtype):
        return {k: (t.to(dev, dtype) if t.is_floating_point() else t.to(dev))
                if torch.is_tensor(t) else t for k, t in aux.items()}

    ref_model = TorchPopulationSMFModel(aux_data=moved("cpu", torch.float64), dtype=torch.float64)

    def full_loss(p):
        return ref_model.calc_loss_from_sumstats(ref_model.calc_partial_sumstats_from_params(p))

    ref = torch.autograd.functional.hvp(full_loss, guess.double(), v.double())[1]
    on_dev = moved(DEV, torch.float32)
    comp = TorchPopulationSMFModel(aux_data=on_dev).calc_hvp_from_params(guess.to(DEV), v.to(DEV))
    got = GroupedBinnedPopulationSMFModel(aux_data=on_dev).calc_hvp_from_params(guess.to(DEV),
                                                                               v.to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == guess.shape
    _check([got], [comp], [ref], ["params"], "model hvp")
