"""gaussian_binned_sum_fine on the CPU: the float64 torch path (the dense dPhi table, no
truncation) against the ndtr composite under autograd, the argument contract, and the model,
the example and the benchmark around the op."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _edges(nb, lo=9.0, hi=11.0):
    return tuple(float(v) for v in np.linspace(lo, hi, nb + 1))


def _inputs(n, nb, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * n + nb)
    mu = 8.8 + 2.4 * torch.rand(n, generator=g, dtype=F64)
    sigma = (2.0 / nb) * (0.5 + 4.0 * torch.rand(n, generator=g, dtype=F64))
    w = torch.randn(n, generator=g, dtype=F64)
    return mu, sigma, w


def _modes(mu, sigma, w, sigma_mode, w_mode):
    if sigma_mode == "broadcast":
        sigma = sigma[:1].clone() if sigma.numel() else torch.tensor([0.07], dtype=F64)
    w = {"none": None, "per-object": w, "one-element": torch.tensor([-0.7], dtype=F64)}[w_mode]
    return mu, sigma, w


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _composite(mu, sigma, w, edges):
    e = torch.tensor(edges, dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1)[:, None])
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1)[:, None]
    return d.sum(0)


def _grads(fn, ops, nb):
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in ops]
    out = fn(*leaves)
    cot = torch.linspace(0.5, 1.5, nb, dtype=out.dtype)
    live = [t for t in leaves if t is not None]
    return out.detach(), torch.autograd.grad(out, live, cot, allow_unused=True)


@pytest.mark.parametrize("w_mode", ["none", "per-object", "one-element"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n", [0, 1, 1000])
@pytest.mark.parametrize("nb", [33, 257])
def test_forward_and_gradients_match_the_composite(nb, n, sigma_mode, w_mode):
    from multigrad_amd.ops import FineBins, gaussian_binned_sum_fine
    edges = _edges(nb)
    bins = FineBins(edges)
    assert bins.nb == nb and bins.edges == edges and bins.device == torch.device("cpu")
    assert bins.edges_dev.dtype == torch.float32 and bins.edges_dev.shape == (nb + 1,)
    ops = _modes(*_inputs(n, nb), sigma_mode, w_mode)
    out, grads = _grads(lambda m, s, w: gaussian_binned_sum_fine(bins, m, s, w), ops, nb)
    full = lambda t: t.expand(n) if t.numel() == 1 else t  # noqa: E731
    ref, gref = _grads(lambda m, s, w: _composite(m, full(s), None if w is None else full(w),
                                                  edges), ops, nb)
    assert out.shape == (nb,) and out.dtype == F64
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12 * max(_amax(ref), 1.0))
    live = [t for t in ops if t is not None]
    assert len(grads) == len(gref) == len(live)
    for g, r, t in zip(grads, gref, live):
        assert g.shape == t.shape
        r = torch.zeros_like(t) if r is None else r
        np.testing.assert_allclose(g, r, rtol=1e-12, atol=1e-12 * max(_amax(r), 1.0))
    if n == 0:
        assert (out == 0).all()


def test_method_and_function_agree_and_shapes_are_kept():
    from multigrad_amd.ops import FineBins, gaussian_binned_sum_fine
    nb = 40
    bins = FineBins(np.asarray(_edges(nb)))
    mu, sigma, w = _inputs(60, nb)
    a = bins.sum(mu.reshape(6, 10), sigma.reshape(6, 10), w.reshape(6, 10))
    assert torch.equal(a, gaussian_binned_sum_fine(bins, mu, sigma, w))
    # non-contiguous inputs are copied
    buf = torch.zeros(120, dtype=F64)
    buf[::2] = mu
    assert torch.equal(a, bins.sum(buf[::2], sigma, w))
    m = mu.reshape(6, 10).clone().requires_grad_(True)
    (g,) = torch.autograd.grad(bins.sum(m, sigma.reshape(6, 10)).sum(), m)
    assert g.shape == (6, 10)
    # a CPU tensor of edges is a host sequence too
    assert torch.equal(a, FineBins(torch.tensor(_edges(nb), dtype=F64)).sum(mu, sigma, w))


@pytest.mark.parametrize("nb", [1, 10, 32])
def test_few_bins_are_bitwise_the_single_op(nb):
    from multigrad_amd.ops import FineBins, gaussian_binned_sum
    edges = _edges(nb)
    for dtype in (F64, torch.float32):
        mu, sigma, w = (t.to(dtype) for t in _inputs(500, nb))
        ops = [t.clone().requires_grad_(True) for t in (mu, sigma, w)]
        ref_ops = [t.clone().requires_grad_(True) for t in (mu, sigma, w)]
        out = FineBins(edges).sum(*ops)
        ref = gaussian_binned_sum(ref_ops[0], ref_ops[1], edges, ref_ops[2])
        assert torch.equal(out, ref)
        cot = torch.linspace(0.5, 1.5, nb, dtype=dtype)
        for g, r in zip(torch.autograd.grad(out, ops, cot), torch.autograd.grad(ref, ref_ops, cot)):
            assert torch.equal(g, r)


@pytest.mark.parametrize("refine", [4, 8])
def test_merged_fine_bins_equal_the_coarse_op(refine):
    from multigrad_amd.ops import FineBins, gaussian_binned_sum
    nbc = 12
    coarse = np.asarray(_edges(nbc))
    fine = np.concatenate([(coarse[:-1, None] + np.diff(coarse)[:, None] *
                            np.arange(refine)[None, :] / refine).reshape(-1), coarse[-1:]])
    assert fine.size == nbc * refine + 1 and (fine[::refine] == coarse).all()
    mu, sigma, w = _inputs(800, nbc * refine)
    out = FineBins(fine).sum(mu, sigma, w).reshape(nbc, refine).sum(1)
    ref = gaussian_binned_sum(mu, sigma, tuple(coarse), w)
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-12 * float(ref.abs().max()))


def test_gradcheck_float64():
    from multigrad_amd.ops import FineBins
    bins = FineBins(_edges(35))
    mu, sigma, w = (t.requires_grad_(True) for t in _inputs(12, 35, seed=1))
    assert torch.autograd.gradcheck(lambda m, s, x: bins.sum(m, s, x), (mu, sigma, w))
    s1 = sigma.detach()[:1].clone().requires_grad_(True)
    w1 = w.detach()[:1].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda m, s, x: bins.sum(m, s, x), (mu, s1, w1))


def test_chunking():
    from multigrad_amd.ops import FineBins
    from multigrad_amd.ops import binned_fine as bf
    nb = 50
    bins = FineBins(_edges(nb))
    mu, sigma, w = _inputs(23, nb, seed=3)
    a, ga = _grads(lambda m, s, x: bins.sum(m, s, x), (mu, sigma, w), nb)
    b, gb = _grads(lambda m, s, x: bins.sum(m, s, x, chunk=5), (mu, sigma, w), nb)
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)
    for x, y in zip(ga, gb):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-14)
    # the default chunk keeps the dPhi table of a chunk at 2^21 elements
    seen = []
    orig = bf._torch_forward
    bf._torch_forward = lambda m, s, x, e, chunk: seen.append(chunk) or orig(m, s, x, e, chunk)
    try:
        for n_bins in (33, 4096):
            FineBins(_edges(n_bins)).sum(mu, sigma)
    finally:
        bf._torch_forward = orig
    assert seen == [min(1 << 16, (1 << 21) // 33), 512]
    assert all(c * k <= 1 << 21 for c, k in zip(seen, (33, 4096)))


def test_plan_errors():
    from multigrad_amd.ops import FineBins
    from multigrad_amd.ops.binned_fine import MAX_FINE_BINS
    assert MAX_FINE_BINS == 4096
    FineBins(_edges(4096))
    for bad in ([1.0], [], _edges(4097)):
        with pytest.raises(ValueError, match="4096"):
            FineBins(bad)
    for bad in ([0.0, 2.0, 1.0, 3.0], [0.0, 1.0, 1.0], [0.0, float("nan"), 2.0],
                [0.0, 1.0, float("inf")]):
        with pytest.raises(ValueError, match="increasing"):
            FineBins(bad)
    with pytest.raises(TypeError, match="setup"):
        FineBins(torch.empty(5, device="meta"))


def test_operand_errors():
    from multigrad_amd.ops import FineBins
    from multigrad_amd.ops import gaussian_binned_sum_fine as f
    bins = FineBins(_edges(40))
    mu, sigma, w = _inputs(10, 40)
    with pytest.raises(TypeError, match="FineBins"):
        f(_edges(40), mu, sigma)
    with pytest.raises(TypeError, match="tensors"):
        f(bins, mu.numpy(), sigma)
    with pytest.raises(TypeError, match="weights"):
        f(bins, mu, sigma, [1.0] * 10)
    with pytest.raises(ValueError, match="sigma has 3"):
        f(bins, mu, sigma[:3])
    with pytest.raises(ValueError, match="weights has 4"):
        f(bins, mu, sigma, w[:4])
    with pytest.raises(ValueError, match="sigma must have mu's dtype"):
        f(bins, mu, sigma.float())
    with pytest.raises(ValueError, match="weights must have mu's dtype"):
        f(bins, mu, sigma, w.float())
    with pytest.raises(ValueError, match="weights must have mu's dtype and device"):
        f(bins, mu, sigma, torch.empty(10, dtype=F64, device="meta"))
    with pytest.raises(ValueError, match="floating"):
        f(bins, torch.arange(10), torch.arange(10))
    with pytest.raises(ValueError, match="mu lives on"):
        f(bins, torch.empty(10, dtype=F64, device="meta"),
          torch.empty(10, dtype=F64, device="meta"))


def test_double_backward_raises():
    from multigrad_amd.ops import FineBins
    bins = FineBins(_edges(33))
    mu, sigma, w = (t.requires_grad_(True) for t in _inputs(20, 33, seed=5))
    out = bins.sum(mu, sigma, w)
    (g,) = torch.autograd.grad((out * out).sum(), mu, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_forward_ad_raises_not_implemented():
    import torch.autograd.forward_ad as fwad
    from multigrad_amd.ops import FineBins
    bins = FineBins(_edges(33))
    mu, sigma, w = _inputs(20, 33, seed=5)
    with fwad.dual_level():
        with pytest.raises(NotImplementedError):
            bins.sum(fwad.make_dual(mu, torch.ones_like(mu)), sigma, w)


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; "
            "assert 'multigrad_amd.ops.binned_fine' not in sys.modules; "
            "f, B = o.gaussian_binned_sum_fine, o.FineBins; "
            "assert 'multigrad_amd.ops.binned_fine' in sys.modules; "
            "assert {'gaussian_binned_sum_fine', 'FineBins'} <= set(o.__all__); "
            "assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def _fine_model64(refine=8):
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (FineBinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       fine_population_data)
    data = make_population_data(8, 2000, seed=3, device="cpu")
    aux = fine_population_data(data, refine=refine)
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    return (FineBinnedPopulationSMFModel(aux_data=aux64, dtype=F64),
            TorchPopulationSMFModel(aux_data=aux64, dtype=F64), data)


def test_fine_population_data_refines_the_coarse_bins():
    new, _, data = _fine_model64(refine=8)
    aux = new.aux_data
    coarse = np.asarray(data["bins"].edges)
    nb = 8 * (coarse.size - 1)
    assert new.bins.nb == nb > 32 and aux["scale"].shape == aux["target"].shape == (nb,)
    fine = aux["edges"].numpy()
    assert (fine[::8] == coarse.astype(np.float32)).all() and (np.diff(fine) > 0).all()
    np.testing.assert_allclose(aux["scale"].numpy(),
                               np.repeat(8.0 * np.asarray(data["bins"].scale), 8), rtol=1e-6)
    assert bool((aux["target"] > 0).all())
    # the target is the model's own sumstats at the truth: the loss vanishes there
    assert float(new.calc_loss_from_params(data["truth"].double())) < 1e-8


def test_fine_model_matches_the_dense_composite_model():
    new, ref, data = _fine_model64()
    guess = data["guess"].double()
    l1, g1 = new.calc_loss_and_grad_from_params(guess)
    l0, g0 = ref.calc_loss_and_grad_from_params(guess)
    assert float(g0.abs().max()) > 0
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-10)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-10,
                               atol=1e-10 * float(g0.abs().max()))


def test_jacobian_auto_mode_falls_back_to_reverse():
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (FineBinnedPopulationSMFModel,
                                                       fine_population_data)
    data = make_population_data(8, 2000, seed=3, device="cpu")
    m = FineBinnedPopulationSMFModel(aux_data=fine_population_data(data, refine=4))
    p = data["guess"]
    with pytest.raises(NotImplementedError):
        m.calc_sumstats_jacobian_from_params(p, mode="forward")
    S, J, _, used = m._sumstats_jacobian(p, mode="auto")
    assert used == "reverse"
    Sr, Jr = m.calc_sumstats_jacobian_from_params(p, mode="reverse")
    assert Jr.shape == (S.numel(), 8) and float(Jr.abs().max()) > 0
    assert torch.equal(S, Sr) and torch.equal(J, Jr)


CASES = [
    ("examples/user_model_fine.py", ["--num-halos", "3000", "--num-steps", "150"]),
    ("benchmarks/binned_fine_op.py", ["--cpu"]),
]


@pytest.mark.parametrize("script,args", CASES, ids=[c[0] for c in CASES])
def test_script_runs(tmp_path, script, args):
    env = dict(os.environ, MULTIGRAD_PROGRESS="0", OMP_NUM_THREADS="2",
               HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", MPLBACKEND="Agg")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
