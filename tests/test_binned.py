"""gaussian_binned_sum on the CPU: the torch path of the op (the formulas the HIP kernels
implement) against autograd and the plain ndtr expression, the model that uses it, the
argument checks, and the example and benchmark scripts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _composite(mu, sigma, edges, w=None):
    e = torch.as_tensor(edges, dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1)[:, None])
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1)[:, None]
    return d.sum(0)


def _inputs(n, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mu = 9.0 + 1.5 * torch.rand(n, generator=g, dtype=dtype)
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g, dtype=dtype)
    w = torch.randn(n, generator=g, dtype=dtype)
    return mu, sigma, w


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("w_mode", ["none", "per-object", "broadcast"])
def test_gradcheck_float64(sigma_mode, w_mode):
    from multigrad_amd.ops import gaussian_binned_sum
    mu, sigma, w = _inputs(7)
    edges = (9.2, 9.6, 9.9, 10.4)
    mu.requires_grad_(True)
    sigma = (sigma if sigma_mode == "per-object" else sigma[:1]).clone().requires_grad_(True)
    if w_mode == "none":
        assert torch.autograd.gradcheck(lambda m, s: gaussian_binned_sum(m, s, edges), (mu, sigma))
    else:
        w = (w if w_mode == "per-object" else w[:1]).clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda m, s, ww: gaussian_binned_sum(m, s, edges, ww),
                                        (mu, sigma, w))


def test_matches_ndtr_expression_chunked():
    from multigrad_amd.ops import gaussian_binned_sum
    n, nb = 1000, 10
    mu, sigma, w = _inputs(n, seed=3)
    edges = np.linspace(9.0, 10.5, nb + 1)
    leaves = [t.clone().requires_grad_(True) for t in (mu, sigma, w)]
    out = gaussian_binned_sum(leaves[0].reshape(10, 100), leaves[1], edges, leaves[2], chunk=96)
    ref_leaves = [t.clone().requires_grad_(True) for t in (mu, sigma, w)]
    ref = _composite(*ref_leaves[:2], edges, ref_leaves[2])
    assert out.shape == (nb,)
    np.testing.assert_allclose(out.detach(), ref.detach(), rtol=0, atol=1e-12)
    gS = torch.linspace(0.5, 1.5, nb, dtype=torch.float64)
    got = torch.autograd.grad(out, leaves, gS)
    want = torch.autograd.grad(ref, ref_leaves, gS)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    # edges as a CPU tensor and as a list give the same result
    again = gaussian_binned_sum(mu, sigma, torch.tensor(edges), w, chunk=96)
    assert torch.equal(again, out.detach())


def test_binned_population_model_matches_torch_model():
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(2000, 40_000, seed=11, device="cpu")
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    ref = TorchPopulationSMFModel(aux_data=aux)
    new = BinnedPopulationSMFModel(aux_data=aux)
    assert isinstance(new.edges, tuple) and len(new.edges) == 11
    l0, g0 = ref.calc_loss_and_grad_from_params(data["guess"])
    l1, g1 = new.calc_loss_and_grad_from_params(data["guess"])
    assert g1.dtype == torch.float32
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-5)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-5)


def test_argument_errors_and_empty_input():
    from multigrad_amd.ops import gaussian_binned_sum
    mu, sigma, w = _inputs(5)
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma, np.linspace(0, 1, 35))          # nb = 34 > 32
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma, np.linspace(0, 1, 34))          # nb = 33
    gaussian_binned_sum(mu, sigma, np.linspace(0, 1, 33))              # nb = 32 is allowed
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma, [9.0, 9.5, 9.4, 10.0])          # unsorted
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma, [9.0, 9.5, 9.5])                # not strictly increasing
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma[:3], [9.0, 9.5])                 # wrong-length sigma
    with pytest.raises(ValueError):
        gaussian_binned_sum(mu, sigma, [9.0, 9.5], w[:2])              # wrong-length weights
    e_mu = torch.zeros(0, dtype=torch.float64, requires_grad=True)
    e_sig = torch.ones(1, dtype=torch.float64, requires_grad=True)
    e_w = torch.zeros(0, dtype=torch.float64, requires_grad=True)
    out = gaussian_binned_sum(e_mu, e_sig, [9.0, 9.5, 10.0], e_w)
    assert out.shape == (2,) and (out == 0).all()
    gm, gs, gw = torch.autograd.grad(out.sum(), (e_mu, e_sig, e_w))
    assert gm.shape == (0,) and gw.shape == (0,) and gs.shape == (1,) and float(gs) == 0.0


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; assert 'multigrad_amd.ops.binned' not in sys.modules; "
            "f = o.gaussian_binned_sum; assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


CASES = [
    ("examples/user_model_binned.py", ["--num-halos", "3000", "--num-steps", "150"]),
    ("benchmarks/binned_op.py", ["--cpu"]),
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
