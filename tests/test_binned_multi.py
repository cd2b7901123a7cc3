"""gaussian_binned_sum_multi on the CPU: the torch path of the op (the formulas the HIP
kernels implement) against the single op channel by channel and against autograd, the
conditional model that uses it, the argument checks, and the example and benchmark scripts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("none", "per-object", "one-element", "positive")


def _inputs(n, C, seed=0, dtype=torch.float64):
    """mu, sigma and C weights whose kinds cycle over None, per-object (both signs),
    one-element and per-object positive."""
    g = torch.Generator().manual_seed(seed)
    mu = 9.0 + 1.5 * torch.rand(n, generator=g, dtype=dtype)
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g, dtype=dtype)
    ws = []
    for c in range(C):
        kind = KINDS[c % 4]
        if kind == "none":
            ws.append(None)
        elif kind == "per-object":
            ws.append(torch.randn(n, generator=g, dtype=dtype))
        elif kind == "one-element":
            ws.append(torch.tensor([-0.7 - 0.1 * c], dtype=dtype))
        else:
            ws.append(0.5 + torch.rand(n, generator=g, dtype=dtype))
    return mu, sigma, ws


def _leaf(t):
    return None if t is None else t.clone().requires_grad_(True)


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("C", [1, 2, 3, 5, 8])
def test_rows_and_gradients_match_the_single_op(C, sigma_mode):
    from multigrad_amd.ops import gaussian_binned_sum, gaussian_binned_sum_multi
    n, nb = 300, 6
    edges = np.linspace(9.1, 10.4, nb + 1)
    mu, sigma, ws = _inputs(n, C, seed=C)
    sigma = sigma if sigma_mode == "per-object" else sigma[:1]
    G = torch.linspace(0.5, 1.5, C * nb, dtype=torch.float64).reshape(C, nb)

    a = [_leaf(mu), _leaf(sigma)] + [_leaf(w) for w in ws]
    out = gaussian_binned_sum_multi(a[0].reshape(3, 100), a[1], edges, a[2:])
    assert out.shape == (C, nb) and out.dtype == torch.float64
    leaves = [t for t in a if t is not None]
    got = torch.autograd.grad(out, leaves, G)

    b = [_leaf(mu), _leaf(sigma)] + [_leaf(w) for w in ws]
    rows = torch.stack([gaussian_binned_sum(b[0], b[1], edges, b[2 + c]) for c in range(C)])
    want = torch.autograd.grad(rows, [t for t in b if t is not None], G)

    np.testing.assert_allclose(out.detach(), rows.detach(), rtol=0, atol=1e-12)
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert x.shape == y.shape
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)
    # a tuple of weights and edges given as a list or a CPU tensor: identical results
    for conv in (list, torch.tensor):
        again = gaussian_binned_sum_multi(mu, sigma, conv(list(edges)), tuple(ws))
        assert torch.equal(again, out.detach())


def test_gradcheck_float64():
    from multigrad_amd.ops import gaussian_binned_sum_multi
    mu, sigma, ws = _inputs(7, 3, seed=1)
    edges = (9.2, 9.6, 9.9, 10.4)
    w1, w2 = ws[1], ws[2]
    for sig in (sigma, sigma[:1]):
        args = tuple(t.clone().requires_grad_(True) for t in (mu, sig, w1, w2))
        f = lambda m, s, u, v: gaussian_binned_sum_multi(m, s, edges, [None, u, v])
        assert f(*args).shape == (3, 3)
        assert torch.autograd.gradcheck(f, args)


def test_repeated_tensor_gets_the_summed_gradient():
    from multigrad_amd.ops import gaussian_binned_sum_multi
    mu, sigma, ws = _inputs(50, 2, seed=2)
    edges = np.linspace(9.1, 10.4, 5)
    G = torch.tensor([[1.0, 2.0, 3.0, 4.0], [-0.5, 0.25, 2.0, 1.5]], dtype=torch.float64)
    w = ws[1].clone().requires_grad_(True)
    out = gaussian_binned_sum_multi(mu, sigma, edges, [w, w])
    (both,) = torch.autograd.grad(out, w, G)
    u, v = ws[1].clone().requires_grad_(True), ws[1].clone().requires_grad_(True)
    gu, gv = torch.autograd.grad(gaussian_binned_sum_multi(mu, sigma, edges, [u, v]), (u, v), G)
    assert float(gu.abs().max()) > 0 and float(gv.abs().max()) > 0
    np.testing.assert_allclose(both, gu + gv, rtol=0, atol=1e-13)


def test_chunk_independence():
    from multigrad_amd.ops import gaussian_binned_sum_multi
    mu, sigma, ws = _inputs(23, 4, seed=3)
    edges = np.linspace(9.1, 10.4, 4)
    G = torch.linspace(0.5, 1.5, 12, dtype=torch.float64).reshape(4, 3)
    res = []
    for chunk in (5, None):
        a = [_leaf(mu), _leaf(sigma[:1])] + [_leaf(w) for w in ws]
        out = gaussian_binned_sum_multi(a[0], a[1], edges, a[2:], chunk=chunk)
        res.append([out.detach()] + list(torch.autograd.grad(out, [t for t in a if t is not None],
                                                              G)))
    for x, y in zip(*res):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)


def test_argument_errors():
    from multigrad_amd.ops import gaussian_binned_sum_multi as f
    from multigrad_amd.ops.binned_multi import MAX_CHANNELS
    assert MAX_CHANNELS == 8
    mu, sigma, ws = _inputs(5, 2)
    w = ws[1]
    ok = [9.0, 9.5, 10.0]
    with pytest.raises(ValueError, match="weights"):
        f(mu, sigma, ok, w)                                   # a bare tensor
    with pytest.raises(ValueError, match="weights"):
        f(mu, sigma, ok, torch.stack([w, w], dim=1))          # an [N, C] tensor
    with pytest.raises(ValueError, match="weights"):
        f(mu, sigma, ok, [])                                  # C = 0
    with pytest.raises(ValueError, match="weights"):
        f(mu, sigma, ok, [None] * 9)                          # C = 9
    assert f(mu, sigma, ok, [None] * 8).shape == (8, 2)       # 8 is allowed
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        f(mu, sigma, ok, [None, w[:3]])                       # wrong element count
    with pytest.raises(ValueError, match=r"weights\[0\]"):
        f(mu, sigma, ok, [w.float(), None])                   # wrong dtype
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        f(mu, sigma, ok, [w, w.to("meta")])                   # wrong device
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        f(mu, sigma, ok, [w, 2.0])                            # not a tensor
    with pytest.raises(ValueError, match="sigma"):
        f(mu, sigma[:3], ok, [None, w])
    with pytest.raises(ValueError, match="sigma"):
        f(mu, sigma.float(), ok, [None, w])
    with pytest.raises(ValueError):
        f(mu, sigma, np.linspace(0, 1, 34), [None, w])        # nb = 33
    assert f(mu, sigma, np.linspace(0, 1, 33), [None, w]).shape == (2, 32)
    for bad in ([9.0, 9.5, 9.4, 10.0], [9.0, 9.5, 9.5], [9.0, float("inf")]):
        with pytest.raises(ValueError):
            f(mu, sigma, bad, [None, w])
    with pytest.raises(TypeError, match="setup"):
        f(mu, sigma, torch.tensor(ok, device="meta"), [None, w])   # device edges
    with pytest.raises(TypeError):
        f(mu.numpy(), sigma, ok, [None, w])


def test_empty_input():
    from multigrad_amd.ops import gaussian_binned_sum_multi
    z = lambda n: torch.zeros(n, dtype=torch.float64, requires_grad=True)
    one = lambda: torch.ones(1, dtype=torch.float64, requires_grad=True)
    mu, sigma, w, wb = z(0), one(), z(0), one()
    out = gaussian_binned_sum_multi(mu, sigma, [9.0, 9.5, 10.0], [None, w, wb])
    assert out.shape == (3, 2) and (out == 0).all()
    g = torch.autograd.grad(out.sum(), (mu, sigma, w, wb))
    assert g[0].shape == (0,) and g[2].shape == (0,)
    assert g[1].shape == (1,) and float(g[1]) == 0.0
    assert g[3].shape == (1,) and float(g[3]) == 0.0


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; "
            "assert 'multigrad_amd.ops.binned_multi' not in sys.modules; "
            "f = o.gaussian_binned_sum_multi; "
            "assert 'multigrad_amd.ops.binned_multi' in sys.modules; "
            "assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_conditional_model_matches_three_single_op_calls():
    from dataclasses import dataclass

    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (ConditionalBinnedPopulationSMFModel,
                                                       conditional_population_data)
    from multigrad_amd.ops import gaussian_binned_sum

    @dataclass(eq=False)
    class ThreeCalls(ConditionalBinnedPopulationSMFModel):
        def _sums(self, mu, sigma, weights):
            return torch.stack([gaussian_binned_sum(mu, sigma, self.edges, w) for w in weights])

    data = make_population_data(2000, 40_000, seed=11, device="cpu")
    aux = conditional_population_data(data)
    nb = aux["edges"].numel() - 1
    assert aux["y"].shape == aux["x"].shape
    assert float(aux["y"].min()) >= 0.5 and float(aux["y"].max()) <= 1.5
    assert aux["target"].shape == (3 * nb,) and (aux["target"] > 0).all()
    assert aux["scale"].shape == (3 * nb,)
    new = ConditionalBinnedPopulationSMFModel(aux_data=aux)
    ref = ThreeCalls(aux_data=aux)
    l0, g0 = ref.calc_loss_and_grad_from_params(data["guess"])
    l1, g1 = new.calc_loss_and_grad_from_params(data["guess"])
    assert g1.dtype == torch.float32 and float(g1.abs().max()) > 0
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-5)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-5)


CASES = [
    ("examples/user_model_conditional.py", ["--num-halos", "3000", "--num-steps", "150"]),
    ("benchmarks/binned_multi_op.py", ["--cpu"]),
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
