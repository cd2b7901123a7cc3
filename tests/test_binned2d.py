"""gaussian_binned_sum_2d on the CPU: the torch path of the op (the formulas the HIP kernels
implement) against autograd and the plain einsum composite, the joint model that uses it, the
argument checks, and the example and benchmark scripts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(mu, sigma, edges):
    e = torch.as_tensor(edges, dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1)[:, None])
    return cdf[:, 1:] - cdf[:, :-1]


def _composite(mu_x, sigma_x, mu_y, sigma_y, edges_x, edges_y, w=None):
    px, py = _table(mu_x, sigma_x, edges_x), _table(mu_y, sigma_y, edges_y)
    if w is not None:
        px = px * w.reshape(-1)[:, None]
    return torch.einsum("ij,ik->jk", px, py)


def _inputs(n, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mu_x = 9.0 + 1.5 * torch.rand(n, generator=g, dtype=dtype)
    sigma_x = 0.1 + 0.4 * torch.rand(n, generator=g, dtype=dtype)
    mu_y = -12.5 + 3.0 * torch.rand(n, generator=g, dtype=dtype)
    sigma_y = 0.2 + 0.6 * torch.rand(n, generator=g, dtype=dtype)
    w = torch.randn(n, generator=g, dtype=dtype)
    return mu_x, sigma_x, mu_y, sigma_y, w


@pytest.mark.parametrize("sigma_x_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("sigma_y_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("w_mode", ["none", "per-object", "broadcast"])
def test_gradcheck_float64(sigma_x_mode, sigma_y_mode, w_mode):
    from multigrad_amd.ops import gaussian_binned_sum_2d
    mu_x, sigma_x, mu_y, sigma_y, w = _inputs(7)
    ex, ey = (9.2, 9.6, 9.9, 10.4), (-12.0, -11.1, -10.0)
    leaf = lambda t, mode: (t if mode == "per-object" else t[:1]).clone().requires_grad_(True)
    args = [mu_x.requires_grad_(True), leaf(sigma_x, sigma_x_mode), mu_y.requires_grad_(True),
            leaf(sigma_y, sigma_y_mode)]
    if w_mode == "none":
        f = lambda a, b, c, d: gaussian_binned_sum_2d(a, b, c, d, ex, ey)
    else:
        args.append(leaf(w, w_mode))
        f = lambda a, b, c, d, ww: gaussian_binned_sum_2d(a, b, c, d, ex, ey, ww)
    assert f(*args).shape == (3, 2)
    assert torch.autograd.gradcheck(f, tuple(args))


def test_matches_einsum_composite_chunked():
    from multigrad_amd.ops import gaussian_binned_sum_2d
    n, nbx, nby = 1000, 10, 6
    ops = _inputs(n, seed=3)
    ex, ey = np.linspace(9.0, 10.5, nbx + 1), np.linspace(-12.0, -10.0, nby + 1)
    leaves = [t.clone().requires_grad_(True) for t in ops]
    out = gaussian_binned_sum_2d(leaves[0].reshape(10, 100), *leaves[1:4], ex, ey, leaves[4],
                                 chunk=96)
    ref_leaves = [t.clone().requires_grad_(True) for t in ops]
    ref = _composite(*ref_leaves[:4], ex, ey, ref_leaves[4])
    assert out.shape == (nbx, nby)
    np.testing.assert_allclose(out.detach(), ref.detach(), rtol=0, atol=1e-12)
    G = torch.linspace(0.5, 1.5, nbx * nby, dtype=torch.float64).reshape(nbx, nby)
    got = torch.autograd.grad(out, leaves, G)
    want = torch.autograd.grad(ref, ref_leaves, G)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    # edges as a list, a numpy array or a CPU tensor give identical results
    for conv in (list, np.asarray, torch.tensor):
        again = gaussian_binned_sum_2d(*ops[:4], conv(list(ex)), conv(list(ey)), ops[4], chunk=96)
        assert torch.equal(again, out.detach())


def test_argument_errors():
    from multigrad_amd.ops import gaussian_binned_sum_2d
    mu_x, sigma_x, mu_y, sigma_y, w = _inputs(5)
    ok = [9.0, 9.5, 10.0]
    f = gaussian_binned_sum_2d
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y, sigma_y, np.linspace(0, 1, 34), ok)             # nbx = 33
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y, sigma_y, ok, np.linspace(0, 1, 34))             # nby = 33
    assert f(mu_x, sigma_x, mu_y, sigma_y, np.linspace(0, 1, 33),
             np.linspace(0, 1, 33)).shape == (32, 32)                          # 32 is allowed
    for bad in ([9.0, 9.5, 9.4, 10.0], [9.0, 9.5, 9.5]):                       # unsorted, repeated
        with pytest.raises(ValueError):
            f(mu_x, sigma_x, mu_y, sigma_y, bad, ok)
        with pytest.raises(ValueError):
            f(mu_x, sigma_x, mu_y, sigma_y, ok, bad)
    with pytest.raises(ValueError):
        f(mu_x, sigma_x[:3], mu_y, sigma_y, ok, ok)                            # wrong-length sigma_x
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y, sigma_y[:3], ok, ok)                            # wrong-length sigma_y
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y, sigma_y, ok, ok, w[:2])                         # wrong-length weights
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y[:4], sigma_y, ok, ok)                            # wrong-length mu_y
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y[:1], sigma_y, ok, ok)                            # mu_y never broadcasts
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y.float(), sigma_y, ok, ok)                        # mixed dtype
    with pytest.raises(ValueError):
        f(mu_x, sigma_x, mu_y, sigma_y, ok, ok, w.float())


def test_empty_input():
    from multigrad_amd.ops import gaussian_binned_sum_2d
    z = lambda n: torch.zeros(n, dtype=torch.float64, requires_grad=True)
    one = lambda: torch.ones(1, dtype=torch.float64, requires_grad=True)
    mu_x, mu_y, w, sigma_x, sigma_y = z(0), z(0), z(0), one(), one()
    out = gaussian_binned_sum_2d(mu_x, sigma_x, mu_y, sigma_y, [9.0, 9.5, 10.0],
                                 [-1.0, 0.0, 1.0, 2.0], w)
    assert out.shape == (2, 3) and (out == 0).all()
    g = torch.autograd.grad(out.sum(), (mu_x, sigma_x, mu_y, sigma_y, w))
    assert g[0].shape == (0,) and g[2].shape == (0,) and g[4].shape == (0,)
    assert g[1].shape == (1,) and float(g[1]) == 0.0
    assert g[3].shape == (1,) and float(g[3]) == 0.0


def test_marginal_is_the_1d_op():
    """One y bin more than 50 sigma beyond every object: Py = 1 in float64."""
    from multigrad_amd.ops import gaussian_binned_sum, gaussian_binned_sum_2d
    mu_x, sigma_x, mu_y, sigma_y, w = _inputs(500, seed=5)
    ex = np.linspace(9.0, 10.5, 11)
    ey = (float(mu_y.min()) - 60.0, float(mu_y.max()) + 60.0)
    out = gaussian_binned_sum_2d(mu_x, sigma_x, mu_y, sigma_y, ex, ey, w)
    ref = gaussian_binned_sum(mu_x, sigma_x, ex, w)
    assert out.shape == (10, 1)
    np.testing.assert_allclose(out[:, 0], ref, rtol=0, atol=1e-12)


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; "
            "assert 'multigrad_amd.ops.binned2d' not in sys.modules; "
            "f = o.gaussian_binned_sum_2d; assert 'multigrad_amd.ops.binned2d' in sys.modules; "
            "assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_joint_model_matches_plain_ndtr_model():
    from dataclasses import dataclass

    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (JointBinnedPopulationSMFModel,
                                                       joint_population_data)

    @dataclass(eq=False)
    class Plain(JointBinnedPopulationSMFModel):
        def _cells(self, mu_x, sigma_x, mu_y, sigma_y):
            return _composite(mu_x, sigma_x, mu_y, sigma_y, self.edges, self.edges_y)

    data = make_population_data(2000, 40_000, seed=11, device="cpu")
    aux = joint_population_data(data)
    assert aux["y"].shape == aux["x"].shape and len(aux["edges_y"]) == 5
    assert aux["target"].shape == (40,) and (aux["target"] > 0).all()
    new = JointBinnedPopulationSMFModel(aux_data=aux)
    ref = Plain(aux_data=aux)
    assert isinstance(new.edges_y, tuple)
    l0, g0 = ref.calc_loss_and_grad_from_params(data["guess"])
    l1, g1 = new.calc_loss_and_grad_from_params(data["guess"])
    assert g1.dtype == torch.float32 and float(g1.abs().max()) > 0
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-5)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-5)


CASES = [
    ("examples/user_model_joint.py", ["--num-halos", "3000", "--num-steps", "150"]),
    ("benchmarks/binned2d_op.py", ["--cpu"]),
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
