"""Second-order autograd of gaussian_binned_sum on the CPU (the torch path of the second
backward, whose formulas the HIP kernel of csrc/binned_hvp.hip implements) and the
model-level Hessian products ``OnePointModel.calc_hvp_from_params`` /
``calc_hessian_from_params``: against torch's own double backward of the ndtr expression,
against the plain-torch population model, on several gloo ranks, for degenerate models, and
the example script."""
import os
import subprocess
import sys
from dataclasses import dataclass

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distributed import run_distributed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _composite(mu, sigma, edges, w=None):
    e = torch.as_tensor(edges, dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1)[:, None])
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1)[:, None]
    return d.sum(0)


def _inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    mu = 9.0 + 1.5 * torch.rand(n, generator=g, dtype=F64)
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g, dtype=F64)
    w = torch.randn(n, generator=g, dtype=F64)
    return mu, sigma, w


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("w_mode", ["none", "per-object", "broadcast"])
def test_gradgradcheck_float64(sigma_mode, w_mode):
    from multigrad_amd.ops import gaussian_binned_sum
    mu, sigma, w = _inputs(7)
    edges = (9.2, 9.6, 9.9, 10.4)
    mu.requires_grad_(True)
    sigma = (sigma if sigma_mode == "per-object" else sigma[:1]).clone().requires_grad_(True)
    if w_mode == "none":
        assert torch.autograd.gradgradcheck(lambda m, s: gaussian_binned_sum(m, s, edges),
                                            (mu, sigma))
    else:
        w = (w if w_mode == "per-object" else w[:1]).clone().requires_grad_(True)
        assert torch.autograd.gradgradcheck(lambda m, s, ww: gaussian_binned_sum(m, s, edges, ww),
                                            (mu, sigma, w))


def _second_order(fn, leaves, g, cots):
    """Gradients of sum_i (a_i dmu_i + b_i dsigma_i + c_i dw_i) w.r.t. (mu, sigma, w, g); a
    cotangent that is None leaves its first-order gradient out of the scalar."""
    out = fn(*leaves)
    first = torch.autograd.grad(out, leaves, g, create_graph=True)
    pairs = [(f, c) for f, c in zip(first, cots) if c is not None]
    return torch.autograd.grad([f for f, _ in pairs], leaves + [g], [c for _, c in pairs],
                               allow_unused=True)


# (sigma mode, weights mode, cotangents left out): without weights there is no c
SECOND_ORDER = [(s, w, d) for s, w in (("per-object", "per-object"), ("broadcast", "broadcast"),
                                       ("per-object", "none"))
                for d in ("", "a", "b", "c", "ab", "bc") if not (w == "none" and "c" in d)]


@pytest.mark.parametrize("sigma_mode,w_mode,drop", SECOND_ORDER)
def test_second_order_matches_ndtr_composite(sigma_mode, w_mode, drop):
    from multigrad_amd.ops import gaussian_binned_sum
    n, nb = 1000, 10
    mu, sigma, w = _inputs(n, seed=3)
    sigma = sigma if sigma_mode == "per-object" else sigma[:1]
    ops = [mu, sigma] + ([] if w_mode == "none" else [w if w_mode == "per-object" else w[:1]])
    edges = np.linspace(9.0, 10.5, nb + 1)
    gen = torch.Generator().manual_seed(5)
    cots = [torch.randn(t.shape, generator=gen, dtype=F64) for t in ops]
    for k, name in enumerate("abc"[:len(ops)]):
        if name in drop:
            cots[k] = None
    got, want = [], []
    for res, fn in ((got, lambda m, s, ww=None: gaussian_binned_sum(m, s, edges, ww, chunk=64)),
                    (want, lambda m, s, ww=None: _composite(m, s, edges, ww))):
        leaves = [t.clone().requires_grad_(True) for t in ops]
        g = torch.linspace(0.5, 1.5, nb, dtype=F64).requires_grad_(True)
        res.extend(_second_order(fn, leaves, g, cots))
    assert len(got) == len(ops) + 1
    for name, a, b in zip(("mu", "sigma", "w", "g") if len(ops) == 3 else ("mu", "sigma", "g"),
                          got, want):
        if b is None:   # the scalar does not depend on it (w with only c given): None or zeros
            assert a is None or not a.any(), name
        else:
            assert a.shape == b.shape, name
            np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * float(b.abs().max()),
                                       err_msg=name)


def test_functional_hessian_and_third_order():
    from multigrad_amd.ops import gaussian_binned_sum
    mu, sigma, w = _inputs(5, seed=2)
    edges = (9.2, 9.6, 9.9, 10.4)
    gS = torch.tensor([0.5, 1.0, 1.5], dtype=F64)

    def scalar(fn):
        return lambda m, s: (fn(m, s) ** 2 * gS).sum()

    got = torch.autograd.functional.hessian(
        scalar(lambda m, s: gaussian_binned_sum(m, s, edges, w)), (mu, sigma))
    want = torch.autograd.functional.hessian(
        scalar(lambda m, s: _composite(m, s, edges, w)), (mu, sigma))
    for i in range(2):
        for j in range(2):
            np.testing.assert_allclose(got[i][j], want[i][j], rtol=1e-9, atol=1e-12)
    # third order is out of scope: torch's error for a once-differentiable backward
    m = mu.clone().requires_grad_(True)
    out = gaussian_binned_sum(m, sigma, edges, w)
    (g1,) = torch.autograd.grad(out.sum(), m, create_graph=True)
    (g2,) = torch.autograd.grad((g1 * g1).sum(), m, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g2.sum().backward()
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g2.sum(), m)
    # with a constant cotangent the second-order result carries no graph at all
    (g2,) = torch.autograd.grad(g1.sum(), m, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g2.sum(), m)


def test_empty_input_and_first_order_unchanged():
    from multigrad_amd.ops import gaussian_binned_sum
    e_mu = torch.zeros(0, dtype=F64, requires_grad=True)
    e_sig = torch.ones(1, dtype=F64, requires_grad=True)
    out = gaussian_binned_sum(e_mu, e_sig, [9.0, 9.5, 10.0])
    gm, gs = torch.autograd.grad(out.sum(), (e_mu, e_sig), create_graph=True)
    (hs,) = torch.autograd.grad(gs.sum(), e_sig, allow_unused=True)
    assert gm.shape == (0,) and (hs is None or float(hs) == 0.0)
    # create_graph does not change the first-order values
    mu, sigma, w = (t.requires_grad_(True) for t in _inputs(300, seed=4))
    edges = np.linspace(9.0, 10.5, 6)
    a = torch.autograd.grad(gaussian_binned_sum(mu, sigma, edges, w).sum(), (mu, sigma, w))
    b = torch.autograd.grad(gaussian_binned_sum(mu, sigma, edges, w).sum(), (mu, sigma, w),
                            create_graph=True)
    assert all(torch.equal(x, y.detach()) for x, y in zip(a, b))


# ---------------------------------------------------------------------------- models
def _population_aux(nparam=12, nhalo=900, seed=11):
    """Float64 aux data of the whole catalog (a one-process communicator, whatever the world
    is) of the population model, built as
    test_binned.py::test_binned_population_model_matches_torch_model does."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import torch_population_data
    from multigrad_amd.parallel.comm import SerialComm
    data = make_population_data(nparam, nhalo, seed=seed, device="cpu", comm=SerialComm())
    PopulationSMFModel(aux_data=data, comm=SerialComm()).set_target_from_truth()
    aux = torch_population_data(data)
    aux = {k: v.double() if torch.is_tensor(v) and v.is_floating_point() else v
           for k, v in aux.items()}
    return aux, data["guess"].double()


def _shard(aux, rank, size):
    idx = torch.from_numpy(np.array_split(np.arange(aux["x"].numel()), size)[rank])
    return dict(aux, x=aux["x"][idx], pop=aux["pop"][idx])


def _torch_hessian(aux, guess):
    from multigrad_amd.models.torch_population import TorchPopulationSMFModel
    ref = TorchPopulationSMFModel(aux_data=aux, dtype=F64)

    def full_loss(p):
        return ref.calc_loss_from_sumstats(ref.calc_partial_sumstats_from_params(p))

    return torch.autograd.functional.hessian(full_loss, guess)


@pytest.mark.parametrize("kind", ["binned", "grouped"])
def test_hessian_matches_plain_torch_model(kind):
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       GroupedBinnedPopulationSMFModel)
    aux, guess = _population_aux()
    H_ref = _torch_hessian(aux, guess)
    cls = BinnedPopulationSMFModel if kind == "binned" else GroupedBinnedPopulationSMFModel
    model = cls(aux_data=aux, dtype=F64)
    H = model.calc_hessian_from_params(guess)
    assert H.shape == (guess.numel(), guess.numel()) and H.dtype == F64
    assert torch.equal(H, H.T)
    scale = float(H_ref.abs().max())
    np.testing.assert_allclose(H, H_ref, rtol=1e-9, atol=1e-11 * scale)
    v = torch.randn(guess.numel(), generator=torch.Generator().manual_seed(1), dtype=F64)
    np.testing.assert_allclose(model.calc_hvp_from_params(guess, v), H_ref @ v, rtol=1e-9,
                               atol=1e-11 * scale * float(v.abs().sum()))


def _ranks_hvp(rank, size):
    from multigrad_amd.models.torch_population import GroupedBinnedPopulationSMFModel
    aux, guess = _population_aux()
    model = GroupedBinnedPopulationSMFModel(aux_data=_shard(aux, rank, size), dtype=F64)
    v = torch.randn(guess.numel(), generator=torch.Generator().manual_seed(1), dtype=F64)
    return model.calc_hvp_from_params(guess, v).numpy()


@pytest.mark.parametrize("size", [2, 3])
def test_hvp_on_several_ranks_matches_one_rank(size):
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    one = _ranks_hvp(0, 1)
    res = run_distributed(_ranks_hvp, size)
    for r in res:
        assert np.array_equal(r, res[0])      # identical on all ranks
    assert np.abs(res[0] - one).max() <= 1e-10 * np.abs(one).max()


def _toy_models():
    import multigrad_amd as mg
    from multigrad_amd.ops import gaussian_binned_sum
    x = 9.0 + 1.5 * torch.rand(200, generator=torch.Generator().manual_seed(7), dtype=F64)
    edges = (9.2, 9.6, 9.9, 10.4)
    coef = torch.tensor([0.3, -1.2, 2.0], dtype=F64)
    A = torch.randn(3, 4, generator=torch.Generator().manual_seed(8), dtype=F64)

    @dataclass(eq=False)
    class LinearLoss(mg.OnePointModel):       # the loss is linear in the sumstats
        def calc_partial_sumstats_from_params(self, params, randkey=None):
            return gaussian_binned_sum(x + params[0], torch.exp(params[1]).reshape(1), edges)

        def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
            return (coef * sumstats).sum()

    @dataclass(eq=False)
    class LinearSumstats(mg.OnePointModel):   # the sumstats are linear in the parameters
        def calc_partial_sumstats_from_params(self, params, randkey=None):
            return A @ params

        def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
            return (sumstats ** 3).sum()

    @dataclass(eq=False)
    class BothLinear(LinearSumstats):
        def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
            return (coef * sumstats).sum()

    kw = dict(device="cpu", dtype=F64)
    return LinearLoss(**kw), LinearSumstats(**kw), BothLinear(**kw), A


def test_degenerate_models():
    lin_loss, lin_stats, both, A = _toy_models()
    p2 = torch.tensor([0.1, -1.0], dtype=F64)
    H = lin_loss.calc_hessian_from_params(p2)
    ref = torch.autograd.functional.hessian(
        lambda p: lin_loss.calc_loss_from_sumstats(lin_loss.calc_partial_sumstats_from_params(p)),
        p2)
    assert float(ref.abs().max()) > 0
    np.testing.assert_allclose(H, ref, rtol=1e-9, atol=1e-12)
    p4 = torch.tensor([0.5, -0.3, 0.2, 1.1], dtype=F64)
    H = lin_stats.calc_hessian_from_params(p4)
    ref = A.T @ torch.diag(6.0 * (A @ p4)) @ A
    np.testing.assert_allclose(H, ref, rtol=1e-12, atol=1e-12)
    v = torch.ones(4, dtype=F64)
    hv = both.calc_hvp_from_params(p4, v)
    assert hv.shape == (4,) and float(hv.abs().max()) == 0.0


SCRIPTS = [
    ("examples/user_model_errors.py", ["--num-pops", "3", "--num-halos", "3000", "--num-steps",
                                       "40"], "1-sigma"),
    ("benchmarks/binned_hvp.py", ["--cpu"], '"speedup"'),
]


@pytest.mark.parametrize("script,args,expect", SCRIPTS, ids=[c[0] for c in SCRIPTS])
def test_script_runs(tmp_path, script, args, expect):
    env = dict(os.environ, MULTIGRAD_PROGRESS="0", OMP_NUM_THREADS="2",
               HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", MPLBACKEND="Agg")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert expect in r.stdout
