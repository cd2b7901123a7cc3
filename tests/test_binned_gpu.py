"""gaussian_binned_sum on the MI355X: the HIP kernels (csrc/binned.hip) against the float64
torch expression evaluated on the float32-rounded inputs, as in test_kernels_gpu.py.

Forward, per bin:   |out - ref| <= 2.2e-7 * sum_i |w_i| + 2e-5 * |ref|   (float32-erf contract)
Gradients, per element and for reduced (broadcast) gradients:
                    rtol = 2e-4, atol = 2e-5 * max |g_ref|, cotangent linspace(0.5, 1.5, nb)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(1, 1), (63, 4), (257, 5), (1023, 10), (200_003, 17), (200_003, 32)]


def _edges(nb):
    # float32-representable edges (the kernels hold them in float32)
    return tuple(float(v) for v in np.linspace(9.2, 10.4, nb + 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """float32 inputs on the host: means around the bins, widths 0.1-0.5, weights of both
    signs with exact zeros."""
    g = torch.Generator().manual_seed(seed + n)
    mu = 9.0 + 1.6 * torch.rand(n, generator=g)
    if n == 1:
        mu = torch.tensor([9.7])
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g)
    w = torch.randn(n, generator=g)
    w[::7] = 0.0
    if n == 1:
        w = torch.tensor([-1.3])
    return mu, sigma, w


def _oracle(mu, sigma, w, edges, wrt):
    """float64 bin sums and the gradients of sum_k gS_k out_k w.r.t. the tensors in ``wrt``
    (names), on the float32-rounded inputs.  sigma / w may have one element (broadcast)."""
    t = dict(mu=mu.double().clone(), sigma=sigma.double().clone(),
             w=None if w is None else w.double().clone())
    for k in wrt:
        t[k].requires_grad_(True)
    e = torch.tensor(edges, dtype=torch.float64)
    cdf = torch.special.ndtr((e[None, :] - t["mu"][:, None]) / t["sigma"].reshape(-1, 1))
    d = cdf[:, 1:] - cdf[:, :-1]
    if t["w"] is not None:
        d = d * t["w"].reshape(-1, 1)
    out = d.sum(0)
    gS = torch.linspace(0.5, 1.5, len(edges) - 1, dtype=torch.float64)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], gS) if wrt else ()
    absw = float(mu.numel()) if w is None else float(w.double().abs().sum()) * (
        mu.numel() if w.numel() == 1 and mu.numel() > 1 else 1)
    return out.detach(), dict(zip(wrt, grads)), absw


@functools.lru_cache(maxsize=None)
def _case(n, nb, sigma_mode, w_mode):
    mu, sigma, w = _inputs(n)
    sigma = sigma if sigma_mode == "per-object" else sigma[:1].clone()
    w = None if w_mode == "none" else w
    wrt = ("mu", "sigma") + (() if w is None else ("w",))
    return (mu, sigma, w), _oracle(mu, sigma, w, _edges(nb), wrt)


def _run(mu, sigma, w, edges, wrt):
    from multigrad_amd.ops import gaussian_binned_sum
    t = dict(mu=mu, sigma=sigma, w=w)
    for k in wrt:
        t[k] = t[k].detach().requires_grad_(True)
    out = gaussian_binned_sum(t["mu"], t["sigma"], edges, t["w"])
    gS = torch.linspace(0.5, 1.5, len(edges) - 1, dtype=torch.float64).to(out)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], gS) if wrt else ()
    return out.detach(), dict(zip(wrt, grads))


def _check(out, grads, ref, gref, absw):
    out = out.cpu().double().numpy()
    ref = ref.numpy()
    assert np.isfinite(out).all()
    err = np.abs(out - ref)
    tol = 2.2e-7 * absw + 2e-5 * np.abs(ref)
    print("forward err/tol", float((err / tol).max()))
    assert (err <= tol).all(), (err, tol)
    for k, g in grads.items():
        g = g.cpu().double().numpy().reshape(-1)
        r = gref[k].numpy().reshape(-1)
        assert g.shape == r.shape and np.isfinite(g).all()
        atol = 2e-5 * float(np.abs(r).max())
        print(k, "grad err/tol", float((np.abs(g - r) / (atol + 2e-4 * np.abs(r))).max()))
        np.testing.assert_allclose(g, r, rtol=2e-4, atol=atol, err_msg=k)


@pytest.mark.parametrize("w_mode", ["none", "per-object"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_forward_and_gradients_match_fp64(n, nb, sigma_mode, w_mode):
    (mu, sigma, w), (ref, gref, absw) = _case(n, nb, sigma_mode, w_mode)
    dev = [None if t is None else t.to(DEV) for t in (mu, sigma, w)]
    out, grads = _run(*dev, _edges(nb), tuple(gref))
    assert out.shape == (nb,) and out.dtype == torch.float32 and out.is_cuda
    _check(out, grads, ref, gref, absw)


def test_broadcast_weights():
    mu, sigma, w = _inputs(1023)
    w1 = torch.tensor([-0.7])
    edges = _edges(10)
    ref, gref, absw = _oracle(mu, sigma, w1, edges, ("mu", "sigma", "w"))
    out, grads = _run(mu.to(DEV), sigma.to(DEV), w1.to(DEV), edges, ("mu", "sigma", "w"))
    assert grads["w"].shape == (1,)
    _check(out, grads, ref, gref, absw)
    # both operands broadcast: two reduced gradients from one pass
    ref, gref, absw = _oracle(mu, sigma[:1], w1, edges, ("sigma", "w"))
    out, grads = _run(mu.to(DEV), sigma[:1].to(DEV), w1.to(DEV), edges, ("sigma", "w"))
    _check(out, grads, ref, gref, absw)


def test_edge_inputs_stay_finite_and_accurate():
    n, nb = 1023, 10
    edges = _edges(nb)
    mu, sigma, w = (t.clone() for t in _inputs(n))
    sigma[:200] = 1e-3                       # step functions
    mu[0] = edges[3]                         # exactly on an edge (a step function)
    mu[300] = edges[5]                       # exactly on an edge, ordinary width
    mu[400:420] = edges[0] - 50.0 * sigma[400:420]     # 50 sigma below every edge
    mu[420:440] = edges[-1] + 50.0 * sigma[420:440]    # 50 sigma above every edge
    w[[0, 300, 400, 420]] = 1.0
    wrt = ("mu", "sigma", "w")
    ref, gref, absw = _oracle(mu, sigma, w, edges, wrt)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), w.to(DEV), edges, wrt)
    _check(out, grads, ref, gref, absw)


@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout):
    n, nb = 1023, 10
    edges = _edges(nb)
    mu, sigma, w = _inputs(n)
    ref, gref, absw = _oracle(mu, sigma, w, edges, ("mu", "sigma", "w"))
    if layout == "offset":                   # a 4-byte-offset pointer: scalar loads
        buf = torch.zeros(n + 1, device=DEV)
        buf[1:] = mu.to(DEV)
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
    else:                                    # non-contiguous
        buf = torch.zeros(2 * n, device=DEV)
        buf[::2] = mu.to(DEV)
        view = buf[::2]
        assert not view.is_contiguous()
    out, grads = _run(view, sigma.to(DEV), w.to(DEV), edges, ("mu", "sigma", "w"))
    _check(out, grads, ref, gref, absw)
    # the same values from an aligned contiguous tensor: same bits (the load path does not
    # change the arithmetic)
    out2, grads2 = _run(mu.to(DEV), sigma.to(DEV), w.to(DEV), edges, ("mu", "sigma", "w"))
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize("wrt", [("mu",), ("sigma",), ("w",), ("mu", "w"), ("sigma", "w")])
def test_gradient_subsets(wrt):
    n, nb = 1023, 10
    edges = _edges(nb)
    mu, sigma, w = _inputs(n)
    ref, gref, absw = _oracle(mu, sigma, w, edges, wrt)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), w.to(DEV), edges, wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, ref, gref, absw)


def test_bitwise_deterministic():
    n, nb = 200_003, 17
    mu, sigma, w = (t.to(DEV) for t in _inputs(n))
    wrt = ("mu", "sigma", "w")
    a = _run(mu, sigma[:1].clone(), w, _edges(nb), wrt)
    b = _run(mu, sigma[:1].clone(), w, _edges(nb), wrt)
    assert torch.equal(a[0], b[0])
    for k in wrt:
        assert torch.equal(a[1][k], b[1][k]), k


def test_float64_device_input_takes_torch_path():
    from multigrad_amd.ops import gaussian_binned_sum
    n, nb = 1023, 10
    edges = _edges(nb)
    mu, sigma, w = _inputs(n)
    ref, gref, _ = _oracle(mu, sigma, w, edges, ("mu", "sigma", "w"))
    leaves = [t.double().to(DEV).requires_grad_(True) for t in (mu, sigma, w)]
    out = gaussian_binned_sum(leaves[0], leaves[1], edges, leaves[2])
    assert out.dtype == torch.float64 and out.is_cuda
    gS = torch.linspace(0.5, 1.5, nb, dtype=torch.float64, device=DEV)
    grads = torch.autograd.grad(out, leaves, gS)
    np.testing.assert_allclose(out.detach().cpu(), ref, rtol=0, atol=1e-12)
    for g, k in zip(grads, ("mu", "sigma", "w")):
        np.testing.assert_allclose(g.cpu(), gref[k], rtol=0, atol=1e-12)


def test_device_edges_raise():
    from multigrad_amd.ops import gaussian_binned_sum
    mu, sigma, _ = (t.to(DEV) for t in _inputs(63))
    with pytest.raises(TypeError, match="setup"):
        gaussian_binned_sum(mu, sigma, torch.tensor(_edges(4), device=DEV))


def test_captured_engine_matches_eager_and_fp64_model():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    guess = data["guess"]
    m = BinnedPopulationSMFModel(aux_data=aux)
    ref = m.run_adam(guess, nsteps=6, learning_rate=1e-3, use_engine=False)
    eng = GraphAdamEngine(m, graph=True)
    traj = eng.run_adam(guess, nsteps=6, learning_rate=1e-3)
    assert eng.use_graph and eng.graph is not None and eng.fallback_reason is None, \
        eng.fallback_reason
    torch.testing.assert_close(traj, ref, rtol=1e-5, atol=1e-6)

    # float64 torch model on the same float32-rounded data and parameters
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    m64 = TorchPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    p64 = guess.double()
    loss64, grad64 = m64.calc_loss_and_grad_from_params(p64)
    loss, grad = m.calc_loss_and_grad_from_params(guess)
    S64 = m64.calc_sumstats_from_params(p64)
    S = m.calc_sumstats_from_params(guess)
    scale = aux64["scale"]
    nhalo = aux["x"].numel()
    # forward contract on the bin sums (weights 1: sum |w| = number of halos), in S units
    tolS = (2.2e-7 * nhalo + 2e-5 * (S64 / scale).abs()) * scale
    errS = (S.double() - S64).abs()
    print("sumstats err/tol", float((errS / tolS).max()))
    assert (errS <= tolS).all(), (errS, tolS)
    # the loss: the forward tolerance pushed through dL/dS (first order), plus 1e-5 relative
    # for evaluating log10 / mean of the loss itself in float32 (a few 1e-7 relative per op
    # on |log10 S| ~ 2-4 against differences of ~0.1)
    dLdS = m64.calc_dloss_dsumstats(S64)
    tolL = float((dLdS.abs() * tolS).sum()) + 1e-5 * abs(float(loss64))
    print("loss err/tol", abs(float(loss) - float(loss64)) / tolL)
    assert abs(float(loss) - float(loss64)) <= tolL
    g64 = grad64.cpu().numpy()
    np.testing.assert_allclose(grad.cpu().double().numpy(), g64, rtol=2e-4,
                               atol=2e-5 * float(np.abs(g64).max()))
