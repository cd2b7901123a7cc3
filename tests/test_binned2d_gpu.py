"""gaussian_binned_sum_2d on the MI355X: the HIP kernels (csrc/binned2d.hip) against the float64
torch expression (einsum of the two probability tables, never N x nbx x nby) evaluated on the
float32-rounded inputs.

Forward, per cell:  |out - ref| <= 4.4e-7 * sum_i |w_i| + 2e-5 * |ref|
                    (each factor of a cell carries the 1-D bin error 2.2e-7 and lies in [0, 1])
Gradients, per element and for reduced (broadcast) gradients:
                    rtol = 2e-4, atol = 2e-5 * max |g_ref|,
                    cotangent linspace(0.5, 1.5, nbx * nby).reshape(nbx, nby)
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(1, 1, 1), (63, 4, 5), (257, 5, 32), (1023, 32, 32), (1025, 10, 3), (200_003, 17, 9),
          (200_003, 32, 32)]
NAMES = ("mu_x", "sigma_x", "mu_y", "sigma_y", "w")


def _edges(nbx, nby):
    # float32-representable edges (the kernels hold them in float32)
    ex = tuple(float(v) for v in np.linspace(9.2, 10.4, nbx + 1).astype(np.float32))
    ey = tuple(float(v) for v in np.linspace(-12.0, -10.0, nby + 1).astype(np.float32))
    return ex, ey


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """float32 inputs on the host: means around the grid, widths 0.1-0.5 and 0.2-0.8, weights of
    both signs with exact zeros."""
    g = torch.Generator().manual_seed(seed + n)
    t = dict(mu_x=9.0 + 1.6 * torch.rand(n, generator=g),
             sigma_x=0.1 + 0.4 * torch.rand(n, generator=g),
             mu_y=-12.5 + 3.0 * torch.rand(n, generator=g),
             sigma_y=0.2 + 0.6 * torch.rand(n, generator=g),
             w=torch.randn(n, generator=g))
    t["w"][::7] = 0.0
    if n == 1:
        t.update(mu_x=torch.tensor([9.7]), mu_y=torch.tensor([-11.2]), w=torch.tensor([-1.3]))
    return t


def _cotangent(nbx, nby):
    return torch.linspace(0.5, 1.5, nbx * nby, dtype=torch.float64).reshape(nbx, nby)


def _tables(t, ex, ey):
    def axis(mu, sigma, e):
        e = torch.tensor(e, dtype=torch.float64)
        cdf = torch.special.ndtr((e[None, :] - mu[:, None]) / sigma.reshape(-1, 1))
        return cdf[:, 1:] - cdf[:, :-1]
    return axis(t["mu_x"], t["sigma_x"], ex), axis(t["mu_y"], t["sigma_y"], ey)


def _oracle(t, ex, ey, wrt):
    """float64 cell sums and the gradients of sum_jk G_jk out_jk w.r.t. the operands named in
    ``wrt``, on the float32-rounded inputs; sigmas / w may have one element (broadcast)."""
    t = {k: None if v is None else v.double().clone() for k, v in t.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    px, py = _tables(t, ex, ey)
    if t["w"] is not None:
        px = px * t["w"].reshape(-1, 1)
    out = torch.einsum("ij,ik->jk", px, py)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], _cotangent(*out.shape)) if wrt else ()
    n, w = t["mu_x"].numel(), t["w"]
    absw = float(n) if w is None else float(w.detach().abs().sum()) * (
        n if w.numel() == 1 and n > 1 else 1)
    return out.detach(), {k: g.detach() for k, g in zip(wrt, grads)}, absw


@functools.lru_cache(maxsize=None)
def _case(n, nbx, nby, sigma_mode, w_mode):
    t = dict(_inputs(n))
    if sigma_mode == "broadcast":
        t["sigma_x"], t["sigma_y"] = t["sigma_x"][:1].clone(), t["sigma_y"][:1].clone()
    if w_mode == "none":
        t["w"] = None
    wrt = tuple(k for k in NAMES if t[k] is not None)
    return t, _oracle(t, *_edges(nbx, nby), wrt)


def _run(t, ex, ey, wrt):
    from multigrad_amd.ops import gaussian_binned_sum_2d
    t = {k: None if v is None else v.to(DEV) for k, v in t.items()}
    for k in wrt:
        t[k] = t[k].detach().requires_grad_(True)
    out = gaussian_binned_sum_2d(t["mu_x"], t["sigma_x"], t["mu_y"], t["sigma_y"], ex, ey, t["w"])
    grads = torch.autograd.grad(out, [t[k] for k in wrt], _cotangent(*out.shape).to(out)) \
        if wrt else ()
    return out.detach(), dict(zip(wrt, grads))


def _check(out, grads, ref, gref, absw):
    out = out.cpu().double().numpy()
    ref = ref.numpy()
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref)
    tol = 4.4e-7 * absw + 2e-5 * np.abs(ref)
    print("forward err/tol", float((err / tol).max()))
    assert (err <= tol).all(), (err, tol)
    assert set(grads) == set(gref)
    for k, g in grads.items():
        g = g.cpu().double().numpy().reshape(-1)
        r = gref[k].numpy().reshape(-1)
        assert g.shape == r.shape and np.isfinite(g).all()
        atol = 2e-5 * float(np.abs(r).max())
        print(k, "grad err/tol", float((np.abs(g - r) / (atol + 2e-4 * np.abs(r))).max()))
        np.testing.assert_allclose(g, r, rtol=2e-4, atol=atol, err_msg=k)


@pytest.mark.parametrize("w_mode", ["none", "per-object"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("n,nbx,nby", SHAPES)
def test_forward_and_gradients_match_fp64(n, nbx, nby, sigma_mode, w_mode):
    t, (ref, gref, absw) = _case(n, nbx, nby, sigma_mode, w_mode)
    out, grads = _run(t, *_edges(nbx, nby), tuple(gref))
    assert out.shape == (nbx, nby) and out.dtype == torch.float32 and out.is_cuda
    _check(out, grads, ref, gref, absw)


def test_broadcast_weights_and_everything_broadcast():
    ex, ey = _edges(10, 6)
    t = dict(_inputs(1023))
    t["w"] = torch.tensor([-0.7])
    ref, gref, absw = _oracle(t, ex, ey, NAMES)
    out, grads = _run(t, ex, ey, NAMES)
    assert grads["w"].shape == (1,)
    _check(out, grads, ref, gref, absw)
    # everything broadcast: three reduced gradients from one pass
    t["sigma_x"], t["sigma_y"] = t["sigma_x"][:1].clone(), t["sigma_y"][:1].clone()
    ref, gref, absw = _oracle(t, ex, ey, NAMES)
    out, grads = _run(t, ex, ey, NAMES)
    assert all(grads[k].shape == (1,) for k in ("sigma_x", "sigma_y", "w"))
    _check(out, grads, ref, gref, absw)


def test_everything_broadcast_over_several_workgroups():
    """Three reduced gradients through the [blocks, 4] slab and its fixed-order reduce: 3001
    objects, four per thread, are three workgroups of the backward."""
    ex, ey = _edges(10, 6)
    t = dict(_inputs(3001))
    t["sigma_x"], t["sigma_y"] = t["sigma_x"][:1].clone(), t["sigma_y"][:1].clone()
    t["w"] = torch.tensor([-0.7])
    ref, gref, absw = _oracle(t, ex, ey, NAMES)
    out, grads = _run(t, ex, ey, NAMES)
    assert all(grads[k].shape == (1,) for k in ("sigma_x", "sigma_y", "w"))
    _check(out, grads, ref, gref, absw)


def test_edge_inputs_stay_finite_and_accurate():
    ex, ey = _edges(10, 6)
    t = {k: v.clone() for k, v in _inputs(1023).items()}
    t["sigma_x"][:100] = 1e-3                 # step functions on x
    t["sigma_y"][50:150] = 1e-3               # on y, and on both for 50..99
    t["mu_x"][0] = ex[3]                      # exactly on an edge (a step function)
    t["mu_y"][60] = ey[2]
    t["mu_x"][300] = ex[5]                    # exactly on an edge, ordinary width
    t["mu_y"][301] = ey[4]
    far = {"x_below": slice(400, 420), "x_above": slice(420, 440), "y_below": slice(440, 460),
           "y_above": slice(460, 480)}
    t["mu_x"][far["x_below"]] = ex[0] - 50.0 * t["sigma_x"][far["x_below"]]
    t["mu_x"][far["x_above"]] = ex[-1] + 50.0 * t["sigma_x"][far["x_above"]]
    t["mu_y"][far["y_below"]] = ey[0] - 50.0 * t["sigma_y"][far["y_below"]]
    t["mu_y"][far["y_above"]] = ey[-1] + 50.0 * t["sigma_y"][far["y_above"]]
    for s in far.values():                    # inside the grid on the other axis
        t["w"][s] = 1.0
    t["mu_y"][400:440] = -11.0
    t["mu_x"][440:480] = 9.8
    t["w"][[0, 60, 300, 301]] = 1.0
    ref, gref, absw = _oracle(t, ex, ey, NAMES)
    out, grads = _run(t, ex, ey, NAMES)
    _check(out, grads, ref, gref, absw)
    # the far objects alone: every cell absolutely ~ 0 and finite, every gradient finite
    only = {k: v[400:480].clone() for k, v in t.items()}
    out, grads = _run(only, ex, ey, NAMES)
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 4.4e-7 * 80
    assert all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout):
    from multigrad_amd.ops import gaussian_binned_sum_2d
    n = 1023
    ex, ey = _edges(10, 6)
    t = _inputs(n)
    ref, gref, absw = _oracle(t, ex, ey, NAMES)
    if layout == "offset":                   # a 4-byte-offset pointer: scalar loads
        buf = torch.zeros(n + 1, device=DEV)
        buf[1:] = t["mu_y"].to(DEV)
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
    else:                                    # non-contiguous: copied
        buf = torch.zeros(2 * n, device=DEV)
        buf[::2] = t["mu_y"].to(DEV)
        view = buf[::2]
        assert not view.is_contiguous()
    d = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    view.requires_grad_(True)
    out = gaussian_binned_sum_2d(d["mu_x"], d["sigma_x"], view, d["sigma_y"], ex, ey, d["w"])
    leaves = [d["mu_x"], d["sigma_x"], view, d["sigma_y"], d["w"]]
    grads = dict(zip(NAMES, torch.autograd.grad(out, leaves, _cotangent(10, 6).to(out))))
    _check(out.detach(), grads, ref, gref, absw)
    # the same values from aligned contiguous tensors: same bits (the load path does not
    # change the arithmetic)
    out2, grads2 = _run(t, ex, ey, NAMES)
    assert torch.equal(out.detach(), out2)
    assert all(torch.equal(grads[k], grads2[k]) for k in NAMES)


@pytest.mark.parametrize("wrt", [("mu_x",), ("sigma_y",), ("w",), ("mu_x", "mu_y"),
                                 ("sigma_x", "w")])
def test_gradient_subsets(wrt):
    ex, ey = _edges(10, 6)
    t = _inputs(1023)
    ref, gref, absw = _oracle(t, ex, ey, wrt)
    out, grads = _run(t, ex, ey, wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, ref, gref, absw)


def test_bitwise_deterministic():
    ex, ey = _edges(17, 9)
    t = dict(_inputs(200_003))
    t["sigma_x"], t["sigma_y"] = t["sigma_x"][:1].clone(), t["sigma_y"][:1].clone()
    a = _run(t, ex, ey, NAMES)
    b = _run(t, ex, ey, NAMES)
    assert torch.equal(a[0], b[0])
    for k in NAMES:
        assert torch.equal(a[1][k], b[1][k]), k


def test_float64_device_input_takes_torch_path():
    from multigrad_amd.ops import gaussian_binned_sum_2d
    ex, ey = _edges(10, 6)
    t = _inputs(1023)
    ref, gref, _ = _oracle(t, ex, ey, NAMES)
    d = {k: v.double().to(DEV).requires_grad_(True) for k, v in t.items()}
    out = gaussian_binned_sum_2d(d["mu_x"], d["sigma_x"], d["mu_y"], d["sigma_y"], ex, ey, d["w"])
    assert out.dtype == torch.float64 and out.is_cuda
    grads = torch.autograd.grad(out, [d[k] for k in NAMES], _cotangent(10, 6).to(DEV))
    np.testing.assert_allclose(out.detach().cpu(), ref, rtol=0, atol=1e-12)
    for g, k in zip(grads, NAMES):
        np.testing.assert_allclose(g.cpu(), gref[k], rtol=0, atol=1e-12)


def test_device_edges_raise():
    from multigrad_amd.ops import gaussian_binned_sum_2d
    t = {k: v.to(DEV) for k, v in _inputs(63).items()}
    ex, ey = _edges(4, 5)
    args = (t["mu_x"], t["sigma_x"], t["mu_y"], t["sigma_y"])
    with pytest.raises(TypeError, match="setup"):
        gaussian_binned_sum_2d(*args, torch.tensor(ex, device=DEV), ey)
    with pytest.raises(TypeError, match="setup"):
        gaussian_binned_sum_2d(*args, ex, torch.tensor(ey, device=DEV))


def test_marginal_matches_the_1d_oracle():
    """One y bin more than 50 sigma beyond every object: Py = 1, so out[:, 0] is the 1-D sum."""
    from multigrad_amd.ops import gaussian_binned_sum_2d
    n, nbx = 1023, 10
    ex, _ = _edges(nbx, 1)
    t = _inputs(n)
    ey = (float(t["mu_y"].min()) - 60.0, float(t["mu_y"].max()) + 60.0)
    e = torch.tensor(ex, dtype=torch.float64)
    cdf = torch.special.ndtr((e[None, :] - t["mu_x"].double()[:, None])
                             / t["sigma_x"].double()[:, None])
    ref = ((cdf[:, 1:] - cdf[:, :-1]) * t["w"].double()[:, None]).sum(0).numpy()
    d = {k: v.to(DEV) for k, v in t.items()}
    out = gaussian_binned_sum_2d(d["mu_x"], d["sigma_x"], d["mu_y"], d["sigma_y"], ex, ey, d["w"])
    assert out.shape == (nbx, 1)
    err = np.abs(out[:, 0].cpu().double().numpy() - ref)
    tol = 2.2e-7 * float(t["w"].double().abs().sum()) + 2e-5 * np.abs(ref)
    print("marginal err/tol", float((err / tol).max()))
    assert (err <= tol).all(), (err, tol)


def test_captured_engine_matches_eager_and_fp64_model():
    """The joint model (10 x 4 cells) at 20 000 populations / 400 000 halos on one rank.  At the
    starting parameters the smallest cell holds 0.0048 of the summed sumstats (0.0023 of the
    target's); on the CPU the float32 torch path of the model sits at <= 0.014 of every bound
    below (sumstats 0.005, loss 0.0006, gradient 0.014 of the tolerance)."""
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (JointBinnedPopulationSMFModel,
                                                       joint_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    aux = joint_population_data(data)
    guess = data["guess"]
    m = JointBinnedPopulationSMFModel(aux_data=aux)
    ref = m.run_adam(guess, nsteps=6, learning_rate=1e-3, use_engine=False)
    eng = GraphAdamEngine(m, graph=True)
    traj = eng.run_adam(guess, nsteps=6, learning_rate=1e-3)
    assert eng.use_graph and eng.graph is not None and eng.fallback_reason is None, \
        eng.fallback_reason
    torch.testing.assert_close(traj, ref, rtol=1e-5, atol=1e-6)

    # float64 torch path of the same model on the same float32-rounded data and parameters
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    m64 = JointBinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    p64 = guess.double()
    loss64, grad64 = m64.calc_loss_and_grad_from_params(p64)
    loss, grad = m.calc_loss_and_grad_from_params(guess)
    S64 = m64.calc_sumstats_from_params(p64)
    S = m.calc_sumstats_from_params(guess)
    assert S.dtype == torch.float32
    scale = aux64["scale"]
    nhalo = aux["x"].numel()
    # forward contract on the cell sums (weights 1: sum |w| = number of halos), in S units
    tolS = (4.4e-7 * nhalo + 2e-5 * (S64 / scale).abs()) * scale
    errS = (S.double() - S64).abs()
    print("sumstats err/tol", float((errS / tolS).max()))
    assert (errS <= tolS).all(), (errS, tolS)
    # the loss: the forward tolerance pushed through dL/dS (first order), plus 1e-5 relative
    # for evaluating log10 / mean of the loss itself in float32
    dLdS = m64.calc_dloss_dsumstats(S64)
    tolL = float((dLdS.abs() * tolS).sum()) + 1e-5 * abs(float(loss64))
    print("loss err/tol", abs(float(loss) - float(loss64)) / tolL)
    assert abs(float(loss) - float(loss64)) <= tolL
    g64 = grad64.cpu().numpy()
    np.testing.assert_allclose(grad.cpu().double().numpy(), g64, rtol=2e-4,
                               atol=2e-5 * float(np.abs(g64).max()))
