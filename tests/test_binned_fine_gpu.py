"""gaussian_binned_sum_fine on the MI355X: the HIP kernels (csrc/binned_fine.hip) against the
float64 torch path of the op (dense, untruncated) on the float32-rounded inputs and edges.

Forward, per bin k, with the window of object i the bins that overlap (mu_i - 5.5 sigma_i,
mu_i + 5.5 sigma_i), W_k / n_k the summed |w_i| / the number of the objects whose window reaches
bin k, A_k = sum_i |w_i| dPhi_ik and W = sum_i |w_i|:
    |out_k - ref_k| <= 3.2e-7 W_k + 1e-6 A_k + 2^-30 max|w| n_k + 2e-8 (W - W_k)
Gradients, per element:
    rtol = 2e-4, atol = 2e-5 * max |ref|
and for a reduced (broadcast) gradient, with t_i the float64 per-object terms,
    |g - ref| <= 2e-4 * sum_i |t_i| + 2e-5 * max_i |t_i|
Cotangent: linspace(0.5, 1.5, nb) in float32 (the oracle takes the same rounded values).

Inputs: means over the range of the edges widened by a tenth on both sides, the first four
objects 100 sigma beyond either end (N = 1: one object half a sigma below the last edge);
sigma = ratio * (mean bin width) * U(0.75, 1.25) with ratio 0.05 (inside one bin), 2 and 50
(hundreds of bins); signed weights with every 7th an exact zero.
Geometric edges: the last bin is 20 times as wide as the first.  The oracle runs in float64 on
the device (the op's torch path), once per case.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = 5.5
NS = [1, 257, 4099]
NBS = [33, 64, 257, 4096]
KINDS = ["uniform", "geometric"]
RATIOS = [0.05, 2.0, 50.0]
E0, E1 = 9.0, 11.0


@functools.lru_cache(maxsize=None)
def _edges(nb, kind="uniform"):
    """float32-representable host edges (the kernels hold them in float32)."""
    if kind == "uniform":
        e = np.linspace(E0, E1, nb + 1)
    else:
        r = 20.0 ** (1.0 / (nb - 1))
        e = E0 + (E1 - E0) * (r ** np.arange(nb + 1) - 1.0) / (r ** nb - 1.0)
    e = e.astype(np.float32)
    assert (np.diff(e) > 0).all()
    return tuple(float(v) for v in e)


@functools.lru_cache(maxsize=None)
def _bins(nb, kind="uniform", dev="cuda"):
    from multigrad_amd.ops import FineBins
    return FineBins(_edges(nb, kind), device=DEV if dev == "cuda" else "cpu")


@functools.lru_cache(maxsize=None)
def _inputs(n, nb, ratio):
    g = torch.Generator().manual_seed(1000 * n + nb)
    span = E1 - E0
    mu = E0 - 0.1 * span + 1.2 * span * torch.rand(n, generator=g)
    sigma = ratio * (span / nb) * (0.75 + 0.5 * torch.rand(n, generator=g))
    w = torch.randn(n, generator=g)
    w[::7] = 0.0
    if n == 1:
        # half a sigma below the last edge: the end of the range, where the cotangent falls
        # from 1.5 to 0, dominates both gradients (far inside the range they are near-
        # cancellations, which float32 cannot hold to a relative tolerance)
        mu, w = E1 - 0.5 * sigma, torch.tensor([-1.3])
    else:
        mu[0:2] = E0 - 100.0 * sigma[0:2]
        mu[2:4] = E1 + 100.0 * sigma[2:4]
        w[0:4] = 1.0
    return mu, sigma, w


def _modes(mu, sigma, w, sigma_mode, w_mode):
    sigma = sigma if sigma_mode == "per-object" else sigma[:1].clone()
    w = {"none": None, "per-object": w, "one-element": torch.tensor([-0.7])}[w_mode]
    return mu, sigma, w


def _cotangent(nb, like):
    """float32 values on every side: with 4096 bins the difference of two neighbours,
    h_e = g_{e-1} - g_e = 2.4e-4, would otherwise carry the rounding of the cotangent itself."""
    return torch.linspace(0.5, 1.5, nb, dtype=torch.float32).to(like)


def _oracle(bins, mu, sigma, w, wrt):
    """On the device in float64: the bins, the forward tolerance, the gradients of
    sum_k g_k out_k for the operands named in ``wrt`` and, for a broadcast operand, the
    per-object terms t_i of its gradient.  Everything comes back on the host."""
    n, nb = mu.numel(), bins.nb
    t = {"mu": mu.double().to(DEV), "sigma": sigma.double().to(DEV),
         "weights": None if w is None else w.double().to(DEV)}
    for k in wrt:
        t[k].requires_grad_(True)
    out = bins.sum(t["mu"], t["sigma"], t["weights"])
    assert out.dtype == torch.float64 and out.shape == (nb,)
    cot = _cotangent(nb, out)
    grads = dict(zip(wrt, torch.autograd.grad(out, [t[k] for k in wrt], cot))) if wrt else {}
    m, s = t["mu"].detach(), t["sigma"].detach().expand(n)
    absw = torch.ones(n, dtype=torch.float64, device=DEV) if w is None else \
        t["weights"].detach().abs().expand(n).contiguous()
    e = torch.tensor(bins.edges, dtype=torch.float64, device=DEV)
    tolparts = torch.zeros(2, nb, dtype=torch.float64, device=DEV)  # W_k, n_k
    for lo in range(0, n, 512):
        hi = min(lo + 512, n)
        wlo, whi = (m[lo:hi] - T * s[lo:hi])[:, None], (m[lo:hi] + T * s[lo:hi])[:, None]
        reach = ((e[None, 1:] > wlo) & (e[None, :-1] < whi)).double()
        tolparts[0] += absw[lo:hi] @ reach
        tolparts[1] += reach.sum(0)
    A = bins.sum(m, t["sigma"].detach(), absw)
    W = absw.sum()
    tol = 3.2e-7 * tolparts[0] + 1e-6 * A + 2.0 ** -30 * absw.max() * tolparts[1] + \
        2e-8 * (W - tolparts[0])
    terms = {}
    for k in wrt:
        if t[k].numel() == 1 and n > 1:
            full = {q: (None if v is None else v.detach()) for q, v in t.items()}
            full[k] = full[k].expand(n).clone().requires_grad_(True)
            o = bins.sum(full["mu"], full["sigma"], full["weights"])
            (terms[k],) = torch.autograd.grad(o, full[k], cot)
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    return out.detach().cpu(), tol.cpu(), cpu(grads), cpu(terms)


def _wrt_all(w):
    return ("mu", "sigma") + (("weights",) if w is not None else ())


@functools.lru_cache(maxsize=None)
def _case(n, nb, kind, ratio, sigma_mode="per-object", w_mode="per-object"):
    ops = _modes(*_inputs(n, nb, ratio), sigma_mode, w_mode)
    return ops, _oracle(_bins(nb, kind), *ops, _wrt_all(ops[2]))


def _run(bins, mu, sigma, w, wrt):
    t = {"mu": mu, "sigma": sigma, "weights": w}
    for k in wrt:
        t[k] = t[k].detach().requires_grad_(True)
    out = bins.sum(t["mu"], t["sigma"], t["weights"])
    grads = torch.autograd.grad(out, [t[k] for k in wrt], _cotangent(bins.nb, out)) if wrt else ()
    return out.detach(), dict(zip(wrt, grads))


def _check(out, grads, oracle):
    ref, tol, gref, terms = oracle
    out = out.cpu().double().numpy()
    assert out.shape == tuple(ref.shape) and np.isfinite(out).all()
    err = np.abs(out - ref.numpy())
    tol = tol.numpy()
    print("forward err/tol", float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    for k, g in grads.items():
        g = g.cpu().double().numpy().reshape(-1)
        r = gref[k].numpy().reshape(-1)
        assert g.shape == r.shape and np.isfinite(g).all()
        if k in terms:
            a = terms[k].abs().numpy()
            gtol = 2e-4 * a.sum() + 2e-5 * a.max()
            print(k, "reduced grad err/tol", float(np.abs(g - r).max() / max(gtol, 1e-300)))
            assert (np.abs(g - r) <= gtol).all(), k
        else:
            atol = 2e-5 * float(np.abs(r).max())
            print(k, "grad err/tol",
                  float((np.abs(g - r) / np.maximum(atol + 2e-4 * np.abs(r), 1e-300)).max()))
            np.testing.assert_allclose(g, r, rtol=2e-4, atol=atol, err_msg=k)


def _dev(ops):
    return tuple(None if t is None else t.to(DEV) for t in ops)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("n", NS)
def test_forward_and_gradients_match_fp64(n, nb, kind, ratio):
    ops, oracle = _case(n, nb, kind, ratio)
    out, grads = _run(_bins(nb, kind), *_dev(ops), tuple(oracle[2]))
    assert out.shape == (nb,) and out.dtype == torch.float32 and out.is_cuda
    for k, t in zip(("mu", "sigma", "weights"), ops):
        assert grads[k].shape == t.shape
    _check(out, grads, oracle)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("nb,kind", [(64, "geometric"), (4096, "uniform")])
@pytest.mark.parametrize("w_mode", ["none", "per-object", "one-element"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
def test_operand_modes(sigma_mode, w_mode, nb, kind, ratio):
    ops, oracle = _case(4099, nb, kind, ratio, sigma_mode, w_mode)
    out, grads = _run(_bins(nb, kind), *_dev(ops), tuple(oracle[2]))
    assert grads["sigma"].shape == ops[1].shape
    if ops[2] is not None:
        assert grads["weights"].shape == ops[2].shape
    _check(out, grads, oracle)


@pytest.mark.parametrize("nb,ratio", [(33, 2.0), (4096, 2.0), (257, 50.0)])
def test_order_independent_and_bitwise_deterministic(nb, ratio):
    bins = _bins(nb)
    ops = _dev(_inputs(4099, nb, ratio))
    wrt = ("mu", "sigma", "weights")
    a = _run(bins, *ops, wrt)
    b = _run(bins, *ops, wrt)
    assert torch.equal(a[0], b[0])
    for k in wrt:
        assert torch.equal(a[1][k], b[1][k]), k
    perm = torch.randperm(4099, generator=torch.Generator().manual_seed(3)).to(DEV)
    c = _run(bins, *(t[perm] for t in ops), wrt)
    assert torch.equal(a[0], c[0])
    for k in wrt:  # the gradients are per object: the same values at the permuted places
        assert torch.equal(a[1][k][perm], c[1][k]), k
    # no weights: the same, at the fixed scale
    d = bins.sum(ops[0], ops[1])
    assert torch.equal(d, bins.sum(ops[0][perm], ops[1][perm]))


@pytest.mark.parametrize("w", [0.37, -1.3e-3, 5.0e4])
def test_identical_objects_sum_exactly(w):
    """1024 objects of weight w and one object of weight 1024 w: the scale moves by 2^10 and
    the integers are the same, so the bits are."""
    nb = 257
    bins = _bins(nb)
    mu, sigma = torch.tensor([9.83], device=DEV), torch.tensor([0.021], device=DEV)
    many = bins.sum(mu.expand(1024).contiguous(), sigma.expand(1024).contiguous(),
                    torch.full((1024,), w, device=DEV))
    one = bins.sum(mu, sigma, torch.tensor([1024.0 * w], device=DEV))
    assert float(one.abs().sum()) > 0
    assert torch.equal(many, one)


def _view(t, layout):
    n = t.numel()
    if layout == "offset":                   # a 4-byte-offset pointer: scalar loads
        buf = torch.zeros(n + 1, device=DEV)
        buf[1:] = t.to(DEV)
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
    else:                                    # non-contiguous
        buf = torch.zeros(2 * n, device=DEV)
        buf[::2] = t.to(DEV)
        view = buf[::2]
        assert not view.is_contiguous()
    return view


@pytest.mark.parametrize("which", ["mu", "sigma", "weights"])
@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout, which):
    nb = 257
    ops, oracle = _case(4099, nb, "uniform", 2.0)
    wrt = tuple(oracle[2])
    dops = list(_dev(ops))
    k = ("mu", "sigma", "weights").index(which)
    dops[k] = _view(ops[k], layout)
    out, grads = _run(_bins(nb), *dops, wrt)
    _check(out, grads, oracle)
    out2, grads2 = _run(_bins(nb), *_dev(ops), wrt)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize("sigma_mode,w_mode", [("per-object", "per-object"),
                                               ("broadcast", "one-element")])
@pytest.mark.parametrize("wrt", [("mu",), ("sigma",), ("weights",), ("mu", "weights")],
                         ids=["mu", "sigma", "weights", "mu+weights"])
def test_gradient_subsets(wrt, sigma_mode, w_mode):
    nb = 257
    ops = _modes(*_inputs(4099, nb, 2.0), sigma_mode, w_mode)
    oracle = _oracle(_bins(nb), *ops, wrt)
    out, grads = _run(_bins(nb), *_dev(ops), wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, oracle)


def test_float64_device_input_takes_torch_path():
    nb = 257
    ops, (ref, _, gref, _) = _case(4099, nb, "uniform", 2.0)
    wrt = tuple(gref)
    out, grads = _run(_bins(nb), *(t.double().to(DEV) for t in ops), wrt)
    assert out.dtype == torch.float64 and out.is_cuda
    # the dense table without truncation: the float64 CPU path of the same op
    cpu = _run(_bins(nb, dev="cpu"), *(t.double() for t in ops), wrt)
    np.testing.assert_allclose(out.cpu(), cpu[0], rtol=0, atol=1e-12 * float(ref.abs().max()))
    for k in wrt:
        np.testing.assert_allclose(grads[k].cpu(), cpu[1][k], rtol=0,
                                   atol=1e-12 * float(gref[k].abs().max()))


@pytest.mark.parametrize("w_mode", ["per-object", "one-element"])
def test_nan_weight_gives_nan_everywhere(w_mode):
    nb = 257
    mu, sigma, w = _inputs(4099, nb, 2.0)
    if w_mode == "per-object":
        w = w.clone()
        w[1] = float("nan")      # an object 100 sigma below the range: its window is empty
    else:
        w = torch.tensor([float("nan")])
    out = _bins(nb).sum(*_dev((mu, sigma, w)))
    assert out.shape == (nb,) and torch.isnan(out).all()
    mu = mu.clone()
    mu[5] = float("nan")
    assert torch.isnan(_bins(nb).sum(mu.to(DEV), sigma.to(DEV))).all()


def test_zero_weights_give_zeros():
    nb = 257
    mu, sigma, w = _inputs(4099, nb, 2.0)
    out = _bins(nb).sum(*_dev((mu, sigma, torch.zeros_like(w))))
    assert out.shape == (nb,) and (out == 0).all()
    out = _bins(nb).sum(*_dev((mu, sigma, torch.zeros(1))))
    assert (out == 0).all()


def test_agrees_with_the_slices_composite():
    """gaussian_binned_sum on 33-edge slices, concatenated: each side meets its own forward
    contract (the single op's: 2.2e-7 W + 2e-5 |ref|), so they agree within the sum."""
    from multigrad_amd.ops import FineBins, gaussian_binned_sum
    nb = 100
    edges = _edges(nb)
    bins = FineBins(edges, device=DEV)
    ops = _inputs(4099, nb, 2.0)
    ref, tol, _, _ = _oracle(bins, *ops, ())
    mu, sigma, w = _dev(ops)
    out = bins.sum(mu, sigma, w)
    comp = torch.cat([gaussian_binned_sum(mu, sigma, edges[k:k + 33], w)
                      for k in range(0, nb, 32)])
    assert comp.shape == (nb,)
    err = (out.double() - comp.double()).abs().cpu().numpy()
    both = tol.numpy() + 2.2e-7 * float(ops[2].abs().sum()) + 2e-5 * np.abs(ref.numpy())
    print("fine vs slices err/tol", float((err / both).max()))
    assert (err <= both).all()


def test_few_bins_are_the_single_op():
    from multigrad_amd.ops import FineBins, gaussian_binned_sum
    edges = _edges(32)
    mu, sigma, w = _dev(_inputs(4099, 32, 2.0))
    assert torch.equal(FineBins(edges, device=DEV).sum(mu, sigma, w),
                       gaussian_binned_sum(mu, sigma, edges, w))


def test_operands_off_the_plans_device_raise():
    mu, sigma, _ = _inputs(257, 64, 2.0)
    with pytest.raises(ValueError, match="mu"):
        _bins(64).sum(mu, sigma)
    from multigrad_amd.ops import FineBins
    with pytest.raises(TypeError, match="setup"):
        FineBins(torch.tensor(_edges(64), device=DEV))


def test_captured_engine_matches_eager_and_fp64_model():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (FineBinnedPopulationSMFModel,
                                                       fine_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    aux = fine_population_data(data, refine=8)
    guess = data["guess"]
    m = FineBinnedPopulationSMFModel(aux_data=aux)
    nb = m.bins.nb
    assert nb > 32 and aux["scale"].shape == (nb,)
    ref = m.run_adam(guess, nsteps=6, learning_rate=1e-3, use_engine=False)
    eng = GraphAdamEngine(m, graph=True)
    traj = eng.run_adam(guess, nsteps=6, learning_rate=1e-3)
    assert eng.use_graph and eng.graph is not None and eng.fallback_reason is None, \
        eng.fallback_reason
    torch.testing.assert_close(traj, ref, rtol=1e-5, atol=1e-6)

    # float64 torch path of the same model on the same float32-rounded data and parameters
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    m64 = FineBinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    assert m64.bins.edges == m.bins.edges
    p64 = guess.double()
    loss64, grad64 = m64.calc_loss_and_grad_from_params(p64)
    loss, grad = m.calc_loss_and_grad_from_params(guess)
    S64 = m64.calc_sumstats_from_params(p64)
    S = m.calc_sumstats_from_params(guess)
    assert S.dtype == torch.float32 and S.shape == (nb,)
    scale = aux64["scale"]
    # forward contract with unit weights: W_k = n_k = the objects whose window reaches bin k,
    # A_k the bin sum itself; the windows from the float64 model's mu and sigma
    th = p64.reshape(-1, 2)
    a, sigma = m64.groups.gather(th[:, 0], torch.pow(10.0, th[:, 1]))
    mu = aux64["x"] + a
    e = torch.tensor(m.bins.edges, dtype=torch.float64, device=DEV)
    nk = torch.zeros(nb, dtype=torch.float64, device=DEV)
    for lo in range(0, mu.numel(), 1 << 16):
        wlo = (mu[lo:lo + (1 << 16)] - T * sigma[lo:lo + (1 << 16)])[:, None]
        whi = (mu[lo:lo + (1 << 16)] + T * sigma[lo:lo + (1 << 16)])[:, None]
        nk += ((e[None, 1:] > wlo) & (e[None, :-1] < whi)).sum(0)
    tolS = ((3.2e-7 + 2.0 ** -30) * nk + 1e-6 * (S64 / scale).abs() +
            2e-8 * (mu.numel() - nk)) * scale
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
