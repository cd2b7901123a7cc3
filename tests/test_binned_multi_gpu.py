"""gaussian_binned_sum_multi on the MI355X: the HIP kernels (csrc/binned_multi.hip) against
the float64 torch path of the op evaluated on the float32-rounded inputs and edges.

Forward, per row c and bin k:
    |out - ref| <= 2.2e-7 * sum_i |w_c,i| + 2e-5 * |ref|          (float32-erf contract)
Weight gradients, per element and reduced (one-element weights):
    rtol = 2e-4, atol = 2e-5 * max |ref|
dmu, dsigma (sums over channels whose terms may cancel): with t_c,i channel c's float64
contribution (the oracle evaluated channel by channel) and A_i = sum_c |t_c,i|,
    |g_i - ref_i| <= 2e-4 * A_i + 2e-5 * max_i A_i
and for a broadcast sigma the same with g, ref and A summed over i.
Cotangent: G[c] = linspace(0.5, 1.5, nb) * (1 + c/4).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(1, 1), (63, 4), (257, 5), (1023, 10), (200_003, 17), (200_003, 32)]
KINDS = ("none", "per-object", "one-element", "positive")


def _edges(nb):
    # float32-representable edges (the kernels hold them in float32)
    return tuple(float(v) for v in np.linspace(9.2, 10.4, nb + 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(n, C, seed=0):
    """float32 inputs on the host: means around the bins, widths 0.1-0.5 and C weights whose
    kinds cycle over None, per-object (both signs, exact zeros), one-element and per-object
    positive (uniform in [0.5, 1.5])."""
    g = torch.Generator().manual_seed(seed + n)
    mu = 9.0 + 1.6 * torch.rand(n, generator=g)
    if n == 1:
        mu = torch.tensor([9.7])
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g)
    ws = []
    for c in range(C):
        kind = KINDS[c % 4]
        if kind == "none":
            ws.append(None)
        elif kind == "per-object":
            w = torch.randn(n, generator=g)
            w[::7] = 0.0
            ws.append(torch.tensor([-1.3]) if n == 1 else w)
        elif kind == "one-element":
            ws.append(torch.tensor([-0.7 - 0.05 * c]))
        else:
            ws.append(0.5 + torch.rand(n, generator=g))
    return mu, sigma, tuple(ws)


def _cotangent(C, nb, like=None):
    G = torch.linspace(0.5, 1.5, nb, dtype=torch.float64)[None, :] * \
        (1.0 + torch.arange(C, dtype=torch.float64)[:, None] / 4.0)
    return G if like is None else G.to(like)


def _names(ws):
    return ("mu", "sigma") + tuple(f"w{c}" for c, w in enumerate(ws) if w is not None)


def _oracle(mu, sigma, ws, edges, wrt):
    """The float64 torch path of the op on the float32-rounded inputs: the rows, the gradients
    of sum_ck G_ck out_ck w.r.t. the operands named in ``wrt`` ("mu", "sigma", "w<c>"), the
    per-row sum_i |w_c,i| and the absolute channel sums A (per object) for mu and sigma."""
    from multigrad_amd.ops import gaussian_binned_sum_multi
    C, n = len(ws), mu.numel()
    t = {"mu": mu.double().clone(), "sigma": sigma.double().clone()}
    for c, w in enumerate(ws):
        t[f"w{c}"] = None if w is None else w.double().clone()
    for k in wrt:
        t[k].requires_grad_(True)
    wl = [t[f"w{c}"] for c in range(C)]
    out = gaussian_binned_sum_multi(t["mu"], t["sigma"], edges, wl)
    assert out.dtype == torch.float64
    G = _cotangent(C, len(edges) - 1)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], G) if wrt else ()
    absw = [float(n) if w is None else
            float(w.double().abs().sum()) * (n if w.numel() == 1 and n > 1 else 1) for w in ws]
    A = {}
    per_object = [k for k in ("mu", "sigma") if k in wrt]
    if per_object:
        m1 = mu.double().clone().requires_grad_(True)
        s1 = sigma.double().expand(n).clone().requires_grad_(True)  # per object even if broadcast
        A = {k: torch.zeros(n, dtype=torch.float64) for k in per_object}
        for c in range(C):
            w = None if ws[c] is None else ws[c].double()
            row = gaussian_binned_sum_multi(m1, s1, edges, [w])
            tm, ts = torch.autograd.grad(row, (m1, s1), G[c:c + 1])
            for k, v in (("mu", tm), ("sigma", ts)):
                if k in A:
                    A[k] += v.abs()
    return out.detach(), dict(zip(wrt, grads)), absw, A


@functools.lru_cache(maxsize=None)
def _case(n, nb, C, sigma_mode):
    mu, sigma, ws = _inputs(n, C)
    sigma = sigma if sigma_mode == "per-object" else sigma[:1].clone()
    return (mu, sigma, ws), _oracle(mu, sigma, ws, _edges(nb), _names(ws))


def _run(mu, sigma, ws, edges, wrt, op=None):
    from multigrad_amd.ops import gaussian_binned_sum_multi
    C = len(ws)
    t = {"mu": mu, "sigma": sigma}
    t.update({f"w{c}": w for c, w in enumerate(ws)})
    for k in wrt:
        t[k] = t[k].detach().requires_grad_(True)
    out = (op or gaussian_binned_sum_multi)(t["mu"], t["sigma"], edges,
                                            [t[f"w{c}"] for c in range(C)])
    G = _cotangent(C, len(edges) - 1, out)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], G) if wrt else ()
    return out.detach(), dict(zip(wrt, grads))


def _fwd_tol(ref, absw):
    return 2.2e-7 * np.asarray(absw)[:, None] + 2e-5 * np.abs(ref)


def _check(out, grads, ref, gref, absw, A):
    out = out.cpu().double().numpy()
    ref = ref.numpy()
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref)
    tol = _fwd_tol(ref, absw)
    print("forward err/tol", float((err / tol).max()))
    assert (err <= tol).all(), (err, tol)
    for k, g in grads.items():
        g = g.cpu().double().numpy().reshape(-1)
        r = gref[k].numpy().reshape(-1)
        assert g.shape == r.shape and np.isfinite(g).all()
        if k in ("mu", "sigma"):
            a = A[k].numpy()
            if r.size != a.size:  # broadcast sigma: the sums over i
                tol = 2e-4 * a.sum() + 2e-5 * a.max()
            else:
                tol = 2e-4 * a + 2e-5 * a.max()
            err = np.abs(g - r)
            print(k, "grad err/tol", float((err / tol).max()))
            assert (err <= tol).all(), (k, float((err / tol).max()))
        else:
            atol = 2e-5 * float(np.abs(r).max())
            print(k, "grad err/tol", float((np.abs(g - r) / (atol + 2e-4 * np.abs(r))).max()))
            np.testing.assert_allclose(g, r, rtol=2e-4, atol=atol, err_msg=k)


def _to_dev(ws):
    return [None if w is None else w.to(DEV) for w in ws]


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("n,nb", SHAPES)
def test_forward_and_gradients_match_fp64(n, nb, C, sigma_mode):
    (mu, sigma, ws), (ref, gref, absw, A) = _case(n, nb, C, sigma_mode)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), _to_dev(ws), _edges(nb), tuple(gref))
    assert out.shape == (C, nb) and out.dtype == torch.float32 and out.is_cuda
    for c, w in enumerate(ws):
        if w is not None:
            assert grads[f"w{c}"].shape == w.shape
    assert grads["sigma"].shape == sigma.shape
    _check(out, grads, ref, gref, absw, A)


def test_edge_inputs_stay_finite_and_accurate():
    n, nb, C = 1023, 10, 4
    edges = _edges(nb)
    mu, sigma, ws = _inputs(n, C)
    mu, sigma = mu.clone(), sigma.clone()
    ws = [None if w is None else w.clone() for w in ws]
    sigma[:200] = 1e-3                       # step functions
    mu[0] = edges[3]                         # exactly on an edge (a step function)
    mu[300] = edges[5]                       # exactly on an edge, ordinary width
    mu[400:420] = edges[0] - 50.0 * sigma[400:420]     # 50 sigma below every edge
    mu[420:440] = edges[-1] + 50.0 * sigma[420:440]    # 50 sigma above every edge
    ws[1][[0, 300, 400, 420]] = 1.0
    wrt = _names(ws)
    ref, gref, absw, A = _oracle(mu, sigma, ws, edges, wrt)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), _to_dev(ws), edges, wrt)
    _check(out, grads, ref, gref, absw, A)


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


@pytest.mark.parametrize("which", ["mu", "weight"])
@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout, which):
    n, nb, C = 1023, 10, 4
    edges = _edges(nb)
    (mu, sigma, ws), (ref, gref, absw, A) = _case(n, nb, C, "per-object")
    wrt = tuple(gref)
    dmu, dws = mu.to(DEV), _to_dev(ws)
    if which == "mu":
        dmu = _view(mu, layout)
    else:
        dws[3] = _view(ws[3], layout)
    out, grads = _run(dmu, sigma.to(DEV), dws, edges, wrt)
    _check(out, grads, ref, gref, absw, A)
    # the same values from aligned contiguous tensors: same bits (the load path does not
    # change the arithmetic)
    out2, grads2 = _run(mu.to(DEV), sigma.to(DEV), _to_dev(ws), edges, wrt)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("C,wrt", [
    (4, ("mu",)), (4, ("sigma",)), (4, ("w1",)), (4, ("mu", "w3")), (5, ("w4",))],
    ids=["mu", "sigma", "w1", "mu+w3", "second-pass-w4"])
def test_gradient_subsets(C, wrt, sigma_mode):
    n, nb = 1023, 10
    edges = _edges(nb)
    mu, sigma, ws = _inputs(n, C)
    sigma = sigma if sigma_mode == "per-object" else sigma[:1].clone()
    ws = list(ws)
    if C == 5:  # the cycle makes channel 4 None: give the second pass a weight tensor
        ws[4] = _inputs(n, 4, seed=1)[2][3]
    ref, gref, absw, A = _oracle(mu, sigma, ws, edges, wrt)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), _to_dev(ws), edges, wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, ref, gref, absw, A)


@pytest.mark.parametrize("wrt", [("w1",), ("mu", "w2"), ("sigma", "w3")],
                         ids=["w1", "mu+w2", "sigma+w3"])
def test_gradient_subsets_over_many_workgroups(wrt):
    """The slab + reduce path with a one-element weight (channel 2) that does or does not want
    its gradient, next to per-object weight gradients, and a broadcast sigma."""
    n, nb, C = 200_003, 17, 4
    edges = _edges(nb)
    mu, sigma, ws = _inputs(n, C)
    sigma = sigma[:1].clone()
    ref, gref, absw, A = _oracle(mu, sigma, ws, edges, wrt)
    out, grads = _run(mu.to(DEV), sigma.to(DEV), _to_dev(ws), edges, wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, ref, gref, absw, A)


def test_bitwise_deterministic():
    n, nb, C = 200_003, 17, 5
    mu, sigma, ws = _inputs(n, C)
    wrt = _names(ws)
    args = (mu.to(DEV), sigma[:1].to(DEV), _to_dev(ws), _edges(nb), wrt)
    a = _run(*args)
    b = _run(*args)
    assert torch.equal(a[0], b[0])
    for k in wrt:
        assert torch.equal(a[1][k], b[1][k]), k


def test_float64_device_input_takes_torch_path():
    n, nb, C = 1023, 10, 4
    edges = _edges(nb)
    (mu, sigma, ws), (ref, gref, _, _) = _case(n, nb, C, "per-object")
    wrt = tuple(gref)
    out, grads = _run(mu.double().to(DEV), sigma.double().to(DEV),
                      [None if w is None else w.double().to(DEV) for w in ws], edges, wrt)
    assert out.dtype == torch.float64 and out.is_cuda
    np.testing.assert_allclose(out.cpu(), ref, rtol=0, atol=1e-12)
    for k in wrt:
        np.testing.assert_allclose(grads[k].cpu(), gref[k], rtol=0, atol=1e-12)


def test_device_edges_raise():
    from multigrad_amd.ops import gaussian_binned_sum_multi
    mu, sigma, ws = _inputs(63, 2)
    with pytest.raises(TypeError, match="setup"):
        gaussian_binned_sum_multi(mu.to(DEV), sigma.to(DEV), torch.tensor(_edges(4), device=DEV),
                                  _to_dev(ws))


@pytest.mark.parametrize("n,nb,C", [(1023, 10, 4), (200_003, 17, 5)])
def test_rows_agree_with_the_single_op(n, nb, C):
    """Row c against gaussian_binned_sum(..., weights[c]) on the device, within the sum of both
    forward tolerances (not bitwise: the traversal may differ)."""
    from multigrad_amd.ops import gaussian_binned_sum, gaussian_binned_sum_multi
    (mu, sigma, ws), (ref, _, absw, _) = _case(n, nb, C, "per-object")
    dmu, dsig, dws = mu.to(DEV), sigma.to(DEV), _to_dev(ws)
    out = gaussian_binned_sum_multi(dmu, dsig, _edges(nb), dws)
    single = torch.stack([gaussian_binned_sum(dmu, dsig, _edges(nb), w) for w in dws])
    err = (out.double() - single.double()).abs().cpu().numpy()
    tol = 2.0 * _fwd_tol(ref.numpy(), absw)
    print("multi vs single err/tol", float((err / tol).max()))
    assert (err <= tol).all()


def test_captured_engine_matches_eager_and_fp64_model():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (ConditionalBinnedPopulationSMFModel,
                                                       conditional_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    aux = conditional_population_data(data)
    guess = data["guess"]
    m = ConditionalBinnedPopulationSMFModel(aux_data=aux)
    ref = m.run_adam(guess, nsteps=6, learning_rate=1e-3, use_engine=False)
    eng = GraphAdamEngine(m, graph=True)
    traj = eng.run_adam(guess, nsteps=6, learning_rate=1e-3)
    assert eng.use_graph and eng.graph is not None and eng.fallback_reason is None, \
        eng.fallback_reason
    torch.testing.assert_close(traj, ref, rtol=1e-5, atol=1e-6)

    # float64 torch path of the same model on the same float32-rounded data and parameters
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    m64 = ConditionalBinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    p64 = guess.double()
    loss64, grad64 = m64.calc_loss_and_grad_from_params(p64)
    loss, grad = m.calc_loss_and_grad_from_params(guess)
    S64 = m64.calc_sumstats_from_params(p64)
    S = m.calc_sumstats_from_params(guess)
    nb = aux["edges"].numel() - 1
    assert S.dtype == torch.float32 and S.shape == (3 * nb,)
    scale = aux64["scale"]
    # forward contract per statistic with sum |w| = number of halos, sum q, sum y; in S units
    a64 = p64.reshape(-1, 2)[:, 0][aux64["pop"]]
    q64 = torch.sigmoid(m64.q_slope * (aux64["x"] + a64 - m64.q_mass))
    absw = torch.stack([torch.tensor(float(aux["x"].numel()), dtype=torch.float64, device=DEV),
                        q64.sum(), aux64["y"].sum()]).repeat_interleave(nb)
    tolS = (2.2e-7 * absw + 2e-5 * (S64 / scale).abs()) * scale
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
