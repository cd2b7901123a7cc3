"""gaussian_binned_sum_by_group on the MI355X: the HIP kernels (csrc/binned_group.hip) against
the float64 torch path of the op evaluated on the float32-rounded inputs and edges.

Forward, per group g and bin k:
    |out - ref| <= 3.2e-7 * W_g + 2e-5 * A_gk
with W_g = sum_{i in g} |w_i| (a one-element weight counts L_g * |w|, no weights L_g) and
A_gk = sum_{i in g} |w_i| dPhi_ik.
Gradients, per element:
    rtol = 2e-4, atol = 2e-5 * max |ref|
and for a reduced (broadcast) gradient, with t_i the float64 per-object terms,
    |g - ref| <= 2e-4 * sum_i |t_i| + 2e-5 * max_i |t_i|
Cotangent: G[g, k] = linspace(0.5, 1.5, nb)[k] * (1 + (g mod 5) / 4).

Index layouts (the smallest at which the segmented reduction can go wrong; a chunk is 1024
sorted positions, four per thread, 64 lanes per wave):
  tiny       N = 1, G = 1
  small      N = 63, G = 5, random
  sizes      group counts SIZES: runs that end inside a thread's four entries, across lanes,
             waves and a chunk edge, a run covering a whole chunk, empty groups first, in the
             middle and last
  singletons one object per group and three empty groups at the end
  one_group  N = 200 003, G = 1: every chunk is single-key, one carry level
  two_level  N = 600 001, G = 300, half of the objects in group 1: 586 chunks, so the carry
             list of 1172 entries needs a further level
  pow2_19    N = 2^19, G = 256 groups of 2048 objects: every group boundary falls on a chunk
             edge, so the carry list of level 1 is [-1, 0, 0, -1, -1, 1, 1, -1, ...], one
             full chunk of 1024 slots whose first and last key are both the unused -1 with
             every real partial between them
  pow2_20    N = 2^20, G = 512 groups of 2048: two such carry chunks, so a carry level
             itself emits carries
each sorted (the plan has no perm) and shuffled (operands read through perm).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIZES = [0, 1, 3, 4, 5, 0, 63, 65, 255, 257, 700, 1, 1024, 0, 2500, 2, 0]
LAYOUTS = [("small", 4), ("sizes", 5), ("sizes", 10), ("sizes", 32), ("singletons", 17),
           ("one_group", 10), ("two_level", 10), ("pow2_19", 10), ("pow2_20", 5)]
ORDERS = ["sorted", "shuffled"]


def _edges(nb):
    # float32-representable edges (the kernels hold them in float32)
    return tuple(float(v) for v in np.linspace(9.2, 10.4, nb + 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _index(layout, order):
    """(index, G) on the host."""
    g = torch.Generator().manual_seed(17)
    if layout == "tiny":
        idx, G = torch.zeros(1, dtype=torch.int64), 1
    elif layout == "small":
        idx, G = torch.randint(0, 5, (63,), generator=g).sort().values, 5
    elif layout == "sizes":
        idx, G = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES)), len(SIZES)
        assert idx.numel() == 4880
    elif layout == "singletons":
        idx, G = torch.arange(1500), 1503
    elif layout == "one_group":
        idx, G = torch.zeros(200_003, dtype=torch.int64), 1
    elif layout == "two_level":
        n, G = 600_001, 300
        idx = torch.randint(0, G, (n,), generator=g)
        idx[torch.randperm(n, generator=g)[: n // 2]] = 1
        idx = idx.sort().values
    elif layout in ("pow2_19", "pow2_20"):
        G = 256 if layout == "pow2_19" else 512
        idx = torch.repeat_interleave(torch.arange(G), 2048)
    else:
        raise KeyError(layout)
    if order == "shuffled":
        idx = idx[torch.randperm(idx.numel(), generator=g)]
    return idx, G


@functools.lru_cache(maxsize=None)
def _plan(layout, order):
    from multigrad_amd.ops import GroupIndex
    idx, G = _index(layout, order)
    plan = GroupIndex(idx.to(DEV), G)
    assert (plan.perm is None) == (order == "sorted" or G == 1)  # one group is always sorted
    return plan


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """float32 inputs on the host: means around the bins, widths 0.1-0.5, signed weights with
    every 7th an exact zero."""
    g = torch.Generator().manual_seed(seed + n)
    mu = 9.0 + 1.6 * torch.rand(n, generator=g)
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g)
    w = torch.randn(n, generator=g)
    w[::7] = 0.0
    if n == 1:
        mu, w = torch.tensor([9.7]), torch.tensor([-1.3])
    return mu, sigma, w


def _modes(mu, sigma, w, sigma_mode, w_mode):
    sigma = sigma if sigma_mode == "per-object" else sigma[:1].clone()
    w = {"none": None, "per-object": w, "one-element": torch.tensor([-0.7])}[w_mode]
    return mu, sigma, w


def _cotangent(G, nb, like=None):
    c = torch.linspace(0.5, 1.5, nb, dtype=torch.float64)[None, :] * \
        (1.0 + (torch.arange(G) % 5).double()[:, None] / 4.0)
    return c if like is None else c.to(like)


def _oracle(idx, G, mu, sigma, w, edges, wrt):
    """The float64 torch path on the float32-rounded inputs: the rows, W_g, A_gk, the
    gradients of sum_gk G_gk out_gk for the operands named in ``wrt`` and, for a broadcast
    operand, the per-object terms t_i of its gradient."""
    from multigrad_amd.ops import GroupIndex
    plan = GroupIndex(idx, G)
    n = mu.numel()
    t = {"mu": mu.double().clone(), "sigma": sigma.double().clone(),
         "weights": None if w is None else w.double().clone()}
    for k in wrt:
        t[k].requires_grad_(True)
    out = plan.binned_sum(t["mu"], t["sigma"], edges, t["weights"])
    assert out.dtype == torch.float64 and out.shape == (G, len(edges) - 1)
    cot = _cotangent(G, len(edges) - 1)
    grads = dict(zip(wrt, torch.autograd.grad(out, [t[k] for k in wrt], cot))) if wrt else {}
    absw = torch.ones(n, dtype=torch.float64) if w is None else w.double().abs().expand(n)
    W = torch.zeros(G, dtype=torch.float64).index_add_(0, idx, absw)
    A = plan.binned_sum(mu.double(), sigma.double(), edges, absw.contiguous())
    terms = {}
    for k in wrt:
        if t[k].numel() == 1 and n > 1:  # the per-object terms of a reduced gradient
            full = {q: (None if v is None else v.detach()) for q, v in t.items()}
            full[k] = full[k].expand(n).clone().requires_grad_(True)
            o = plan.binned_sum(full["mu"], full["sigma"], edges, full["weights"])
            (terms[k],) = torch.autograd.grad(o, full[k], cot)
    return out.detach(), W, A, grads, terms


def _wrt_all(w):
    return ("mu", "sigma") + (("weights",) if w is not None else ())


@functools.lru_cache(maxsize=None)
def _case(layout, nb, order, sigma_mode="per-object", w_mode="per-object"):
    idx, G = _index(layout, order)
    ops = _modes(*_inputs(idx.numel()), sigma_mode, w_mode)
    return ops, _oracle(idx, G, *ops, _edges(nb), _wrt_all(ops[2]))


def _run(plan, mu, sigma, w, edges, wrt):
    t = {"mu": mu, "sigma": sigma, "weights": w}
    for k in wrt:
        t[k] = t[k].detach().requires_grad_(True)
    out = plan.binned_sum(t["mu"], t["sigma"], edges, t["weights"])
    cot = _cotangent(plan.num_groups, len(edges) - 1, out)
    grads = torch.autograd.grad(out, [t[k] for k in wrt], cot) if wrt else ()
    return out.detach(), dict(zip(wrt, grads))


def _fwd_tol(W, A):
    return 3.2e-7 * W.numpy()[:, None] + 2e-5 * A.numpy()


def _check(out, grads, oracle, empty=None):
    ref, W, A, gref, terms = oracle
    out = out.cpu().double().numpy()
    assert out.shape == tuple(ref.shape) and np.isfinite(out).all()
    err = np.abs(out - ref.numpy())
    tol = _fwd_tol(W, A)
    print("forward err/tol", float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    if empty is not None:
        assert (out[empty] == 0).all()
    for k, g in grads.items():
        g = g.cpu().double().numpy().reshape(-1)
        r = gref[k].numpy().reshape(-1)
        assert g.shape == r.shape and np.isfinite(g).all()
        if k in terms:
            a = terms[k].abs().numpy()
            tol = 2e-4 * a.sum() + 2e-5 * a.max()
            print(k, "reduced grad err/tol", float(np.abs(g - r).max() / tol))
            assert (np.abs(g - r) <= tol).all(), k
        else:
            atol = 2e-5 * float(np.abs(r).max())
            print(k, "grad err/tol", float((np.abs(g - r) / (atol + 2e-4 * np.abs(r))).max()))
            np.testing.assert_allclose(g, r, rtol=2e-4, atol=atol, err_msg=k)


def _dev(ops):
    return tuple(None if t is None else t.to(DEV) for t in ops)


def _empty_groups(layout, order):
    idx, G = _index(layout, order)
    return np.bincount(idx.numpy(), minlength=G) == 0


CASES = [("tiny", 1, "sorted")] + [(a, b, o) for a, b in LAYOUTS for o in ORDERS]


@pytest.mark.parametrize("layout,nb,order", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_forward_and_gradients_match_fp64(layout, nb, order):
    ops, oracle = _case(layout, nb, order)
    plan = _plan(layout, order)
    out, grads = _run(plan, *_dev(ops), _edges(nb), tuple(oracle[3]))
    assert out.shape == (plan.num_groups, nb) and out.dtype == torch.float32 and out.is_cuda
    for k, t in zip(("mu", "sigma", "weights"), ops):
        assert grads[k].shape == t.shape
    _check(out, grads, oracle, _empty_groups(layout, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("w_mode", ["none", "per-object", "one-element"])
@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
def test_operand_modes(sigma_mode, w_mode, order):
    ops, oracle = _case("sizes", 10, order, sigma_mode, w_mode)
    out, grads = _run(_plan("sizes", order), *_dev(ops), _edges(10), tuple(oracle[3]))
    assert grads["sigma"].shape == ops[1].shape
    if ops[2] is not None:
        assert grads["weights"].shape == ops[2].shape
    _check(out, grads, oracle, _empty_groups("sizes", order))


@pytest.mark.parametrize("order", ORDERS)
def test_edge_inputs_stay_finite_and_accurate(order):
    nb = 10
    edges = _edges(nb)
    idx, G = _index("sizes", order)
    mu, sigma, w = (t.clone() for t in _inputs(idx.numel()))
    sigma[:200] = 1e-3                       # step functions
    mu[0] = edges[3]                         # exactly on an edge (a step function)
    mu[300] = edges[5]                       # exactly on an edge, ordinary width
    mu[400:420] = edges[0] - 50.0 * sigma[400:420]     # 50 sigma below every edge
    mu[420:440] = edges[-1] + 50.0 * sigma[420:440]    # 50 sigma above every edge
    w[[0, 300, 400, 420]] = 1.0
    wrt = ("mu", "sigma", "weights")
    oracle = _oracle(idx, G, mu, sigma, w, edges, wrt)
    out, grads = _run(_plan("sizes", order), *_dev((mu, sigma, w)), edges, wrt)
    _check(out, grads, oracle)


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


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("which", ["mu", "weights"])
@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout, which, order):
    nb = 10
    edges = _edges(nb)
    ops, oracle = _case("sizes", nb, order)
    wrt = tuple(oracle[3])
    plan = _plan("sizes", order)
    dops = list(_dev(ops))
    k = 0 if which == "mu" else 2
    dops[k] = _view(ops[k], layout)
    out, grads = _run(plan, *dops, edges, wrt)
    _check(out, grads, oracle)
    # the same values from aligned contiguous tensors: same bits (the load path does not
    # change the arithmetic)
    out2, grads2 = _run(plan, *_dev(ops), edges, wrt)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize("sigma_mode,w_mode", [("per-object", "per-object"),
                                               ("broadcast", "one-element")])
@pytest.mark.parametrize("wrt", [("mu",), ("sigma",), ("weights",), ("mu", "weights")],
                         ids=["mu", "sigma", "weights", "mu+weights"])
def test_gradient_subsets(wrt, sigma_mode, w_mode):
    nb = 10
    edges = _edges(nb)
    idx, G = _index("sizes", "shuffled")
    ops = _modes(*_inputs(idx.numel()), sigma_mode, w_mode)
    oracle = _oracle(idx, G, *ops, edges, wrt)
    out, grads = _run(_plan("sizes", "shuffled"), *_dev(ops), edges, wrt)
    assert set(grads) == set(wrt)
    _check(out, grads, oracle)


def test_bitwise_deterministic():
    nb = 10
    idx, _ = _index("two_level", "shuffled")
    ops = _inputs(idx.numel())
    wrt = ("mu", "sigma", "weights")
    args = (_plan("two_level", "shuffled"), *_dev(ops), _edges(nb), wrt)
    a = _run(*args)
    b = _run(*args)
    assert torch.equal(a[0], b[0])
    for k in wrt:
        assert torch.equal(a[1][k], b[1][k]), k


def test_float64_device_input_takes_torch_path():
    nb = 10
    ops, (ref, _, _, gref, _) = _case("sizes", nb, "shuffled")
    wrt = tuple(gref)
    out, grads = _run(_plan("sizes", "shuffled"), *(t.double().to(DEV) for t in ops), _edges(nb),
                      wrt)
    assert out.dtype == torch.float64 and out.is_cuda
    np.testing.assert_allclose(out.cpu(), ref, rtol=0, atol=1e-12)
    for k in wrt:
        np.testing.assert_allclose(grads[k].cpu(), gref[k], rtol=0, atol=1e-12)


def test_device_edges_raise():
    mu, sigma, w = _dev(_inputs(63))
    with pytest.raises(TypeError, match="setup"):
        _plan("small", "sorted").binned_sum(mu, sigma, torch.tensor(_edges(4), device=DEV), w)


def _single_tol(ref_row, W_g):
    return 2.2e-7 * W_g + 2e-5 * np.abs(ref_row)


def test_one_group_agrees_with_the_single_op():
    """G = 1 against gaussian_binned_sum on the device, within the sum of both forward
    tolerances (not bitwise: the traversal differs)."""
    from multigrad_amd.ops import gaussian_binned_sum
    nb = 10
    ops, (ref, W, A, _, _) = _case("one_group", nb, "sorted")
    dops = _dev(ops)
    out = _plan("one_group", "sorted").binned_sum(dops[0], dops[1], _edges(nb), dops[2])
    single = gaussian_binned_sum(dops[0], dops[1], _edges(nb), dops[2])
    err = (out[0].double() - single.double()).abs().cpu().numpy()
    tol = _fwd_tol(W, A)[0] + _single_tol(ref.numpy()[0], float(W[0]))
    print("group vs single err/tol", float((err / tol).max()))
    assert (err <= tol).all()


@pytest.mark.parametrize("order", ORDERS)
def test_rows_agree_with_the_single_op_on_slices(order):
    from multigrad_amd.ops import gaussian_binned_sum
    nb = 10
    ops, (ref, W, A, _, _) = _case("sizes", nb, order)
    idx, G = _index("sizes", order)
    plan = _plan("sizes", order)
    dops = _dev(ops)
    out = plan.binned_sum(dops[0], dops[1], _edges(nb), dops[2])
    perm = torch.argsort(idx, stable=True).to(DEV)
    smu, ssig, sw = (t[perm] for t in dops)
    tol = _fwd_tol(W, A)
    lo = 0
    for g, L in enumerate(SIZES):
        if L:
            row = gaussian_binned_sum(smu[lo:lo + L], ssig[lo:lo + L], _edges(nb), sw[lo:lo + L])
            err = (out[g].double() - row.double()).abs().cpu().numpy()
            assert (err <= tol[g] + _single_tol(ref.numpy()[g], float(W[g]))).all(), g
        lo += L


@pytest.mark.parametrize("layout", ["sizes", "two_level"])
def test_agrees_with_the_segment_sum_composite(layout):
    """plan.segment_sum over the nb columns of a device ndtr table meets the same forward
    contract, so the two agree within twice the tolerance."""
    nb = 10
    ops, (ref, W, A, _, _) = _case(layout, nb, "shuffled")
    plan = _plan(layout, "shuffled")
    mu, sigma, w = _dev(ops)
    out = plan.binned_sum(mu, sigma, _edges(nb), w)
    e = torch.tensor(_edges(nb), device=DEV)
    cdf = torch.special.ndtr((e[:, None] - mu[None, :]) / sigma[None, :])
    comp = torch.stack(plan.segment_sum(*((cdf[1:] - cdf[:-1]) * w[None, :]).unbind(0)), dim=1)
    err = (out.double() - comp.double()).abs().cpu().numpy()
    tol = 2.0 * _fwd_tol(W, A)
    print("group vs composite err/tol", float((err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all()


def test_captured_engine_matches_eager_and_fp64_model():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (SampleBinnedPopulationSMFModel,
                                                       sample_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    aux = sample_population_data(data)
    guess = data["guess"]
    m = SampleBinnedPopulationSMFModel(aux_data=aux)
    assert m.samples.perm is not None
    ref = m.run_adam(guess, nsteps=6, learning_rate=1e-3, use_engine=False)
    eng = GraphAdamEngine(m, graph=True)
    traj = eng.run_adam(guess, nsteps=6, learning_rate=1e-3)
    assert eng.use_graph and eng.graph is not None and eng.fallback_reason is None, \
        eng.fallback_reason
    torch.testing.assert_close(traj, ref, rtol=1e-5, atol=1e-6)

    # float64 torch path of the same model on the same float32-rounded data and parameters
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    m64 = SampleBinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    p64 = guess.double()
    loss64, grad64 = m64.calc_loss_and_grad_from_params(p64)
    loss, grad = m.calc_loss_and_grad_from_params(guess)
    S64 = m64.calc_sumstats_from_params(p64)
    S = m.calc_sumstats_from_params(guess)
    nb = aux["edges"].numel() - 1
    ns = aux["nsamples"]
    assert S.dtype == torch.float32 and S.shape == (ns * nb,)
    scale = aux64["scale"]
    # forward contract per sample: unit weights, so W_g = L_g and A_gk = the bin sum itself
    W = m.samples.counts.double().repeat_interleave(nb)
    tolS = (3.2e-7 * W + 2e-5 * (S64 / scale).abs()) * scale
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
