"""GroupIndex.gather / segment_sum on the MI355X: the HIP kernels (csrc/groups.hip) against
float64 ``index_add_`` on the CPU over the float32-rounded inputs.

gather forward : bitwise equal to ``values[index]``.
segment_sum (and the backward of gather), per group g of L_g objects:
    |got - ref| <= summation_depth(L_g) * 2**-24 * sum_{i in g} |x_i|
with summation_depth(L) <= 4 + 2 ceil(log2(max(L, 2))) asserted separately.
"""
import functools
import math

import numpy as np
import pytest
import torch

from multigrad_amd.ops import GroupIndex, group_gather, segment_sum
from multigrad_amd.ops.groups import CHUNK, summation_depth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = CHUNK
BIG = 600_001 if T <= 1024 else T * T // 2 + T + 1   # > one chunk of carries for one group


def _sizes_to_ids(sizes):
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(sizes.numel()), sizes)


def _geometric_sizes(n, g, seed=5):
    """Geometric group sizes (mean ~ n/g), about 10 % of the groups empty, summing to n."""
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.empty(g).geometric_(0.9 * g / n, generator=gen).long()
    sizes[torch.rand(g, generator=gen) < 0.1] = 0
    ends = torch.cumsum(sizes, 0).clamp_(max=n)
    sizes = torch.diff(ends, prepend=torch.zeros(1, dtype=torch.int64))
    sizes[0] += n - int(sizes.sum())
    return sizes


# name -> (sorted ids, G)
SHAPES = {
    "1x1": lambda: (torch.zeros(1, dtype=torch.int64), 1),
    "3x5": lambda: (torch.tensor([1, 1, 4]), 5),
    "T": lambda: (torch.zeros(T, dtype=torch.int64), 1),
    "T+1": lambda: (torch.zeros(T + 1, dtype=torch.int64), 1),
    "3T+1": lambda: (torch.zeros(3 * T + 1, dtype=torch.int64), 1),
    "singletons": lambda: (torch.arange(2 * T + 3), 2 * T + 3),
    "chunk-edge": lambda: (_sizes_to_ids([T, T - 1, 1, 2, 0, 5]), 6),
    "geometric": lambda: (_sizes_to_ids(_geometric_sizes(200_003, 20_000)), 20_000),
    "one-big": lambda: (_sizes_to_ids([BIG - 11, 3, 0, 8]), 4),
}


@functools.lru_cache(maxsize=None)
def _index(shape, order):
    ids, g = SHAPES[shape]()
    if order == "shuffled":
        ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(3))]
    return ids, g


@functools.lru_cache(maxsize=None)
def _plan(shape, order):
    ids, g = _index(shape, order)
    return GroupIndex(ids.to(DEV), g)


def _randn(n, seed):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    x[::7] = 0.0
    return x if n > 1 else torch.tensor([-1.3])


@functools.lru_cache(maxsize=None)
def _case(shape, order):
    """Four float32 columns of N and of G values (host), the float64 segment sums of the
    former, and the per-group tolerance unit depth * 2**-24 * sum |x|."""
    ids, g = _index(shape, order)
    n = ids.numel()
    xs = tuple(_randn(n, 10 + c) for c in range(4))
    vals = tuple(_randn(g, 20 + c) if g > 1 else torch.tensor([1.5 - c]) for c in range(4))
    counts = torch.bincount(ids, minlength=g)
    depth = torch.zeros(g, dtype=torch.float64)
    for L in torch.unique(counts).tolist():
        depth[counts == L] = summation_depth(L)
    ref, tol = [], []
    for x in xs:
        ref.append(torch.zeros(g, dtype=torch.float64).index_add_(0, ids, x.double()))
        tol.append(depth * 2.0 ** -24 *
                   torch.zeros(g, dtype=torch.float64).index_add_(0, ids, x.double().abs()))
    return ids, g, xs, vals, counts, tuple(ref), tuple(tol)


def _assert_sums(got, ref, tol, counts, what):
    assert len(got) == len(ref)
    for c, (o, r, t) in enumerate(zip(got, ref, tol)):
        assert o.dtype == torch.float32 and o.is_cuda and o.is_contiguous() and o.shape == r.shape
        o = o.cpu().double()
        assert torch.isfinite(o).all()
        err = (o - r).abs()
        worst = float((err / t.clamp_min(1e-300)).max()) if err.numel() else 0.0
        print(what, "column", c, "max err/tol", worst)
        assert (err <= t).all(), (what, c, worst)
        assert (o[counts == 0] == 0).all()


def test_summation_depth_cap():
    for L in list(range(0, 5000)) + [T * T, 599_990, 4_000_000, 10 ** 8, 2 ** 31 - 1]:
        d = summation_depth(L)
        assert 0 <= d <= 4 + 2 * math.ceil(math.log2(max(L, 2))), (L, d)
    assert summation_depth(1) == 0 and summation_depth(2) == 1


@pytest.mark.parametrize("ncols", [1, 2, 4])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gather_and_segment_sum(shape, order, ncols):
    ids, g, xs, vals, counts, ref, tol = _case(shape, order)
    plan = _plan(shape, order)
    assert plan.n == ids.numel() and plan.num_groups == g and plan.device == DEV
    assert plan.is_sorted == bool((ids[1:] >= ids[:-1]).all())
    assert torch.equal(plan.counts.cpu(), counts)
    # segment sum
    got = plan.segment_sum(*[x.to(DEV) for x in xs[:ncols]])
    assert isinstance(got, tuple)
    _assert_sums(got, ref[:ncols], tol[:ncols], counts, "segment_sum")
    # gather: exact, and its backward is the segment sum of the cotangents
    leaves = [v.to(DEV).requires_grad_(True) for v in vals[:ncols]]
    out = plan.gather(*leaves)
    assert isinstance(out, tuple) and len(out) == ncols
    for o, v in zip(out, leaves):
        assert o.is_contiguous() and o.shape == (ids.numel(),)
        assert torch.equal(o.detach(), v.detach()[ids.to(DEV)])
    grads = torch.autograd.grad(out, leaves, [x.to(DEV) for x in xs[:ncols]])
    _assert_sums(grads, ref[:ncols], tol[:ncols], counts, "gather backward")


def test_five_operands_take_two_launches():
    ids, g, xs, vals, counts, ref, tol = _case("chunk-edge", "shuffled")
    plan = _plan("chunk-edge", "shuffled")
    cols = [x.to(DEV) for x in xs] + [xs[1].to(DEV)]
    got = segment_sum(plan, *cols)
    _assert_sums(got, ref + (ref[1],), tol + (tol[1],), counts, "segment_sum x5")
    vs = [v.to(DEV) for v in vals] + [vals[2].to(DEV)]
    out = group_gather(plan, *vs)
    assert len(out) == 5
    for o, v in zip(out, vs):
        assert torch.equal(o, v[ids.to(DEV)])


def test_segment_sum_backward_is_gather():
    ids, g, xs, vals, counts, ref, tol = _case("chunk-edge", "shuffled")
    plan = _plan("chunk-edge", "shuffled")
    x = xs[0].to(DEV).requires_grad_(True)
    tot, = plan.segment_sum(x)
    ct = vals[0].to(DEV)
    gx, = torch.autograd.grad(tot, x, ct)
    assert torch.equal(gx, ct[ids.to(DEV)])


def test_missing_gradients():
    ids, g, xs, vals, counts, ref, tol = _case("geometric", "shuffled")
    plan = _plan("geometric", "shuffled")
    # only one operand requires grad
    a = vals[0].to(DEV).requires_grad_(True)
    b = vals[1].to(DEV)
    oa, ob = plan.gather(a, b)
    ga, = torch.autograd.grad((oa * xs[0].to(DEV)).sum() + ob.sum(), a)
    _assert_sums((ga,), ref[:1], tol[:1], counts, "one leaf")
    # both require grad, the second output is unused: its gradient is None, not zeros
    a = vals[0].to(DEV).requires_grad_(True)
    b = vals[1].to(DEV).requires_grad_(True)
    oa, ob = plan.gather(a, b)
    ga, gb = torch.autograd.grad(oa, (a, b), xs[0].to(DEV), allow_unused=True)
    assert gb is None
    _assert_sums((ga,), ref[:1], tol[:1], counts, "unused output")


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_memory_layouts(layout, order):
    ids, g, xs, vals, counts, ref, tol = _case("geometric", order)
    plan = _plan("geometric", order)
    n = ids.numel()
    x = xs[0].to(DEV)
    if layout == "offset":                   # a 4-byte-offset pointer: scalar loads
        buf = torch.zeros(n + 1, device=DEV)
        buf[1:] = x
        view = buf[1:]
        assert view.data_ptr() % 16 == 4
    else:                                    # non-contiguous
        buf = torch.zeros(2 * n, device=DEV)
        buf[::2] = x
        view = buf[::2]
        assert not view.is_contiguous()
    got, other = plan.segment_sum(view, xs[1].to(DEV))
    want, other2 = plan.segment_sum(x, xs[1].to(DEV))
    assert torch.equal(got, want) and torch.equal(other, other2)
    _assert_sums((got,), ref[:1], tol[:1], counts, layout)
    # a non-contiguous incoming gradient of gather
    a = vals[0].to(DEV).requires_grad_(True)
    out, = plan.gather(a)
    ga, = torch.autograd.grad(out, a, view if layout == "strided" else buf[1:])
    assert torch.equal(ga, want)


def test_bitwise_deterministic():
    ids, g, xs, vals, counts, ref, tol = _case("geometric", "shuffled")
    plan = _plan("geometric", "shuffled")
    cols = [x.to(DEV) for x in xs[:2]]
    a = plan.segment_sum(*cols)
    b = plan.segment_sum(*cols)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # a second plan of the same index gives the same bits too
    c = GroupIndex(ids.to(DEV), g).segment_sum(*cols)
    assert all(torch.equal(p, q) for p, q in zip(a, c))


def test_float64_device_input_takes_torch_path():
    ids, g, xs, vals, counts, ref, tol = _case("geometric", "shuffled")
    plan = _plan("geometric", "shuffled")
    x = xs[0].double().to(DEV).requires_grad_(True)
    tot, = plan.segment_sum(x)
    assert tot.dtype == torch.float64 and tot.is_cuda
    np.testing.assert_allclose(tot.detach().cpu(), ref[0], rtol=0, atol=1e-12)
    v = vals[0].double().to(DEV)
    out, = plan.gather(v)
    assert torch.equal(out, v[ids.to(DEV)])
    gx, = torch.autograd.grad(tot, x, v)
    assert torch.equal(gx, out)


def test_captured_engine_matches_eager_and_fp64_model():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       TorchPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(20_000, 400_000, seed=11, device=DEV)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    guess = data["guess"]
    m = GroupedBinnedPopulationSMFModel(aux_data=aux)
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
    # the binning op's forward contract on the bin sums (the gather in front of it is exact)
    tolS = (2.2e-7 * nhalo + 2e-5 * (S64 / scale).abs()) * scale
    errS = (S.double() - S64).abs()
    print("sumstats err/tol", float((errS / tolS).max()))
    assert (errS <= tolS).all(), (errS, tolS)
    dLdS = m64.calc_dloss_dsumstats(S64)
    tolL = float((dLdS.abs() * tolS).sum()) + 1e-5 * abs(float(loss64))
    print("loss err/tol", abs(float(loss) - float(loss64)) / tolL)
    assert abs(float(loss) - float(loss64)) <= tolL
    g64 = grad64.cpu().numpy()
    np.testing.assert_allclose(grad.cpu().double().numpy(), g64, rtol=2e-4,
                               atol=2e-5 * float(np.abs(g64).max()))
