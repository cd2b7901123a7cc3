"""GroupIndex / gather / segment_sum on the CPU: the contract of the plan and of the two ops
(the torch path, which is also the numerics oracle of the HIP kernels), autograd to second
order, the model that uses them, and the example and benchmark scripts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multigrad_amd.ops import GroupIndex, group_gather, segment_sum
from multigrad_amd.ops.groups import CHUNK, summation_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 9 objects in 7 groups; groups 0, 3 and 6 (start, middle, end) are empty
IDS = [2, 1, 5, 2, 2, 4, 1, 5, 2]
G = 7


def _vals(n, seed, dtype=torch.float64):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=dtype)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_plan_and_tuple_contract(idtype):
    index = torch.tensor(IDS, dtype=idtype)
    plan = GroupIndex(index, G)
    assert (plan.n, plan.num_groups, plan.device, plan.is_sorted) == (9, G, index.device, False)
    assert plan.counts.tolist() == [0, 2, 4, 0, 1, 2, 0]
    assert plan.offsets.tolist() == [0, 0, 2, 6, 6, 7, 9]
    assert plan.ids.dtype == torch.int32 and plan.ids.tolist() == IDS
    assert plan.sorted_ids.tolist() == sorted(IDS)
    # the permutation is the stable sort: objects of a group stay in object order
    assert plan.perm.tolist() == [1, 6, 0, 3, 4, 8, 5, 2, 7]
    a, b = _vals(G, 1), _vals(G, 2)
    out = plan.gather(a, b)
    assert isinstance(out, tuple) and len(out) == 2
    long_index = index.long()
    assert torch.equal(out[0], a[long_index]) and torch.equal(out[1], b[long_index])
    assert all(o.is_contiguous() and o.shape == (9,) for o in out)
    one = plan.gather(a)
    assert isinstance(one, tuple) and len(one) == 1
    x, y = _vals(9, 3), _vals(9, 4)
    tot = plan.segment_sum(x, y)
    assert isinstance(tot, tuple) and len(tot) == 2
    for t, src in zip(tot, (x, y)):
        ref = torch.zeros(G, dtype=torch.float64).index_add_(0, long_index, src)
        np.testing.assert_allclose(t, ref, rtol=0, atol=1e-12)
        assert t.shape == (G,) and t.is_contiguous()
        assert (t[[0, 3, 6]] == 0).all()          # empty groups: exactly 0
    # the functional aliases and five operands (more than one launch's worth)
    assert torch.equal(group_gather(plan, a)[0], out[0])
    assert torch.equal(segment_sum(plan, x)[0], tot[0])
    five = plan.gather(a, b, a, b, a)
    assert len(five) == 5 and torch.equal(five[4], out[0])


def test_sorted_index_and_index_shape():
    index = torch.tensor([[0, 0, 1], [1, 3, 3]])
    plan = GroupIndex(index, 4)
    assert plan.is_sorted and plan.perm is None and plan.n == 6
    v = _vals(4, 5)
    out, = plan.gather(v)
    assert out.shape == (6,) and torch.equal(out, v[index.reshape(-1)])
    x = _vals(6, 6)
    tot, = plan.segment_sum(x.reshape(2, 3))      # operands are treated as flat, too
    np.testing.assert_allclose(tot, [x[0] + x[1], x[2] + x[3], 0.0, x[4] + x[5]], atol=1e-12)
    leaf = x.reshape(2, 3).clone().requires_grad_(True)
    g, = torch.autograd.grad(plan.segment_sum(leaf)[0], leaf, v)
    assert g.shape == (2, 3) and torch.equal(g.reshape(-1), out)


def test_empty_index():
    plan = GroupIndex(torch.zeros(0, dtype=torch.int64), 3)
    assert plan.n == 0 and plan.is_sorted and plan.counts.tolist() == [0, 0, 0]
    v = _vals(3, 7).requires_grad_(True)
    out, = plan.gather(v)
    assert out.shape == (0,)
    gv, = torch.autograd.grad(out.sum(), v)
    assert torch.equal(gv, torch.zeros(3, dtype=torch.float64))
    x = torch.zeros(0, dtype=torch.float64, requires_grad=True)
    tot, = plan.segment_sum(x)
    assert tot.shape == (3,) and (tot == 0).all()
    gx, = torch.autograd.grad(tot.sum(), x)
    assert gx.shape == (0,)


def test_errors():
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        GroupIndex(torch.tensor([0, 4, 1]), 4)               # out of range
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        GroupIndex(torch.tensor([0, -1, 1]), 4)              # negative
    with pytest.raises(TypeError):
        GroupIndex(torch.tensor([0.0, 1.0]), 4)              # not an integer index
    plan = GroupIndex(torch.tensor(IDS), G)
    with pytest.raises(ValueError, match="elements"):
        plan.gather(_vals(G + 1, 1))                         # wrong operand length
    with pytest.raises(ValueError, match="elements"):
        plan.segment_sum(_vals(8, 1))
    with pytest.raises(ValueError, match="dtype and device"):
        plan.gather(_vals(G, 1), _vals(G, 2, torch.float32))  # dtype mismatch
    with pytest.raises(ValueError, match="dtype and device"):
        plan.segment_sum(_vals(9, 1), _vals(9, 2).to("meta"))  # device mismatch
    with pytest.raises(ValueError, match="plan"):
        plan.gather(_vals(G, 1).to("meta"))                  # not the plan's device
    with pytest.raises(ValueError):
        plan.gather()
    with pytest.raises(TypeError):
        plan.gather(torch.arange(G))                         # integer operand


def test_none_output_gradient_is_not_materialised():
    plan = GroupIndex(torch.tensor(IDS), G)
    a = _vals(G, 1).requires_grad_(True)
    b = _vals(G, 2).requires_grad_(True)
    oa, ob = plan.gather(a, b)
    ct = _vals(9, 3)
    ga, gb = torch.autograd.grad(oa, (a, b), ct, allow_unused=True)
    assert gb is None                                        # a zero column never existed
    ref = torch.zeros(G, dtype=torch.float64).index_add_(0, torch.tensor(IDS), ct)
    np.testing.assert_allclose(ga, ref, rtol=0, atol=1e-12)
    # an operand that does not require grad gets no gradient either
    c = _vals(G, 4)
    oa, oc = plan.gather(a, c)
    ga2, = torch.autograd.grad((oa * ct).sum() + oc.sum(), a)
    np.testing.assert_allclose(ga2, ref, rtol=0, atol=1e-12)
    x = _vals(9, 5).requires_grad_(True)
    y = _vals(9, 6).requires_grad_(True)
    tx, ty = plan.segment_sum(x, y)
    gx, gy = torch.autograd.grad(ty, (x, y), c, allow_unused=True)
    assert gx is None and torch.equal(gy, c[torch.tensor(IDS)])


def test_gradcheck_and_gradgradcheck_float64():
    plan = GroupIndex(torch.tensor([2, 0, 3, 2, 2, 0, 3]), 4)    # N = 7, G = 4, group 1 empty
    a = _vals(4, 1).requires_grad_(True)
    b = _vals(4, 2).requires_grad_(True)
    x = _vals(7, 3).requires_grad_(True)
    y = _vals(7, 4).requires_grad_(True)
    assert torch.autograd.gradcheck(plan.gather, (a, b))
    assert torch.autograd.gradgradcheck(plan.gather, (a, b))
    assert torch.autograd.gradcheck(plan.segment_sum, (x, y))
    assert torch.autograd.gradgradcheck(plan.segment_sum, (x, y))
    # through a nonlinearity, so that the second order is not identically zero
    f = lambda a, x: (plan.gather(a)[0] ** 2 * x).sum() + (plan.segment_sum(x * x)[0] * a).sum()
    assert torch.autograd.gradcheck(f, (a, x)) and torch.autograd.gradgradcheck(f, (a, x))


def test_summation_depth():
    for L in list(range(0, 3 * CHUNK)) + [CHUNK * CHUNK, 599_990, 4_000_000, 10 ** 8, 2 ** 31 - 1]:
        d = summation_depth(L)
        assert 0 <= d <= 4 + 2 * math.ceil(math.log2(max(L, 2))), (L, d)
        assert d <= max(L - 1, 0)
    assert [summation_depth(L) for L in (0, 1, 2, 3)] == [0, 0, 1, 2]
    # the depth grows with the logarithm of L, not with L
    assert summation_depth(10 ** 8) <= summation_depth(10 ** 4) + 3 * 14


def _float64_population(npop, nhalo):
    """``npop`` populations (two parameters each) over ``nhalo`` halos."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import torch_population_data
    data = make_population_data(2 * npop, nhalo, seed=11, device="cpu")
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    aux = torch_population_data(data)
    aux64 = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
             for k, v in aux.items()}
    return aux, aux64, data["guess"]


def test_grouped_model_matches_binned_model_float64():
    from multigrad_amd.models.torch_population import (BinnedPopulationSMFModel,
                                                       GroupedBinnedPopulationSMFModel)
    aux, aux64, guess = _float64_population(200, 4000)
    ref = BinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    new = GroupedBinnedPopulationSMFModel(aux_data=aux64, dtype=torch.float64)
    assert new.groups.n == 4000 and new.groups.num_groups == 200
    l0, g0 = ref.calc_loss_and_grad_from_params(guess.double())
    l1, g1 = new.calc_loss_and_grad_from_params(guess.double())
    assert g1.dtype == torch.float64
    np.testing.assert_allclose(float(l1), float(l0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=0, atol=1e-12)


def test_generic_engine_matches_eager():
    from multigrad_amd.engine.generic import GraphAdamEngine
    from multigrad_amd.models.torch_population import GroupedBinnedPopulationSMFModel
    from multigrad_amd.parallel import comm as C
    C.set_world_comm(None)
    aux, _, guess = _float64_population(200, 4000)
    m = GroupedBinnedPopulationSMFModel(aux_data=aux)
    ref = m.run_adam(guess, nsteps=5, learning_rate=1e-3, use_engine=False)
    traj = GraphAdamEngine(m).run_adam(guess, nsteps=5, learning_rate=1e-3)
    assert traj.shape == (6, 400)
    torch.testing.assert_close(traj, ref, rtol=0, atol=0)
    assert not torch.equal(traj[-1], traj[0])


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; "
            "assert 'multigrad_amd.ops.groups' not in sys.modules; "
            "p = o.GroupIndex; o.group_gather; o.segment_sum; "
            "assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


CASES = [
    ("examples/user_model_groups.py", ["--num-objects", "3000", "--num-steps", "150"]),
    ("benchmarks/group_ops.py", ["--cpu"]),
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
