"""gaussian_binned_sum_by_group on the CPU: the torch path of the op (the formulas the HIP
kernels implement) against the ndtr + index_add_ composite, the single op and autograd, the
per-sample model that uses it, the argument checks, and the example and benchmark scripts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distributed import run_distributed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _inputs(n, G, seed=0, shuffled=True, empty=()):
    """mu, sigma, signed weights and a group index that leaves the groups in ``empty``
    without objects."""
    g = torch.Generator().manual_seed(seed)
    mu = 9.0 + 1.5 * torch.rand(n, generator=g, dtype=F64)
    sigma = 0.1 + 0.4 * torch.rand(n, generator=g, dtype=F64)
    w = torch.randn(n, generator=g, dtype=F64)
    live = torch.tensor([k for k in range(G) if k not in empty])
    index = live[torch.randint(0, live.numel(), (n,), generator=g)]
    if not shuffled:
        index = index.sort().values
    return mu, sigma, w, index


def _composite(index, G, mu, sigma, edges, w):
    e = torch.as_tensor(np.asarray(edges), dtype=mu.dtype)
    cdf = torch.special.ndtr((e[None, :] - mu.reshape(-1)[:, None]) / sigma.reshape(-1, 1))
    d = cdf[:, 1:] - cdf[:, :-1]
    if w is not None:
        d = d * w.reshape(-1, 1)
    return torch.zeros(G, e.numel() - 1, dtype=mu.dtype).index_add_(0, index, d)


def _leaf(t):
    return None if t is None else t.clone().requires_grad_(True)


@pytest.mark.parametrize("sigma_mode", ["per-object", "broadcast"])
@pytest.mark.parametrize("weights", ["none", "per-object", "one-element"])
@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_rows_and_gradients_match_the_composite(shuffled, weights, sigma_mode):
    from multigrad_amd.ops import GroupIndex, gaussian_binned_sum_by_group
    n, G, nb = 300, 7, 6
    edges = np.linspace(9.1, 10.4, nb + 1)
    mu, sigma, w, index = _inputs(n, G, seed=3, shuffled=shuffled, empty=(2,))
    sigma = sigma if sigma_mode == "per-object" else sigma[:1]
    w = {"none": None, "per-object": w, "one-element": torch.tensor([-0.7], dtype=F64)}[weights]
    plan = GroupIndex(index, G)
    assert (plan.perm is None) == (not shuffled)
    cot = torch.linspace(0.5, 1.5, G * nb, dtype=F64).reshape(G, nb)

    a = [_leaf(mu), _leaf(sigma), _leaf(w)]
    out = gaussian_binned_sum_by_group(plan, a[0].reshape(3, 100), a[1], edges, a[2])
    assert out.shape == (G, nb) and out.dtype == F64
    assert (out[2] == 0).all()
    got = torch.autograd.grad(out, [t for t in a if t is not None], cot)

    b = [_leaf(mu), _leaf(sigma), _leaf(w)]
    ref = _composite(index, G, *b[:2], edges, b[2])
    want = torch.autograd.grad(ref, [t for t in b if t is not None], cot)
    np.testing.assert_allclose(out.detach(), ref.detach(), rtol=0, atol=1e-12)
    for x, y in zip(got, want):
        assert x.shape == y.shape
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)
    # the method of the plan, and edges given as a list or a CPU tensor: identical results
    assert torch.equal(plan.binned_sum(mu, sigma, edges, w), out.detach())
    for conv in (list, torch.tensor):
        assert torch.equal(plan.binned_sum(mu, sigma, conv(list(edges)), w), out.detach())


def test_one_group_and_column_sums_equal_the_single_op():
    from multigrad_amd.ops import GroupIndex, gaussian_binned_sum
    n, nb = 200, 5
    edges = np.linspace(9.1, 10.4, nb + 1)
    mu, sigma, w, index = _inputs(n, 6, seed=4)
    one = GroupIndex(torch.zeros(n, dtype=torch.int64), 1).binned_sum(mu, sigma, edges, w)
    single = gaussian_binned_sum(mu, sigma, edges, w)
    assert one.shape == (1, nb)
    np.testing.assert_allclose(one[0], single, rtol=0, atol=1e-12)
    rows = GroupIndex(index, 6).binned_sum(mu, sigma, edges, w)
    np.testing.assert_allclose(rows.sum(0), single, rtol=0, atol=1e-12)


def test_gradcheck_float64():
    from multigrad_amd.ops import GroupIndex
    mu, sigma, w, index = _inputs(40, 6, seed=1, empty=(4,))
    plan = GroupIndex(index, 6)
    assert int(plan.counts[4]) == 0 and plan.perm is not None
    edges = (9.2, 9.6, 9.9, 10.4)
    for sig, wt in ((sigma, w), (sigma[:1], w[:1])):
        args = tuple(t.clone().requires_grad_(True) for t in (mu, sig, wt))
        f = lambda m, s, u: plan.binned_sum(m, s, edges, u)
        assert f(*args).shape == (6, 3)
        assert torch.autograd.gradcheck(f, args)


def test_chunk_independence():
    from multigrad_amd.ops import GroupIndex
    mu, sigma, w, index = _inputs(23, 4, seed=3)
    plan = GroupIndex(index, 4)
    edges = np.linspace(9.1, 10.4, 4)
    cot = torch.linspace(0.5, 1.5, 12, dtype=F64).reshape(4, 3)
    res = []
    for chunk in (7, None):
        a = [_leaf(mu), _leaf(sigma[:1]), _leaf(w)]
        out = plan.binned_sum(a[0], a[1], edges, a[2], chunk=chunk)
        res.append([out.detach()] + list(torch.autograd.grad(out, a, cot)))
    for x, y in zip(*res):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12)


def test_argument_errors():
    from multigrad_amd.ops import GroupIndex
    from multigrad_amd.ops import gaussian_binned_sum_by_group as f
    mu, sigma, w, index = _inputs(5, 3)
    plan = GroupIndex(index, 3)
    ok = [9.0, 9.5, 10.0]
    assert f(plan, mu, sigma, ok, w).shape == (3, 2)
    with pytest.raises(TypeError, match="GroupIndex"):
        f(index, mu, sigma, ok, w)                               # not a plan
    with pytest.raises(ValueError, match="mu"):
        f(plan, mu[:4], sigma[:4], ok)                           # wrong element count
    with pytest.raises(ValueError, match="sigma"):
        f(plan, mu, sigma[:3], ok)
    with pytest.raises(ValueError, match="weights"):
        f(plan, mu, sigma, ok, w[:3])
    with pytest.raises(ValueError, match="sigma"):
        f(plan, mu, sigma.float(), ok)                           # wrong dtype
    with pytest.raises(ValueError, match="weights"):
        f(plan, mu, sigma, ok, w.float())
    with pytest.raises(ValueError, match="sigma"):
        f(plan, mu, sigma.to("meta"), ok)                        # wrong device
    with pytest.raises(ValueError, match="weights"):
        f(plan, mu, sigma, ok, w.to("meta"))
    with pytest.raises(ValueError, match="mu"):
        f(plan, torch.arange(5), torch.arange(5), ok)            # not floating point
    with pytest.raises(ValueError, match="the plan on"):
        f(plan, mu.to("meta"), sigma.to("meta"), ok)             # not the plan's device
    with pytest.raises(ValueError):
        f(plan, mu, sigma, np.linspace(0, 1, 34))                # nb = 33
    assert f(plan, mu, sigma, np.linspace(0, 1, 33)).shape == (3, 32)
    for bad in ([9.0, 9.5, 9.4, 10.0], [9.0, 9.5, 9.5], [9.0, float("inf")], [9.0]):
        with pytest.raises(ValueError):
            f(plan, mu, sigma, bad)
    with pytest.raises(TypeError, match="setup"):
        f(plan, mu, sigma, torch.tensor(ok, device="meta"))      # device edges
    with pytest.raises(TypeError):
        f(plan, mu.numpy(), sigma, ok)
    with pytest.raises(TypeError):
        f(plan, mu, sigma, ok, 2.0)


def test_empty_inputs():
    from multigrad_amd.ops import GroupIndex
    z = lambda n: torch.zeros(n, dtype=F64, requires_grad=True)
    one = lambda: torch.ones(1, dtype=F64, requires_grad=True)
    none = torch.zeros(0, dtype=torch.int64)
    for G in (4, 0):
        plan = GroupIndex(none, G)
        mu, sigma, w = z(0), one(), one()
        out = plan.binned_sum(mu, sigma, [9.0, 9.5, 10.0], w)
        assert out.shape == (G, 2) and out.dtype == F64 and (out == 0).all()
        g = torch.autograd.grad(out.sum(), (mu, sigma, w))
        assert g[0].shape == (0,)
        assert g[1].shape == (1,) and float(g[1]) == 0.0
        assert g[2].shape == (1,) and float(g[2]) == 0.0
        mu, sigma, w = z(0), z(0), z(0)
        out = plan.binned_sum(mu, sigma, [9.0, 9.5, 10.0], w)
        g = torch.autograd.grad(out.sum(), (mu, sigma, w))
        assert all(t.shape == (0,) for t in g)


def test_double_backward_raises():
    from multigrad_amd.ops import GroupIndex
    mu, sigma, w, index = _inputs(20, 3, seed=5)
    mu = mu.requires_grad_(True)
    out = GroupIndex(index, 3).binned_sum(mu, sigma, [9.0, 9.5, 10.0], w)
    # a cotangent that depends on mu, so that the first backward is part of the graph
    (g,) = torch.autograd.grad((out * out).sum(), mu, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # with a constant cotangent the first backward is not recorded at all: no silent zeros
    (g,) = torch.autograd.grad(out.sum(), mu, create_graph=True)
    assert not g.requires_grad


def test_forward_ad_raises_not_implemented():
    import torch.autograd.forward_ad as fwad
    from multigrad_amd.ops import GroupIndex
    mu, sigma, w, index = _inputs(20, 3, seed=5)
    plan = GroupIndex(index, 3)
    with fwad.dual_level():
        dual = fwad.make_dual(mu, torch.ones_like(mu))
        with pytest.raises(NotImplementedError):
            plan.binned_sum(dual, sigma, [9.0, 9.5, 10.0], w)


def test_lazy_export_does_not_load_the_extension():
    code = ("import sys, multigrad_amd.ops as o; "
            "assert 'multigrad_amd.ops.binned_group' not in sys.modules; "
            "f = o.gaussian_binned_sum_by_group; "
            "assert 'multigrad_amd.ops.binned_group' in sys.modules; "
            "assert 'multigrad_amd._C' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def _sample_model64(nsamples=3, comm=None):
    """The per-sample model in float64 on one rank's full catalog, its masked-weights twin and
    the guess."""
    from dataclasses import dataclass

    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (SampleBinnedPopulationSMFModel,
                                                       sample_population_data)
    from multigrad_amd.ops import gaussian_binned_sum
    from multigrad_amd.parallel.comm import SerialComm

    @dataclass(eq=False)
    class MaskedCalls(SampleBinnedPopulationSMFModel):
        def _sums(self, mu, sigma):
            s = self.aux_data["sample"]
            return torch.stack([gaussian_binned_sum(mu, sigma, self.edges, (s == k).to(mu.dtype))
                                for k in range(self.aux_data["nsamples"])])

    comm = comm or SerialComm()
    data = make_population_data(400, 6000, seed=11, device="cpu", comm=comm)
    aux = sample_population_data(data, nsamples=nsamples)
    aux = {k: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
           for k, v in aux.items()}
    new = SampleBinnedPopulationSMFModel(aux_data=aux, dtype=F64, comm=comm)
    with torch.no_grad():
        aux["target"] = new.calc_sumstats_from_params(data["truth"].double())
    return new, MaskedCalls(aux_data=aux, dtype=F64, comm=comm), data["guess"].double()


def test_sample_model_matches_masked_single_op_calls():
    new, ref, guess = _sample_model64()
    aux = new.aux_data
    nb = aux["edges"].numel() - 1
    assert aux["sample"].shape == aux["x"].shape and new.samples.perm is not None
    assert int(aux["sample"].min()) == 0 and int(aux["sample"].max()) == 2
    assert aux["target"].shape == (3 * nb,) and (aux["target"] > 0).all()
    assert aux["scale"].shape == (3 * nb,)
    S0, S1 = ref.calc_sumstats_from_params(guess), new.calc_sumstats_from_params(guess)
    np.testing.assert_allclose(S1.numpy(), S0.numpy(), rtol=0, atol=1e-10 * float(S0.abs().max()))
    l0, g0 = ref.calc_loss_and_grad_from_params(guess)
    l1, g1 = new.calc_loss_and_grad_from_params(guess)
    assert g1.dtype == F64 and float(g1.abs().max()) > 0
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-10)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-10,
                               atol=1e-10 * float(g0.abs().max()))


def test_jacobian_auto_mode_falls_back_to_reverse():
    from multigrad_amd.models.population import make_population_data
    from multigrad_amd.models.torch_population import (SampleBinnedPopulationSMFModel,
                                                       sample_population_data)
    data = make_population_data(8, 2000, seed=3, device="cpu")
    m = SampleBinnedPopulationSMFModel(aux_data=sample_population_data(data, nsamples=2))
    p = data["guess"]
    with pytest.raises(NotImplementedError):
        m.calc_sumstats_jacobian_from_params(p, mode="forward")
    S, J, _, used = m._sumstats_jacobian(p, mode="auto")
    assert used == "reverse"
    Sr, Jr = m.calc_sumstats_jacobian_from_params(p, mode="reverse")
    Sa, Ja = m.calc_sumstats_jacobian_from_params(p)
    assert Ja.shape == (S.numel(), 8) and float(Ja.abs().max()) > 0
    assert torch.equal(Sa, Sr) and torch.equal(Ja, Jr) and torch.equal(J, Jr)


def _two_rank_body(rank, size):
    import multigrad_amd as mg
    from multigrad_amd.models.torch_population import SampleBinnedPopulationSMFModel
    full, _, guess = _sample_model64()
    l0, g0 = full.calc_loss_and_grad_from_params(guess)
    aux = dict(full.aux_data)
    n = aux["x"].numel()
    lo, hi = rank * n // size, (rank + 1) * n // size
    for k in ("x", "pop", "sample"):
        aux[k] = aux[k][lo:hi].clone()
    half = SampleBinnedPopulationSMFModel(aux_data=aux, dtype=torch.float64,
                                          comm=mg.get_world_comm())
    assert half.comm.size == size and half.samples.n == hi - lo
    l1, g1 = half.calc_loss_and_grad_from_params(guess)
    np.testing.assert_allclose(float(l1), float(l0), rtol=1e-10)
    np.testing.assert_allclose(g1.numpy(), g0.numpy(), rtol=1e-10,
                               atol=1e-10 * float(g0.abs().max()))
    return float(l1)


def test_two_ranks_equal_one_rank():
    res = run_distributed(_two_rank_body, 2)
    assert res[0] == res[1]


CASES = [
    ("examples/user_model_samples.py", ["--num-halos", "3000", "--num-steps", "150"]),
    ("benchmarks/binned_group_op.py", ["--cpu"]),
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
