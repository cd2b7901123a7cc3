"""The HMC sampler on the CPU: the three vector ops (torch fallbacks of csrc/hmc.hip) against
float64, reversibility, a chain against an independent float64 numpy HMC fed the same noise,
the moments of a whitened Gaussian, warm-up adaptation, the bounds Jacobian, two gloo ranks
against one, and the model front end.  The bodies that take a ``device`` run again on the
GPU from test_hmc_gpu.py."""
import math
import os
import subprocess
import sys
from dataclasses import dataclass

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distributed import run_distributed  # noqa: E402

from multigrad_amd.ops.hmc import hmc_commit_, hmc_leapfrog_, hmc_momentum_  # noqa: E402
from multigrad_amd.optim.hmc import KeyNoise, hmc_sample, run_hmc, warmup_windows  # noqa: E402
from multigrad_amd.optim.lbfgs import GenericObjective  # noqa: E402
from multigrad_amd.optim.transforms import Bounds  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
U24 = 2.0 ** -24
SIZES = (1, 3, 1023, 1025, 200_003)


# ---------------------------------------------------------------- kernels
def _vectors(n, device, offset, seed=0):
    """q, p, g, inv_mass (per element), z: float32 of n elements; with ``offset`` each is a
    view 4 bytes into a larger buffer, which no float4 can load."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    out = []
    for k in range(5):
        t = torch.randn(n, generator=gen, dtype=torch.float32)
        if k == 3:
            t = 0.25 + 4.0 * torch.rand(n, generator=gen, dtype=torch.float32)
        buf = torch.zeros(n + 1, dtype=torch.float32, device=device)
        view = buf[1:] if offset else buf[:n]
        view.copy_(t)
        out.append(view)
    return out


def _ke_out(device):
    return torch.zeros(1, dtype=torch.float64, device=device)


def check_leapfrog(device, n, bcast, move):
    """One launch against float64 on the float32 inputs, on the aligned and the 4-byte-offset
    views; both give the same bits, and so do two runs."""
    a, b = 0.0371, (0.0742 if move else 0.0)
    results = []
    for offset in (False, True, False):
        q, p, g, im, _ = _vectors(n, device, offset)
        if bcast:
            im = im[:1].clone()
        q0, p0 = q.double().cpu(), p.double().cpu()
        gd, md = g.double().cpu(), im.double().cpu()
        ke = _ke_out(device)
        hmc_leapfrog_(q, p, g, im, a, b, ke)
        pk, qk = p.double().cpu(), q.double().cpu()
        p_ref = p0 - a * gd
        err = (pk - p_ref).abs() - 2 * U24 * (p0.abs() + (a * gd).abs())
        assert float(err.max()) <= 0, f"p: {float(err.max())}"
        step = b * md * pk  # from the kernel's own float32 p'
        q_ref = q0 + step
        err = (qk - q_ref).abs() - 3 * U24 * (q0.abs() + step.abs())
        assert float(err.max()) <= 0, f"q: {float(err.max())}"
        if not move:
            assert torch.equal(qk, q0)
        ke_ref = 0.5 * float((pk * pk * md).sum())
        assert abs(float(ke) - ke_ref) <= 1e-12 * ke_ref, (float(ke), ke_ref)
        results.append((p.cpu().clone(), q.cpu().clone(), ke.cpu().clone()))
    for r in results[1:]:
        for x, y in zip(results[0], r):
            assert torch.equal(x, y)
    # without ke_out the vectors come out the same
    q, p, g, im, _ = _vectors(n, device, False)
    hmc_leapfrog_(q, p, g, im[:1].clone() if bcast else im, a, b)
    assert torch.equal(p.cpu(), results[0][0]) and torch.equal(q.cpu(), results[0][1])


def check_momentum(device, n, bcast):
    results = []
    for offset in (False, True, False):
        _, p, _, im, z = _vectors(n, device, offset)
        if bcast:
            im = im[:1].clone()
        ke = _ke_out(device)
        hmc_momentum_(z, im, p, ke)
        zd = z.double().cpu()
        ref = zd / im.double().cpu().sqrt()
        ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-300))) - 23)
        assert float(((p.double().cpu() - ref).abs() / ulp).max()) <= 2.0
        ke_ref = 0.5 * float((zd * zd).sum())
        assert abs(float(ke) - ke_ref) <= 1e-12 * ke_ref
        results.append((p.cpu().clone(), ke.cpu().clone()))
    for r in results[1:]:
        assert torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1])


def check_commit(device, n):
    """Five successive vectors against numpy's mean and variance; exact track and sample rows."""
    for offset in (False, True):
        gen = torch.Generator().manual_seed(n)
        qs = (3.0 + 2.0 * torch.randn(5, n + 1, generator=gen, dtype=torch.float32)).to(device)
        qs = qs[:, 1:] if offset else qs[:, :n]
        buf = torch.zeros(3, n + 1, dtype=torch.float32, device=device)
        mean, m2, row = (buf[k, 1:] if offset else buf[k, :n] for k in range(3))
        idx = torch.tensor(sorted({0, n // 2, n - 1}), dtype=torch.int64, device=device)
        trow = torch.zeros(idx.numel(), dtype=torch.float32, device=device)
        for i in range(5):
            hmc_commit_(qs[i], i + 1, mean, m2, idx, trow, row)
            assert torch.equal(row, qs[i]) and torch.equal(trow, qs[i][idx])
        ref = qs.double().cpu().numpy()
        assert np.abs(mean.double().cpu().numpy() - ref.mean(0)).max() <= 8 * U24 * np.abs(ref).max()
        m2_ref = ref.var(0) * 5
        assert np.all(np.abs(m2.double().cpu().numpy() - m2_ref) <= 1e-5 * m2_ref)
        # each part alone: only the track, only the sample row
        trow.zero_()
        hmc_commit_(qs[0], 1, None, None, idx, trow, None)
        assert torch.equal(trow, qs[0][idx])
        row.zero_()
        hmc_commit_(qs[1], 1, None, None, None, None, row)
        assert torch.equal(row, qs[1])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("move", [False, True])
def test_leapfrog(n, bcast, move):
    check_leapfrog(CPU, n, bcast, move)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bcast", [False, True])
def test_momentum(n, bcast):
    check_momentum(CPU, n, bcast)


@pytest.mark.parametrize("n", SIZES)
def test_commit(n):
    check_commit(CPU, n)


# ---------------------------------------------------------------- targets and the reference
class Gaussian:
    """Diagonal Gaussian: loss = 1/2 sum ((x - mu)/s)^2, evaluated in float64 on ``device``."""

    def __init__(self, mu, s, device=CPU):
        self.mu_np, self.s_np = np.asarray(mu, dtype=np.float64), np.asarray(s, dtype=np.float64)
        self.mu = torch.as_tensor(self.mu_np, device=device)
        self.s2 = torch.as_tensor(self.s_np ** 2, device=device)

    def __call__(self, x):
        r = x.double() - self.mu
        return 0.5 * (r * r / self.s2).sum(), r / self.s2


def matched(d, device=CPU):
    return Gaussian(np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d), device)


def wide(device=CPU):
    s = np.logspace(-1.0, 1.0, 50)
    return Gaussian(np.linspace(-1.0, 1.0, 50), s, device)


class SharedNoise:
    """Noise both the package and the reference read: numpy streams keyed by (seed, t)."""

    def __init__(self, seed):
        self.seed = seed

    def normal(self, t, n, device):
        z = np.random.default_rng([self.seed, t, 0]).standard_normal(n).astype(np.float32)
        return torch.from_numpy(z).to(device)

    def uniforms(self, t):
        u = np.random.default_rng([self.seed, t, 1]).random(2)
        return float(u[0]), float(u[1])


def reference_hmc(target, q0, inv_mass, eps, L, niter, noise, jitter, dtype=np.float64):
    """Plain numpy HMC, written independently of the package."""
    mu, s2 = target.mu_np.astype(dtype), (target.s_np ** 2).astype(dtype)
    im = np.broadcast_to(np.asarray(inv_mass, dtype=dtype), mu.shape)

    def U(x):
        return float(0.5 * np.sum(((x - mu) ** 2 / s2).astype(np.float64)))

    def grad(x):
        return (x - mu) / s2

    def K(mom):
        return float(0.5 * np.sum((mom * mom * im).astype(np.float64)))

    q = np.asarray(q0, dtype=dtype).copy()
    chain, accepts, margins = [], [], []
    for t in range(niter):
        u_acc, u_jit = noise.uniforms(t)
        e = dtype(eps * (1.0 + jitter * (2.0 * u_jit - 1.0)))
        mom = noise.normal(t, q.size, "cpu").numpy().astype(dtype) / np.sqrt(im)
        h0 = U(q) + K(mom)
        x = q.copy()
        mom = mom - dtype(0.5) * e * grad(x)
        for i in range(L):
            x = x + e * im * mom
            mom = mom - (e if i < L - 1 else dtype(0.5) * e) * grad(x)
        a = math.exp(min(0.0, -((U(x) + K(mom)) - h0)))
        if u_acc < a:
            q = x
        accepts.append(u_acc < a)
        margins.append(abs(u_acc - a))
        chain.append(q.copy())
    return np.array(chain), np.array(accepts), min(margins)


# ---------------------------------------------------------------- reversibility
def test_leapfrog_is_reversible():
    d, L, eps = 257, 10, math.pi / 20
    tg = matched(d)
    im = torch.as_tensor(tg.s_np ** 2, dtype=torch.float32)
    gen = torch.Generator().manual_seed(5)
    q0 = torch.as_tensor(tg.mu_np + tg.s_np, dtype=torch.float32)
    q = q0.clone()
    p = torch.randn(d, generator=gen) / im.sqrt()

    def run():
        g = tg(q)[1].float()
        hmc_leapfrog_(q, p, g, im, 0.5 * eps, eps)
        for i in range(L):
            g = tg(q)[1].float()
            if i < L - 1:
                hmc_leapfrog_(q, p, g, im, eps, eps)
            else:
                hmc_leapfrog_(q, p, g, im, 0.5 * eps, 0.0)

    run()
    assert float(((q - q0).abs() / im.sqrt()).max()) > 0.1  # it went somewhere
    p.neg_()
    run()
    dev = float(((q.double() - q0.double()).abs() / torch.as_tensor(tg.s_np)).max())
    print(f"reversibility: max |q - q0| / s = {dev:.3e}")
    assert dev <= 1e-5


# ---------------------------------------------------------------- chain against the reference
def check_chain(device, seed=0):
    d, niter = 257, 20
    tg = matched(d, device)
    noise = SharedNoise(seed)
    q0 = tg.mu_np + 0.5 * tg.s_np
    kw = dict(eps=math.pi / 20, L=10, niter=niter, noise=noise, jitter=0.2)
    ref, acc_ref, margin = reference_hmc(matched(d), q0.astype(np.float32), tg.s_np ** 2, **kw)
    obj = GenericObjective(tg, torch.as_tensor(q0, dtype=torch.float32, device=device))
    res = hmc_sample(obj, nsamples=niter, warmup=0, nleapfrog=10, step_size=math.pi / 20,
                     jitter=0.2, noise=noise,
                     inv_mass=torch.as_tensor(tg.s_np ** 2, dtype=torch.float32))
    got = res.samples.double().cpu().numpy()
    moved = np.concatenate([[True], np.any(got[1:] != got[:-1], axis=1)])
    first = bool(np.any(got[0] != q0.astype(np.float32)))
    acc = np.concatenate([[first], moved[1:]])
    dev = float((np.abs(got - ref) / tg.s_np).max())
    print(f"chain on {device}: {int(acc_ref.sum())}/{niter} accepted, closest |u - a| = "
          f"{margin:.2e}, max |q - q_ref| / s = {dev:.3e}")
    assert np.array_equal(acc, acc_ref)
    assert abs(res.accept_rate - acc_ref.mean()) < 1e-12
    assert dev <= 5e-5
    assert res.nfev == niter * 10 + 1 and res.n_divergent == 0
    return dev


def test_chain_matches_reference():
    check_chain(CPU)


# ---------------------------------------------------------------- moments
@pytest.fixture(scope="module")
def moments_run():
    tg = matched(50)
    x0 = torch.as_tensor(tg.mu_np, dtype=torch.float32)
    kw = dict(nsamples=2000, warmup=0, nleapfrog=10, step_size=math.pi / 20, jitter=0.0,
              inv_mass=torch.as_tensor(tg.s_np ** 2, dtype=torch.float32), randkey=3)
    full = run_hmc(tg, x0, history="full", track=[0, 49], **kw)
    mom = run_hmc(tg, x0, history="moments", track=[0, 49], **kw)
    return tg, full, mom


def test_moments_of_a_whitened_gaussian(moments_run):
    tg, res, _ = moments_run
    n = 2000
    x = res.samples.double().numpy()
    assert x.shape == (n, 50) and res.potential.shape == (n,)
    dm = float((np.abs(x.mean(0) - tg.mu_np) / tg.s_np).max()) * math.sqrt(n)
    ds = float(np.abs(x.std(0, ddof=1) / tg.s_np - 1.0).max()) * math.sqrt(n)
    print(f"accept {res.accept_rate:.3f}; mean off by {dm:.2f}/sqrt(n), std by {ds:.2f}/sqrt(n)")
    assert res.accept_rate >= 0.9
    assert dm <= 6.0 and ds <= 5.0
    assert res.n_divergent == 0 and res.warmup_windows == [] and res.step_size == math.pi / 20
    assert torch.equal(res.tracked, res.samples[:, [0, 49]])
    assert torch.equal(res.x, res.samples[-1])


def test_moments_history_matches_full(moments_run):
    _, full, mom = moments_run
    assert mom.samples is None and torch.equal(mom.tracked, full.tracked)
    x = full.samples.double().numpy()
    assert np.abs(mom.mean.double().numpy() - x.mean(0)).max() <= 8 * U24 * np.abs(x).max()
    v = x.var(0, ddof=1)
    assert np.all(np.abs(mom.var.double().numpy() - v) <= 1e-4 * v)
    assert torch.equal(mom.mean, full.mean) and torch.equal(mom.var, full.var)


# ---------------------------------------------------------------- adaptation
def test_warmup_windows():
    assert warmup_windows(1000) == [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)]
    assert warmup_windows(150) == [(75, 100)]
    assert warmup_windows(300) == [(75, 100), (100, 150), (150, 250)]
    assert warmup_windows(100) == [(15, 90)]
    assert warmup_windows(19) == [] and warmup_windows(0) == []


def check_adaptation(device, warmup, nsamples, seed=1):
    tg = wide(device)
    x0 = torch.as_tensor(tg.mu_np + tg.s_np, dtype=torch.float32, device=device)
    res = run_hmc(tg, x0, nsamples=nsamples, warmup=warmup, step_size=0.01, jitter=0.0,
                  randkey=seed, history="moments")
    ratio = res.inv_mass.double().cpu().numpy() / tg.s_np ** 2
    print(f"adaptation on {device}: inv_mass / s^2 in [{ratio.min():.2f}, {ratio.max():.2f}], "
          f"step {res.step_size:.3f}, accept {res.accept_rate:.3f}, {res.n_divergent} divergent")
    assert res.warmup_windows == warmup_windows(warmup)
    return res, ratio


def test_adaptation_finds_the_scales():
    res, ratio = check_adaptation(CPU, 1000, 1000)
    assert ratio.min() >= 0.5 and ratio.max() <= 2.0
    assert 0.7 <= res.accept_rate <= 0.95


def test_adaptation_switches():
    tg = wide()
    x0 = torch.as_tensor(tg.mu_np, dtype=torch.float32)
    res = run_hmc(tg, x0, nsamples=5, warmup=160, step_size=0.01, adapt_mass=False)
    assert res.warmup_windows == [] and res.inv_mass.numel() == 1 and res.step_size != 0.01
    res = run_hmc(tg, x0, nsamples=5, warmup=10, step_size=0.01)
    assert res.warmup_windows == [] and res.inv_mass.numel() == 1
    res = run_hmc(tg, x0, nsamples=5, warmup=30, step_size=0.01, adapt_step_size=False,
                  inv_mass=0.5)
    assert res.step_size == 0.01 and res.inv_mass.numel() == 50
    with pytest.raises(ValueError):
        run_hmc(tg, x0, nsamples=5, warmup=0, inv_mass=torch.zeros(50))
    with pytest.raises(ValueError):
        run_hmc(tg, x0, nsamples=5, warmup=0, history="some")


def test_key_noise_recipe():
    from multigrad_amd.utils.random import init_randkey
    key = init_randkey(7)
    noise = KeyNoise(7)
    k = key.fold_in(4)
    assert torch.equal(noise.normal(4, 9, "cpu"), torch.randn(9, generator=k.generator("cpu")))
    assert noise.uniforms(4) == tuple(k.numpy_rng().random(2))
    sharded = KeyNoise(key, rank=2)
    assert torch.equal(sharded.normal(4, 9, "cpu"),
                       torch.randn(9, generator=k.fold_in(3).generator("cpu")))
    assert sharded.uniforms(4) == noise.uniforms(4)


# ---------------------------------------------------------------- bounds
SPEC = [(-1.0, 2.5), (0.5, None), (None, -0.25), (None, None)]


def test_log_dpdu_matches_autograd():
    b = Bounds.from_spec(SPEC * 9, 36, dtype=torch.float64)
    base = torch.tensor([-1e4, -30.0, -2.0, -1e-3, 0.0, 0.4, 3.0, 50.0, 1e4], dtype=torch.float64)
    u = base.repeat_interleave(4).requires_grad_(True)
    ref = torch.log(b.dpdu(u))
    (dref,) = torch.autograd.grad(ref.sum(), u)
    u = u.detach()
    torch.testing.assert_close(b.log_dpdu(u), ref.detach(), rtol=1e-5, atol=1e-12)
    torch.testing.assert_close(b.dlog_dpdu(u), dref, rtol=1e-5, atol=1e-12)
    # float32, as the sampler calls them
    b32 = Bounds.from_spec(SPEC * 9, 36, dtype=torch.float32)
    torch.testing.assert_close(b32.log_dpdu(u.float()).double(), ref.detach(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(b32.dlog_dpdu(u.float()).double(), dref, rtol=1e-5, atol=1e-7)


def test_flat_loss_in_a_box_is_sampled_uniformly():
    """The bound is 6 standard errors of the mean of n independent uniform draws.  The draws
    of a chain are not independent: in the unbounded coordinate the flat box is a Cauchy
    density, whose tails HMC leaves slowly (measured over 64 coordinates: the variance of the
    chain's mean is 3 to 5 times that of independent draws for trajectories of 10 to 40
    steps), so for the chain the bound is about 3 of its own standard errors."""
    n = 1000

    def flat(x):
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x)

    res = run_hmc(flat, torch.full((2,), 0.3), nsamples=n, warmup=0, nleapfrog=5,
                  step_size=0.2, jitter=0.5, param_bounds=[(0.0, 1.0)] * 2, randkey=0)
    x = res.samples.double().numpy()
    off = np.abs(x.mean(0) - 0.5) * math.sqrt(12 * n)
    print(f"uniform box: accept {res.accept_rate:.3f}, mean off by {off} / sqrt(12 n), "
          f"var {x.var(0)} (1/12 = {1 / 12:.4f})")
    assert x.min() >= 0.0 and x.max() <= 1.0
    assert off.max() <= 6.0
    assert float(res.x.min()) >= 0.0 and float(res.x.max()) <= 1.0
    assert np.abs(res.mean.double().numpy() - x.mean(0)).max() <= 8 * U24
    assert res.n_divergent == 0 and res.accept_rate > 0.5


# ---------------------------------------------------------------- two ranks against one
def _toy_model(rank=0, size=1):
    """Three parameters, 2000 objects in two groups, binned; this rank's shard of them."""
    import multigrad_amd as mg
    from multigrad_amd.ops import gaussian_binned_sum
    from multigrad_amd.ops.groups import GroupIndex
    gen = torch.Generator().manual_seed(21)
    x = 9.0 + 1.5 * torch.rand(2000, generator=gen, dtype=torch.float64)
    grp = torch.randint(0, 2, (2000,), generator=gen)
    x, grp = (torch.tensor_split(t, size)[rank] for t in (x, grp))
    target = torch.tensor([310.0, 420.0, 95.0, 330.0], dtype=torch.float64)

    @dataclass(eq=False)
    class ToyModel(mg.OnePointModel):
        def __post_init__(self):
            super().__post_init__()
            self.plan = GroupIndex(grp, 2)

        def calc_partial_sumstats_from_params(self, params, randkey=None):
            (shift,) = self.plan.gather(params[:2])
            return gaussian_binned_sum(x + shift, torch.pow(10.0, params[2:]), (9.2, 9.5, 9.8, 10.1, 10.4))

        def calc_loss_from_sumstats(self, sumstats, sumstats_aux=None, randkey=None):
            r = torch.log(sumstats / target)
            return (r * r).sum()

    return ToyModel(device="cpu", dtype=torch.float64)


def _toy_chain(rank, size):
    model = _toy_model(rank, size)
    res = model.run_hmc(torch.tensor([0.1, -0.2, -0.6], dtype=torch.float64), nsamples=20,
                        warmup=0, nleapfrog=5, step_size=0.01, loss_scale=50.0, randkey=4)
    return {"samples": res.samples.numpy(), "accept": res.accept_rate,
            "potential": res.potential}


def test_two_ranks_match_one_rank():
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    one = _toy_chain(0, 1)
    res = run_distributed(_toy_chain, 2)
    assert np.array_equal(res[0]["samples"], res[1]["samples"])
    assert np.array_equal(res[0]["potential"], res[1]["potential"])
    assert 0.0 < one["accept"] and len(np.unique(one["samples"][:, 0])) > 5
    ref = one["samples"]
    assert np.abs(res[0]["samples"] - ref).max() <= 1e-5 * np.abs(ref).max()


# ---------------------------------------------------------------- front end
def grouped_model(device):
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(8, 2000, seed=3, device=torch.device(device))
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    return GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data)), data


FRONT_END_SCALE = 1e4  # the stiffest direction then has a width of 6e-3, the softest of 0.8


def check_front_end(device):
    model, data = grouped_model(device)
    fit = model.run_gauss_newton(data["guess"])
    best = torch.as_tensor(fit.x, dtype=torch.float32, device=device)
    res = model.run_hmc(best, nsamples=300, warmup=100, nleapfrog=2, step_size=0.005,
                        loss_scale=FRONT_END_SCALE, randkey=1, track=[1, 6])
    assert res.samples.shape == (300, 8) and res.tracked.shape == (300, 2)
    assert res.mean.shape == (8,) and res.var.shape == (8,) and res.x.shape == (8,)
    assert res.potential.shape == (300,) and res.inv_mass.shape == (8,)
    assert res.warmup_windows == [(15, 90)]
    for t in (res.samples, res.tracked, res.mean, res.var, res.x, res.inv_mass):
        assert t.device.type == torch.device(device).type and bool(torch.isfinite(t).all())
    assert np.isfinite(res.potential).all() and math.isfinite(res.step_size) and res.step_size > 0
    assert res.n_divergent == 0 and res.nfev == 400 * 2 + 1
    assert torch.equal(res.tracked, res.samples[:, [1, 6]])
    std = res.samples.double().std(0)
    print(f"front end on {device}: accept {res.accept_rate:.3f}, step {res.step_size:.4f}, "
          f"posterior std {std.cpu().numpy()}")
    # the width is resolved: far above the float32 spacing of the parameters, and the chain moved
    assert float(std.min()) > 1e3 * U24 * float(best.abs().max()) and res.accept_rate > 0.3
    return res


def test_front_end():
    check_front_end("cpu")


def test_front_end_engine_objective_on_the_cpu():
    """A model with the fused-engine protocol samples over the engine objective; its results
    come back in the user's parameter order."""
    import multigrad_amd.parallel.comm as C
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    C.set_world_comm(None)
    data = make_population_data(num_params=120, num_halos=4000, seed=11, device="cpu")
    m = PopulationSMFModel(aux_data=data)
    m.set_target_from_truth()
    res = m.run_hmc(data["guess"], nsamples=6, warmup=4, nleapfrog=3, step_size=1e-3,
                    loss_scale=10.0, track=[0, 119])
    assert res.samples.shape == (6, 120) and res.nfev == 10 * 3 + 1
    assert torch.equal(res.tracked, res.samples[:, [0, 119]])
    assert torch.equal(res.x, res.samples[-1]) and bool(torch.isfinite(res.samples).all())
    assert res.accept_rate > 0 and res.n_divergent == 0


def _sharded_chain(rank, size):
    import multigrad_amd as mg
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    comm = mg.get_world_comm()
    data = make_population_data(num_params=120, num_halos=4000, seed=11, comm=comm, device="cpu")
    m = PopulationSMFModel(aux_data=data, comm=comm)
    m.set_target_from_truth()
    res = m.run_hmc(data["guess"], nsamples=8, warmup=30, nleapfrog=3, step_size=0.02,
                    loss_scale=10.0, track=[0, 61, 119], zero=True, chunks=3)
    return {"samples": res.samples.numpy(), "tracked": res.tracked.numpy(),
            "mean": res.mean.numpy(), "var": res.var.numpy(), "x": res.x.numpy(),
            "inv_mass": res.inv_mass.numpy(), "potential": res.potential,
            "accept": res.accept_rate, "step": res.step_size, "reduction": res.reduction}


def test_sharded_vectors_on_two_ranks():
    """ZeRO-sharded engine objective: each rank holds half of every vector, the kinetic
    energies are summed over the ranks, and every rank returns the same full-length results."""
    res = run_distributed(_sharded_chain, 2)
    for k, v in res[0].items():
        assert np.array_equal(np.asarray(v), np.asarray(res[1][k])), k
    r = res[0]
    assert r["reduction"] == "host"
    assert r["samples"].shape == (8, 120) and r["inv_mass"].shape == (120,)
    assert np.isfinite(r["samples"]).all() and np.isfinite(r["potential"]).all()
    assert np.array_equal(r["tracked"], r["samples"][:, [0, 61, 119]])
    assert np.array_equal(r["x"], r["samples"][-1])
    assert np.abs(r["mean"] - r["samples"].mean(0)).max() <= 8 * U24 * np.abs(r["samples"]).max()
    assert r["accept"] > 0 and (r["inv_mass"] > 0).all()
    assert len(np.unique(r["samples"][:, 0])) > 1 and len(np.unique(r["samples"][:, 119])) > 1


def test_metrics_and_check_hooks(tmp_path, monkeypatch):
    import json
    path = tmp_path / "hmc.jsonl"
    monkeypatch.setenv("MULTIGRAD_METRICS", str(path))
    monkeypatch.setenv("MULTIGRAD_CHECK_EVERY", "2")
    res = run_hmc(matched(5), torch.zeros(5), nsamples=3, warmup=2, step_size=0.1)
    recs = [json.loads(line) for line in open(path)]
    assert [r["step"] for r in recs] == [0, 1, 2, 3, 4]
    # the logger keeps float32
    assert abs(recs[-1]["loss"] - res.potential[-1]) <= 2 * U24 * abs(res.potential[-1])


def test_example_runs():
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "user_model_posterior.py"),
                          "--nsamples", "100", "--warmup", "60"], env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "posterior" in out.stdout and "Hessian" in out.stdout
