"""Gaussian parameter priors on the CPU: the two vector ops (torch fallbacks of csrc/prior.hip)
against float64, a chain with a prior against an independent float64 numpy HMC fed the same
noise, the moments of a Gaussian posterior, the bounds Jacobian with a prior, the MAP of a
separable quadratic through the device L-BFGS(-B), two gloo ranks against one, and the front
ends.  The bodies that take a ``device`` run again on the GPU from test_prior_gpu.py.

``u = 2^-24`` throughout; every bound is derived from the operation order the ops document."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hmc as T  # noqa: E402
from distributed import run_distributed  # noqa: E402

import multigrad_amd as mg  # noqa: E402
from multigrad_amd import GaussianPrior  # noqa: E402
from multigrad_amd.ops.hmc import hmc_leapfrog_  # noqa: E402
from multigrad_amd.ops.prior import gaussian_prior_grad_, hmc_leapfrog_prior_  # noqa: E402
from multigrad_amd.optim.hmc import hmc_sample, run_hmc  # noqa: E402
from multigrad_amd.optim.lbfgs import GenericObjective, run_lbfgs_device  # noqa: E402
from multigrad_amd.optim.lbfgsb import run_lbfgsb_device  # noqa: E402
from multigrad_amd.optim.prior import PriorObjective  # noqa: E402
from multigrad_amd.optim.transforms import Bounds  # noqa: E402

CPU = T.CPU
U24 = T.U24
SIZES = T.SIZES
KINDS = ("elem", "prior_bcast", "mass_bcast", "both_bcast")


def f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------- kernels
def prior_vectors(n, device, offset, bcast):
    """q, p, g, inv_mass as test_hmc._vectors builds them, and a prior: mean (normal) and
    inv_var (0.25 .. 4.25, every seventh entry 0: a flat parameter) -- of n elements on the
    same kind of view, or of one element each."""
    q, p, g, im, _ = T._vectors(n, device, offset)
    _, _, _, w, m = T._vectors(n, device, offset, seed=1)
    w[::7] = 0.0
    if bcast:
        m, w = m[:1].clone(), w[:1].clone() + 0.5
    return q, p, g, im, m, w


def check_prior_grad(device, n, bcast):
    """``out = fmaf(c w, d, g)`` with ``d = x - m`` against float64 on the float32 inputs
    (``c`` rounded to float32 in the reference).  One rounding each for ``d`` (u |d|, which
    reaches the result as u |c w d|), for ``c w`` (u |c w d|) and for the fma (u |out| <=
    u (|g| + |c w d|)): u (3 |c w d| + |g|) to first order, bounded by 4u (|g| + |c w d|).
    The penalty's products and sum are fp64 from the fp32 values: 1e-12 relative, as the
    kinetic energy of test_hmc.  Aligned, 4-byte-offset and aligned views give the same bits,
    ``out is g`` gives the bits of a separate ``out``, and a flat entry leaves ``g`` as it is."""
    c = 0.731
    results = []
    for offset in (False, True, False):
        x, _, g, _, m, w = prior_vectors(n, device, offset, bcast)
        xd, gd, md, wd = (t.double().cpu() for t in (x, g, m, w))
        g0 = g.clone()
        buf = torch.zeros(n + 1, dtype=torch.float32, device=device)
        out = buf[1:] if offset else buf[:n]
        pen = T._ke_out(device)
        assert gaussian_prior_grad_(x, g, m, w, c, out, pen) is out
        assert torch.equal(g, g0)
        term = f32(c) * wd * (xd - md)
        ref = gd + term
        err = (out.double().cpu() - ref).abs() - 4 * U24 * (gd.abs() + term.abs())
        print(f"grad n={n}: max excess {float(err.max()):.3e}")
        assert float(err.max()) <= 0
        pen_ref = 0.5 * float((wd * (xd - md) ** 2).sum())
        print(f"pen {float(pen):.17g} ref {pen_ref:.17g}")
        assert abs(float(pen) - pen_ref) <= 1e-12 * pen_ref
        if not bcast:
            flat = (w == 0).cpu()
            assert bool(flat.any()) and torch.equal(out.cpu()[flat], g0.cpu()[flat])
        # in place, and without the penalty
        gaussian_prior_grad_(x, g, m, w, c, g)
        assert torch.equal(g, out)
        results.append((out.cpu().clone(), pen.cpu().clone()))
    for r in results[1:]:
        assert torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1])


def check_leapfrog_prior(device, n, kind, move):
    """``s = fmaf(-a, g, p)``, ``p' = fmaf(-(ap w), q - m, s)`` against float64 on the float32
    inputs, ``a`` and ``ap`` rounded to float32 in the reference.  Roundings: the first fma
    u |s| <= u (|p| + |a g|); ``d = q - m`` and ``ap w`` one each, u |ap w d| each; the second
    fma u |p'| <= u (|p| + |a g| + |ap w d|): u (2 |p| + 2 |a g| + 3 |ap w d|) to first order,
    inside the bound u (2 |p| + 2 |a g| + 4 |ap w d|).  ``q'`` is checked against the op's own
    float32 ``p'`` with test_hmc.check_leapfrog's bound; ``ke`` (from ``p'``) and ``pen`` (from
    the input ``q``) to 1e-12 relative.  The three views and two runs give the same bits."""
    a, b, ap = 0.0371, (0.0742 if move else 0.0), 0.0529
    results = []
    for offset in (False, True, False):
        q, p, g, im, m, w = prior_vectors(n, device, offset, kind in ("prior_bcast", "both_bcast"))
        if kind in ("mass_bcast", "both_bcast"):
            im = im[:1].clone()
        q0, p0, gd, imd, md, wd = (t.double().cpu() for t in (q, p, g, im, m, w))
        ke, pen = T._ke_out(device), T._ke_out(device)
        hmc_leapfrog_prior_(q, p, g, im, a, b, m, w, ap, ke, pen)
        pk, qk = p.double().cpu(), q.double().cpu()
        t1, t2 = f32(a) * gd, f32(ap) * wd * (q0 - md)
        err = (pk - (p0 - t1 - t2)).abs() - U24 * (2 * p0.abs() + 2 * t1.abs() + 4 * t2.abs())
        print(f"leapfrog n={n} {kind}: p max excess {float(err.max()):.3e}")
        assert float(err.max()) <= 0
        step = b * imd * pk
        err = (qk - (q0 + step)).abs() - 3 * U24 * (q0.abs() + step.abs())
        assert float(err.max()) <= 0, f"q: {float(err.max())}"
        if not move:
            assert torch.equal(qk, q0)
        ke_ref = 0.5 * float((pk * pk * imd).sum())
        pen_ref = 0.5 * float((wd * (q0 - md) ** 2).sum())
        print(f"ke {float(ke):.17g} ref {ke_ref:.17g}; pen {float(pen):.17g} ref {pen_ref:.17g}")
        assert abs(float(ke) - ke_ref) <= 1e-12 * ke_ref
        assert abs(float(pen) - pen_ref) <= 1e-12 * pen_ref
        results.append((p.cpu().clone(), q.cpu().clone(), ke.cpu().clone(), pen.cpu().clone()))
    for r in results[1:]:
        for x, y in zip(results[0], r):
            assert torch.equal(x, y)
    # each energy alone, and none: the vectors and the energies come out the same
    for want_ke, want_pen in ((True, False), (False, True), (False, False)):
        q, p, g, im, m, w = prior_vectors(n, device, False, kind in ("prior_bcast", "both_bcast"))
        if kind in ("mass_bcast", "both_bcast"):
            im = im[:1].clone()
        ke, pen = T._ke_out(device), T._ke_out(device)
        hmc_leapfrog_prior_(q, p, g, im, a, b, m, w, ap, ke if want_ke else None,
                            pen if want_pen else None)
        assert torch.equal(p.cpu(), results[0][0]) and torch.equal(q.cpu(), results[0][1])
        assert not want_ke or torch.equal(ke.cpu(), results[0][2])
        assert not want_pen or torch.equal(pen.cpu(), results[0][3])


def check_flat_prior_is_the_flat_leapfrog(device, n, move):
    """With ``inv_var`` all zero ``p``, ``q`` and ``ke`` are bitwise those of ``hmc_leapfrog_``
    on the same inputs: ``fmaf(-0, d, s) = s``.  For ``ke`` this holds at these sizes because
    both kernels' grids are ``ceil(chunks / 256)`` workgroups, below either kernel's resident
    cap, so the slab rows and their sum run in the same order."""
    a, b = 0.0371, (0.0742 if move else 0.0)
    for bcast in (False, True):
        q, p, g, im, m, w = prior_vectors(n, device, False, bcast)
        w.zero_()
        q1, p1 = q.clone(), p.clone()
        ke, ke1, pen = T._ke_out(device), T._ke_out(device), T._ke_out(device)
        hmc_leapfrog_prior_(q, p, g, im, a, b, m, w, 0.0529, ke, pen)
        hmc_leapfrog_(q1, p1, g, im, a, b, ke1)
        assert torch.equal(p, p1) and torch.equal(q, q1) and torch.equal(ke, ke1)
        assert float(pen) == 0.0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bcast", [False, True])
def test_prior_grad(n, bcast):
    check_prior_grad(CPU, n, bcast)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("move", [False, True])
def test_leapfrog_prior(n, kind, move):
    check_leapfrog_prior(CPU, n, kind, move)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("move", [False, True])
def test_flat_prior_is_the_flat_leapfrog(n, move):
    check_flat_prior_is_the_flat_leapfrog(CPU, n, move)


# ---------------------------------------------------------------- the prior object
def test_gaussian_prior_object():
    pr = GaussianPrior([0.0, 1.0, float("nan") if False else 2.0], [1.0, None, 0.5])
    assert np.array_equal(pr.inv_var, [1.0, 0.0, 4.0])
    x = np.array([1.0, 5.0, 3.0])
    assert pr.penalty(x) == 0.5 * (1.0 + 4.0)
    assert np.array_equal(pr.grad(x), [1.0, 0.0, 4.0])
    xt = torch.tensor(x, dtype=torch.float32)
    assert pr.penalty(xt) == 2.5 and torch.equal(pr.grad(xt), torch.tensor([1.0, 0.0, 4.0],
                                                                             dtype=torch.float64))
    # a flat parameter may have any mean
    assert GaussianPrior([0.0, float("inf")], [1.0, float("inf")]).penalty([1.0, 1.0]) == 0.5
    for bad in (lambda: GaussianPrior(0.0, 0.0), lambda: GaussianPrior(0.0, [1.0, -1.0]),
                lambda: GaussianPrior(0.0, float("nan")), lambda: GaussianPrior(float("inf"), 1.0),
                lambda: GaussianPrior([0.0, 1.0], [1.0, 1.0, 1.0]),
                lambda: GaussianPrior([0.0, float("nan")], [1.0, None]),
                lambda: pr.penalty(np.zeros(4))):
        with pytest.raises(ValueError):
            bad()
    # local: scalars stay one element on a layout without padding; user order otherwise
    obj = GenericObjective(T.matched(3), torch.zeros(3))
    m, w = GaussianPrior(0.5, 2.0).local(obj.vector_layout(), CPU)
    assert m.dtype == torch.float32 and m.tolist() == [0.5] and w.tolist() == [0.25]
    m, w = pr.local(obj.vector_layout(), CPU)
    assert m.tolist() == [0.0, 0.0, 2.0] and w.tolist() == [1.0, 0.0, 4.0]
    assert mg.GaussianPrior is GaussianPrior
    import multigrad
    assert multigrad.GaussianPrior is GaussianPrior and "GaussianPrior" in multigrad.__all__


@pytest.mark.parametrize("P", [120, 122])  # 122 parameters: an engine vector of 124
def test_local_on_an_engine_layout_has_no_weight_on_the_padding(P):
    import multigrad_amd.parallel.comm as C
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    C.set_world_comm(None)
    data = make_population_data(num_params=P, num_halos=4000, seed=11, device="cpu")
    m = PopulationSMFModel(aux_data=data)
    m.set_target_from_truth()
    eng = m.fused_engine(comm=None)
    try:
        obj = eng.lbfgs_objective(data["guess"])
        layout = obj.vector_layout()
        sig = np.linspace(0.5, 2.0, P)
        mean, w = GaussianPrior(0.25, sig).local(layout, CPU)
        real = layout.to_local(torch.ones(P)) > 0
        padded = bool((~real).any())
        assert padded == (P == 122)
        assert w.numel() == obj.n_local and mean.numel() == (obj.n_local if padded else 1)
        assert bool((w[~real] == 0).all())
        back = layout.from_local(w)
        assert torch.equal(back, torch.as_tensor(1.0 / sig ** 2, dtype=torch.float32))
        # a scalar prior: one element only where the vector has no padding
        mean, w = GaussianPrior(0.25, 2.0).local(layout, CPU)
        if padded:
            assert w.numel() == obj.n_local and bool((w[~real] == 0).all())
            assert bool((w[real] == 0.25).all())
        else:
            assert w.numel() == 1
    finally:
        eng.close()


# ---------------------------------------------------------------- chain against the reference
def chain_problem(d, device=CPU):
    """Likelihood test_hmc.matched(d); a per-element Gaussian prior, every tenth entry flat;
    the closed-form posterior mean and standard deviation."""
    tg = T.matched(d, device)
    pm = 0.3 * np.cos(np.arange(d))
    ps = np.linspace(0.7, 3.0, d)
    ps[::10] = np.inf
    w = np.where(np.isinf(ps), 0.0, 1.0 / np.where(np.isinf(ps), 1.0, ps) ** 2)
    var = 1.0 / (1.0 / tg.s_np ** 2 + w)
    mean = var * (tg.mu_np / tg.s_np ** 2 + w * pm)
    return tg, GaussianPrior(pm, ps), pm, w, mean, np.sqrt(var)


def reference_hmc_prior(target, pm, w, q0, inv_mass, eps, L, niter, noise, jitter):
    """Plain float64 numpy HMC with the potential ``loss + pen``, written independently of the
    package (the leapfrog takes the gradient of the whole potential)."""
    mu, s2 = target.mu_np, target.s_np ** 2
    im = np.broadcast_to(np.asarray(inv_mass, dtype=np.float64), mu.shape)

    def U(x):
        return float(0.5 * np.sum((x - mu) ** 2 / s2) + 0.5 * np.sum(w * (x - pm) ** 2))

    def grad(x):
        return (x - mu) / s2 + w * (x - pm)

    def K(mom):
        return float(0.5 * np.sum(mom * mom * im))

    q = np.asarray(q0, dtype=np.float64).copy()
    chain, accepts, margins = [], [], []
    for t in range(niter):
        u_acc, u_jit = noise.uniforms(t)
        e = eps * (1.0 + jitter * (2.0 * u_jit - 1.0))
        mom = noise.normal(t, q.size, "cpu").numpy().astype(np.float64) / np.sqrt(im)
        h0 = U(q) + K(mom)
        x = q.copy()
        mom = mom - 0.5 * e * grad(x)
        for i in range(L):
            x = x + e * im * mom
            mom = mom - (e if i < L - 1 else 0.5 * e) * grad(x)
        a = math.exp(min(0.0, -((U(x) + K(mom)) - h0)))
        if u_acc < a:
            q = x
        accepts.append(u_acc < a)
        margins.append(abs(u_acc - a))
        chain.append(q.copy())
    return np.array(chain), np.array(accepts), min(margins)


CHAIN_SEED = 0  # the float64 reference alone keeps |u_accept - a| >= 1e-3 (printed below)


def check_chain(device, seed=CHAIN_SEED):
    """All accept decisions equal those of the float64 reference, and the float32 chain stays
    within 5e-5 posterior standard deviations of it (the bound of test_hmc.check_chain)."""
    d, niter = 257, 20
    tg, prior, pm, w, _, s_post = chain_problem(d, device)
    noise = T.SharedNoise(seed)
    q0 = (tg.mu_np + 0.5 * tg.s_np).astype(np.float32)
    ref, acc_ref, margin = reference_hmc_prior(T.matched(d), pm, w, q0, s_post ** 2,
                                               eps=math.pi / 20, L=10, niter=niter, noise=noise,
                                               jitter=0.2)
    assert margin >= 1e-3, f"seed {seed}: closest |u - a| = {margin:.2e}; pick another seed"
    obj = GenericObjective(tg, torch.as_tensor(q0, device=device))
    res = hmc_sample(obj, nsamples=niter, warmup=0, nleapfrog=10, step_size=math.pi / 20,
                     jitter=0.2, noise=noise, prior=prior,
                     inv_mass=torch.as_tensor(s_post ** 2, dtype=torch.float32))
    got = res.samples.double().cpu().numpy()
    moved = np.concatenate([[True], np.any(got[1:] != got[:-1], axis=1)])
    acc = np.concatenate([[bool(np.any(got[0] != q0))], moved[1:]])
    dev = float((np.abs(got - ref) / s_post).max())
    print(f"chain with a prior on {device}: {int(acc_ref.sum())}/{niter} accepted, closest "
          f"|u - a| = {margin:.2e}, max |q - q_ref| / s_post = {dev:.3e}")
    assert np.array_equal(acc, acc_ref)
    assert dev <= 5e-5
    assert res.nfev == niter * 10 + 1 and res.n_divergent == 0
    # the potential of every draw includes the penalty
    x = got[-1]
    u_ref = float(tg(torch.as_tensor(x, device=device))[0]) + prior.penalty(x)
    assert abs(res.potential[-1] - u_ref) <= 1e-9 * u_ref
    return dev


def test_chain_matches_reference():
    check_chain(CPU)


# ---------------------------------------------------------------- moments
@pytest.fixture(scope="module")
def moments_run():
    tg = T.matched(50)
    prior = GaussianPrior(0.5, np.linspace(0.3, 3.0, 50))
    var = 1.0 / (1.0 / tg.s_np ** 2 + prior.inv_var)
    mean = var * (tg.mu_np / tg.s_np ** 2 + prior.inv_var * 0.5)
    x0 = torch.as_tensor(tg.mu_np, dtype=torch.float32)
    kw = dict(nsamples=2000, warmup=0, nleapfrog=10, step_size=math.pi / 20, jitter=0.0,
              inv_mass=torch.as_tensor(var, dtype=torch.float32), randkey=3, prior=prior)
    full = run_hmc(tg, x0, history="full", **kw)
    mom = run_hmc(tg, x0, history="moments", **kw)
    return mean, np.sqrt(var), full, mom


def test_moments_of_a_gaussian_posterior(moments_run):
    """The bounds of test_hmc.test_moments_of_a_whitened_gaussian against the closed-form
    posterior: the mean within 6 and the standard deviation within 5 standard errors of
    independent draws."""
    m_post, s_post, res, _ = moments_run
    n = 2000
    x = res.samples.double().numpy()
    dm = float((np.abs(x.mean(0) - m_post) / s_post).max()) * math.sqrt(n)
    ds = float(np.abs(x.std(0, ddof=1) / s_post - 1.0).max()) * math.sqrt(n)
    print(f"accept {res.accept_rate:.3f}; mean off by {dm:.2f}/sqrt(n), std by {ds:.2f}/sqrt(n)")
    assert res.accept_rate >= 0.9
    assert dm <= 6.0 and ds <= 5.0
    assert res.n_divergent == 0


def test_moments_history_matches_full(moments_run):
    _, _, full, mom = moments_run
    assert mom.samples is None
    assert torch.equal(mom.mean, full.mean) and torch.equal(mom.var, full.var)
    assert np.array_equal(mom.potential, full.potential)
    x = full.samples.double().numpy()
    assert np.abs(mom.mean.double().numpy() - x.mean(0)).max() <= 8 * U24 * np.abs(x).max()


# ---------------------------------------------------------------- bounds in the sampler
def test_potential_with_bounds_and_a_prior():
    """``potential[i] = loss_scale * loss + pen - sum log dp/du`` at the returned sample,
    recomputed in float64 (the position is float32: 1e-5 relative plus 1e-6)."""
    spec = T.SPEC * 2
    tg = T.Gaussian(np.linspace(0.0, 1.0, 8), np.linspace(0.5, 1.5, 8))
    x0 = torch.tensor([0.5, 1.0, -1.0, 0.2] * 2)
    prior = GaussianPrior(np.linspace(-0.5, 0.5, 8), [0.8, None, 1.5, 0.4] * 2)
    res = run_hmc(tg, x0, nsamples=12, warmup=0, nleapfrog=4, step_size=0.1, loss_scale=0.7,
                  param_bounds=spec, prior=prior, randkey=2)
    flat = run_hmc(tg, x0, nsamples=12, warmup=0, nleapfrog=4, step_size=0.1, loss_scale=0.7,
                   param_bounds=spec, randkey=2)
    b = Bounds.from_spec(spec, 8, dtype=torch.float64)
    assert len(np.unique(res.samples[:, 0].numpy())) > 3
    for i in range(12):
        x = res.samples[i].double()
        u = b.forward(x)
        ref = 0.7 * float(tg(x)[0]) + prior.penalty(x) - float(b.log_dpdu(u).sum())
        assert abs(res.potential[i] - ref) <= 1e-5 * abs(ref) + 1e-6, (i, res.potential[i], ref)
    assert not np.array_equal(res.potential, flat.potential)


# ---------------------------------------------------------------- MAP of a separable quadratic
def map_problem(d, device):
    tg, prior, pm, w, _, _ = chain_problem(d, device)
    a = 1.0 / tg.s_np ** 2
    xmap = (a * tg.mu_np + 2.0 * w * pm) / (a + 2.0 * w)

    def grad64(x):
        x = np.asarray(x, dtype=np.float64)
        return a * (x - tg.mu_np) + 2.0 * w * (x - pm)

    def fun64(x):
        x = np.asarray(x, dtype=np.float64)
        return 0.5 * float(np.sum(a * (x - tg.mu_np) ** 2)) + 2.0 * prior.penalty(x)

    return tg, prior, xmap, grad64, fun64


def check_map(device):
    """``loss + 2 pen`` of a separable quadratic.  The optimizer stops at its own float32
    criterion max|g| <= 1e-5; the float64 gradient at the same x differs from the float32 one
    by the rounding of its two terms, far below 1e-5 here (|terms| ~ 10, u ~ 6e-8): 2e-5.
    ``ftol = 0`` leaves that criterion as the only one: the objective is about 50 at the MAP,
    so the default relative-decrease test (2.2e-9) would stop at a gradient near 3e-4."""
    d = 257
    tg, prior, xmap, grad64, fun64 = map_problem(d, device)
    x0 = torch.zeros(d, device=device)
    res = run_lbfgs_device(tg, x0, prior=prior, prior_weight=2.0, gtol=1e-5, ftol=0.0)
    x = res.x.double().cpu().numpy()
    gmax = float(np.abs(grad64(x)).max())
    print(f"L-BFGS MAP on {device}: nit {res.nit}, {res.message}, max|g64| = {gmax:.3e}, "
          f"max |x - x_map| = {np.abs(x - xmap).max():.3e}")
    assert res.success
    assert gmax <= 2e-5
    assert abs(res.fun - fun64(x)) <= 1e-6 * fun64(x)
    assert abs(res.prior_penalty - prior.penalty(x)) <= 1e-12 * prior.penalty(x)
    assert res.hess_inv is not None
    # a box that cuts the unconstrained MAP: the separable solution is the clipped one
    lo = np.where(np.arange(d) % 3 == 0, xmap + 0.1, -np.inf)
    hi = np.where(np.arange(d) % 3 == 1, xmap - 0.1, np.inf)
    box = np.stack([lo, hi], 1)
    res = run_lbfgsb_device(tg, x0, param_bounds=box, prior=prior, prior_weight=2.0, gtol=1e-5, ftol=0.0)
    xb = res.x.double().cpu().numpy()
    g = grad64(xb)
    at_lo, at_hi = np.arange(d) % 3 == 0, np.arange(d) % 3 == 1
    free = ~(at_lo | at_hi)
    print(f"L-BFGS-B MAP on {device}: nit {res.nit}, {res.message}, free max|g64| = "
          f"{np.abs(g[free]).max():.3e}")
    assert res.success
    assert np.array_equal(xb[at_lo], lo.astype(np.float32)[at_lo].astype(np.float64))
    assert np.array_equal(xb[at_hi], hi.astype(np.float32)[at_hi].astype(np.float64))
    assert (g[at_lo] > 0).all() and (g[at_hi] < 0).all()  # outward: the bound holds them
    assert float(np.abs(g[free]).max()) <= 2e-5
    assert abs(res.prior_penalty - prior.penalty(xb)) <= 1e-12 * prior.penalty(xb)
    # the transform: the prior stays on x
    res = run_lbfgs_device(tg, x0, param_bounds=[(-20.0, 20.0)] * d, prior=prior,
                           prior_weight=2.0, gtol=1e-5, ftol=0.0)
    xt = res.x.double().cpu().numpy()
    gmax = float(np.abs(grad64(xt)).max())
    print(f"L-BFGS MAP (transform) on {device}: nit {res.nit}, {res.message}, max|g64| = {gmax:.3e}")
    assert res.success and gmax <= 2e-5
    assert abs(res.fun - fun64(xt)) <= 1e-6 * fun64(xt)


def test_map_of_a_separable_quadratic():
    check_map(CPU)


def test_prior_objective_protocol():
    """The wrapper adds the weighted penalty and its gradient in a buffer of its own."""
    d = 33
    tg, prior, _, grad64, fun64 = map_problem(d, CPU)
    inner = GenericObjective(tg, torch.linspace(-1.0, 1.0, d))
    obj = PriorObjective(inner, prior, 2.0)
    assert (obj.comm, obj.sharded, obj.n_local) == (inner.comm, inner.sharded, d)
    assert not hasattr(obj, "device_call") and not hasattr(obj, "local_box")
    x = obj.x0()
    f, g = obj(x)
    f0, g0 = inner(x)
    keep = g0.clone()
    xd = x.double().numpy()
    # the objective holds the prior's mean and inverse variance in float32
    assert abs(f - fun64(xd)) <= 1e-6 * fun64(xd)
    assert np.abs(g.double().numpy() - grad64(xd)).max() <= 8 * U24 * np.abs(grad64(xd)).max()
    assert g.data_ptr() != g0.data_ptr() and torch.equal(g0, keep)
    _, _, part = obj.partial_call(x)
    assert part.dtype == torch.float64
    assert abs(float(part) - 2.0 * prior.penalty(xd)) <= 2e-6 * prior.penalty(xd)
    with pytest.raises(ValueError):
        PriorObjective(GenericObjective(tg, torch.zeros(d), bounds=Bounds.from_spec(
            [(-1.0, 1.0)] * d, d, dtype=torch.float32)), prior, 1.0)


# ---------------------------------------------------------------- two ranks against one
def _population(comm):
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    data = make_population_data(num_params=120, num_halos=4000, seed=11, comm=comm, device="cpu")
    m = PopulationSMFModel(aux_data=data, comm=comm)
    m.set_target_from_truth()
    g0 = data["guess"].double().cpu().numpy()
    sig = np.linspace(0.05, 0.5, 120)
    sig[::9] = np.inf
    return m, data, GaussianPrior(g0 + 0.02 * np.cos(np.arange(120)), sig)


def _sharded_runs(rank, size):
    comm = mg.get_world_comm() if size > 1 else None
    m, data, prior = _population(comm)
    zero = dict(zero=True, chunks=3) if size > 1 else {}
    hmc = m.run_hmc(data["guess"], nsamples=8, warmup=0, nleapfrog=3, step_size=0.01,
                    loss_scale=10.0, prior=prior, randkey=5, **zero)
    u_last = 10.0 * float(m.calc_loss_from_params(hmc.x)) + prior.penalty(hmc.x)
    fit = m.run_bfgs(data["guess"], maxsteps=30, method="device", prior=prior, prior_weight=0.1,
                     **zero)
    bare = m.run_bfgs(data["guess"], maxsteps=30, method="device", **zero)
    loss = float(m.calc_loss_from_params(fit.x))
    # one line-search point through the drivers' TrialPoints, bare and with the prior: the
    # host collectives it makes, and what the prior adds to its value
    from multigrad_amd.optim._quasi_newton import TrialPoints
    from multigrad_amd.optim._reduce import DeviceReducer
    eng = m.fused_engine(comm=comm, **zero)
    point = []
    try:
        inner = eng.lbfgs_objective(data["guess"])
        red = DeviceReducer(inner.comm, inner.sharded, inner.device)
        d = None
        for o in (inner, PriorObjective(inner, prior, 0.1)):
            tp = TrialPoints(o, red, o.device)
            x = o.x0()
            g0 = tp.initial(x)[1]
            d = -g0 if d is None else d  # the same point for both
            tp.start(x, d, lambda ga, first: [(ga.double() * d.double()).sum()])
            h0 = comm.host_collectives if comm is not None else 0
            fa, _ = tp(1e-4)
            point.append((fa, (comm.host_collectives if comm is not None else 0) - h0))
        point.append(prior.penalty(inner.full(x + 1e-4 * d)))
    finally:
        if not getattr(eng, "cached", False):
            eng.close()
    return {"samples": hmc.samples.numpy(), "potential": hmc.potential, "accept": hmc.accept_rate,
            "u_last": u_last, "pen_last": prior.penalty(hmc.x), "point": point,
            "x": fit.x.numpy(), "fun": float(fit.fun), "pen": float(fit.prior_penalty),
            "loss": loss, "nit": int(fit.nit), "hc": int(fit.host_collectives),
            "hc_bare": int(bare.host_collectives), "nfev": int(fit.nfev),
            "nfev_bare": int(bare.nfev), "nit_bare": int(bare.nit)}


def _toy_chain(rank, size):
    model = T._toy_model(rank, size)
    prior = GaussianPrior([0.0, 0.0, -0.5], [0.3, None, 0.2])
    x0 = torch.tensor([0.1, -0.2, -0.6], dtype=torch.float64)
    res = model.run_hmc(x0, nsamples=20, warmup=0, nleapfrog=5, step_size=0.01, loss_scale=50.0,
                        randkey=4, prior=prior)
    fit = model.run_bfgs(x0, method="device", prior=prior, prior_weight=0.02)
    return {"samples": res.samples.numpy(), "accept": res.accept_rate,
            "potential": res.potential, "x": fit.x.numpy(), "fun": float(fit.fun)}


def test_two_ranks_match_one_rank():
    """The replicated toy model of test_hmc on two gloo ranks against one, with a prior: the
    assertions of test_hmc.test_two_ranks_match_one_rank, and potentials and ``fun`` that agree
    between the ranks to 1e-12 relative."""
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    one = _toy_chain(0, 1)
    res = run_distributed(_toy_chain, 2)
    assert np.array_equal(res[0]["samples"], res[1]["samples"])
    assert np.abs(res[0]["potential"] - res[1]["potential"]).max() <= \
        1e-12 * np.abs(res[0]["potential"]).max()
    assert abs(res[0]["fun"] - res[1]["fun"]) <= 1e-12 * abs(res[0]["fun"])
    assert 0.0 < one["accept"] and len(np.unique(one["samples"][:, 0])) > 5
    ref = one["samples"]
    assert np.abs(res[0]["samples"] - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(res[0]["potential"] - one["potential"]).max() <= \
        1e-4 * np.abs(one["potential"]).max()
    np.testing.assert_allclose(res[0]["x"], one["x"], rtol=1e-3, atol=1e-4)
    assert res[0]["fun"] == pytest.approx(one["fun"], rel=1e-2, abs=1e-9)


def test_sharded_vectors_on_two_ranks():
    """ZeRO-sharded vectors on two gloo ranks: each rank's penalty is a partial sum that rides
    in the reduction of its evaluation.  Both ranks return the same bits; the iterate agrees
    with one rank as test_lbfgs asks of the run without a prior (the sharded chain draws its
    noise per rank, so it has no one-rank twin: as in test_hmc); and the penalty is counted
    once: ``fun = loss + weight * pen`` and ``potential = loss_scale * loss + pen`` at the
    returned x.  On the CPU the reducer's path is the host all-reduce, so the loop's
    ``host_collectives`` are not 0 there (nor are they without a prior): with a prior the loop
    makes the same number per evaluation as without -- none of its own -- which is counted
    here around one trial point of the drivers' ``TrialPoints``."""
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    one = _sharded_runs(0, 1)
    res = run_distributed(_sharded_runs, 2)
    for k in ("samples", "potential", "x"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert abs(res[0]["fun"] - res[1]["fun"]) <= 1e-12 * abs(res[0]["fun"])
    r = res[0]
    assert 0.0 < r["accept"] and len(np.unique(r["samples"][:, 0])) > 3
    np.testing.assert_allclose(r["x"], one["x"], rtol=1e-3, atol=1e-4)
    assert r["fun"] == pytest.approx(one["fun"], rel=1e-2, abs=1e-9)
    for v in (r, one):
        assert v["pen"] > 0 and v["pen_last"] > 0.01 * v["u_last"]
        assert abs(v["fun"] - (v["loss"] + 0.1 * v["pen"])) <= 1e-5 * v["fun"], v
        assert abs(v["potential"][-1] - v["u_last"]) <= 1e-5 * v["u_last"], v
    print(f"host collectives of the loop, two ranks: {r['hc']} with a prior ({r['nit']} "
          f"iterations, {r['nfev']} evaluations), {r['hc_bare']} without ({r['nit_bare']}, "
          f"{r['nfev_bare']}); one rank: {one['hc']}")
    assert one["hc"] == 0
    for v in (r, one):
        (f_bare, hc_bare), (f_prior, hc_prior), pen = v["point"]
        print(f"one trial point: {hc_bare} host collectives bare, {hc_prior} with the prior")
        assert hc_prior == hc_bare
        assert abs((f_prior - f_bare) - 0.1 * pen) <= 1e-5 * f_prior


# ---------------------------------------------------------------- plumbing
def test_prior_none_is_the_run_without_the_keyword():
    tg = T.matched(9)
    x0 = torch.zeros(9)
    a = run_hmc(tg, x0, nsamples=10, warmup=5, step_size=0.2, randkey=1)
    b = run_hmc(tg, x0, nsamples=10, warmup=5, step_size=0.2, randkey=1, prior=None)
    assert torch.equal(a.x, b.x) and np.array_equal(a.potential, b.potential) and a.nfev == b.nfev
    a = run_lbfgs_device(tg, x0)
    b = run_lbfgs_device(tg, x0, prior=None, prior_weight=3.0)
    assert torch.equal(a.x, b.x) and a.fun == b.fun and a.nfev == b.nfev
    assert "prior_penalty" not in b
    box = [(-0.5, 0.5)] * 9
    a = run_lbfgsb_device(tg, x0, param_bounds=box)
    b = run_lbfgsb_device(tg, x0, param_bounds=box, prior=None)
    assert torch.equal(a.x, b.x) and a.fun == b.fun and a.nfev == b.nfev
    model, data = T.grouped_model("cpu")
    a = model.run_bfgs(data["guess"], maxsteps=5, method="device")
    b = model.run_bfgs(data["guess"], maxsteps=5, method="device", prior=None)
    assert torch.equal(a.x, b.x) and a.fun == b.fun and a.nfev == b.nfev


def test_wrong_length_prior_raises_in_every_front_end():
    tg = T.matched(9)
    x0 = torch.zeros(9)
    bad = GaussianPrior(np.zeros(8), 1.0)
    model, data = T.grouped_model("cpu")
    calls = [lambda: run_hmc(tg, x0, nsamples=2, warmup=0, prior=bad),
             lambda: hmc_sample(GenericObjective(tg, x0), nsamples=2, warmup=0, prior=bad),
             lambda: run_lbfgs_device(tg, x0, prior=bad),
             lambda: run_lbfgs_device(tg, x0, prior=bad, param_bounds=[(-1.0, 1.0)] * 9),
             lambda: run_lbfgsb_device(tg, x0, prior=bad, param_bounds=[(-1.0, 1.0)] * 9),
             lambda: model.run_hmc(data["guess"], nsamples=2, warmup=0, prior=GaussianPrior(
                 np.zeros(3), 1.0)),
             lambda: model.run_bfgs(data["guess"], method="device", prior=GaussianPrior(
                 np.zeros(3), 1.0)),
             lambda: model.run_bfgs(data["guess"], method="scipy", prior=GaussianPrior(
                 np.zeros(3), 1.0))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        run_hmc(tg, x0, nsamples=2, warmup=0, prior=(0.0, 1.0))


def test_scipy_method_with_a_prior():
    """``method="scipy"``: the wrapped function is what scipy minimises, at scipy's own
    tolerances (``pgtol = 1e-5``).  The float64 toy model of test_hmc, so the gradient bound of
    the MAP test holds with room (float64 throughout)."""
    import multigrad_amd.parallel.comm as C
    C.set_world_comm(None)
    model = T._toy_model()
    x0 = torch.tensor([0.1, -0.2, -0.6], dtype=torch.float64)
    prior = GaussianPrior([0.0, 0.0, -0.5], [0.3, None, 0.2])
    res = model.run_bfgs(x0, method="scipy", prior=prior, prior_weight=0.5)
    x = torch.as_tensor(res.x, dtype=torch.float64)
    loss, grad = model.calc_loss_and_grad_from_params(x)
    g = grad.double().numpy() + 0.5 * np.asarray(prior.grad(np.asarray(res.x)))
    print(f"scipy with a prior: {res.message}, max|g| = {np.abs(g).max():.3e}")
    assert res.success and float(np.abs(g).max()) <= 2e-5
    assert abs(res.prior_penalty - prior.penalty(res.x)) <= 1e-12 * res.prior_penalty
    assert abs(res.fun - (float(loss) + 0.5 * res.prior_penalty)) <= 1e-12 * abs(res.fun)
    flat = model.run_bfgs(x0, method="scipy")
    assert np.abs(np.asarray(flat.x) - np.asarray(res.x)).max() > 1e-2


def test_model_front_ends_on_the_generic_path():
    """``OnePointModel.run_hmc`` / ``run_bfgs`` without a fused engine, all bounds modes."""
    model, data = T.grouped_model("cpu")
    g0 = data["guess"].double().cpu().numpy()
    prior = GaussianPrior(g0, 0.3)
    box = [(float(v) - 1.0, float(v) + 1.0) for v in g0]
    for kw in ({}, dict(param_bounds=box), dict(param_bounds=box, bounds_mode="transform")):
        res = model.run_bfgs(data["guess"], method="device", maxsteps=40, prior=prior,
                             prior_weight=0.2, **kw)
        loss = float(model.calc_loss_from_params(res.x))
        assert res.prior_penalty > 0
        assert abs(res.fun - (loss + 0.2 * res.prior_penalty)) <= 1e-5 * abs(res.fun), kw
    res = model.run_hmc(data["guess"], nsamples=5, warmup=0, nleapfrog=2, step_size=1e-3,
                        loss_scale=100.0, prior=prior)
    x = res.samples[-1]
    ref = 100.0 * float(model.calc_loss_from_params(x)) + prior.penalty(x)
    assert abs(res.potential[-1] - ref) <= 1e-5 * abs(ref)


def test_example_runs():
    import subprocess
    env = dict(os.environ, MULTIGRAD_PROGRESS="0")
    out = subprocess.run([sys.executable, os.path.join(T.ROOT, "examples", "user_model_prior.py"),
                          "--nsamples", "60", "--warmup", "40"], env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "MAP" in out.stdout and "posterior" in out.stdout
