"""The prior kernels (csrc/prior.hip) and the front ends on the GPU: the bodies of
test_prior.py on ``cuda``, the kernels against the CPU fallbacks, the host-side argument
checks of the extension, and the fused engine's objective with a prior."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hmc as T  # noqa: E402
import test_prior as P  # noqa: E402

from multigrad_amd import GaussianPrior  # noqa: E402
from multigrad_amd.ops.prior import gaussian_prior_grad_, hmc_leapfrog_prior_  # noqa: E402
from multigrad_amd.optim.prior import PriorObjective  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U24 = T.U24
# the first size whose chunks exceed 2048 workgroups of 256 threads: a second grid-stride trip
SIZES = T.SIZES + (4 * 256 * 2048 + 5,)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bcast", [False, True])
def test_prior_grad(n, bcast):
    P.check_prior_grad(DEV, n, bcast)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("move", [False, True])
def test_leapfrog_prior(n, kind, move):
    P.check_leapfrog_prior(DEV, n, kind, move)


@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("move", [False, True])
def test_flat_prior_is_the_flat_leapfrog(n, move):
    P.check_flat_prior_is_the_flat_leapfrog(DEV, n, move)


def test_kernels_match_the_cpu_formulas():
    """One step and one penalty give what the torch fallbacks give, to rounding: the vectors
    within a few float32 spacings at their magnitude (|p|, |q| < 8, |g + c w d| < 32), the
    penalties -- fp64 sums of the same float32 values on both sides -- to 1e-12, the kinetic
    energy (from each side's own float32 p') to 1e-5 as in test_hmc_gpu."""
    n = 1025
    q, p, g, im, m, w = P.prior_vectors(n, T.CPU, False, False)
    qd, pd, gd, imd, md, wd = (t.to(DEV) for t in (q, p, g, im, m, w))
    ke, pen, ked, pend = (T._ke_out(d) for d in (T.CPU, T.CPU, DEV, DEV))
    hmc_leapfrog_prior_(q, p, g, im, 0.05, 0.1, m, w, 0.07, ke, pen)
    hmc_leapfrog_prior_(qd, pd, gd, imd, 0.05, 0.1, md, wd, 0.07, ked, pend)
    torch.testing.assert_close(pd.cpu(), p, rtol=0, atol=4 * U24 * 8)
    torch.testing.assert_close(qd.cpu(), q, rtol=0, atol=8 * U24 * 8)
    assert abs(float(ked) - float(ke)) <= 1e-5 * float(ke)
    assert abs(float(pend) - float(pen)) <= 1e-12 * float(pen)
    out, outd = torch.empty_like(g), torch.empty_like(gd)
    gaussian_prior_grad_(q, g, m, w, 0.9, out, pen)
    gaussian_prior_grad_(q.to(DEV), gd, md, wd, 0.9, outd, pend)
    torch.testing.assert_close(outd.cpu(), out, rtol=0, atol=4 * U24 * 32)
    assert abs(float(pend) - float(pen)) <= 1e-12 * float(pen)


def test_the_extension_refuses_bad_arguments():
    """Host-side checks only: nothing is launched."""
    q, p, g, im, m, w = P.prior_vectors(64, DEV, False, False)
    out = torch.empty_like(g)
    f32_energy = torch.zeros(1, device=DEV)
    from multigrad_amd.ops._ext import ext
    bad = [lambda: hmc_leapfrog_prior_(q, p, g[:32], im, 0.1, 0.1, m, w, 0.1),
           lambda: hmc_leapfrog_prior_(q, p, g, im[:7], 0.1, 0.1, m, w, 0.1),
           lambda: hmc_leapfrog_prior_(q, p, g, im, 0.1, 0.1, m[:7], w[:7], 0.1),
           lambda: hmc_leapfrog_prior_(q, q, g, im, 0.1, 0.1, m, w, 0.1),
           lambda: hmc_leapfrog_prior_(q, p, p, im, 0.1, 0.1, m, w, 0.1),
           lambda: hmc_leapfrog_prior_(q, p, g, im, 0.1, 0.1, m, w, 0.1, None, f32_energy),
           lambda: hmc_leapfrog_prior_(q, p, g, im, 0.1, 0.1, m, w, 0.1, f32_energy),
           lambda: ext().hmc_leapfrog_prior(q, p, g, im, 0.1, 0.1, m, w, 0.1, None,
                                            T._ke_out(DEV), None),  # no workspace
           lambda: gaussian_prior_grad_(q, g[:32], m, w, 1.0, out),
           lambda: gaussian_prior_grad_(q, g, m[:7], w[:7], 1.0, out),
           lambda: gaussian_prior_grad_(q, g, m, w, 1.0, q),
           lambda: gaussian_prior_grad_(q, g, m, w, 1.0, out, f32_energy),
           lambda: ext().gaussian_prior_grad(q, g, m, w, 1.0, out, T._ke_out(DEV), None)]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()


def test_chain_matches_reference():
    P.check_chain(DEV)


def test_map_of_a_separable_quadratic():
    P.check_map(DEV)


# ---------------------------------------------------------------- the fused engine's objective
def _population():
    import multigrad_amd.parallel.comm as C
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    C.set_world_comm(None)
    data = make_population_data(num_params=120, num_halos=4000, seed=11, device=DEV)
    m = PopulationSMFModel(aux_data=data)
    m.set_target_from_truth()
    g0 = data["guess"].double().cpu().numpy()
    sig = np.linspace(0.05, 0.5, 120)
    sig[::9] = np.inf
    return m, data, GaussianPrior(g0 + 0.02 * np.cos(np.arange(120)), sig)


def test_engine_objective_with_a_prior():
    """``PriorObjective(engine objective).device_call`` is the bare objective's loss and
    gradient plus the float64 prior terms, within the bound of the gradient op (4u (|g| +
    |c w d|), plus the float32 rounding of the prior's mean and inverse variance: 2u |c w d|
    and u |c w m|); the padding of the engine vector gets no force."""
    m, data, prior = _population()
    weight = 0.3
    eng = m.fused_engine(comm=None)
    try:
        inner = eng.lbfgs_objective(data["guess"])
        obj = PriorObjective(inner, prior, weight)
        layout = inner.vector_layout()
        real = layout.to_local(torch.ones(120, device=DEV)) > 0
        x = inner.x0() + 0.01 * real
        lt0, g0 = inner.device_call(x)
        lt0, g0 = float(lt0.double()), g0.clone()
        lt, g = obj.device_call(x)
        xu = layout.from_local(x).double().cpu().numpy()
        pen = prior.penalty(xu)
        assert abs(float(lt) - (lt0 + weight * pen)) <= 1e-6 * abs(float(lt))
        term = weight * layout.to_local(torch.as_tensor(prior.grad(xu), device=DEV)).double()
        mloc = layout.to_local(torch.as_tensor(np.where(prior.inv_var > 0, prior.mean, 0.0),
                                               device=DEV)).double()
        wloc = layout.to_local(torch.as_tensor(prior.inv_var, device=DEV)).double()
        bound = U24 * (4 * g0.double().abs() + 6 * term.abs() + weight * wloc * mloc.abs())
        err = (g.double() - (g0.double() + term)).abs() - bound
        print(f"engine objective with a prior: max excess {float(err.max()):.3e}")
        assert float(err.max()) <= 0
        assert torch.equal(g[~real], g0[~real])
        assert g.data_ptr() != g0.data_ptr()
    finally:
        if not getattr(eng, "cached", False):
            eng.close()


def test_model_run_bfgs_with_a_prior():
    m, data, prior = _population()
    weight = 0.1
    res = m.run_bfgs(data["guess"], maxsteps=30, method="device", prior=prior,
                     prior_weight=weight)
    loss = float(m.calc_loss_from_params(res.x))
    print(f"engine MAP: nit {res.nit}, fun {res.fun:.6e}, loss {loss:.6e}, "
          f"pen {res.prior_penalty:.6e}")
    assert res.prior_penalty > 0
    assert abs((res.fun - weight * res.prior_penalty) - loss) <= 1e-5 * abs(loss)
    assert abs(res.prior_penalty - prior.penalty(res.x)) <= 1e-12 * res.prior_penalty
    g0 = data["guess"].double().cpu().numpy()
    box = [(float(v) - 0.01, float(v) + 0.01) for v in g0]
    res = m.run_bfgs(data["guess"], maxsteps=30, method="device", prior=prior,
                     prior_weight=weight, param_bounds=box)
    x = res.x.double().cpu().numpy()
    lo, hi = np.array(box, dtype=np.float32).astype(np.float64).T
    assert (x >= lo).all() and (x <= hi).all()
    loss = float(m.calc_loss_from_params(res.x))
    assert abs((res.fun - weight * res.prior_penalty) - loss) <= 1e-5 * abs(loss)


def test_engine_chain_takes_the_device_path():
    """A chain with a prior over the fused engine's objective stays on the device: one host
    call, then L device calls per iteration (counted as
    test_hmc_gpu.test_engine_objective_takes_the_device_path counts them), and the potential
    of the last draw is ``loss_scale * loss + pen`` there."""
    from multigrad_amd.engine._objective import _EngineObjective
    m, data, prior = _population()
    calls = {"device": 0, "host": 0}
    dev_call, host_call = _EngineObjective.device_call, _EngineObjective.__call__

    def count_device(self, x):
        calls["device"] += 1
        return dev_call(self, x)

    def count_host(self, x):
        calls["host"] += 1
        return host_call(self, x)

    _EngineObjective.device_call, _EngineObjective.__call__ = count_device, count_host
    try:
        res = m.run_hmc(data["guess"], nsamples=20, warmup=10, nleapfrog=4, step_size=0.01,
                        adapt_step_size=False, loss_scale=10.0, prior=prior)
    finally:
        _EngineObjective.device_call, _EngineObjective.__call__ = dev_call, host_call
    assert res.nfev == (10 + 20) * 4 + 1
    assert calls["host"] == 1 and calls["device"] == res.nfev
    assert res.n_divergent == 0 and res.accept_rate > 0.3
    assert len(torch.unique(res.samples[:, 0])) > 3
    x = res.samples[-1]
    ref = 10.0 * float(m.calc_loss_from_params(x)) + prior.penalty(x)
    print(f"engine chain: accept {res.accept_rate:.3f}, U {res.potential[-1]:.6e}, ref {ref:.6e}")
    assert math.isfinite(ref) and abs(res.potential[-1] - ref) <= 1e-5 * abs(ref)
    flat = m.run_hmc(data["guess"], nsamples=20, warmup=10, nleapfrog=4, step_size=0.01,
                     adapt_step_size=False, loss_scale=10.0)
    assert not torch.equal(flat.samples, res.samples)


# ---------------------------------------------------------------- two ranks on one GPU
def _two_rank_runs(rank, size):
    import multigrad_amd as mg
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    comm = mg.get_world_comm()
    data = make_population_data(6000, 400_000, seed=21, comm=comm, device=DEV, placement="hashed")
    model = PopulationSMFModel(aux_data=data, comm=comm)
    model.set_target_from_truth()
    g0 = data["guess"].double().cpu().numpy()
    sig = np.linspace(0.05, 0.5, g0.size)
    sig[::9] = np.inf
    prior = GaussianPrior(g0 + 0.02 * np.cos(np.arange(g0.size)), sig)
    res = model.run_bfgs(data["guess"], maxsteps=10, method="device", prior=prior,
                         prior_weight=0.1)
    loss = float(model.calc_loss_from_params(res.x))
    hmc = model.run_hmc(data["guess"], nsamples=4, warmup=0, nleapfrog=3, step_size=0.01,
                        loss_scale=10.0, prior=prior, history="moments", track=[0, 5999])
    u_last = 10.0 * float(model.calc_loss_from_params(hmc.x)) + prior.penalty(hmc.x)
    return (res.x.cpu().numpy(), float(res.fun), int(res.nit), int(res.host_collectives),
            res.reduction, float(res.prior_penalty), loss, hmc.potential, u_last, hmc.reduction)


def test_two_ranks_on_one_gpu_no_host_collectives():
    """ZeRO-sharded vectors over two ranks that share the GPU, with a prior: every rank's
    partial penalty travels in the wide one-shot reduction its evaluation makes anyway, so the
    L-BFGS iterations make no host collective (as
    test_lbfgs_comm_gpu.test_device_lbfgs_multirank_one_gpu_no_host_collectives asserts without
    a prior, with its tolerances against one rank), and the penalty is counted once."""
    import multigrad_amd.parallel.comm as C
    from distributed import run_distributed
    C.set_world_comm(None)
    x1, f1, nit1, _, _, pen1, _, _, _, _ = _two_rank_runs(0, 1)
    res = run_distributed(_two_rank_runs, 2, timeout=600)
    for x, f, nit, host, how, pen, loss, pot, u_last, how_hmc in res:
        assert host == 0, f"{host} host collectives in the L-BFGS iterations ({how})"
        assert how == "xgmi wide one-shot" and how_hmc == "xgmi wide one-shot"
        assert nit == nit1
        assert f == pytest.approx(f1, rel=2e-4, abs=1e-9)
        np.testing.assert_allclose(x, x1, rtol=2e-4, atol=2e-5)
        assert pen > 0 and abs((f - 0.1 * pen) - loss) <= 1e-5 * abs(loss)
        assert abs(pot[-1] - u_last) <= 1e-5 * abs(u_last)
    np.testing.assert_array_equal(res[1][0], res[0][0])
    assert abs(res[1][1] - res[0][1]) <= 1e-12 * abs(res[0][1])
    assert np.abs(res[1][7] - res[0][7]).max() <= 1e-12 * np.abs(res[0][7]).max()
