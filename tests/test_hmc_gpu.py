"""The HMC kernels (csrc/hmc.hip) and the sampler on the GPU: the bodies of test_hmc.py on
``cuda``, and the device-resident trajectory over the fused engine's objective."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hmc as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("move", [False, True])
def test_leapfrog(n, bcast, move):
    T.check_leapfrog(DEV, n, bcast, move)


@pytest.mark.parametrize("n", T.SIZES)
@pytest.mark.parametrize("bcast", [False, True])
def test_momentum(n, bcast):
    T.check_momentum(DEV, n, bcast)


@pytest.mark.parametrize("n", T.SIZES)
def test_commit(n):
    T.check_commit(DEV, n)


def test_kernels_match_the_cpu_formulas():
    """One trajectory step and one commit give what the torch fallbacks give, to rounding."""
    from multigrad_amd.ops.hmc import hmc_commit_, hmc_leapfrog_
    n = 1025
    q, p, g, im, _ = T._vectors(n, T.CPU, False)
    qd, pd, gd, imd = (t.to(DEV) for t in (q, p, g, im))
    ke, ked = T._ke_out(T.CPU), T._ke_out(DEV)
    hmc_leapfrog_(q, p, g, im, 0.05, 0.1, ke)
    hmc_leapfrog_(qd, pd, gd, imd, 0.05, 0.1, ked)
    torch.testing.assert_close(pd.cpu(), p, rtol=0, atol=4 * T.U24 * 8)
    torch.testing.assert_close(qd.cpu(), q, rtol=0, atol=8 * T.U24 * 8)
    assert abs(float(ked) - float(ke)) <= 1e-5 * float(ke)
    mean, m2 = torch.zeros(n), torch.zeros(n)
    meand, m2d = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for c, v in enumerate((q, p, g), 1):
        hmc_commit_(v, c, mean, m2)
        hmc_commit_(v.to(DEV), c, meand, m2d)
    torch.testing.assert_close(meand.cpu(), mean, rtol=0, atol=8 * T.U24 * 8)
    torch.testing.assert_close(m2d.cpu(), m2, rtol=1e-5, atol=1e-5)


def test_the_extension_refuses_bad_arguments():
    from multigrad_amd.ops.hmc import hmc_commit_, hmc_leapfrog_
    q, p, g, im, _ = T._vectors(64, DEV, False)
    with pytest.raises(RuntimeError):
        hmc_leapfrog_(q, p, g[:32], im, 0.1, 0.1)
    with pytest.raises(RuntimeError):
        hmc_leapfrog_(q, q, g, im, 0.1, 0.1)
    with pytest.raises(RuntimeError):
        hmc_leapfrog_(q, p, g, im[:7], 0.1, 0.1)
    with pytest.raises(RuntimeError):
        hmc_leapfrog_(q, p, g, im, 0.1, 0.1, torch.zeros(1, device=DEV))  # fp32 energy
    with pytest.raises(RuntimeError):
        hmc_commit_(q, 1, p, None)
    # an index outside q is never read: its row entry keeps its value
    row = torch.full((2,), -7.0, device=DEV)
    hmc_commit_(q, 1, None, None, torch.tensor([3, 64], device=DEV), row, None)
    assert float(row[0]) == float(q[3]) and float(row[1]) == -7.0


def test_chain_matches_reference():
    T.check_chain(DEV)


def test_adaptation_finds_the_scales():
    res, ratio = T.check_adaptation(DEV, 300, 100)
    assert ratio.min() >= 0.25 and ratio.max() <= 4.0
    assert math.isfinite(res.step_size) and res.step_size > 0


def test_front_end():
    T.check_front_end(DEV)


def test_engine_objective_takes_the_device_path():
    """The small population model of test_engine.py has a fused engine: its trajectories stay
    on the device (``device_call``), L evaluations per iteration after the first one."""
    import multigrad_amd.parallel.comm as C
    from multigrad_amd.engine._objective import _EngineObjective
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    C.set_world_comm(None)
    data = make_population_data(num_params=120, num_halos=4000, seed=11, device=DEV)
    m = PopulationSMFModel(aux_data=data)
    m.set_target_from_truth()
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
        res = m.run_hmc(data["guess"], nsamples=30, warmup=10, nleapfrog=4, step_size=0.05,
                        adapt_step_size=False, loss_scale=10.0, history="moments",
                        track=[0, 57, 119])
    finally:
        _EngineObjective.device_call, _EngineObjective.__call__ = dev_call, host_call
    assert res.nfev == (10 + 30) * 4 + 1
    assert calls["host"] == 1 and calls["device"] == res.nfev  # the first goes through __call__
    assert res.samples is None and res.tracked.shape == (30, 3)
    assert res.mean.shape == (120,) and res.var.shape == (120,) and res.x.shape == (120,)
    for t in (res.tracked, res.mean, res.var, res.x):
        assert t.is_cuda and bool(torch.isfinite(t).all())
    assert res.n_divergent == 0 and res.accept_rate > 0.3
    assert np.isfinite(res.potential).all()
    # user order: the last tracked row is the last position
    assert torch.equal(res.tracked[-1], res.x[[0, 57, 119]])
