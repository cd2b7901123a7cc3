"""The sumstat Jacobian and run_gauss_newton on the MI355X: the grouped population model
(gather + gaussian_binned_sum, forward mode through csrc/binned_jvp.hip) and the quick-start
SMF model, whose fused op has no forward rule (reverse fallback)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _grouped():
    """4 populations x 2 parameters, 20 000 halos, on the device."""
    from multigrad_amd.models.population import PopulationSMFModel, make_population_data
    from multigrad_amd.models.torch_population import (GroupedBinnedPopulationSMFModel,
                                                       torch_population_data)
    data = make_population_data(8, 20_000, seed=3, device=DEV)
    PopulationSMFModel(aux_data=data).set_target_from_truth()
    return GroupedBinnedPopulationSMFModel(aux_data=torch_population_data(data)), data["guess"]


def _term_sums(model, guess):
    """A[k, j] = scale_k sum_i |t_ij dout_k/d(mu, sigma)_i| in float64 for the unit tangent of
    parameter j: t = 1 on the offsets of population c for j = 2c, and ln(10) sigma_c on its
    widths for j = 2c + 1."""
    d = model.aux_data
    th = guess.double().cpu().reshape(-1, 2)
    pop = d["pop"].cpu()
    x = d["x"].double().cpu()
    e = torch.tensor(model.edges, dtype=torch.float64)
    sigma = torch.pow(10.0, th[:, 1])[pop]
    z = (e[None, :] - (x + th[:, 0][pop])[:, None]) / sigma[:, None]
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    dmu = (-(phi[:, 1:] - phi[:, :-1]) / sigma[:, None]).abs()
    zphi = z * phi
    dsig = (-(zphi[:, 1:] - zphi[:, :-1]) / sigma[:, None]).abs() * (math.log(10.0) * sigma)[:, None]
    A = torch.zeros(len(model.edges) - 1, th.numel(), dtype=torch.float64)
    for c in range(th.shape[0]):
        A[:, 2 * c] = dmu[pop == c].sum(0)
        A[:, 2 * c + 1] = dsig[pop == c].sum(0)
    return A * d["scale"].double().cpu()[:, None]


def test_forward_jacobian_matches_reverse_on_the_device():
    model, guess = _grouped()
    s_f, j_f = model.calc_sumstats_jacobian_from_params(guess, mode="forward")
    s_r, j_r = model.calc_sumstats_jacobian_from_params(guess, mode="reverse")
    assert j_f.is_cuda and j_f.shape == (s_f.numel(), 8) and torch.equal(s_f, s_r)
    A = _term_sums(model, guess)
    diff = (j_f.double().cpu() - j_r.double().cpu()).abs()
    bound = 2e-4 * A + 2e-5 * A.max(0, keepdim=True).values
    for j in range(8):
        print(f"column {j}: max |J| {float(j_r[:, j].abs().max()):.3e} max |forward - reverse| "
              f"{float(diff[:, j].max()):.3e} worst diff/bound "
              f"{float((diff[:, j] / bound[:, j]).max()):.3e}")
    assert float(j_r.abs().max()) > 0
    assert bool((diff <= bound).all())


def test_grouped_model_fit_uses_the_forward_jacobian():
    model, guess = _grouped()
    res = model.run_gauss_newton(guess)
    print(f"grouped model: loss={res.fun:.3e} nit={res.nit} nfev={res.nfev} {res.message}")
    assert res.jac_mode == "forward"
    assert res.nit <= 20 and res.fun <= 1e-6


def test_docs_model_falls_back_to_reverse_and_converges():
    from multigrad_amd.models.smf import DocsSMFModel, make_docs_data
    model = DocsSMFModel(aux_data=make_docs_data(device=DEV), device=DEV)
    guess = torch.tensor([-1.0, 0.0], device=DEV)
    with pytest.raises(NotImplementedError):
        model.calc_sumstats_jacobian_from_params(guess, mode="forward")
    res = model.run_gauss_newton(guess)
    print(f"DocsSMFModel: x={res.x} loss={res.fun:.3e} nit={res.nit} nfev={res.nfev}")
    assert res.jac_mode == "reverse"
    assert res.success and res.nit <= 50
    assert np.abs(np.asarray(res.x) - np.array([-2.0, -0.5])).max() <= 1e-4
